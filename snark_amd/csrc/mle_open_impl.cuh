// Multilinear openings on the device: the quotient tables of a table at a point (ark-poly-commit MultilinearPC::open, PST13).
// With f^(0) = f and f^(j+1)[i] = f^(j)[2i] + p_j (f^(j)[2i+1] - f^(j)[2i]) -- the rule of mle_fold_kernel -- the quotients are
//     q_j[i] = f^(j)[2i+1] - f^(j)[2i],   i < 2^(v-1-j),   j = 0 .. v-1
// so that f~(X) - f~(p) = sum_j (X_j - p_j) q_j~(X_{j+1}, .., X_{v-1}).  Output of one table, N = 2^v Fr, every element written:
// level j at elements N - 2^(v-j) .. N - 2^(v-j) + 2^(v-1-j) - 1 (the levels back to back, largest first), element N - 1 = f~(p).
//
// Decomposition (gfx950, wave64, workgroups of 256 lanes).  A lane owns E consecutive entries (policy MLE_OPEN_LANE_ENTRIES, a power
// of two, 8 by default), a workgroup K = 256 E; blockIdx.y is the table, a grid-stride loop keeps the grid below MLE_MAX_GRID.
//   mle_open_kernel   one pass over a table of `len` entries = log2 min(K, len) halvings on chip:
//                       log2 E      in the lane's registers
//                       6           across the wave: lane l takes the value of lane l + 2^s (fr_shfl_down); the lanes whose low
//                                   s + 1 bits are zero hold a pair and store its quotient
//                       2           across the four waves: their values through 128 bytes of LDS, thread 0 halves twice
//                     Every quotient goes straight to its final place in the caller's output; the workgroup's one surviving value goes
//                     to a scratch row of len / K entries, the input of the next pass, or -- when it is the last of its table -- to
//                     element N - 1 and to rem_out.  A table shorter than a workgroup, a wave or a lane's E runs the levels that exist.
// A call runs ceil(v / log2 K) passes (at least one: v = 0 copies the entry), ping-pong between two scratch rows of count N / K and
// count N / K^2 entries: the table is read once, the quotients are written once.  No launch reads what it writes; no atomics, no
// host wait between the passes, no scratch memory in the kernel.  Every output is fully reduced (Fr::sub / add / mul reduce), so the
// bytes do not depend on E.
//
// Scratch of one call (MleScratch, grow-only, reserved before the first launch):
//     32 v                     the point                      32 count (N / K + N / K^2)   the pass rows
//     32 count N + 32 count    the quotients and values of the host variant and of ark355_mle_open_dev (with the staged input, `in`)
#pragma once
#include "mle_impl.cuh"
#include "fr_wave.cuh"

namespace ark355 {

constexpr uint32_t MLE_OPEN_LANE_ENTRIES_DEFAULT = 8, MLE_OPEN_LANE_ENTRIES_MAX = 8;

// policy MLE_OPEN_LANE_ENTRIES -> the entries a lane owns: <= 0 selects the default, anything else is clamped to 1 .. 8 and rounded
// down to a power of two
static inline uint32_t mle_open_lane_entries(int32_t policy) {
  if (policy <= 0) return MLE_OPEN_LANE_ENTRIES_DEFAULT;
  uint32_t e = (uint32_t)policy > MLE_OPEN_LANE_ENTRIES_MAX ? MLE_OPEN_LANE_ENTRIES_MAX : (uint32_t)policy;
  while (e & (e - 1)) e &= e - 1;
  return e;
}

// the halvings of a full pass: log2(256 E)
static inline uint32_t mle_open_pass_levels(uint32_t E) { return E >= 8 ? 11 : (E >= 4 ? 10 : (E >= 2 ? 9 : 8)); }

// where level j of a table of N = 2^v entries starts inside its output, in elements
ARK_HD uint64_t mle_open_level_offset(uint64_t N, uint32_t j) { return N - (N >> j); }

// One pass.  in: tables of `len` = 2^a entries at stride in_stride, the state after `level` halvings of tables of N entries
// (len = N >> level); pt[t] = the coordinate of halving level + t.  q: the caller's output, table c at c N.  next: the row of
// len / K survivors at stride next_stride, written only while len > K; otherwise the one survivor goes to q[c N + N - 1] and rem[c].
template <class Fr, int E>
__global__ void __launch_bounds__(MLE_THREADS)
mle_open_kernel(const Fr* __restrict__ in, uint64_t in_stride, uint64_t len, const Fr* __restrict__ pt, uint64_t N, uint32_t level,
                Fr* __restrict__ q, Fr* __restrict__ next, uint64_t next_stride, Fr* __restrict__ rem) {
  constexpr uint32_t LOG_E = E == 8 ? 3 : (E == 4 ? 2 : (E == 2 ? 1 : 0));
  constexpr uint64_t K = (uint64_t)MLE_THREADS * E;
  __shared__ uint32_t wave_val[2][MLE_THREADS / 64][Fr::N];
  const uint32_t tid = threadIdx.x;
  const Fr* p = in + (uint64_t)blockIdx.y * in_stride;
  Fr* o = q + (uint64_t)blockIdx.y * N;
  const uint64_t groups = len > K ? len / K : 1;           // len and K are powers of two
  const uint32_t n = (uint32_t)(len > K ? K : len);        // entries of one workgroup
  const uint32_t mine = n >= E ? ((uint64_t)tid * E < n ? E : 0) : (tid == 0 ? n : 0);   // entries of this lane: E, 0, or all n < E
  const uint32_t lanes = n >= E ? n / E : 1;               // lanes that hold a value after the register halvings
  uint32_t k = 0;
  for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x, k++) {
    const uint64_t first = (g * MLE_THREADS + tid) * E;    // this lane's first entry; first >> t its first index after t halvings
    Fr a[E];
#pragma unroll
    for (int e = 0; e < E; e++) a[e] = (uint32_t)e < mine ? evals_load(p + first + e) : Fr::zero();
    uint32_t t = 0;                                        // halvings done in this pass
#pragma unroll
    for (uint32_t s = 0; s < LOG_E; s++) {
      if ((mine >> s) >= 2) {
        const Fr r = evals_load(pt + s);
        Fr* row = o + mle_open_level_offset(N, level + s) + (first >> (s + 1));
#pragma unroll
        for (int i = 0; i < (E >> (s + 1)); i++) {
          if ((uint32_t)i < (mine >> (s + 1))) {
            const Fr d = Fr::sub(a[2 * i + 1], a[2 * i]);
            evals_store(row + i, d);
            a[i] = Fr::add(a[2 * i], Fr::mul(r, d));
          }
        }
      }
    }
    while (t < LOG_E && (n >> t) >= 2) t++;                // uniform over the workgroup: min(LOG_E, log2 n)
    Fr v = a[0];
    const uint64_t lane_index = g * MLE_THREADS + tid;     // index of this lane's value among the table's values after t halvings
    for (uint32_t s = 0; s < 6 && (lanes >> s) >= 2; s++, t++) {   // uniform: every lane of the workgroup shuffles
      const Fr hi = fr_shfl_down(v, 1u << s);
      const Fr d = Fr::sub(hi, v);
      if ((tid & ((2u << s) - 1)) == 0 && tid < lanes) evals_store(o + mle_open_level_offset(N, level + t) + (lane_index >> (s + 1)), d);
      v = Fr::add(v, Fr::mul(evals_load(pt + t), d));
    }
    const uint32_t waves = lanes > 64 ? lanes / 64 : 1;    // 1, 2 or 4 waves hold a value
    if (waves > 1) {
      uint32_t (*buf)[Fr::N] = wave_val[k & 1];            // two buffers in turn: thread 0 may still read while a wave comes back
      if ((tid & 63u) == 0) {
#pragma unroll
        for (int i = 0; i < Fr::N; i++) buf[tid >> 6][i] = v.l[i];
      }
      __syncthreads();
      if (tid == 0) {                                      // straight-line on purpose: an indexed array of Fr would live in scratch memory
        Fr w0 = v, w1;
#pragma unroll
        for (int i = 0; i < Fr::N; i++) w1.l[i] = buf[1][i];
        if (waves == 4) {
          Fr w2, w3;
#pragma unroll
          for (int i = 0; i < Fr::N; i++) {
            w2.l[i] = buf[2][i];
            w3.l[i] = buf[3][i];
          }
          const Fr r = evals_load(pt + t);
          Fr* row = o + mle_open_level_offset(N, level + t) + 2 * g;
          const Fr d0 = Fr::sub(w1, w0), d1 = Fr::sub(w3, w2);
          evals_store(row, d0);
          evals_store(row + 1, d1);
          w0 = Fr::add(w0, Fr::mul(r, d0));
          w1 = Fr::add(w2, Fr::mul(r, d1));
          t++;
        }
        const Fr d = Fr::sub(w1, w0);
        evals_store(o + mle_open_level_offset(N, level + t) + g, d);
        v = Fr::add(w0, Fr::mul(evals_load(pt + t), d));
      }
    }
    if (tid == 0) {
      if (len > K) {
        evals_store(next + (uint64_t)blockIdx.y * next_stride + g, v);
      } else {
        evals_store(o + N - 1, v);
        if (rem) evals_store(rem + blockIdx.y, v);
      }
    }
  }
}

// the pass rows of one call: the one place of the quotients that may allocate
template <class Fr>
static void mle_open_reserve(MleScratch& ms, uint32_t v, uint64_t count, uint32_t E) {
  const uint64_t N = 1ull << v, K = (uint64_t)MLE_THREADS * E;
  ms.pt.ensure((size_t)(v + 1) * sizeof(Fr));
  if (N > K) ms.row_a.ensure((size_t)(count * (N / K)) * sizeof(Fr));
  if (N / K > K) ms.row_b.ensure((size_t)(count * (N / K / K)) * sizeof(Fr));
}

// d_q = the count x N quotient layout of the `count` tables at d_in at the point pt[0 .. v) (Montgomery, host), d_rem (may be
// nullptr) = the count values, on `st` (queued, not waited for)
template <class Fr>
static void mle_open_run(const Fr* d_in, uint32_t v, uint64_t count, const Fr* pt, Fr* d_q, Fr* d_rem, MleScratch& ms, uint32_t E,
                         hipStream_t st) {
  if (!count) return;
  const uint64_t N = 1ull << v, K = (uint64_t)MLE_THREADS * E;
  ms.host.resize((size_t)(v + 1) * sizeof(Fr));
  if (v) {
    memcpy(ms.host.data(), pt, (size_t)v * sizeof(Fr));
    ARK_CHECK_HIP(hipMemcpyAsync(ms.pt.p, ms.host.data(), (size_t)v * sizeof(Fr), hipMemcpyHostToDevice, st));
  }
  const Fr* d_pt = ms.pt.as<Fr>();
  const Fr* cur = d_in;
  uint64_t len = N;
  uint32_t level = 0, pass = 0;
  for (;;) {
    Fr* nxt = (pass & 1u) ? ms.row_b.as<Fr>() : ms.row_a.as<Fr>();
    const uint64_t groups = len > K ? len / K : 1;
    const dim3 grid((uint32_t)(groups > MLE_MAX_GRID ? MLE_MAX_GRID : groups), (uint32_t)count);
#define ARK_MLE_OPEN_LAUNCH(E_)                                                                                                  \
  ARK_LAUNCH((mle_open_kernel<Fr, E_>), grid, dim3(MLE_THREADS), 0, st, cur, len, len, d_pt + level, N, level, d_q, nxt, groups, d_rem)
    switch (E) {
      case 1: ARK_MLE_OPEN_LAUNCH(1); break;
      case 2: ARK_MLE_OPEN_LAUNCH(2); break;
      case 4: ARK_MLE_OPEN_LAUNCH(4); break;
      default: ARK_MLE_OPEN_LAUNCH(8); break;
    }
#undef ARK_MLE_OPEN_LAUNCH
    ARK_CHECK_LAUNCH();
    if (len <= K) break;
    cur = nxt;
    len = groups;
    level += mle_open_pass_levels(E);
    pass++;
  }
}

}  // namespace ark355
