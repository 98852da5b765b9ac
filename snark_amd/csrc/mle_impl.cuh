// Multilinear extensions on the device: the eq table, fixing the low variables, evaluation at a point.  The semantics are ark-poly's
// DenseMultilinearExtension (evaluate, fix_variables; little-endian variable order): a table f of N = 2^v Montgomery Fr, index
// i = sum_j b_j 2^j, f~(x) = sum_i f[i] prod_j (b_j x_j + (1 - b_j)(1 - x_j)).  Variable 0 is the lowest index bit.
//     eq    out[i] = prod_j (b_j p_j + (1 - b_j)(1 - p_j))
//     fix   variables 0 .. k-1 of `count` back-to-back tables to p_0 .. p_{k-1}: k halvings f'[i] = f[2i] + p (f[2i+1] - f[2i]),
//           the old variable j + 1 becomes variable j; count x 2^(v-k) out, back to back
//     eval  fix with k = v: count values
//
// Decomposition (gfx950, wave64, workgroups of 256 lanes).
//   mle_eq_kernel    a lane owns the 2^L indices that share their high v - L bits, L = min(v, 3): the product over the high bits
//                    once (v - L multiplications, the factors p_j / 1 - p_j read from a table of 2 v elements the host uploads), then
//                    L doublings in registers (2 + 4 + 8 multiplications): v + 11 multiplications for eight outputs instead of 8 v
//   mle_fold_kernel  one halving: a lane owns SUMCHECK_LANE_PAIRS consecutive outputs of one table (policy, see sumcheck_impl.cuh;
//                    it moves borders and never a byte), reads 2 x 32 bytes an output, writes 32; blockIdx.y is the table; a
//                    grid-stride loop keeps the grid below 2^20 workgroups at any size
// fix runs k launches of mle_fold_kernel, ping-pong between two scratch buffers of count N / 2 and count N / 4 elements, the last
// launch into the caller's output: no launch reads what it writes, and `out` may not overlap `evals` (a lane's output index is
// another lane's input).  Every output is fully reduced (Fr::add / sub / mul reduce), so the bytes do not depend on the route.
// No atomics, no host wait between the launches, no scratch memory in any kernel.
//
// Scratch of one call (MleScratch, grow-only, owned by the context, reserved before the first launch):
//     32 * 2 v           the factors of eq                 32 count (N / 2 + N / 4)   ping-pong of fix / eval
//     32 count N (+ out) staging of the host variants
// The quotient tables of an opening (mle_open_impl.cuh) keep their own fields of MleScratch.
#pragma once
#include <vector>
#include "common.h"
#include "field.cuh"
#include "evals_impl.cuh"

namespace ark355 {

constexpr uint32_t MLE_THREADS = 256;
constexpr uint32_t MLE_MAX_VARS = 40;
constexpr uint32_t MLE_MAX_GRID = 1u << 20;               // workgroups of one launch; beyond it a lane strides
constexpr uint32_t MLE_EQ_LOW = 3;                        // index bits a lane of mle_eq_kernel expands in registers

struct MleScratch {
  DevBuf pt;                         // eq: p_j, 1 - p_j for j < v
  DevBuf a, b;                       // ping-pong of the halvings
  DevBuf in, out;                    // staging of the host variants
  DevBuf row_a, row_b;               // mle_open_impl.cuh: the surviving values of a pass, the input of the next
  DevBuf q, rem;                     // mle_open_impl.cuh: quotients and values of the host variant and of ark355_mle_open_dev
  std::vector<unsigned char> host;   // host image of `pt`: alive until the call's last wait
};

// out[(h << L) | e] for e < 2^L: pt[2 j] = p_j, pt[2 j + 1] = 1 - p_j
template <class Fr, int L>
__global__ void __launch_bounds__(MLE_THREADS)
mle_eq_kernel(const Fr* __restrict__ pt, uint32_t v, uint64_t lanes, Fr* __restrict__ out) {
  for (uint64_t h = (uint64_t)blockIdx.x * MLE_THREADS + threadIdx.x; h < lanes; h += (uint64_t)gridDim.x * MLE_THREADS) {
    Fr vals[1 << L];
    vals[0] = Fr::one();
    bool have = false;
    for (uint32_t j = L; j < v; j++) {
      const Fr f = evals_load(pt + 2 * j + (((h >> (j - L)) & 1u) ? 0u : 1u));
      vals[0] = have ? Fr::mul(vals[0], f) : f;
      have = true;
    }
#pragma unroll
    for (int j = L - 1; j >= 0; j--) {                    // split every entry on bit j
      const Fr pj = evals_load(pt + 2 * j), qj = evals_load(pt + 2 * j + 1);
#pragma unroll
      for (int s = 0; s < (1 << L); s += 2 << j) {
        const Fr base = vals[s];
        vals[s + (1 << j)] = Fr::mul(base, pj);
        vals[s] = Fr::mul(base, qj);
      }
    }
#pragma unroll
    for (int e = 0; e < (1 << L); e++) evals_store(out + (h << L) + e, vals[e]);
  }
}

// out[c out_stride + i] = in[c in_stride + 2 i] + r (in[c in_stride + 2 i + 1] - in[c in_stride + 2 i]) for i < half, c = blockIdx.y
template <class Fr>
__global__ void __launch_bounds__(MLE_THREADS)
mle_fold_kernel(const Fr* __restrict__ in, uint64_t in_stride, uint64_t half, Fr r, Fr* __restrict__ out, uint64_t out_stride,
                uint32_t run) {
  const Fr* p = in + (uint64_t)blockIdx.y * in_stride;
  Fr* o = out + (uint64_t)blockIdx.y * out_stride;
  const uint64_t step = (uint64_t)gridDim.x * MLE_THREADS * run;
  for (uint64_t first = ((uint64_t)blockIdx.x * MLE_THREADS + threadIdx.x) * run; first < half; first += step) {
    for (uint32_t e = 0; e < run && first + e < half; e++) {
      const uint64_t i = first + e;
      const Fr lo = evals_load(p + 2 * i), hi = evals_load(p + 2 * i + 1);
      evals_store(o + i, Fr::add(lo, Fr::mul(r, Fr::sub(hi, lo))));
    }
  }
}

static inline uint32_t mle_grid(uint64_t lanes) {
  const uint64_t g = (lanes + MLE_THREADS - 1) / MLE_THREADS;
  return (uint32_t)(g < 1 ? 1 : (g > MLE_MAX_GRID ? MLE_MAX_GRID : g));
}

// one halving of `count` tables on `st`
template <class Fr>
static void mle_fold_launch(const Fr* in, uint64_t in_stride, uint64_t half, const Fr& r, Fr* out, uint64_t out_stride, uint32_t count,
                            uint32_t run, hipStream_t st) {
  if (!count || !half) return;
  ARK_LAUNCH((mle_fold_kernel<Fr>), dim3(mle_grid((half + run - 1) / run), count), dim3(MLE_THREADS), 0, st, in, in_stride, half, r, out,
             out_stride, run);
  ARK_CHECK_LAUNCH();
}

// the ping-pong buffers of a fix of k variables: the one place of fix / eval that may allocate
template <class Fr>
static void mle_fix_reserve(MleScratch& ms, uint32_t v, uint64_t count, uint32_t k) {
  const uint64_t N = 1ull << v;
  if (k >= 2) ms.a.ensure((size_t)(count * (N / 2)) * sizeof(Fr));
  if (k >= 3) ms.b.ensure((size_t)(count * (N / 4)) * sizeof(Fr));
}

// d_out = the `count` tables at d_in with variables 0 .. k-1 fixed to pt[0 .. k) (Montgomery, host) on `st` (queued, not waited for)
template <class Fr>
static void mle_fix_run(const Fr* d_in, uint32_t v, uint64_t count, const Fr* pt, uint32_t k, Fr* d_out, MleScratch& ms, uint32_t run,
                        hipStream_t st) {
  if (!count) return;
  uint64_t len = 1ull << v;
  if (k == 0) {
    ARK_CHECK_HIP(hipMemcpyAsync(d_out, d_in, (size_t)(count * len) * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    return;
  }
  const Fr* cur = d_in;
  for (uint32_t j = 0; j < k; j++) {
    const uint64_t half = len >> 1;
    Fr* dst = j + 1 == k ? d_out : ((j & 1u) ? ms.b.as<Fr>() : ms.a.as<Fr>());
    mle_fold_launch<Fr>(cur, len, half, pt[j], dst, half, (uint32_t)count, run, st);
    cur = dst;
    len = half;
  }
}

// d_out[i] = eq(pt, i) for i < 2^v on `st` (queued); ms.pt holds 2 v elements
template <class Fr>
static void mle_eq_run(uint32_t v, const Fr* pt, Fr* d_out, MleScratch& ms, hipStream_t st) {
  ms.host.resize((size_t)(2 * v + 2) * sizeof(Fr));
  Fr* t = reinterpret_cast<Fr*>(ms.host.data());
  for (uint32_t j = 0; j < v; j++) {
    t[2 * j] = pt[j];
    t[2 * j + 1] = Fr::sub(Fr::one(), pt[j]);
  }
  if (v) ARK_CHECK_HIP(hipMemcpyAsync(ms.pt.p, t, (size_t)(2 * v) * sizeof(Fr), hipMemcpyHostToDevice, st));
  const uint32_t L = v < MLE_EQ_LOW ? v : MLE_EQ_LOW;
  const uint64_t lanes = 1ull << (v - L);
  const Fr* d_pt = ms.pt.as<Fr>();
  switch (L) {
    case 0: ARK_LAUNCH((mle_eq_kernel<Fr, 0>), dim3(mle_grid(lanes)), dim3(MLE_THREADS), 0, st, d_pt, v, lanes, d_out); break;
    case 1: ARK_LAUNCH((mle_eq_kernel<Fr, 1>), dim3(mle_grid(lanes)), dim3(MLE_THREADS), 0, st, d_pt, v, lanes, d_out); break;
    case 2: ARK_LAUNCH((mle_eq_kernel<Fr, 2>), dim3(mle_grid(lanes)), dim3(MLE_THREADS), 0, st, d_pt, v, lanes, d_out); break;
    default: ARK_LAUNCH((mle_eq_kernel<Fr, 3>), dim3(mle_grid(lanes)), dim3(MLE_THREADS), 0, st, d_pt, v, lanes, d_out); break;
  }
  ARK_CHECK_LAUNCH();
}

}  // namespace ark355
