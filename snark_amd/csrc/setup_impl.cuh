// Groth16 generator on the device (circuit_specific_setup, the reference's snark/src/lib.rs:43-46; upstream
// `generate_parameters_with_qap` / `R1CSToQAP::instance_map_with_evaluation`, SURVEY.md Appendix A "Setup"): the scalar
// stages of ark355_setup, from the resident CSR matrices (R1csDev) and the five trapdoor elements to the canonical scalar
// vectors the fixed-base kernels of api_impl.cuh multiply out.  Same values as the host generator Api::setup_scalars --
// field arithmetic is exact, so the order in which a column is summed does not matter.
//
//   S1  Lagrange coefficients  L_k(tau) = Z(tau)/N * w^k / (tau - w^k): a lane owns SETUP_RUN consecutive k, one
//       Montgomery-trick batch inversion per lane.  tau INSIDE the domain (Z(tau) = 0) never reaches that kernel: the host
//       detects it and launches the indicator kernel L_k = [w^k == tau] instead.
//   S2  column-major order of the three matrices, built once: a 32-bit histogram of the column indices (3 m counters, the
//       matrices side by side), an exclusive scan (scan_exclusive of msm_impl.cuh), a scatter of (row, cidx).  An entry
//       finds its row by bisection of row_ptr, so no lane walks a row either.
//   S3  gather  u_j = sum_i L_i A[i][j] (+ L_{n+j} for j < ell), v_j, w_j: one lane per column of at most
//       SETUP_LANE_COL entries.  A longer column (One, hot variables) is cut into chunks of SETUP_CHUNK entries, one
//       workgroup each (eight entries per lane, wave shuffles, four wave sums through LDS), and one wave per heavy column
//       adds the chunk sums.  The heavy list is built by the gather lanes with ONE 64-bit atomic per heavy column
//       (column count in the high word, chunk count in the low word), which keeps the chunk bases sorted by slot.
//   S4  combination  gamma_abc_j = (beta u_j + alpha v_j + w_j) / gamma (j < ell), l_j = (..) / delta (j >= ell), and the
//       Montgomery -> canonical conversion of u, v, w; h_i = Z(tau)/delta * tau^i as a running product per lane run.
#pragma once
#include "common.h"
#include "msm_impl.cuh"
#include "witness_impl.cuh"

namespace ark355 {

constexpr uint32_t SETUP_THREADS = 256;
constexpr uint32_t SETUP_RUN = 8;                         // domain points per lane of S1: one inversion per eight coefficients
constexpr uint32_t SETUP_H_RUN = 16;                      // powers of tau per lane of the h kernel
constexpr uint32_t SETUP_LANE_COL = 64;                   // the longest column a single lane sums
constexpr uint32_t SETUP_CHUNK = SETUP_THREADS * 8;       // entries of a heavy column per workgroup

template <class Fr>
ARK_D Fr fr_pow(Fr x, uint64_t e) {
  Fr r = Fr::one();
  while (e) {
    if (e & 1) r = Fr::mul_ni(r, x);
    x = Fr::sqr_ni(x);
    e >>= 1;
  }
  return r;
}

// S1.  tau is outside the domain: every denominator tau - w^k is non-zero.
template <class Fr>
__global__ void __launch_bounds__(SETUP_THREADS)
setup_lagrange_kernel(Fr* __restrict__ L, uint64_t N, Fr tau, Fr omega, Fr omega_inv, Fr cN) {
  const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * SETUP_RUN;
  if (first >= N) return;
  const uint32_t cnt = (first + SETUP_RUN <= N) ? SETUP_RUN : (uint32_t)(N - first);
  Fr pref[SETUP_RUN];
  Fr p = fr_pow(omega, first), acc = Fr::one();
#pragma unroll
  for (uint32_t j = 0; j < SETUP_RUN; j++) {
    if (j < cnt) {                                      // prefix products of this run's denominators
      acc = Fr::mul(acc, Fr::sub(tau, p));
      pref[j] = acc;
      p = Fr::mul(p, omega);
    }
  }
  Fr inv = Fr::inv(acc);
#pragma unroll
  for (uint32_t jj = 0; jj < SETUP_RUN; jj++) {
    const uint32_t j = SETUP_RUN - 1 - jj;
    if (j < cnt) {
      p = Fr::mul(p, omega_inv);                        // w^(first + j)
      const Fr iv = j > 0 ? Fr::mul(inv, pref[j - 1]) : inv;
      inv = Fr::mul(inv, Fr::sub(tau, p));
      L[first + j] = Fr::mul(Fr::mul(iv, p), cN);
    }
  }
}

// S1 for tau = w^k0: L_k = [w^k == tau], as `evaluate_all_lagrange_coefficients` upstream returns it
template <class Fr>
__global__ void __launch_bounds__(SETUP_THREADS)
setup_indicator_kernel(Fr* __restrict__ L, uint64_t N, Fr tau, Fr omega) {
  const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * SETUP_RUN;
  if (first >= N) return;
  const uint32_t cnt = (first + SETUP_RUN <= N) ? SETUP_RUN : (uint32_t)(N - first);
  Fr p = fr_pow(omega, first);
  for (uint32_t j = 0; j < cnt; j++) {
    L[first + j] = (p == tau) ? Fr::one() : Fr::zero();
    p = Fr::mul(p, omega);
  }
}

// S2: cnt[col0 + col[t]]++ for the nnz entries of one matrix
static __global__ void __launch_bounds__(SETUP_THREADS)
setup_col_count_kernel(const uint32_t* __restrict__ col, uint32_t nnz, uint32_t col0, uint32_t* __restrict__ cnt) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nnz) return;
  atomicAdd(&cnt[col0 + col[t]], 1u);
}

// S2: entry t of one matrix -> (row, cidx) at the next free place of its column.  The row is the last i with
// row_ptr[i] <= t (rows may be empty).
static __global__ void __launch_bounds__(SETUP_THREADS)
setup_col_scatter_kernel(const uint32_t* __restrict__ rp, const uint32_t* __restrict__ col, const uint32_t* __restrict__ cidx,
                         uint32_t n, uint32_t nnz, uint32_t col0, uint32_t* __restrict__ cursor, uint2* __restrict__ ent) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t64 >= nnz) return;
  const uint32_t t = (uint32_t)t64;
  uint32_t lo = 0, hi = n;                              // rp[lo] <= t < rp[hi]  (rp[0] = 0, rp[n] = nnz)
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (rp[mid] <= t) lo = mid;
    else hi = mid;
  }
  const uint32_t pos = atomicAdd(&cursor[col0 + col[t]], 1u);
  ent[pos] = make_uint2(lo, cidx[t]);
}

// one term of a column sum: L_row * coefficient (cidx 0 = the coefficient one)
template <class Fr>
ARK_D Fr setup_term(const uint2 e, const Fr* __restrict__ L, const Fr* __restrict__ pool) {
  Fr v = L[e.x];
  if (e.y != 0) v = Fr::mul(v, pool[e.y]);
  return v;
}

// S3: column j of the 3 m side-by-side columns (u: [0, m), v: [m, 2m), w: [2m, 3m)).  Heavy columns only enter the list.
template <class Fr>
__global__ void __launch_bounds__(SETUP_THREADS)
setup_gather_kernel(const uint32_t* __restrict__ off, const uint2* __restrict__ ent, const Fr* __restrict__ L,
                    const Fr* __restrict__ pool, uint32_t cols, uint32_t ell, uint64_t n, Fr* __restrict__ uvw,
                    unsigned long long* __restrict__ heavy_ctr, uint32_t* __restrict__ heavy_col,
                    uint32_t* __restrict__ heavy_base) {
  const uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j64 >= cols) return;
  const uint32_t j = (uint32_t)j64;
  const uint32_t lo = off[j], hi = off[j + 1], len = hi - lo;
  if (len > SETUP_LANE_COL) {
    const uint32_t chunks = (len + SETUP_CHUNK - 1) / SETUP_CHUNK;
    const unsigned long long old = atomicAdd(heavy_ctr, (1ull << 32) | (unsigned long long)chunks);
    const uint32_t slot = (uint32_t)(old >> 32);
    heavy_col[slot] = j;
    heavy_base[slot] = (uint32_t)old;
    return;
  }
  Fr acc = (j < ell) ? L[n + j] : Fr::zero();            // the input-consistency rows of A: u_j += L_{n+j}
  for (uint32_t t = lo; t < hi; t++) acc = Fr::add(acc, setup_term(ent[t], L, pool));
  uvw[j] = acc;
}

template <class Fr>
ARK_D Fr setup_wave_sum(Fr v) {
  for (int mask = 32; mask >= 1; mask >>= 1) {
    Fr o;
#pragma unroll
    for (int i = 0; i < Fr::N; i++) o.l[i] = (uint32_t)__shfl_xor((int)v.l[i], mask, 64);
    v = Fr::add(v, o);
  }
  return v;
}

// S3: one workgroup per chunk of a heavy column.  item -> slot: the last slot with heavy_base[slot] <= item.
template <class Fr>
__global__ void __launch_bounds__(SETUP_THREADS)
setup_heavy_kernel(const uint32_t* __restrict__ off, const uint2* __restrict__ ent, const Fr* __restrict__ L,
                   const Fr* __restrict__ pool, const uint32_t* __restrict__ heavy_col, const uint32_t* __restrict__ heavy_base,
                   uint32_t n_heavy, Fr* __restrict__ partial) {
  __shared__ uint32_t wave_sum[SETUP_THREADS / 64][Fr::N];
  const uint32_t item = blockIdx.x, tid = threadIdx.x;
  uint32_t s = 0, e = n_heavy;
  while (e - s > 1) {
    const uint32_t mid = s + ((e - s) >> 1);
    if (heavy_base[mid] <= item) s = mid;
    else e = mid;
  }
  const uint32_t j = heavy_col[s], c = item - heavy_base[s];
  const uint32_t lo = off[j] + c * SETUP_CHUNK;
  const uint32_t end = off[j + 1], hi = (end - lo > SETUP_CHUNK) ? lo + SETUP_CHUNK : end;
  Fr acc = Fr::zero();
  for (uint32_t t = lo + tid; t < hi; t += SETUP_THREADS) acc = Fr::add(acc, setup_term(ent[t], L, pool));
  acc = setup_wave_sum(acc);
  if ((tid & 63u) == 0) {
#pragma unroll
    for (int i = 0; i < Fr::N; i++) wave_sum[tid >> 6][i] = acc.l[i];
  }
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < SETUP_THREADS / 64; w++) {
      Fr o;
#pragma unroll
      for (int i = 0; i < Fr::N; i++) o.l[i] = wave_sum[w][i];
      acc = Fr::add(acc, o);
    }
    partial[item] = acc;
  }
}

// S3: one wave per heavy column adds its chunk sums
template <class Fr>
__global__ void __launch_bounds__(64)
setup_heavy_sum_kernel(const uint32_t* __restrict__ heavy_col, const uint32_t* __restrict__ heavy_base, uint32_t n_heavy,
                       uint32_t n_items, const Fr* __restrict__ partial, const Fr* __restrict__ L, uint32_t ell, uint64_t n,
                       Fr* __restrict__ uvw) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  const uint32_t b0 = heavy_base[s], b1 = (s + 1 < n_heavy) ? heavy_base[s + 1] : n_items;
  Fr acc = Fr::zero();
  for (uint32_t i = b0 + lane; i < b1; i += 64) acc = Fr::add(acc, partial[i]);
  acc = setup_wave_sum(acc);
  if (lane == 0) {
    const uint32_t j = heavy_col[s];
    if (j < ell) acc = Fr::add(acc, L[n + j]);
    uvw[j] = acc;
  }
}

// S4: canonical u, v, w (m each), l (m - ell) and gamma_abc (ell) from the Montgomery sums
template <class Fr>
__global__ void __launch_bounds__(SETUP_THREADS)
setup_combine_kernel(const Fr* __restrict__ uvw, uint32_t m, uint32_t ell, Fr alpha, Fr beta, Fr gamma_inv, Fr delta_inv,
                     Fr* __restrict__ cu, Fr* __restrict__ cv, Fr* __restrict__ cw, Fr* __restrict__ cl,
                     Fr* __restrict__ cgabc) {
  const uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j64 >= m) return;
  const uint32_t j = (uint32_t)j64;
  const Fr u = uvw[j], v = uvw[(uint64_t)m + j], w = uvw[2ull * m + j];
  const Fr abc = Fr::add(Fr::add(Fr::mul(beta, u), Fr::mul(alpha, v)), w);
  if (j < ell) cgabc[j] = Fr::from_mont(Fr::mul(abc, gamma_inv));
  else cl[j - ell] = Fr::from_mont(Fr::mul(abc, delta_inv));
  cu[j] = Fr::from_mont(u);
  cv[j] = Fr::from_mont(v);
  cw[j] = Fr::from_mont(w);
}

// S4: h_i = h0 tau^i (h0 = Z(tau) / delta), canonical
template <class Fr>
__global__ void __launch_bounds__(SETUP_THREADS)
setup_h_kernel(Fr* __restrict__ out, uint64_t count, Fr tau, Fr h0) {
  const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * SETUP_H_RUN;
  if (first >= count) return;
  const uint32_t cnt = (first + SETUP_H_RUN <= count) ? SETUP_H_RUN : (uint32_t)(count - first);
  Fr p = Fr::mul(fr_pow(tau, first), h0);
  for (uint32_t i = 0; i < cnt; i++) {
    out[first + i] = Fr::from_mont(p);
    p = Fr::mul(p, tau);
  }
}

// canonical scalars of the generator, resident: u, v, w (m), l (w), gamma_abc (ell), h (N - 1; only when asked for)
struct SetupScalarsDev {
  DevBuf u, v, w, l, gabc, h;
};

static inline uint32_t setup_grid(uint64_t lanes) { return (uint32_t)((lanes + SETUP_THREADS - 1) / SETUP_THREADS); }

// td: tau, alpha, beta, gamma, delta in Montgomery form (gamma, delta non-zero).  Everything is queued on `st`; the one
// host wait in here reads the heavy-column counter (8 bytes).  All scratch of the transposition is gone on return.
template <class Curve>
static void setup_scalars_dev(const R1csDev& r1, const typename Curve::Fr td[5], bool want_h, SetupScalarsDev& out,
                              hipStream_t st) {
  using Fr = typename Curve::Fr;
  const uint64_t n = r1.n, ell = r1.ell, m = r1.m, N = r1.N;
  uint64_t nnz = 0;
  for (int k = 0; k < 3; k++) nnz += r1.nnz[k];
  ARK_REQUIRE(3 * m + 1 < (1ull << 32) && nnz < (1ull << 32) && n < (1ull << 32), ARK355_EINVAL,
              "instance too large for the device generator (3 (ell + w) and the non-zeros of A, B, C together must stay below 2^32)");
  const Fr tau = td[0], alpha = td[1], beta = td[2];
  const Fr gamma_inv = Fr::inv(td[3]), delta_inv = Fr::inv(td[4]);
  const Fr omega = ntt_root<Fr>(r1.log_n, false), omega_inv = ntt_root<Fr>(r1.log_n, true);
  const Fr zt = Fr::sub(fr_pow_u64(tau, N), Fr::one());
  Fr nn = Fr::zero();
  nn.l[0] = (uint32_t)N;
  nn.l[1] = (uint32_t)(N >> 32);
  const Fr cN = Fr::mul(zt, Fr::inv(Fr::to_mont(nn)));
  const uint32_t cols = (uint32_t)(3 * m);

  DevBuf d_uvw((size_t)cols * sizeof(Fr));
  {
    DevBuf d_L(N * sizeof(Fr));
    const uint32_t lg_grid = setup_grid((N + SETUP_RUN - 1) / SETUP_RUN);
    if (zt.is_zero()) {
      ARK_LAUNCH((setup_indicator_kernel<Fr>), dim3(lg_grid), dim3(SETUP_THREADS), 0, st, d_L.as<Fr>(), N, tau, omega);
    } else {
      ARK_LAUNCH((setup_lagrange_kernel<Fr>), dim3(lg_grid), dim3(SETUP_THREADS), 0, st, d_L.as<Fr>(), N, tau, omega, omega_inv, cN);
    }
    ARK_CHECK_LAUNCH();

    // column-major order: counters and offsets of the 3 m columns (+ the total), then (row, cidx) per entry
    DevBuf d_cnt(((size_t)cols + 1) * 4), d_off(((size_t)cols + 1) * 4), d_cur(((size_t)cols + 1) * 4), d_ent((size_t)nnz * sizeof(uint2)), aux;
    ARK_CHECK_HIP(hipMemsetAsync(d_cnt.p, 0, ((size_t)cols + 1) * 4, st));
    for (int k = 0; k < 3; k++) {
      if (!r1.nnz[k]) continue;
      ARK_LAUNCH(setup_col_count_kernel, dim3(setup_grid(r1.nnz[k])), dim3(SETUP_THREADS), 0, st, r1.col[k].as<const uint32_t>(),
                 (uint32_t)r1.nnz[k], (uint32_t)(k * m), d_cnt.as<uint32_t>());
      ARK_CHECK_LAUNCH();
    }
    scan_exclusive(st, d_cnt.as<const uint32_t>(), d_off.as<uint32_t>(), cols, d_off.as<uint32_t>() + cols, aux);
    ARK_CHECK_HIP(hipMemcpyAsync(d_cur.p, d_off.p, (size_t)cols * 4, hipMemcpyDeviceToDevice, st));
    for (int k = 0; k < 3; k++) {
      if (!r1.nnz[k]) continue;
      ARK_LAUNCH(setup_col_scatter_kernel, dim3(setup_grid(r1.nnz[k])), dim3(SETUP_THREADS), 0, st,
                 r1.row_ptr[k].as<const uint32_t>(), r1.col[k].as<const uint32_t>(), r1.cidx[k].as<const uint32_t>(), (uint32_t)n,
                 (uint32_t)r1.nnz[k], (uint32_t)(k * m), d_cur.as<uint32_t>(), d_ent.as<uint2>());
      ARK_CHECK_LAUNCH();
    }

    // gather; a column of more than SETUP_LANE_COL entries goes to the heavy list (at most nnz / SETUP_LANE_COL of them)
    const size_t heavy_cap = (size_t)(nnz / SETUP_LANE_COL) + 1;
    DevBuf d_ctr(8), d_hcol(heavy_cap * 4), d_hbase(heavy_cap * 4);
    ARK_CHECK_HIP(hipMemsetAsync(d_ctr.p, 0, 8, st));
    ARK_LAUNCH((setup_gather_kernel<Fr>), dim3(setup_grid(cols)), dim3(SETUP_THREADS), 0, st, d_off.as<const uint32_t>(),
               d_ent.as<const uint2>(), d_L.as<const Fr>(), r1.pool.as<const Fr>(), cols, (uint32_t)ell, n, d_uvw.as<Fr>(),
               d_ctr.as<unsigned long long>(), d_hcol.as<uint32_t>(), d_hbase.as<uint32_t>());
    ARK_CHECK_LAUNCH();
    unsigned long long ctr = 0;
    ARK_CHECK_HIP(hipMemcpyAsync(&ctr, d_ctr.p, 8, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    const uint32_t n_heavy = (uint32_t)(ctr >> 32), n_items = (uint32_t)ctr;
    if (n_heavy) {
      DevBuf d_part((size_t)n_items * sizeof(Fr));
      ARK_LAUNCH((setup_heavy_kernel<Fr>), dim3(n_items), dim3(SETUP_THREADS), 0, st, d_off.as<const uint32_t>(),
                 d_ent.as<const uint2>(), d_L.as<const Fr>(), r1.pool.as<const Fr>(), d_hcol.as<const uint32_t>(),
                 d_hbase.as<const uint32_t>(), n_heavy, d_part.as<Fr>());
      ARK_CHECK_LAUNCH();
      ARK_LAUNCH((setup_heavy_sum_kernel<Fr>), dim3(n_heavy), dim3(64), 0, st, d_hcol.as<const uint32_t>(),
                 d_hbase.as<const uint32_t>(), n_heavy, n_items, d_part.as<const Fr>(), d_L.as<const Fr>(), (uint32_t)ell, n,
                 d_uvw.as<Fr>());
      ARK_CHECK_LAUNCH();
      ARK_CHECK_HIP(hipStreamSynchronize(st));          // d_part is freed here
    }
    ARK_CHECK_HIP(hipStreamSynchronize(st));            // so is the column-major scratch
  }

  out.u.alloc(m * sizeof(Fr));
  out.v.alloc(m * sizeof(Fr));
  out.w.alloc(m * sizeof(Fr));
  out.l.alloc(r1.w * sizeof(Fr));
  out.gabc.alloc(ell * sizeof(Fr));
  ARK_LAUNCH((setup_combine_kernel<Fr>), dim3(setup_grid(m)), dim3(SETUP_THREADS), 0, st, d_uvw.as<const Fr>(), (uint32_t)m,
             (uint32_t)ell, alpha, beta, gamma_inv, delta_inv, out.u.as<Fr>(), out.v.as<Fr>(), out.w.as<Fr>(), out.l.as<Fr>(),
             out.gabc.as<Fr>());
  ARK_CHECK_LAUNCH();
  if (want_h) {
    out.h.alloc((N - 1) * sizeof(Fr));
    if (N > 1) {
      ARK_LAUNCH((setup_h_kernel<Fr>), dim3(setup_grid((N - 1 + SETUP_H_RUN - 1) / SETUP_H_RUN)), dim3(SETUP_THREADS), 0, st,
                 out.h.as<Fr>(), N - 1, tau, Fr::mul(zt, delta_inv));
      ARK_CHECK_LAUNCH();
    }
  }
  ARK_CHECK_HIP(hipStreamSynchronize(st));              // d_uvw is freed on return
}

}  // namespace ark355
