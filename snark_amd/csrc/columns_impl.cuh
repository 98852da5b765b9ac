// Column polynomials of any GR1CS predicate at a point, on the device: the generator's half of a resident system.  For the t
// matrices M_0 .. M_{t-1} (n rows, m = num_instance + num_witness columns) of one predicate and a vector y of n Fr
//     out[k][j] = sum over the STORED entries (i, j, c) of M_k of c * y[i]          (= (M_k^T y)_j, mat_vec_mul transposed)
// and, with y = (L_i(tau))_i over H_N, out[k][j] = sum_i M_k[i][j] L_i(tau): the column polynomials of the predicate at tau,
// R1CSToQAP::instance_map_with_evaluation's a, b, c for any arity (rows n .. N-1 are zero rows and contribute nothing).
// setup_impl.cuh computes the same sums for Groth16 only (R1csDev, three matrices, the instance rows u_j += L_{n+j}, canonical
// output and the alpha/beta/gamma/delta combination behind them); here the resident Gr1csPred arrays are read where they lie
// (the Gr1csMat table, the shared pool, pool index 0 = one: no multiply), the output is Montgomery, y is any vector, and the
// scratch is the context's and grows only -- no allocation, no free and no wait for one inside a call.
//
//   C1  column-major order of the t matrices side by side (t m columns):
//         cols_count_kernel    cnt[k m + col]++ for every stored entry, all matrices in ONE launch (grid.y = t)
//         scan_exclusive       (msm_impl.cuh) the offsets and, behind them, the total
//         cols_scatter_kernel  entry e of M_k -> (row, pool index) at the next free place of its column (grid.y = t); the row
//                              is found by bisection of row_ptr.  The places inside a column come from atomics, so their order
//                              differs from run to run: field addition is exact, the sums do not.
//   C2  gather:
//         cols_gather_kernel   one lane per column of at most lane_max (policy COLS_LANE_MAX) entries.  A longer column (the
//                              constant One, hot variables) enters the heavy list with ONE 64-bit atomic (heavy columns in the
//                              high word, chunks in the low word: the chunk bases come out sorted by slot).
//         cols_heavy_kernel    one workgroup per chunk of COLS_CHUNK entries of a heavy column: eight entries per lane, a wave
//                              reduction by shuffles, the four wave sums through LDS
//         cols_heavy_sum_kernel one wave per heavy column adds its chunk sums
//       The one host wait before the end reads the heavy counter (8 bytes) to size the last two grids.
//   C3  Lagrange vector for columns_at / lagrange_fr: setup_lagrange_kernel, or setup_indicator_kernel when tau lies in H_N
//       (both of setup_impl.cuh, unchanged); it stays in the scratch and never visits the host.
//
// Scratch of one call (ColumnsScratch, bytes; nnz = the stored entries of the t matrices together, H = nnz / (lane_max + 1) + 1
// the most heavy columns there can be, I = nnz / COLS_CHUNK + H the most chunks):
//     8 (t m + 1)  counters / cursors and offsets      8 nnz   (row, pool index) pairs     8 H + 8   heavy list and its counter
//     32 I         chunk sums                          32 N    Lagrange vector (columns_at)
//     32 (y_len + t m)  staging of y and of the output (host variants only)
#pragma once
#include <string>
#include "common.h"
#include "msm_impl.cuh"
#include "gr1cs_impl.cuh"
#include "setup_impl.cuh"

namespace ark355 {

constexpr uint32_t COLS_THREADS = 256;
constexpr uint32_t COLS_LANE_MAX_DEFAULT = SETUP_LANE_COL;     // 64: the generator's measured choice (setup_impl.cuh)
constexpr uint32_t COLS_LANE_MAX_LIMIT = 1u << 20;
constexpr uint32_t COLS_CHUNK = COLS_THREADS * 8;              // entries of a heavy column per workgroup: eight per lane

// policy COLS_LANE_MAX -> the longest column one lane sums: <= 0 selects the default, anything else is clamped to the limit
static inline uint32_t cols_lane_max(int32_t policy) {
  if (policy <= 0) return COLS_LANE_MAX_DEFAULT;
  return (uint32_t)policy > COLS_LANE_MAX_LIMIT ? COLS_LANE_MAX_LIMIT : (uint32_t)policy;
}

// grow-only scratch of a context
struct ColumnsScratch {
  DevBuf cnt, off, ent, ctr, hcol, hbase, part, scan_aux;
  DevBuf lag;            // the Lagrange vector of columns_at / the host variant of lagrange_fr
  DevBuf y, out;         // staging of the host variants
};

struct ColumnsDims {
  uint64_t n = 0, cols = 0, nnz = 0, max_nnz = 0;
  uint32_t log_domain = 0;          // columns_at only
};

// What one call needs and what refuses it; no HIP call.  with_domain: the domain rule of ark355_gr1cs_quotient.
static inline int32_t columns_dims(const Gr1csDev& g, const Gr1csPred& P, bool with_domain, uint32_t log_n, uint32_t two_adicity,
                                   ColumnsDims* d, std::string* why) {
  d->n = P.n;
  d->cols = (uint64_t)P.arity * g.m;
  d->nnz = 0;
  d->max_nnz = 0;
  for (uint32_t k = 0; k < P.arity; k++) {
    d->nnz += P.nnz[k];
    d->max_nnz = std::max(d->max_nnz, P.nnz[k]);
  }
  if (with_domain) {
    uint32_t log_domain = log_n;
    if (log_n == 0) {
      log_domain = 1;
      while ((1ull << log_domain) < P.n) log_domain++;
    }
    d->log_domain = log_domain;
    if (log_domain > two_adicity) {
      *why = "the evaluation domain exceeds the largest radix-2 domain of Fr";
      return ARK355_E_POLY_DEGREE_TOO_LARGE;
    }
    if ((1ull << log_domain) < P.n) {
      *why = "2^log_n is below the predicate's row count";
      return ARK355_EINVAL;
    }
  }
  if (d->cols + 1 >= (1ull << 32)) {
    *why = "arity * (num_instance + num_witness) + 1 must stay below 2^32";
    return ARK355_EINVAL;
  }
  if (d->nnz >= (1ull << 32)) {
    *why = "the non-zeros of the predicate's matrices together must stay below 2^32";
    return ARK355_EINVAL;
  }
  return ARK355_OK;
}

// C1: one lane per stored entry of matrix blockIdx.y; the matrix's entry count is rp[n]
static __global__ void __launch_bounds__(COLS_THREADS)
cols_count_kernel(const Gr1csMat* __restrict__ mats, uint32_t n, uint32_t m, uint32_t* __restrict__ cnt) {
  const Gr1csMat M = mats[blockIdx.y];
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= M.rp[n]) return;
  atomicAdd(&cnt[blockIdx.y * m + M.col[e]], 1u);
}

// C1: entry e of matrix blockIdx.y -> (row, pool index) at the next free place of its column.  The row is the last i with
// rp[i] <= e (rows may be empty).
static __global__ void __launch_bounds__(COLS_THREADS)
cols_scatter_kernel(const Gr1csMat* __restrict__ mats, uint32_t n, uint32_t m, uint32_t* __restrict__ cursor,
                    uint2* __restrict__ ent) {
  const Gr1csMat M = mats[blockIdx.y];
  const uint64_t e64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e64 >= M.rp[n]) return;
  const uint32_t e = (uint32_t)e64;
  uint32_t lo = 0, hi = n;                               // rp[lo] <= e < rp[hi]  (rp[0] = 0, rp[n] = the entry count > e)
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (M.rp[mid] <= e) lo = mid;
    else hi = mid;
  }
  const uint32_t pos = atomicAdd(&cursor[blockIdx.y * m + M.col[e]], 1u);
  ent[pos] = make_uint2(lo, M.ci[e]);
}

// C2: column j of the t m side-by-side columns.  Heavy columns only enter the list.
template <class Fr>
__global__ void __launch_bounds__(COLS_THREADS)
cols_gather_kernel(const uint32_t* __restrict__ off, const uint2* __restrict__ ent, const Fr* __restrict__ y,
                   const Fr* __restrict__ pool, uint32_t cols, uint32_t lane_max, Fr* __restrict__ out,
                   unsigned long long* __restrict__ heavy_ctr, uint32_t* __restrict__ heavy_col, uint32_t* __restrict__ heavy_base) {
  const uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j64 >= cols) return;
  const uint32_t j = (uint32_t)j64;
  const uint32_t lo = off[j], hi = off[j + 1], len = hi - lo;
  if (len > lane_max) {
    const uint32_t chunks = (len + COLS_CHUNK - 1) / COLS_CHUNK;
    const unsigned long long old = atomicAdd(heavy_ctr, (1ull << 32) | (unsigned long long)chunks);
    const uint32_t slot = (uint32_t)(old >> 32);
    heavy_col[slot] = j;
    heavy_base[slot] = (uint32_t)old;
    return;
  }
  Fr acc = Fr::zero();
  for (uint32_t t = lo; t < hi; t++) acc = Fr::add(acc, setup_term(ent[t], y, pool));
  out[j] = acc;
}

// C2: one workgroup per chunk of a heavy column.  item -> slot: the last slot with heavy_base[slot] <= item.
template <class Fr>
__global__ void __launch_bounds__(COLS_THREADS)
cols_heavy_kernel(const uint32_t* __restrict__ off, const uint2* __restrict__ ent, const Fr* __restrict__ y,
                  const Fr* __restrict__ pool, const uint32_t* __restrict__ heavy_col, const uint32_t* __restrict__ heavy_base,
                  uint32_t n_heavy, Fr* __restrict__ partial) {
  __shared__ uint32_t wave_sum[COLS_THREADS / 64][Fr::N];
  const uint32_t item = blockIdx.x, tid = threadIdx.x;
  uint32_t s = 0, e = n_heavy;
  while (e - s > 1) {
    const uint32_t mid = s + ((e - s) >> 1);
    if (heavy_base[mid] <= item) s = mid;
    else e = mid;
  }
  const uint32_t j = heavy_col[s], c = item - heavy_base[s];
  const uint32_t lo = off[j] + c * COLS_CHUNK;
  const uint32_t end = off[j + 1], hi = (end - lo > COLS_CHUNK) ? lo + COLS_CHUNK : end;
  Fr acc = Fr::zero();
  for (uint32_t t = lo + tid; t < hi; t += COLS_THREADS) acc = Fr::add(acc, setup_term(ent[t], y, pool));
  acc = setup_wave_sum(acc);
  if ((tid & 63u) == 0) {
#pragma unroll
    for (int i = 0; i < Fr::N; i++) wave_sum[tid >> 6][i] = acc.l[i];
  }
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < COLS_THREADS / 64; w++) {
      Fr o;
#pragma unroll
      for (int i = 0; i < Fr::N; i++) o.l[i] = wave_sum[w][i];
      acc = Fr::add(acc, o);
    }
    partial[item] = acc;
  }
}

// C2: one wave per heavy column adds its chunk sums
template <class Fr>
__global__ void __launch_bounds__(64)
cols_heavy_sum_kernel(const uint32_t* __restrict__ heavy_col, const uint32_t* __restrict__ heavy_base, uint32_t n_heavy,
                      uint32_t n_items, const Fr* __restrict__ partial, Fr* __restrict__ out) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  const uint32_t b0 = heavy_base[s], b1 = (s + 1 < n_heavy) ? heavy_base[s + 1] : n_items;
  Fr acc = Fr::zero();
  for (uint32_t i = b0 + lane; i < b1; i += 64) acc = Fr::add(acc, partial[i]);
  acc = setup_wave_sum(acc);
  if (lane == 0) out[heavy_col[s]] = acc;
}

static inline uint32_t cols_grid(uint64_t lanes) { return (uint32_t)((lanes + COLS_THREADS - 1) / COLS_THREADS); }

// the most heavy columns and the most chunks a call can meet
static inline uint64_t cols_heavy_cap(const ColumnsDims& d, uint32_t lane_max) { return d.nnz / ((uint64_t)lane_max + 1) + 1; }
static inline uint64_t cols_item_cap(const ColumnsDims& d, uint32_t lane_max) { return d.nnz / COLS_CHUNK + cols_heavy_cap(d, lane_max); }

// every buffer of columns_run at its size for this call: the one place that may allocate, before the first launch
template <class Fr>
static void columns_reserve(ColumnsScratch& cs, const ColumnsDims& d, uint32_t lane_max) {
  if (!d.nnz) return;
  cs.cnt.ensure((size_t)(d.cols + 1) * 4);
  cs.off.ensure((size_t)(d.cols + 1) * 4);
  cs.ent.ensure((size_t)d.nnz * sizeof(uint2));
  cs.ctr.ensure(8);
  cs.hcol.ensure((size_t)cols_heavy_cap(d, lane_max) * 4);
  cs.hbase.ensure((size_t)cols_heavy_cap(d, lane_max) * 4);
  cs.part.ensure((size_t)cols_item_cap(d, lane_max) * sizeof(Fr));
  cs.scan_aux.ensure((size_t)SCAN_MAX_SPANS * 4);
}

// d_out (t m Fr, Montgomery, matrix-major) = the transposed products with d_y (n Fr) on `st`; every element is written.  The
// scratch was reserved by columns_reserve with the same d and lane_max.  One host wait (the heavy counter); the last kernels
// are queued, not waited for.
template <class Curve>
static void columns_run(const Gr1csDev& g, const Gr1csPred& P, const ColumnsDims& d, const void* d_y, void* d_out,
                        ColumnsScratch& cs, uint32_t lane_max, hipStream_t st) {
  using Fr = typename Curve::Fr;
  const uint32_t cols = (uint32_t)d.cols, n = (uint32_t)d.n, m = (uint32_t)g.m, t = P.arity;
  if (!d.nnz) {                                          // no stored entry (n = 0 included): every column is empty
    ARK_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)cols * sizeof(Fr), st));
    return;
  }
  const Gr1csMat* mats = P.mats.as<Gr1csMat>();
  uint32_t* cnt = cs.cnt.as<uint32_t>();
  uint32_t* off = cs.off.as<uint32_t>();
  ARK_CHECK_HIP(hipMemsetAsync(cnt, 0, ((size_t)cols + 1) * 4, st));
  ARK_CHECK_HIP(hipMemsetAsync(cs.ctr.p, 0, 8, st));
  const dim3 egrid(cols_grid(d.max_nnz), t);
  ARK_LAUNCH(cols_count_kernel, egrid, dim3(COLS_THREADS), 0, st, mats, n, m, cnt);
  ARK_CHECK_LAUNCH();
  scan_exclusive(st, (const uint32_t*)cnt, off, cols, off + cols, cs.scan_aux);
  ARK_CHECK_HIP(hipMemcpyAsync(cnt, off, (size_t)cols * 4, hipMemcpyDeviceToDevice, st));      // the counters become the cursors
  ARK_LAUNCH(cols_scatter_kernel, egrid, dim3(COLS_THREADS), 0, st, mats, n, m, cnt, cs.ent.as<uint2>());
  ARK_CHECK_LAUNCH();
  ARK_LAUNCH((cols_gather_kernel<Fr>), dim3(cols_grid(cols)), dim3(COLS_THREADS), 0, st, (const uint32_t*)off,
             (const uint2*)cs.ent.as<uint2>(), (const Fr*)d_y, (const Fr*)g.pool.as<Fr>(), cols, lane_max, (Fr*)d_out,
             cs.ctr.as<unsigned long long>(), cs.hcol.as<uint32_t>(), cs.hbase.as<uint32_t>());
  ARK_CHECK_LAUNCH();
  unsigned long long ctr = 0;
  ARK_CHECK_HIP(hipMemcpyAsync(&ctr, cs.ctr.p, 8, hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  const uint32_t n_heavy = (uint32_t)(ctr >> 32), n_items = (uint32_t)ctr;
  if (!n_heavy) return;
  ARK_REQUIRE(n_heavy <= cols_heavy_cap(d, lane_max) && n_items <= cols_item_cap(d, lane_max), ARK355_EHIP,
              "columns: the heavy list left its bounds");
  ARK_LAUNCH((cols_heavy_kernel<Fr>), dim3(n_items), dim3(COLS_THREADS), 0, st, (const uint32_t*)off,
             (const uint2*)cs.ent.as<uint2>(), (const Fr*)d_y, (const Fr*)g.pool.as<Fr>(), (const uint32_t*)cs.hcol.as<uint32_t>(),
             (const uint32_t*)cs.hbase.as<uint32_t>(), n_heavy, cs.part.as<Fr>());
  ARK_CHECK_LAUNCH();
  ARK_LAUNCH((cols_heavy_sum_kernel<Fr>), dim3(n_heavy), dim3(64), 0, st, (const uint32_t*)cs.hcol.as<uint32_t>(),
             (const uint32_t*)cs.hbase.as<uint32_t>(), n_heavy, n_items, (const Fr*)cs.part.as<Fr>(), (Fr*)d_out);
  ARK_CHECK_LAUNCH();
}

// L_i(tau) for i < N = 2^log_n into d_L on `st` (queued); tau in Montgomery form.  tau inside H_N gives the indicator vector.
template <class Curve>
static void lagrange_run(uint32_t log_n, const typename Curve::Fr& tau, void* d_L, hipStream_t st) {
  using Fr = typename Curve::Fr;
  const uint64_t N = 1ull << log_n;
  const Fr omega = ntt_root<Fr>(log_n, false), omega_inv = ntt_root<Fr>(log_n, true);
  const Fr zt = Fr::sub(fr_pow2k(tau, log_n), Fr::one());
  const uint32_t grid = setup_grid((N + SETUP_RUN - 1) / SETUP_RUN);
  if (zt.is_zero()) {
    ARK_LAUNCH((setup_indicator_kernel<Fr>), dim3(grid), dim3(SETUP_THREADS), 0, st, (Fr*)d_L, N, tau, omega);
  } else {
    Fr nn = Fr::zero();
    nn.l[0] = (uint32_t)N;
    nn.l[1] = (uint32_t)(N >> 32);
    const Fr cN = Fr::mul(zt, Fr::inv(Fr::to_mont(nn)));
    ARK_LAUNCH((setup_lagrange_kernel<Fr>), dim3(grid), dim3(SETUP_THREADS), 0, st, (Fr*)d_L, N, tau, omega, omega_inv, cN);
  }
  ARK_CHECK_LAUNCH();
}

}  // namespace ark355
