// Column gather: out[k m + j] = sum over the STORED entries (i, j, c) of M_k of c * v[i] for t resident CSR matrices of n rows
// and m columns (a Gr1csMat table, a shared coefficient pool, pool index 0 = the coefficient one: no multiplication) -- the
// transposed products M_k^T v without a transposed copy.  One engine for the three places that need them; what a term is comes
// from a policy struct T:
//     FrTerms<Fr>    (here)             v in Fr: the generator's u, v, w (setup_impl.cuh), mat_vec_t / columns_at (columns_impl.cuh)
//     G1Terms<Curve> (hbasis_impl.cuh)  v affine G1 points, sums in XYZZ: D' = C^T U'
// T names Fr, Value (a sum), Src (an element of v), GATHER_THREADS, and has zero() -- whose image is all zero bytes --,
// add(a, b), term(acc, entry, v, pool) and wave_sum(x), the sum over a wave in lane 0.
//
//   1  column-major order of the t matrices side by side (t m columns):
//        colgather_count_kernel    cnt[k m + col]++ for every stored entry, all matrices in ONE launch (grid.y = t)
//        scan_exclusive            (msm_impl.cuh) the offsets and, behind them, the total
//        colgather_scatter_kernel  entry e of M_k -> (row, pool index) at the next free place of its column (grid.y = t); the
//                                  row is found by bisection of row_ptr, so no lane walks a row.  The places inside a column
//                                  come from atomics, so their order differs from run to run: addition is exact in Fr and the
//                                  group sums are normalised before they leave the device, the results do not.
//   2  gather:
//        colgather_gather_kernel   one lane per column of at most lane_max entries.  A longer column (the constant One, hot
//                                  variables) enters the heavy list with ONE 64-bit atomic (heavy columns in the high word,
//                                  chunks in the low word: the chunk bases come out sorted by slot).
//        colgather_heavy_kernel    one workgroup per chunk of COLGATHER_CHUNK entries of a heavy column: eight entries per lane,
//                                  the wave sums, the four of them through LDS
//        colgather_heavy_sum_kernel one wave per heavy column adds its chunk sums
//      The one host wait reads the heavy counter (8 bytes) to size the last two grids, and checks it against the scratch.
//
// Scratch of one call (ColGatherScratch, bytes; nnz = the stored entries of the t matrices together, H = nnz / (lane_max + 1) + 1
// the most heavy columns there can be, I = nnz / COLGATHER_CHUNK + H the most chunks):
//     8 (t m + 1)  counters / cursors and offsets      8 nnz   (row, pool index) pairs     8 H + 8   heavy list and its counter
//     sizeof(Value) I   chunk sums
#pragma once
#include "common.h"
#include "fr_wave.cuh"
#include "msm_impl.cuh"
#include "witness_impl.cuh"

namespace ark355 {

constexpr uint32_t COLGATHER_THREADS = 256;                       // every kernel but a policy's gather and the heavy sum
constexpr uint32_t COLGATHER_CHUNK = COLGATHER_THREADS * 8;       // entries of a heavy column per workgroup: eight per lane
constexpr uint32_t COLGATHER_LANE_MAX = 64;                       // the longest column one lane sums, where no policy says otherwise

// the matrices of one call; no HIP call reads nnz and max_nnz, they size the scratch and the grids
struct ColGatherIn {
  const Gr1csMat* mats = nullptr;    // device, t of them
  uint32_t t = 0, n = 0, m = 0;
  uint64_t nnz = 0, max_nnz = 0;     // stored entries of all matrices, and of the largest one
  uint32_t cols() const { return (uint32_t)((uint64_t)t * m); }     // the caller has refused t m + 1 >= 2^32
};

struct ColGatherScratch {
  DevBuf cnt, off, ent, ctr, hcol, hbase, part, scan_aux;
};

template <class Fr_>
struct FrTerms {
  using Fr = Fr_;
  using Value = Fr_;
  using Src = Fr_;
  static constexpr uint32_t GATHER_THREADS = COLGATHER_THREADS;
  static ARK_D Value zero() { return Fr::zero(); }
  static ARK_D Value add(const Value& a, const Value& b) { return Fr::add(a, b); }
  static ARK_D void term(Value& acc, const uint2 e, const Src* __restrict__ v, const Fr* __restrict__ pool) {
    Fr x = v[e.x];
    if (e.y != 0) x = Fr::mul(x, pool[e.y]);
    acc = Fr::add(acc, x);
  }
  static ARK_D Value wave_sum(const Value& x) { return fr_wave_sum(x); }
};

// 1: one lane per stored entry of matrix blockIdx.y; the matrix's entry count is rp[n]
static __global__ void __launch_bounds__(COLGATHER_THREADS)
colgather_count_kernel(const Gr1csMat* __restrict__ mats, uint32_t n, uint32_t m, uint32_t* __restrict__ cnt) {
  const Gr1csMat M = mats[blockIdx.y];
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= M.rp[n]) return;
  atomicAdd(&cnt[blockIdx.y * m + M.col[e]], 1u);
}

// 1: entry e of matrix blockIdx.y -> (row, pool index) at the next free place of its column.  The row is the last i with
// rp[i] <= e (rows may be empty).
static __global__ void __launch_bounds__(COLGATHER_THREADS)
colgather_scatter_kernel(const Gr1csMat* __restrict__ mats, uint32_t n, uint32_t m, uint32_t* __restrict__ cursor,
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

// 2: column j of the t m side-by-side columns.  Heavy columns only enter the list.
template <class T>
__global__ void __launch_bounds__(T::GATHER_THREADS)
colgather_gather_kernel(const uint32_t* __restrict__ off, const uint2* __restrict__ ent, const typename T::Src* __restrict__ v,
                        const typename T::Fr* __restrict__ pool, uint32_t cols, uint32_t lane_max, typename T::Value* __restrict__ out,
                        unsigned long long* __restrict__ heavy_ctr, uint32_t* __restrict__ heavy_col, uint32_t* __restrict__ heavy_base) {
  const uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j64 >= cols) return;
  const uint32_t j = (uint32_t)j64;
  const uint32_t lo = off[j], hi = off[j + 1], len = hi - lo;
  if (len > lane_max) {
    const uint32_t chunks = (len + COLGATHER_CHUNK - 1) / COLGATHER_CHUNK;
    const unsigned long long old = atomicAdd(heavy_ctr, (1ull << 32) | (unsigned long long)chunks);
    const uint32_t slot = (uint32_t)(old >> 32);
    heavy_col[slot] = j;
    heavy_base[slot] = (uint32_t)old;
    return;
  }
  typename T::Value acc = T::zero();
  for (uint32_t t = lo; t < hi; t++) T::term(acc, ent[t], v, pool);
  out[j] = acc;
}

// 2: one workgroup per chunk of a heavy column.  item -> slot: the last slot with heavy_base[slot] <= item.
template <class T>
__global__ void __launch_bounds__(COLGATHER_THREADS)
colgather_heavy_kernel(const uint32_t* __restrict__ off, const uint2* __restrict__ ent, const typename T::Src* __restrict__ v,
                       const typename T::Fr* __restrict__ pool, const uint32_t* __restrict__ heavy_col,
                       const uint32_t* __restrict__ heavy_base, uint32_t n_heavy, typename T::Value* __restrict__ partial) {
  using Value = typename T::Value;
  __shared__ uint32_t wave_val[COLGATHER_THREADS / 64][sizeof(Value) / 4];
  const uint32_t item = blockIdx.x, tid = threadIdx.x;
  uint32_t s = 0, e = n_heavy;
  while (e - s > 1) {
    const uint32_t mid = s + ((e - s) >> 1);
    if (heavy_base[mid] <= item) s = mid;
    else e = mid;
  }
  const uint32_t j = heavy_col[s], c = item - heavy_base[s];
  const uint32_t lo = off[j] + c * COLGATHER_CHUNK;
  const uint32_t end = off[j + 1], hi = (end - lo > COLGATHER_CHUNK) ? lo + COLGATHER_CHUNK : end;
  Value acc = T::zero();
  for (uint32_t t = lo + tid; t < hi; t += COLGATHER_THREADS) T::term(acc, ent[t], v, pool);
  acc = T::wave_sum(acc);
  if ((tid & 63u) == 0) memcpy(wave_val[tid >> 6], &acc, sizeof(acc));
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < COLGATHER_THREADS / 64; w++) {
      Value o;
      memcpy(&o, wave_val[w], sizeof(o));
      acc = T::add(acc, o);
    }
    partial[item] = acc;
  }
}

// 2: one wave per heavy column adds its chunk sums
template <class T>
__global__ void __launch_bounds__(64)
colgather_heavy_sum_kernel(const uint32_t* __restrict__ heavy_col, const uint32_t* __restrict__ heavy_base, uint32_t n_heavy,
                           uint32_t n_items, const typename T::Value* __restrict__ partial, typename T::Value* __restrict__ out) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  const uint32_t b0 = heavy_base[s], b1 = (s + 1 < n_heavy) ? heavy_base[s + 1] : n_items;
  typename T::Value acc = T::zero();
  for (uint32_t i = b0 + lane; i < b1; i += 64) acc = T::add(acc, partial[i]);
  acc = T::wave_sum(acc);
  if (lane == 0) out[heavy_col[s]] = acc;
}

// the most heavy columns and the most chunks a call can meet
static inline uint64_t colgather_heavy_cap(uint64_t nnz, uint32_t lane_max) { return nnz / ((uint64_t)lane_max + 1) + 1; }
static inline uint64_t colgather_item_cap(uint64_t nnz, uint32_t lane_max) { return nnz / COLGATHER_CHUNK + colgather_heavy_cap(nnz, lane_max); }

// every buffer of colgather_run at its size for a call over t m = cols columns and nnz stored entries: the one place that may
// allocate, before the first launch
static inline void colgather_reserve(ColGatherScratch& cs, uint64_t cols, uint64_t nnz, uint32_t lane_max, size_t value_bytes) {
  if (!nnz) return;
  cs.cnt.ensure((size_t)(cols + 1) * 4);
  cs.off.ensure((size_t)(cols + 1) * 4);
  cs.ent.ensure((size_t)nnz * sizeof(uint2));
  cs.ctr.ensure(8);
  cs.hcol.ensure((size_t)colgather_heavy_cap(nnz, lane_max) * 4);
  cs.hbase.ensure((size_t)colgather_heavy_cap(nnz, lane_max) * 4);
  cs.part.ensure((size_t)colgather_item_cap(nnz, lane_max) * value_bytes);
  cs.scan_aux.ensure((size_t)SCAN_MAX_SPANS * 4);
}

// d_out (t m Values, matrix-major) = the transposed products with d_v (n Src) on `st`; every element is written.  The scratch
// was reserved by colgather_reserve with the same sizes and lane_max.  One host wait (the heavy counter); the last kernels are
// queued, not waited for.
template <class T>
static void colgather_run(const ColGatherIn& in, const typename T::Src* d_v, const typename T::Fr* d_pool, typename T::Value* d_out,
                          ColGatherScratch& cs, uint32_t lane_max, hipStream_t st) {
  using Value = typename T::Value;
  const uint32_t cols = in.cols();
  if (!in.nnz) {                                         // no stored entry (n = 0 included): every column is empty
    ARK_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)cols * sizeof(Value), st));
    return;
  }
  uint32_t* cnt = cs.cnt.as<uint32_t>();
  uint32_t* off = cs.off.as<uint32_t>();
  const uint2* ent = cs.ent.as<uint2>();
  const uint32_t* hcol = cs.hcol.as<uint32_t>();
  const uint32_t* hbase = cs.hbase.as<uint32_t>();
  ARK_CHECK_HIP(hipMemsetAsync(cnt, 0, ((size_t)cols + 1) * 4, st));
  ARK_CHECK_HIP(hipMemsetAsync(cs.ctr.p, 0, 8, st));
  const dim3 egrid((uint32_t)((in.max_nnz + COLGATHER_THREADS - 1) / COLGATHER_THREADS), in.t);
  ARK_LAUNCH(colgather_count_kernel, egrid, dim3(COLGATHER_THREADS), 0, st, in.mats, in.n, in.m, cnt);
  ARK_CHECK_LAUNCH();
  scan_exclusive(st, (const uint32_t*)cnt, off, cols, off + cols, cs.scan_aux);
  ARK_CHECK_HIP(hipMemcpyAsync(cnt, off, (size_t)cols * 4, hipMemcpyDeviceToDevice, st));      // the counters become the cursors
  ARK_LAUNCH(colgather_scatter_kernel, egrid, dim3(COLGATHER_THREADS), 0, st, in.mats, in.n, in.m, cnt, cs.ent.as<uint2>());
  ARK_CHECK_LAUNCH();
  const uint32_t ggrid = (uint32_t)(((uint64_t)cols + T::GATHER_THREADS - 1) / T::GATHER_THREADS);
  ARK_LAUNCH((colgather_gather_kernel<T>), dim3(ggrid), dim3(T::GATHER_THREADS), 0, st, (const uint32_t*)off, ent, d_v, d_pool, cols,
             lane_max, d_out, cs.ctr.as<unsigned long long>(), cs.hcol.as<uint32_t>(), cs.hbase.as<uint32_t>());
  ARK_CHECK_LAUNCH();
  unsigned long long ctr = 0;
  ARK_CHECK_HIP(hipMemcpyAsync(&ctr, cs.ctr.p, 8, hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  const uint32_t n_heavy = (uint32_t)(ctr >> 32), n_items = (uint32_t)ctr;
  if (!n_heavy) return;
  ARK_REQUIRE(n_heavy <= colgather_heavy_cap(in.nnz, lane_max) && n_items <= colgather_item_cap(in.nnz, lane_max), ARK355_EHIP,
              "columns: the heavy list left its bounds");
  ARK_LAUNCH((colgather_heavy_kernel<T>), dim3(n_items), dim3(COLGATHER_THREADS), 0, st, (const uint32_t*)off, ent, d_v, d_pool, hcol,
             hbase, n_heavy, cs.part.as<Value>());
  ARK_CHECK_LAUNCH();
  ARK_LAUNCH((colgather_heavy_sum_kernel<T>), dim3(n_heavy), dim3(64), 0, st, hcol, hbase, n_heavy, n_items,
             (const Value*)cs.part.as<Value>(), d_out);
  ARK_CHECK_LAUNCH();
}

}  // namespace ark355
