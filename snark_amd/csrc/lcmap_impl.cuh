// finalize() on the device: ConstraintSystem::inline_all_lcs + to_matrices (relations/src/gr1cs/constraint_system.rs:691-804)
// and instance outlining (:826-863, instance_outliner.rs:41-81) from the memory images the reference keeps: LcMap's three
// flat arrays (lc_map.rs:51-56), Variable as a packed u64 (utils/variable.rs:4-14) and interned coefficients
// (field_interner.rs:24-69: entries 0 and 1 of the pool are 1 and -1).
//
// Inlining is (I - L)^-1 V for a strictly lower-triangular L (LC -> LC references) and V (LC -> variable leaves).  It runs in
// rounds: a round takes every LC whose references are all finished (round r = the LCs of depth r; forward references are
// refused first, so the lowest pending LC is always ready and the loop ends after at most n_lcs rounds).
//   lcs_check_*_kernel    every tag, index and coefficient index, before any kernel below dereferences one
//   lcs_ready_kernel      ready flag and expanded size (own leaves + lengths of the referenced, finished LCs) per LC
//   scan_exclusive x 2    segment of each ready LC in the round's buffer; rank in the round's list
//   lcs_expand_kernel     one lane per ready LC: (column, coefficient) of every leaf, pool[c] * entry for every entry of a
//                         referenced LC (the multiply is skipped when c is pool index 0, i.e. one)
//   lcs_compact_lds_kernel / lcs_compact_long_kernel
//                         per LC: sort by column, merge equal columns, drop zero sums -- BEFORE the next round reads it, which
//                         keeps d <- d + d at one entry instead of 2^depth.  Rows of at most LCS_ROW_LDS_MAX entries: one
//                         64-lane workgroup, a bitonic sort of (column << 32 | position) keys in 8 KiB of LDS; longer rows: one
//                         256-lane workgroup and the same network on keys in global memory, correct at any length.  The head
//                         of every run of equal columns adds the run's coefficients (no per-lane array, nothing in scratch).
//   scan_exclusive        of the keep flags: lcs_scatter_kernel appends the kept entries to the arena of finished LCs
//   lcs_finish_kernel     where each LC of the round starts in the arena, its length, its done flag
// Then, per matrix of every predicate: lcs_rowlen_kernel + scan_exclusive give the row pointers (the length of an argument is
// the length of its compacted LC), lcs_fill_kernel copies columns and coefficient indices, lcs_outline_kernel appends the
// closed-form rows of the outliner.  The coefficient pool of the result is
//     [ 1, -1, the polynomials' coefficients | one slot per arena entry ]
// and an arena entry equal to one carries index 0 instead of its slot, so gr1cs_row_dot skips the multiply.
// The result is an ordinary Gr1csDev.
#pragma once
#include "common.h"
#include "msm_impl.cuh"
#include "gr1cs_impl.cuh"

namespace ark355 {

constexpr uint32_t LCS_LDS_KEYS = 1024;                  // 8 KiB of keys per workgroup of the short path: 20 workgroups a CU
constexpr int LCS_TAG_SHIFT = 61;
constexpr uint64_t LCS_PAYLOAD = (1ull << LCS_TAG_SHIFT) - 1;

// slots of the validation word array: the first offending index per reason, ~0 when none
enum LcsErr : uint32_t {
  LCS_E_TAG = 0, LCS_E_INSTANCE, LCS_E_WITNESS, LCS_E_LC, LCS_E_FORWARD, LCS_E_COEFF,       // lc_vars / lc_coeffs
  LCS_E_ARG_TAG, LCS_E_ARG_INSTANCE, LCS_E_ARG_WITNESS, LCS_E_ARG_LC,                       // predicate arguments (flat index)
  LCS_E_COUNT
};

struct LcsDims {
  uint32_t ell, w, n_lcs, n_pool;
};

// per round, read back in one copy
struct LcsRound {
  unsigned long long expanded;   // sum of the sizes in 64 bits: the 32-bit scan is trusted only below 2^32
  uint32_t total;                // the same from the scan
  uint32_t n_ready;
  uint32_t n_long;               // ready LCs above LCS_ROW_LDS_MAX
  uint32_t top;                  // entries in the arena
};

ARK_D unsigned long long lcs_wave_sum(unsigned long long v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, (unsigned)d, 64);
  return v;                      // lane 0 of the wave
}

// first: slot of LCS_E_TAG or of LCS_E_ARG_TAG; self: the LC the entry belongs to (n_lcs for an argument: no forward check)
ARK_D void lcs_check_var(uint64_t v, const LcsDims d, uint64_t self, unsigned long long at, uint32_t first,
                         unsigned long long* err) {
  const uint64_t tag = v >> LCS_TAG_SHIFT, idx = v & LCS_PAYLOAD;
  if (tag > ARK355_VAR_LC) atomicMin(err + first, at);
  else if (tag == ARK355_VAR_INSTANCE && idx >= d.ell) atomicMin(err + first + 1, at);
  else if (tag == ARK355_VAR_WITNESS && idx >= d.w) atomicMin(err + first + 2, at);
  else if (tag == ARK355_VAR_LC) {
    if (idx >= d.n_lcs) atomicMin(err + first + 3, at);
    else if (idx >= self) atomicMin(err + LCS_E_FORWARD, at);
  }
}

// one lane per entry of the map; off: n_lcs + 1 validated offsets
static __global__ void __launch_bounds__(256)
lcs_check_entries_kernel(const uint32_t* __restrict__ off, const uint64_t* __restrict__ vars, const uint32_t* __restrict__ coeffs,
                         const LcsDims d, uint32_t n_entries, unsigned long long* err) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_entries) return;
  uint32_t lo = 0, hi = d.n_lcs;                       // off[lo] <= e, and hi == n_lcs or off[hi] > e
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= e) lo = mid;
    else hi = mid;
  }
  lcs_check_var(vars[e], d, lo, e, LCS_E_TAG, err);
  if (coeffs[e] >= d.n_pool) atomicMin(err + LCS_E_COEFF, (unsigned long long)e);
}

static __global__ void __launch_bounds__(256)
lcs_check_args_kernel(const uint64_t* __restrict__ args, uint64_t n_args, const LcsDims d, unsigned long long* err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_args) return;
  lcs_check_var(args[i], d, d.n_lcs, i, LCS_E_ARG_TAG, err);
}

// column of One, Instance(i), Witness(j).  remap (inside the LC map of an outlined system): One and Instance(0) become
// Witness(w), Instance(i) becomes Witness(w + i)
ARK_D uint32_t lcs_leaf_col(uint64_t v, uint32_t ell, uint32_t w, bool remap) {
  const uint32_t tag = (uint32_t)(v >> LCS_TAG_SHIFT), idx = (uint32_t)(v & LCS_PAYLOAD);
  if (tag == ARK355_VAR_WITNESS) return ell + idx;
  if (tag == ARK355_VAR_ONE) return remap ? ell + w : 0u;
  return remap ? ell + w + idx : idx;
}

// every lane of a wave stays to the end (lcs_wave_sum)
static __global__ void __launch_bounds__(256)
lcs_ready_kernel(const uint32_t* __restrict__ off, const uint64_t* __restrict__ vars, uint32_t n_lcs,
                 const uint32_t* __restrict__ done, const uint32_t* __restrict__ len, uint32_t lds_max,
                 uint32_t* __restrict__ ready, uint32_t* __restrict__ size, LcsRound* __restrict__ round) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long sz = 0, is_long = 0;
  if (k < n_lcs) {
    bool ok = !done[k];
    if (ok) {
      const uint32_t lo = off[k], hi = off[k + 1];
      for (uint32_t e = lo; e < hi; e++) {
        const uint64_t v = vars[e];
        const uint32_t tag = (uint32_t)(v >> LCS_TAG_SHIFT);
        if (tag == ARK355_VAR_ZERO) continue;
        if (tag != ARK355_VAR_LC) {
          sz++;
          continue;
        }
        const uint32_t j = (uint32_t)(v & LCS_PAYLOAD);
        if (!done[j]) {
          ok = false;
          break;
        }
        sz += len[j];
      }
    }
    if (!ok) sz = 0;
    ready[k] = ok ? 1u : 0u;
    size[k] = sz > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sz;
    is_long = sz > lds_max ? 1 : 0;
  }
  const unsigned long long wave_sz = lcs_wave_sum(sz), wave_long = lcs_wave_sum(is_long);
  if ((threadIdx.x & 63u) == 0) {
    if (wave_sz) atomicAdd(&round->expanded, wave_sz);
    if (wave_long) atomicAdd(&round->n_long, (uint32_t)wave_long);
  }
}

static __global__ void __launch_bounds__(256)
lcs_list_kernel(const uint32_t* __restrict__ ready, const uint32_t* __restrict__ rank, uint32_t n_lcs, uint32_t* __restrict__ list) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n_lcs && ready[k]) list[rank[k]] = (uint32_t)k;
}

struct LcsMap {                  // the uploaded map and the state of the rounds
  const uint32_t* off;
  const uint64_t* vars;
  const uint32_t* coeffs;
  const uint32_t* loc;           // start of a finished LC in the arena
  const uint32_t* len;
};

template <class Fr>
__global__ void __launch_bounds__(256)
lcs_expand_kernel(const LcsMap m, const uint32_t* __restrict__ list, uint32_t n_ready, const uint32_t* __restrict__ seg,
                  const Fr* __restrict__ in_pool, const uint32_t* __restrict__ a_col, const Fr* __restrict__ a_coef,
                  uint32_t ell, uint32_t w, int remap, uint32_t* __restrict__ x_col, Fr* __restrict__ x_coef) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_ready) return;
  const uint32_t k = list[r];
  uint32_t o = seg[k];
  const uint32_t lo = m.off[k], hi = m.off[k + 1];
  for (uint32_t e = lo; e < hi; e++) {
    const uint64_t v = m.vars[e];
    const uint32_t tag = (uint32_t)(v >> LCS_TAG_SHIFT), c = m.coeffs[e];
    if (tag == ARK355_VAR_ZERO) continue;
    if (tag != ARK355_VAR_LC) {
      x_col[o] = lcs_leaf_col(v, ell, w, remap != 0);
      x_coef[o++] = in_pool[c];
      continue;
    }
    const uint32_t j = (uint32_t)(v & LCS_PAYLOAD), src = m.loc[j], n = m.len[j];
    if (c == 0) {                // coefficient one: the referenced LC as it is
      for (uint32_t t = 0; t < n; t++) {
        x_col[o] = a_col[src + t];
        x_coef[o++] = a_coef[src + t];
      }
    } else {
      const Fr outer = in_pool[c];
      for (uint32_t t = 0; t < n; t++) {
        x_col[o] = a_col[src + t];
        x_coef[o++] = Fr::mul(outer, a_coef[src + t]);
      }
    }
  }
}

// bitonic network over P = 2^k keys (the padding keys are ~0 and sort last); every lane of the workgroup takes part
ARK_D void lcs_bitonic(unsigned long long* keys, uint32_t P, uint32_t tid, uint32_t lanes) {
  for (uint32_t k = 2; k <= P; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < P; i += lanes) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const unsigned long long a = keys[i], b = keys[p];
          if ((a > b) == ((i & k) == 0)) {
            keys[i] = b;
            keys[p] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

// keys sorted: slot j is the head of a run when its column differs from slot j - 1's; the head adds the run and keeps it
// unless the sum is zero.  Slots that are no heads are flagged out.
template <class Fr>
ARK_D void lcs_merge(const unsigned long long* keys, uint32_t n, uint32_t base, const Fr* __restrict__ x_coef,
                     uint32_t* __restrict__ y_col, Fr* __restrict__ y_coef, uint32_t* __restrict__ y_flag, uint32_t tid,
                     uint32_t lanes) {
  for (uint32_t j = tid; j < n; j += lanes) {
    const unsigned long long key = keys[j];
    const uint32_t col = (uint32_t)(key >> 32);
    uint32_t keep = 0;
    if (j == 0 || (uint32_t)(keys[j - 1] >> 32) != col) {
      Fr acc = x_coef[base + (uint32_t)key];
      for (uint32_t t = j + 1; t < n; t++) {
        const unsigned long long next = keys[t];
        if ((uint32_t)(next >> 32) != col) break;
        acc = Fr::add(acc, x_coef[base + (uint32_t)next]);
      }
      if (!acc.is_zero()) {
        keep = 1;
        y_col[base + j] = col;
        y_coef[base + j] = acc;
      }
    }
    y_flag[base + j] = keep;
  }
}

ARK_D void lcs_load_keys(unsigned long long* keys, uint32_t P, uint32_t n, const uint32_t* __restrict__ x_col, uint32_t tid,
                         uint32_t lanes) {
  for (uint32_t i = tid; i < P; i += lanes) keys[i] = i < n ? ((unsigned long long)x_col[i] << 32 | i) : ~0ull;
  __syncthreads();
}

// one 64-lane workgroup per ready LC; rows above lds_max (<= LCS_LDS_KEYS) are left to lcs_compact_long_kernel
template <class Fr>
__global__ void __launch_bounds__(64)
lcs_compact_lds_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ seg, const uint32_t* __restrict__ size,
                       uint32_t lds_max, const uint32_t* __restrict__ x_col, const Fr* __restrict__ x_coef,
                       uint32_t* __restrict__ y_col, Fr* __restrict__ y_coef, uint32_t* __restrict__ y_flag) {
  __shared__ unsigned long long keys[LCS_LDS_KEYS];
  const uint32_t k = list[blockIdx.x], n = size[k], base = seg[k];
  if (n > lds_max) return;                             // the whole workgroup
  uint32_t P = 1;
  while (P < n) P <<= 1;
  lcs_load_keys(keys, P, n, x_col + base, threadIdx.x, blockDim.x);
  lcs_bitonic(keys, P, threadIdx.x, blockDim.x);
  lcs_merge<Fr>(keys, n, base, x_coef, y_col, y_coef, y_flag, threadIdx.x, blockDim.x);
}

// the same on keys in global memory, for rows of any length: the LC's keys live at long_keys + 2 * seg (P < 2 n)
template <class Fr>
__global__ void __launch_bounds__(256)
lcs_compact_long_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ seg, const uint32_t* __restrict__ size,
                        uint32_t lds_max, const uint32_t* __restrict__ x_col, const Fr* __restrict__ x_coef,
                        unsigned long long* long_keys, uint32_t* __restrict__ y_col, Fr* __restrict__ y_coef,
                        uint32_t* __restrict__ y_flag) {
  const uint32_t k = list[blockIdx.x], n = size[k], base = seg[k];
  if (n <= lds_max) return;
  uint32_t P = 1;
  while (P < n) P <<= 1;
  unsigned long long* keys = long_keys + 2ull * base;
  lcs_load_keys(keys, P, n, x_col + base, threadIdx.x, blockDim.x);
  lcs_bitonic(keys, P, threadIdx.x, blockDim.x);
  lcs_merge<Fr>(keys, n, base, x_coef, y_col, y_coef, y_flag, threadIdx.x, blockDim.x);
}

// kept slots -> the arena; pool_base: index of the arena's first coefficient in the pool of the result
template <class Fr>
__global__ void __launch_bounds__(256)
lcs_scatter_kernel(const uint32_t* __restrict__ y_col, const Fr* __restrict__ y_coef, const uint32_t* __restrict__ y_flag,
                   const uint32_t* __restrict__ pos, uint32_t total, uint32_t top, uint32_t pool_base,
                   uint32_t* __restrict__ a_col, uint32_t* __restrict__ a_ci, Fr* __restrict__ a_coef) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total || !y_flag[e]) return;
  const uint32_t d = top + pos[e];
  const Fr c = y_coef[e];
  a_col[d] = y_col[e];
  a_coef[d] = c;
  a_ci[d] = c == Fr::one() ? 0u : pool_base + d;
}

// pos: total + 1 entries.  The lane behind the last LC adds what the round kept to the arena's size.
static __global__ void __launch_bounds__(256)
lcs_finish_kernel(const uint32_t* __restrict__ list, uint32_t n_ready, const uint32_t* __restrict__ seg,
                  const uint32_t* __restrict__ size, const uint32_t* __restrict__ pos, uint32_t total, uint32_t top,
                  uint32_t* __restrict__ loc, uint32_t* __restrict__ len, uint32_t* __restrict__ done,
                  LcsRound* __restrict__ round) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r == n_ready) round->top = top + pos[total];
  if (r >= n_ready) return;
  const uint32_t k = list[r], s = seg[k];
  loc[k] = top + pos[s];
  len[k] = pos[s + size[k]] - pos[s];
  done[k] = 1;
}

// every lane of a wave stays to the end (lcs_wave_sum)
static __global__ void __launch_bounds__(256)
lcs_rowlen_kernel(const uint64_t* __restrict__ args, uint64_t n, const uint32_t* __restrict__ len, uint32_t* __restrict__ rl,
                  unsigned long long* __restrict__ sum) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long l = 0;
  if (i < n) {
    const uint64_t v = args[i];
    const uint32_t tag = (uint32_t)(v >> LCS_TAG_SHIFT);
    l = tag == ARK355_VAR_ZERO ? 0u : (tag == ARK355_VAR_LC ? len[v & LCS_PAYLOAD] : 1u);
    rl[i] = (uint32_t)l;
  }
  const unsigned long long s = lcs_wave_sum(l);
  if ((threadIdx.x & 63u) == 0 && s) atomicAdd(sum, s);
}

// get_lc + make_row (constraint_system.rs:777-804) of one matrix: a bare variable is its own row with coefficient one and is
// never remapped (the outliner rewrites the LC map only)
static __global__ void __launch_bounds__(256)
lcs_fill_kernel(const uint64_t* __restrict__ args, uint64_t n, const uint32_t* __restrict__ rp, const uint32_t* __restrict__ loc,
                const uint32_t* __restrict__ len, const uint32_t* __restrict__ a_col, const uint32_t* __restrict__ a_ci,
                uint32_t ell, uint32_t w, uint32_t* __restrict__ col, uint32_t* __restrict__ ci) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t v = args[i];
  const uint32_t tag = (uint32_t)(v >> LCS_TAG_SHIFT);
  uint32_t o = rp[i];
  if (tag == ARK355_VAR_ZERO) return;
  if (tag != ARK355_VAR_LC) {
    col[o] = lcs_leaf_col(v, ell, w, false);
    ci[o] = 0;
    return;
  }
  const uint32_t k = (uint32_t)(v & LCS_PAYLOAD), src = loc[k], cnt = len[k];
  for (uint32_t t = 0; t < cnt; t++) {
    col[o] = a_col[src + t];
    ci[o++] = a_ci[src + t];
  }
}

struct LcsOutline {
  uint32_t* rp[3];
  uint32_t* col[3];
  uint32_t* ci[3];
  uint32_t nnz[3];               // before the appended rows
};

// the ell rows of outline_r1cs / outline_sr1cs (instance_outliner.rs:41-81) behind the n rows of the target predicate; ell and
// w are those of the system before outlining.  R1CS: row 0 is w_1 * w_1 = 1, row i is w_1 * w_i' = x_i.  SR1CS: (x_i - w_i')^2 = 0.
static __global__ void __launch_bounds__(256)
lcs_outline_kernel(const LcsOutline o, int mode, uint64_t n, uint32_t ell, uint32_t w, uint32_t minus_one) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ell) return;
  const uint32_t copy = ell + w + i;                   // Witness(w + i)
  if (mode == 1) {
    for (int k = 0; k < 3; k++) {
      const uint32_t at = o.nnz[k] + i;
      o.rp[k][n + i + 1] = at + 1;
      o.col[k][at] = k == 0 ? ell + w : (k == 1 ? copy : i);
      o.ci[k][at] = 0;
    }
  } else {
    const uint32_t at = o.nnz[0] + 2 * i;
    o.rp[0][n + i + 1] = at + 2;
    o.col[0][at] = i;
    o.ci[0][at] = 0;
    o.col[0][at + 1] = copy;
    o.ci[0][at + 1] = minus_one;
    o.rp[1][n + i + 1] = o.nnz[1];
  }
}

static inline uint32_t lcs_grid(uint64_t lanes) { return (uint32_t)((lanes + 255) / 256); }

static inline std::string lcs_who() { return "ark355_gr1cs_from_lcs: "; }

// what the host's numbers decide, before any device work
template <class Curve>
static void lcs_validate_host(const ark355_lc_system_desc& s, const ark355_predicate_lcs_desc* preds, uint32_t n_preds) {
  using Fr = typename Curve::Fr;
  const std::string who = lcs_who();
  ARK_REQUIRE(s.num_instance >= 1, ARK355_EINVAL, who + "num_instance must include the constant One");
  ARK_REQUIRE(s.num_instance < (1ull << 31) && s.num_witness < (1ull << 31) && s.num_instance + s.num_witness < (1ull << 31),
              ARK355_EINVAL, who + "too many variables");
  ARK_REQUIRE(s.outline >= 0 && s.outline <= 2, ARK355_EINVAL, who + "outline must be 0, 1 or 2");
  ARK_REQUIRE(s.n_lcs < (1ull << 31), ARK355_EINVAL, who + "n_lcs reaches 2^31");
  ARK_REQUIRE(s.lc_offsets, ARK355_EINVAL, who + "lc_offsets is NULL");
  ARK_REQUIRE(s.lc_offsets[0] == 0, ARK355_EINVAL, who + "lc_offsets[0] must be 0");
  for (uint64_t k = 0; k < s.n_lcs; k++) {
    ARK_REQUIRE(s.lc_offsets[k + 1] >= s.lc_offsets[k], ARK355_EINVAL,
                who + "lc_offsets[" + std::to_string(k + 1) + "] is below lc_offsets[" + std::to_string(k) + "]");
    ARK_REQUIRE(s.lc_offsets[k + 1] <= 0xFFFFFFFFull, ARK355_EINVAL,
                who + "lc_offsets[" + std::to_string(k + 1) + "]: the map holds 2^32 entries or more");
  }
  const uint64_t T = s.lc_offsets[s.n_lcs];
  ARK_REQUIRE(T == 0 || (s.lc_vars && s.lc_coeffs), ARK355_EINVAL, who + "lc_vars / lc_coeffs is NULL");
  ARK_REQUIRE(s.n_pool >= 2, ARK355_EINVAL, who + "n_pool below 2: pool[0] = 1 and pool[1] = -1 are part of the convention");
  ARK_REQUIRE(s.n_pool <= 0xFFFFFFFFull, ARK355_EINVAL, who + "n_pool reaches 2^32");
  ARK_REQUIRE(s.pool, ARK355_EINVAL, who + "pool is NULL");
  const Fr one = Fr::one(), minus_one = Fr::neg(Fr::one());
  ARK_REQUIRE(memcmp(s.pool, one.l, sizeof(Fr)) == 0, ARK355_EINVAL, who + "pool[0] is not 1");
  ARK_REQUIRE(memcmp(s.pool + sizeof(Fr), minus_one.l, sizeof(Fr)) == 0, ARK355_EINVAL, who + "pool[1] is not -1");
  ARK_REQUIRE(n_preds <= ARK355_GR1CS_MAX_PREDICATES, ARK355_EINVAL, who + "more predicates than ARK355_GR1CS_MAX_PREDICATES");
  ARK_REQUIRE(n_preds == 0 || preds, ARK355_EINVAL, who + "preds is NULL");
  for (uint32_t p = 0; p < n_preds; p++) {
    const ark355_predicate_lcs_desc& d = preds[p];
    ARK_REQUIRE(d.label, ARK355_EINVAL, who + "predicate " + std::to_string(p) + ": label is NULL");
    const std::string pw = who + "predicate \"" + std::string(d.label) + "\": ";
    gr1cs_validate_polynomial(pw, d.arity, d.n_constraints, d.n_terms, d.term_coeff, d.term_ptr, d.term_var, d.term_exp);
    ARK_REQUIRE(d.args, ARK355_EINVAL, pw + "args is NULL");
    for (uint32_t k = 0; k < d.arity; k++)
      ARK_REQUIRE(d.n_constraints == 0 || d.args[k], ARK355_EINVAL, pw + "args[" + std::to_string(k) + "] is NULL");
    for (uint32_t q = 0; q < p; q++)
      ARK_REQUIRE(strcmp(preds[q].label, d.label) != 0, ARK355_EINVAL, pw + "duplicate label");
  }
}

template <class Curve>
static Gr1csDev* lcs_finalize(const ark355_lc_system_desc& s, const ark355_predicate_lcs_desc* preds, uint32_t n_preds,
                              uint32_t lds_max, hipStream_t st) {
  using Fr = typename Curve::Fr;
  const std::string who = lcs_who();
  lcs_validate_host<Curve>(s, preds, n_preds);
  lds_max = lds_max < 1 ? 1 : (lds_max > LCS_LDS_KEYS ? LCS_LDS_KEYS : lds_max);
  const uint64_t ell = s.num_instance, w = s.num_witness, n_lcs = s.n_lcs, T = s.lc_offsets[n_lcs];
  // ---- the outliner's gate: the label must be there (constraint_system.rs:698-704), and of the arity its rows have ----------
  int outline = 0;
  uint32_t target = 0;
  if (s.outline) {
    const char* label = s.outline == 1 ? "R1CS" : "SR1CS";
    for (uint32_t p = 0; p < n_preds; p++) {
      if (strcmp(preds[p].label, label) != 0) continue;
      ARK_REQUIRE(preds[p].arity == (s.outline == 1 ? 3u : 2u), ARK355_EINVAL,
                  who + "predicate \"" + label + "\": arity " + std::to_string(preds[p].arity) + " cannot take the outlined rows");
      outline = s.outline;
      target = p;
    }
  }
  const uint64_t ell_out = ell, w_out = outline ? w + ell : w;
  ARK_REQUIRE(ell_out + w_out < (1ull << 31), ARK355_EINVAL, who + "too many variables after outlining");
  if (outline)
    ARK_REQUIRE(preds[target].n_constraints + ell <= ARK355_GR1CS_MAX_ROWS, ARK355_EINVAL,
                who + "more rows than ARK355_GR1CS_MAX_ROWS after outlining");
  // ---- upload -------------------------------------------------------------------------------------------------------------
  std::vector<uint64_t> arg_base(n_preds + 1, 0);        // flat index of a predicate's first argument
  for (uint32_t p = 0; p < n_preds; p++) arg_base[p + 1] = arg_base[p] + (uint64_t)preds[p].arity * preds[p].n_constraints;
  const uint64_t n_args = arg_base[n_preds];
  std::vector<uint32_t> off32(n_lcs + 1);
  for (uint64_t k = 0; k <= n_lcs; k++) off32[k] = (uint32_t)s.lc_offsets[k];
  DevBuf d_off((n_lcs + 1) * 4), d_vars(T * 8), d_coeffs(T * 4), d_in_pool(s.n_pool * sizeof(Fr)), d_args(n_args * 8);
  DevBuf d_err(LCS_E_COUNT * 8);
  ARK_CHECK_HIP(hipMemcpyAsync(d_off.p, off32.data(), (n_lcs + 1) * 4, hipMemcpyHostToDevice, st));
  if (T) {
    ARK_CHECK_HIP(hipMemcpyAsync(d_vars.p, s.lc_vars, T * 8, hipMemcpyHostToDevice, st));
    ARK_CHECK_HIP(hipMemcpyAsync(d_coeffs.p, s.lc_coeffs, T * 4, hipMemcpyHostToDevice, st));
  }
  ARK_CHECK_HIP(hipMemcpyAsync(d_in_pool.p, s.pool, s.n_pool * sizeof(Fr), hipMemcpyHostToDevice, st));
  for (uint32_t p = 0; p < n_preds; p++) {
    const uint64_t n = preds[p].n_constraints;
    for (uint32_t k = 0; k < preds[p].arity && n; k++)
      ARK_CHECK_HIP(hipMemcpyAsync(d_args.as<uint64_t>() + arg_base[p] + k * n, preds[p].args[k], n * 8, hipMemcpyHostToDevice, st));
  }
  // ---- validation on the device, before any index is followed ----------------------------------------------------------------
  const LcsDims dims{(uint32_t)ell, (uint32_t)w, (uint32_t)n_lcs, (uint32_t)s.n_pool};
  ARK_CHECK_HIP(hipMemsetAsync(d_err.p, 0xFF, LCS_E_COUNT * 8, st));
  if (T) {
    ARK_LAUNCH(lcs_check_entries_kernel, dim3(lcs_grid(T)), dim3(256), 0, st, (const uint32_t*)d_off.as<uint32_t>(),
               (const uint64_t*)d_vars.as<uint64_t>(), (const uint32_t*)d_coeffs.as<uint32_t>(), dims, (uint32_t)T,
               d_err.as<unsigned long long>());
    ARK_CHECK_LAUNCH();
  }
  if (n_args) {
    ARK_LAUNCH(lcs_check_args_kernel, dim3(lcs_grid(n_args)), dim3(256), 0, st, (const uint64_t*)d_args.as<uint64_t>(), n_args, dims,
               d_err.as<unsigned long long>());
    ARK_CHECK_LAUNCH();
  }
  unsigned long long err[LCS_E_COUNT];
  ARK_CHECK_HIP(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  static const char* const entry_msg[6] = {"a tag above 4", "an instance index >= num_instance", "a witness index >= num_witness",
                                           "an LC index >= n_lcs", "an LC that is not below the LC that uses it",
                                           "a coefficient index >= n_pool"};
  for (uint32_t r = 0; r < 6; r++) {
    if (err[r] == ~0ull) continue;
    const char* arr = r == LCS_E_COEFF ? "lc_coeffs[" : "lc_vars[";
    throw HipError{ARK355_EINVAL, who + arr + std::to_string(err[r]) + "]: " + entry_msg[r]};
  }
  for (uint32_t r = LCS_E_ARG_TAG; r < LCS_E_COUNT; r++) {
    if (err[r] == ~0ull) continue;
    uint32_t p = 0;
    while (arg_base[p + 1] <= err[r]) p++;
    const uint64_t rel = err[r] - arg_base[p], n = preds[p].n_constraints;
    throw HipError{ARK355_EINVAL, who + "predicate \"" + preds[p].label + "\": args[" + std::to_string(rel / n) + "][" +
                                      std::to_string(rel % n) + "]: " + entry_msg[r - LCS_E_ARG_TAG]};
  }
  // ---- the head of the result's pool: 1, -1, the polynomials' coefficients; the arena's coefficients follow -----------------
  FrInterner<Fr> head;
  const Fr minus_one_fr = Fr::neg(Fr::one());
  const uint32_t minus_one = head.intern(reinterpret_cast<const uint8_t*>(minus_one_fr.l));
  std::vector<std::vector<uint32_t>> progs(n_preds);
  for (uint32_t p = 0; p < n_preds; p++)
    progs[p] = gr1cs_program<Fr>(head, preds[p].n_terms, preds[p].term_coeff, preds[p].term_ptr, preds[p].term_var, preds[p].term_exp);
  const uint64_t pool_base = head.elems.size();
  // ---- rounds ---------------------------------------------------------------------------------------------------------------
  DevBuf d_done(n_lcs * 4), d_len(n_lcs * 4), d_loc(n_lcs * 4), d_ready(n_lcs * 4), d_size((n_lcs + 1) * 4), d_seg((n_lcs + 1) * 4);
  DevBuf d_rank((n_lcs + 1) * 4), d_list(n_lcs * 4), d_round(sizeof(LcsRound)), aux;
  DevBuf x_col, x_coef, y_col, y_coef, y_flag, pos, long_keys;
  uint64_t cap = T > 1024 ? T : 1024;
  DevBuf a_col(cap * 4), a_ci(cap * 4), pool_buf((pool_base + cap) * sizeof(Fr));
  ARK_CHECK_HIP(hipMemsetAsync(d_done.p, 0, d_done.bytes, st));
  ARK_CHECK_HIP(hipMemsetAsync(d_round.p, 0, sizeof(LcsRound), st));
  const LcsMap map{d_off.as<uint32_t>(), d_vars.as<uint64_t>(), d_coeffs.as<uint32_t>(), d_loc.as<uint32_t>(), d_len.as<uint32_t>()};
  LcsRound* d_r = d_round.as<LcsRound>();
  uint64_t pending = n_lcs, top = 0;
  while (pending) {
    ARK_CHECK_HIP(hipMemsetAsync(d_round.p, 0, offsetof(LcsRound, top), st));              // everything but the arena's size
    ARK_LAUNCH(lcs_ready_kernel, dim3(lcs_grid(n_lcs)), dim3(256), 0, st, map.off, map.vars, (uint32_t)n_lcs,
               (const uint32_t*)d_done.as<uint32_t>(), map.len, lds_max, d_ready.as<uint32_t>(), d_size.as<uint32_t>(), d_r);
    ARK_CHECK_LAUNCH();
    scan_exclusive(st, d_size.as<const uint32_t>(), d_seg.as<uint32_t>(), (uint32_t)n_lcs, &d_r->total, aux);
    scan_exclusive(st, d_ready.as<const uint32_t>(), d_rank.as<uint32_t>(), (uint32_t)n_lcs, &d_r->n_ready, aux);
    LcsRound h;
    ARK_CHECK_HIP(hipMemcpyAsync(&h, d_round.p, sizeof(h), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    ARK_REQUIRE(h.n_ready >= 1 && h.n_ready <= pending, ARK355_EINVAL, who + "no LC is ready: the map is not ordered");
    top = h.top;
    const uint64_t total = h.expanded, n_ready = h.n_ready;
    ARK_REQUIRE(total <= 0xFFFFFFFEull && pool_base + top + total <= 0xFFFFFFFFull, ARK355_ENOMEM,
                who + "the inlined map does not fit 32-bit indices (" + std::to_string(top + total) + " entries)");
    if (top + total > cap) {                                                                // grow the arena, keep what is there
      const uint64_t grown = std::max(2 * cap, top + total);
      DevBuf n_col(grown * 4), n_ci(grown * 4), n_pool((pool_base + grown) * sizeof(Fr));
      if (top) {
        ARK_CHECK_HIP(hipMemcpyAsync(n_col.p, a_col.p, top * 4, hipMemcpyDeviceToDevice, st));
        ARK_CHECK_HIP(hipMemcpyAsync(n_ci.p, a_ci.p, top * 4, hipMemcpyDeviceToDevice, st));
        ARK_CHECK_HIP(hipMemcpyAsync(n_pool.as<Fr>() + pool_base, pool_buf.as<Fr>() + pool_base, top * sizeof(Fr), hipMemcpyDeviceToDevice, st));
        ARK_CHECK_HIP(hipStreamSynchronize(st));
      }
      a_col = std::move(n_col);
      a_ci = std::move(n_ci);
      pool_buf = std::move(n_pool);
      cap = grown;
    }
    Fr* a_coef = pool_buf.as<Fr>() + pool_base;
    x_col.ensure(total * 4);
    y_col.ensure(total * 4);
    y_flag.ensure(total * 4);
    x_coef.ensure(total * sizeof(Fr));
    y_coef.ensure(total * sizeof(Fr));
    pos.ensure((total + 1) * 4);
    ARK_LAUNCH(lcs_list_kernel, dim3(lcs_grid(n_lcs)), dim3(256), 0, st, (const uint32_t*)d_ready.as<uint32_t>(),
               (const uint32_t*)d_rank.as<uint32_t>(), (uint32_t)n_lcs, d_list.as<uint32_t>());
    ARK_CHECK_LAUNCH();
    const uint32_t* list = d_list.as<uint32_t>();
    const uint32_t* seg = d_seg.as<uint32_t>();
    const uint32_t* size = d_size.as<uint32_t>();
    if (total) {
      ARK_LAUNCH((lcs_expand_kernel<Fr>), dim3(lcs_grid(n_ready)), dim3(256), 0, st, map, list, (uint32_t)n_ready, seg,
                 (const Fr*)d_in_pool.as<Fr>(), (const uint32_t*)a_col.as<uint32_t>(), (const Fr*)a_coef, (uint32_t)ell, (uint32_t)w,
                 outline ? 1 : 0, x_col.as<uint32_t>(), x_coef.as<Fr>());
      ARK_CHECK_LAUNCH();
      ARK_LAUNCH((lcs_compact_lds_kernel<Fr>), dim3((uint32_t)n_ready), dim3(64), 0, st, list, seg, size, lds_max,
                 (const uint32_t*)x_col.as<uint32_t>(), (const Fr*)x_coef.as<Fr>(), y_col.as<uint32_t>(), y_coef.as<Fr>(),
                 y_flag.as<uint32_t>());
      ARK_CHECK_LAUNCH();
      if (h.n_long) {
        long_keys.ensure(2 * total * 8);
        ARK_LAUNCH((lcs_compact_long_kernel<Fr>), dim3((uint32_t)n_ready), dim3(256), 0, st, list, seg, size, lds_max,
                   (const uint32_t*)x_col.as<uint32_t>(), (const Fr*)x_coef.as<Fr>(), long_keys.as<unsigned long long>(),
                   y_col.as<uint32_t>(), y_coef.as<Fr>(), y_flag.as<uint32_t>());
        ARK_CHECK_LAUNCH();
      }
    }
    scan_exclusive(st, y_flag.as<const uint32_t>(), pos.as<uint32_t>(), (uint32_t)total, pos.as<uint32_t>() + total, aux);
    if (total) {
      ARK_LAUNCH((lcs_scatter_kernel<Fr>), dim3(lcs_grid(total)), dim3(256), 0, st, (const uint32_t*)y_col.as<uint32_t>(),
                 (const Fr*)y_coef.as<Fr>(), (const uint32_t*)y_flag.as<uint32_t>(), (const uint32_t*)pos.as<uint32_t>(),
                 (uint32_t)total, (uint32_t)top, (uint32_t)pool_base, a_col.as<uint32_t>(), a_ci.as<uint32_t>(), a_coef);
      ARK_CHECK_LAUNCH();
    }
    ARK_LAUNCH(lcs_finish_kernel, dim3(lcs_grid(n_ready + 1)), dim3(256), 0, st, list, (uint32_t)n_ready, seg, size,
               (const uint32_t*)pos.as<uint32_t>(), (uint32_t)total, (uint32_t)top, d_loc.as<uint32_t>(), d_len.as<uint32_t>(),
               d_done.as<uint32_t>(), d_r);
    ARK_CHECK_LAUNCH();
    pending -= n_ready;
  }
  // ---- row pointers of every matrix ------------------------------------------------------------------------------------------
  std::unique_ptr<Gr1csDev> g(new Gr1csDev());
  g->curve = Curve::ID;
  g->ell = ell_out;
  g->w = w_out;
  g->m = ell_out + w_out;
  g->preds.resize(n_preds);
  std::vector<const char*> labels(n_preds);
  for (uint32_t p = 0; p < n_preds; p++) labels[p] = preds[p].label;
  const std::vector<uint32_t> order = gr1cs_label_order(labels);
  for (uint32_t r = 0; r < n_preds; r++) g->preds[order[r]].rank = r;
  uint64_t n_mats = 0, max_rows = 0;
  for (uint32_t p = 0; p < n_preds; p++) {
    n_mats += preds[p].arity;
    max_rows = std::max<uint64_t>(max_rows, preds[p].n_constraints);
  }
  DevBuf d_sums((n_mats + 1) * 8), d_rl(max_rows * 4);
  ARK_CHECK_HIP(hipMemsetAsync(d_sums.p, 0, d_sums.bytes, st));
  uint64_t mi = 0;
  for (uint32_t p = 0; p < n_preds; p++) {
    const ark355_predicate_lcs_desc& d = preds[p];
    Gr1csPred& P = g->preds[p];
    const uint64_t n = d.n_constraints, extra = (outline && p == target) ? ell : 0;
    P.label = d.label;
    P.arity = d.arity;
    P.n = n + extra;
    g->total += P.n;
    ark355_predicate_desc poly{};
    poly.arity = d.arity;
    poly.n_terms = d.n_terms;
    poly.term_coeff = d.term_coeff;
    poly.term_ptr = d.term_ptr;
    poly.term_var = d.term_var;
    poly.term_exp = d.term_exp;
    P.r1cs_shape = gr1cs_is_r1cs_polynomial<Fr>(poly);
    P.degree = gr1cs_program_degree(progs[p]);
    P.prog.alloc(progs[p].size() * 4);
    ARK_CHECK_HIP(hipMemcpyAsync(P.prog.p, progs[p].data(), progs[p].size() * 4, hipMemcpyHostToDevice, st));
    P.nnz.assign(d.arity, 0);
    P.row_ptr.resize(d.arity);
    P.col.resize(d.arity);
    P.cidx.resize(d.arity);
    for (uint32_t k = 0; k < d.arity; k++, mi++) {
      P.row_ptr[k].alloc((P.n + 1) * 4);
      if (n) {
        ARK_LAUNCH(lcs_rowlen_kernel, dim3(lcs_grid(n)), dim3(256), 0, st,
                   (const uint64_t*)d_args.as<uint64_t>() + arg_base[p] + k * n, n, map.len, d_rl.as<uint32_t>(),
                   d_sums.as<unsigned long long>() + mi);
        ARK_CHECK_LAUNCH();
      }
      scan_exclusive(st, d_rl.as<const uint32_t>(), P.row_ptr[k].as<uint32_t>(), (uint32_t)n, P.row_ptr[k].as<uint32_t>() + n, aux);
    }
  }
  std::vector<unsigned long long> sums(n_mats + 1);
  ARK_CHECK_HIP(hipMemcpyAsync(sums.data(), d_sums.p, (n_mats + 1) * 8, hipMemcpyDeviceToHost, st));
  uint32_t top32 = 0;
  ARK_CHECK_HIP(hipMemcpyAsync(&top32, &d_r->top, 4, hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  top = top32;
  // ---- columns and coefficient indices ----------------------------------------------------------------------------------------
  mi = 0;
  for (uint32_t p = 0; p < n_preds; p++) {
    const ark355_predicate_lcs_desc& d = preds[p];
    Gr1csPred& P = g->preds[p];
    const uint64_t n = d.n_constraints;
    const bool outlined = outline && p == target;
    std::vector<Gr1csMat> mats(d.arity);
    LcsOutline o{};
    for (uint32_t k = 0; k < d.arity; k++, mi++) {
      const uint64_t extra = !outlined ? 0 : (outline == 1 ? ell : (k == 0 ? 2 * ell : 0));
      ARK_REQUIRE(sums[mi] + extra <= ARK355_GR1CS_MAX_ROWS, ARK355_EINVAL,
                  who + "predicate \"" + P.label + "\": matrix " + std::to_string(k) + " would hold more entries than ARK355_GR1CS_MAX_ROWS");
      P.nnz[k] = sums[mi] + extra;
      P.col[k].alloc(P.nnz[k] * 4);
      P.cidx[k].alloc(P.nnz[k] * 4);
      if (n) {
        ARK_LAUNCH(lcs_fill_kernel, dim3(lcs_grid(n)), dim3(256), 0, st, (const uint64_t*)d_args.as<uint64_t>() + arg_base[p] + k * n,
                   n, (const uint32_t*)P.row_ptr[k].as<uint32_t>(), map.loc, map.len, (const uint32_t*)a_col.as<uint32_t>(),
                   (const uint32_t*)a_ci.as<uint32_t>(), (uint32_t)ell, (uint32_t)w, P.col[k].as<uint32_t>(), P.cidx[k].as<uint32_t>());
        ARK_CHECK_LAUNCH();
      }
      if (outlined) {
        o.rp[k] = P.row_ptr[k].as<uint32_t>();
        o.col[k] = P.col[k].as<uint32_t>();
        o.ci[k] = P.cidx[k].as<uint32_t>();
        o.nnz[k] = (uint32_t)sums[mi];
      }
      mats[k] = Gr1csMat{P.row_ptr[k].as<uint32_t>(), P.col[k].as<uint32_t>(), P.cidx[k].as<uint32_t>()};
    }
    if (outlined) {
      ARK_LAUNCH(lcs_outline_kernel, dim3(lcs_grid(ell)), dim3(256), 0, st, o, outline, n, (uint32_t)ell, (uint32_t)w, minus_one);
      ARK_CHECK_LAUNCH();
    }
    P.mats.alloc(d.arity * sizeof(Gr1csMat));
    ARK_CHECK_HIP(hipMemcpyAsync(P.mats.p, mats.data(), d.arity * sizeof(Gr1csMat), hipMemcpyHostToDevice, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));                                                // mats leaves this frame
  }
  // ---- the pool: its head in front of the arena's coefficients ----------------------------------------------------------------
  ARK_CHECK_HIP(hipMemcpyAsync(pool_buf.p, head.elems.data(), pool_base * sizeof(Fr), hipMemcpyHostToDevice, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  g->pool_count = pool_base + top;
  g->pool = std::move(pool_buf);
  return g.release();
}

}  // namespace ark355
