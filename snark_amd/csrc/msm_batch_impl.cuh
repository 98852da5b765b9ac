// Batched short MSMs (ark355_msm_batch_dev): many independent inner products sum_i k_i B_i of at most
// MSM_BATCH_SMALL_MAX terms each, over resident window tables, in ONE fixed launch sequence -- a digit kernel, a sum kernel (two
// when the handles of a call mix both row formats), one copy back, one host wait -- whatever the number of segments.
//
// Device replacement for `count` calls of ark-ec `VariableBaseMSM::msm_bigint` (un-vendored crate,
// ark-ec/src/scalar_mul/variable_base/mod.rs) on short vectors: the levels of a multilinear opening (mle_open_impl.cuh), the
// commitments to many small tables.
//
// Why not msm_generic: its pipeline (digits, two-level sort, segment accumulation, merge, row / column sums, bit sums) is built for
// 2^16 .. 2^23 terms and costs 0.35 - 4.4 ms a call whatever the call holds.  A short MSM needs no buckets at all.  With the signed
// digits d_{i,w} of msm_for_each_digit (the very function the sort calls) and b = |d| - 1 the bucket index,
//       sum_i k_i B_i  =  sum_set 2^(c set) sum_b (b + 1) Bucket_{set,b},
//       sum_b (b + 1) Bucket_b  =  sum_k 2^k S_k  +  (S_{c-2} + S'),       S_k = sum of the entries whose index has bit k set,
// S' the sum of the entries with the top bit clear -- the identity of tails28_impl.cuh, applied to the TABLE ROWS an entry names
// instead of to bucket slots.  Every S is a plain sum: a per-lane chain of mixed additions (madd28 / madd28_g2, the accumulation
// kernels' own arithmetic) over the rows +-T[q][i], a wave butterfly, and -- in workgroups of more than one wave -- one more
// butterfly over the waves' sums through LDS.  No sort, no atomics, no doubling, no scratch memory in any loop; an entry takes part
// in (c - 1) / 2 + 1/2 sums on average, i.e. windows x c / 2 ~ 128 mixed additions a scalar at every window size.  The kernel writes
// what stage B of msm_selsum28_kernel writes -- c canonical XYZZ sums per bucket set -- so msm_parts_finish finishes a segment
// unchanged on the host, and one batched inversion normalises all segments of a call.
//
// Scratch (MsmBatchScratch, grow-only, owned by the context, reserved before the first launch; it aliases neither GenericScratch
// nor MleScratch -- the quotients of an opening in MleScratch::q are what these kernels read):
//     segs     one MsmBatchSeg per short segment
//     digits   one word per (scalar, window) of every short segment
//     parts    msm_parts_count(plan) XYZZ sums per short segment
#pragma once
#include <utility>
#include "msm_impl.cuh"

namespace ark355 {

constexpr uint32_t MSM_BATCH_MAX = 4096;                 // ARK355_MSM_BATCH_MAX
constexpr int32_t MSM_BATCH_SMALL_MAX_DEFAULT = 512;     // the measured crossover: DESIGN.md section 31
constexpr int32_t MSM_BATCH_SMALL_MAX_LIMIT = 1 << 14;
constexpr uint32_t MSM_BATCH_THREADS_MAX = 512;          // two waves a SIMD: the register budget of the tail kernels (ARK_TAIL28_WAVES)

// policy MSM_BATCH_SMALL_MAX -> the longest segment of the short route: negative selects the default, 0 switches the route off,
// anything above 2^14 is 2^14
static inline uint64_t msm_batch_small_max(int32_t policy) {
  if (policy < 0) return (uint64_t)MSM_BATCH_SMALL_MAX_DEFAULT;
  return (uint64_t)(policy > MSM_BATCH_SMALL_MAX_LIMIT ? MSM_BATCH_SMALL_MAX_LIMIT : policy);
}

// A digit word: bit 31 = the row enters negated (digit sign ^ the scalar's negate_high flip), bit 30 = the digit is not zero,
// bits 0 .. 29 = the bucket index |d| - 1 (c <= 24).  Window w of scalar i of a segment sits at digits[dig_off + w n + i].
constexpr uint32_t MSM_BATCH_DIGIT_VALID = 1u << 30, MSM_BATCH_DIGIT_NEG = 1u << 31;

struct MsmBatchSeg {
  const void* rows;        // the handle's window table: table block q = 2^(c wstride q) B_i at row q * row_stride + i
  const void* scalars;     // n Fr in device memory
  uint64_t dig_off;        // into the digit words
  uint32_t out_off;        // into the XYZZ sums: [set][c]
  uint32_t n, c, windows, wstride;
  uint32_t row_stride;     // rows per table block (the handle's point count)
  uint32_t packed;         // row format of the table
  int32_t digit_flags;     // msm_digit_flags of the handle's plan
};

// One lane per scalar (grid.y = segment): the digits of msm_for_each_digit, zero digits included
template <class Fr>
__global__ void __launch_bounds__(MSM_THREADS)
msm_batch_digits_kernel(const MsmBatchSeg* __restrict__ segs, int mont, uint32_t* __restrict__ digits) {
  const MsmBatchSeg S = segs[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.n) return;
  uint32_t* dg = digits + S.dig_off + i;
  const uint32_t n = S.n, idx_mask = (1u << (S.c - 1)) - 1u;
  for (uint32_t w = 0; w < S.windows; w++) dg[(uint64_t)w * n] = 0u;
  const Fr k = static_cast<const Fr*>(S.scalars)[i];
  msm_for_each_digit<Fr>(k, mont, i, n, S.c, S.windows, S.digit_flags, S.row_stride, [&](uint32_t w, uint32_t key, uint32_t val) {
    dg[(uint64_t)w * n] = MSM_BATCH_DIGIT_VALID | (val & MSM_BATCH_DIGIT_NEG) | (key & idx_mask);
  });
}

// this lane's (half) row: x, y as 28-bit limbs; returns the OR of the row's words (0: the base at infinity)
template <class P, bool PACKED>
ARK_D uint32_t msm_batch_row(const Row28<P, PACKED>* __restrict__ row, Fp28<P>& px, Fp28<P>& py) {
  using F = Fp28<P>;
  using Row = Row28<P, PACKED>;
  constexpr int Q = Row::Q;
  uint32_t d[4 * Q];
  const uint4* src = reinterpret_cast<const uint4*>(row);
#pragma unroll
  for (int k = 0; k < Q; k++) {
    const uint4 t = src[k];
    d[4 * k + 0] = t.x;
    d[4 * k + 1] = t.y;
    d[4 * k + 2] = t.z;
    d[4 * k + 3] = t.w;
  }
  uint32_t any = 0;
  if constexpr (PACKED) {
#pragma unroll
    for (int k = 0; k < Row::WORDS; k++) any |= d[k];
    px = Row::unpack(d);
    py = Row::unpack(d + Row::NB);
  } else {
#pragma unroll
    for (int k = 0; k < F::N; k++) {
      px.l[k] = d[k];
      py.l[k] = d[F::N + k];
      any |= d[k] | d[F::N + k];
    }
  }
  return any;
}

// The cold paths of the group law -- two operands equal or opposite -- as this kernel reaches them.  The out-of-line helpers of
// msm28_impl.cuh take two Fp28 by value, and the second of them travels through the stack: 3 scratch stores in the caller at each of
// the ten call sites of one mixed and one general addition.  Here the 2 N limbs are 2 N scalar arguments, which all travel in
// registers (at most 29 with `which`), and the helper behind them calls the same arithmetic: the kernel itself makes no scratch
// access at all (libark355.stats.json).  OP: 0 classify (the class in word 0), 1 dbl28_coord_ni, 2 dbl28_g2_coord_ni.
template <class P, int OP, class... U>
ARK_HD_NOINLINE typename Fp28<P>::Vec msm_batch_cold_regs(int which, U... w) {
  using F = Fp28<P>;
  static_assert(sizeof...(U) == 2 * F::N, "x limbs, then y limbs");
  const uint32_t v[] = {w...};
  F a, b;
#pragma unroll
  for (int i = 0; i < F::N; i++) {
    a.l[i] = v[i];
    b.l[i] = v[F::N + i];
  }
  if constexpr (OP == 0) {
    typename F::Vec r = F::zero().to_vec();
    r[0] = (uint32_t)madd28_classify<P>(a, b);
    return r;
  } else if constexpr (OP == 1) {
    return dbl28_coord_ni<P>(a, b, which);
  } else {
    return dbl28_g2_coord_ni<P>(a, b, which);
  }
}
template <class P>
struct MsmBatchCold {
  using F = Fp28<P>;
  template <int OP, size_t... I>
  ARK_D static typename F::Vec call(const F& a, const F& b, int which, std::index_sequence<I...>) {
    return msm_batch_cold_regs<P, OP>(which, a.l[I]..., b.l[I]...);
  }
  ARK_D static int classify(const F& pd, const F& r) { return (int)call<0>(pd, r, 0, std::make_index_sequence<F::N>{})[0]; }
  ARK_D static typename F::Vec dbl(const F& x, const F& y, int which) { return call<1>(x, y, which, std::make_index_sequence<F::N>{}); }
  ARK_D static typename F::Vec dbl_g2(const F& x, const F& y, int which) { return call<2>(x, y, which, std::make_index_sequence<F::N>{}); }
};

// Register budget of the sum kernel.  The mixed addition, the general addition and the walk over the digit words live in one
// kernel: at two waves a SIMD (256 registers, the budget of the tail kernels) that fits G1 of both curves and G2 of BN254 without
// a spill, but G2 over the 14-limb field of BLS12-381 spilled ~130 registers into the loops (104 scratch loads and stores in the
// hot blocks of the listing).  That one instantiation runs one wave a SIMD -- 512 registers, workgroups of at most 256 lanes.
template <class P, bool G2>
struct MsmBatchShape {
  static constexpr bool WIDE = G2 && Fp28<P>::N > 10;
  static constexpr int WAVES = WIDE ? 1 : ARK_TAIL28_WAVES;
  static constexpr uint32_t THREADS_MAX = WIDE ? MSM_BATCH_THREADS_MAX / 2 : MSM_BATCH_THREADS_MAX;
};

// Grid (max c, max bucket sets, segments), one workgroup of 64 .. 512 lanes per output (segment, set, o): o < c - 1 is the sum of
// the rows whose bucket index has bit o set, o = c - 1 the sum of those with the top bit (c - 2) clear.  A lane (lane pair in G2)
// strides over the set's entries t = q n + i -- window wstride q + set of scalar i -- skips forward to its next entry with the bit,
// and adds that row; so all lanes of a wave add together, and the additions executed are the additions needed plus the imbalance of
// the last round.  Workgroups of the other row format than PACKED leave at once.
template <class P, bool G2, bool PACKED>
__global__ void __launch_bounds__((MsmBatchShape<P, G2>::THREADS_MAX), (MsmBatchShape<P, G2>::WAVES))
msm_batch_sum_kernel(const MsmBatchSeg* __restrict__ segs, const uint32_t* __restrict__ digits, void* __restrict__ out) {
  using Cold = MsmBatchCold<P>;
  using T = Tail28<P, G2, Cold>;
  using F = Fp28<P>;
  using Slot = typename T::Slot;
  using Out = typename T::Out;
  using Row = typename std::conditional<G2, Affine28G2<P, PACKED>, Row28<P, PACKED>>::type;
  __shared__ Slot wave_out[MSM_BATCH_THREADS_MAX / 64];
  const MsmBatchSeg S = segs[blockIdx.z];
  const uint32_t o = blockIdx.x, set = blockIdx.y;
  if ((S.packed != 0) != PACKED || o >= S.c || set >= S.wstride) return;
  const uint32_t n = S.n;
  const uint32_t blocks = (S.windows - set + S.wstride - 1) / S.wstride;      // the table blocks this set reads
  const uint32_t count = blocks * n;
  const uint32_t k = o < S.c - 1 ? o : S.c - 2, want = o < S.c - 1 ? 1u : 0u;
  const uint32_t* dg = digits + S.dig_off;
  const Row* rows = static_cast<const Row*>(S.rows);
  const uint32_t item = threadIdx.x / T::LPI, items = blockDim.x / T::LPI;
  Acc28<P> sum;
  bool empty = true;
  sum.x = sum.y = sum.zz = sum.zzz = F::zero();
  uint32_t t = item;
#pragma unroll 1
  for (;;) {
    uint32_t word = 0, q = 0, i = 0;
#pragma unroll 1
    for (; t < count; t += items) {
      q = t / n;
      i = t - q * n;
      word = dg[(uint64_t)(q * S.wstride + set) * n + i];
      if ((word & MSM_BATCH_DIGIT_VALID) && ((word >> k) & 1u) == want) break;
    }
    if (t >= count) break;
    t += items;
    const Row* row = rows + ((size_t)q * S.row_stride + i);
    F px, py;
    if constexpr (G2) {
      const uint32_t any = msm_batch_row<P, PACKED>(&row->half[threadIdx.x & 1u], px, py);
      if ((any | ark_pair_xchg(any)) == 0) continue;       // base at infinity (pair-wide)
      madd28_g2<P, Cold>(sum, empty, px, py, (word >> 31) != 0);
    } else {
      if (msm_batch_row<P, PACKED>(row, px, py) == 0) continue;
      madd28<P, Cold>(sum, empty, px, py, (word >> 31) != 0);
    }
  }
  // the lanes of a wave, then -- through LDS -- the waves of the workgroup: the same butterfly twice
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll 1
  for (int stage = 0;; stage++) {
    T::wave_sum(sum, empty);
    if (waves == 1 || stage == 1) break;
    if (lane < (uint32_t)T::LPI) T::store(&wave_out[wave], sum, empty);
    __syncthreads();
    if (wave != 0) return;
    if (item < waves) {
      T::load(&wave_out[item], sum, empty);
    } else {
      empty = true;
      sum.x = sum.y = sum.zz = sum.zzz = F::zero();
    }
  }
  if (threadIdx.x < (uint32_t)T::LPI) T::store_canonical(static_cast<Out*>(out) + S.out_off + (size_t)set * S.c + o, sum, empty);
}

struct MsmBatchScratch {
  DevBuf segs, digits, parts;
};

// lanes of a sum workgroup: enough for ~4 candidate entries a lane (lane pair), 64 .. cap (MsmBatchShape::THREADS_MAX)
static inline uint32_t msm_batch_threads(uint64_t max_entries, bool g2, uint32_t cap) {
  const uint64_t want = (max_entries + 3) / 4 * (g2 ? 2 : 1);
  uint32_t t = 64;
  while (t < cap && t < want) t <<= 1;
  return t;
}

// The short route of one call: `count` segments described by segs (host), their digits and sums in bs; the sums come back in
// h_parts (XYZZ<F>[parts_total]) after ONE wait.  Every reservation precedes the first launch.
template <class F, class Fr>
static void msm_batch_short_run(MsmBatchScratch& bs, const std::vector<MsmBatchSeg>& segs, uint64_t digits_total, uint32_t parts_total,
                                int mont, std::vector<XYZZ<F>>& h_parts, hipStream_t st) {
  using P = typename Tail28Of<F>::P;
  constexpr bool G2 = Tail28Of<F>::G2;
  const uint32_t count = (uint32_t)segs.size();
  if (!count) return;
  uint32_t max_n = 0, max_c = 0, max_sets = 0;
  uint64_t max_entries = 0;
  bool any_packed = false, any_plain = false;
  for (const MsmBatchSeg& s : segs) {
    max_n = std::max(max_n, s.n);
    max_c = std::max(max_c, s.c);
    max_sets = std::max(max_sets, s.wstride);
    max_entries = std::max(max_entries, (uint64_t)s.n * ((s.windows + s.wstride - 1) / s.wstride));
    (s.packed ? any_packed : any_plain) = true;
  }
  bs.segs.ensure((size_t)count * sizeof(MsmBatchSeg));
  bs.digits.ensure((size_t)digits_total * 4);
  bs.parts.ensure((size_t)parts_total * sizeof(XYZZ<F>));
  h_parts.resize(parts_total);
  ARK_CHECK_HIP(hipMemcpyAsync(bs.segs.p, segs.data(), (size_t)count * sizeof(MsmBatchSeg), hipMemcpyHostToDevice, st));
  const MsmBatchSeg* d_segs = bs.segs.as<MsmBatchSeg>();
  ARK_LAUNCH((msm_batch_digits_kernel<Fr>), dim3((max_n + MSM_THREADS - 1) / MSM_THREADS, count), dim3(MSM_THREADS), 0, st, d_segs, mont,
             bs.digits.as<uint32_t>());
  ARK_CHECK_LAUNCH();
  const dim3 grid(max_c, max_sets, count), block(msm_batch_threads(max_entries, G2, MsmBatchShape<P, G2>::THREADS_MAX));
  if (any_plain) {
    ARK_LAUNCH((msm_batch_sum_kernel<P, G2, false>), grid, block, 0, st, d_segs, (const uint32_t*)bs.digits.as<uint32_t>(), bs.parts.p);
    ARK_CHECK_LAUNCH();
  }
  if (any_packed) {
    ARK_LAUNCH((msm_batch_sum_kernel<P, G2, true>), grid, block, 0, st, d_segs, (const uint32_t*)bs.digits.as<uint32_t>(), bs.parts.p);
    ARK_CHECK_LAUNCH();
  }
  ARK_CHECK_HIP(hipMemcpyAsync(h_parts.data(), bs.parts.p, (size_t)parts_total * sizeof(XYZZ<F>), hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
}

// canonical affine images of `count` XYZZ points with ONE field inversion (Montgomery's trick over the zzz of the finite ones)
template <class F>
static void xyzz_batch_to_affine_host(const XYZZ<F>* in, size_t count, Affine<F>* out) {
  std::vector<F> pre(count);
  F run = F::one();
  for (size_t i = 0; i < count; i++) {
    pre[i] = run;
    if (!in[i].is_inf()) run = F::mul_ni(run, in[i].zzz);
  }
  F inv = F::inv(run);
  for (size_t i = count; i-- > 0;) {
    if (in[i].is_inf()) {
      out[i] = Affine<F>::inf();
      continue;
    }
    const F i3 = F::mul_ni(inv, pre[i]);      // 1/Z^3
    inv = F::mul_ni(inv, in[i].zzz);
    const F iz = F::mul_ni(in[i].zz, i3);     // 1/Z
    const F i2 = F::sqr_ni(iz);               // 1/Z^2
    out[i] = Affine<F>{F::mul_ni(in[i].x, i2), F::mul_ni(in[i].y, i3)};
  }
}

}  // namespace ark355
