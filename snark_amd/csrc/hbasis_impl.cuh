// The h query in the evaluation basis of the coset: what a proving key is turned into, once, when it
// meets its R1CS, so that a proof runs four transforms instead of six.
//
// With H_k = h_query[k] (k <= N - 2, H_{N-1} = O), g the coset generator, w the N-th root of unity and
// c0 = 1 / (N (g^N - 1)):
//     E'_j = sum_k (c0 g^-k w^-jk) H_k        the h query in the Lagrange basis of g H:   sum_k rho_k H_k / (g^N - 1) = sum_j (a'_j b'_j) E'_j
//     U'_j = sum_k (c0      w^-jk) H_k        the same without the coset shift:            sum_k c_k H_k / (g^N - 1)   = sum_j (C z)_j U'_j
//     D'_i = sum_j C[j][i] U'_j               ... gathered by column:                                                 = sum_i z_i D'_i
// Both are radix-2 transforms over G1 POINTS with root w^-1.  Everything here is cold code (run once per key): plain group
// arithmetic from curve.cuh, one lane per butterfly / point / column, no tuning beyond filling the chip.
//
//   T1  hb_load_kernel        Q_k = c0 H_k, written at the bit-reversed index (affine in, XYZZ out; index N - 1 is infinity)
//   T2  hb_shift_kernel       Q_k <- g^-k Q_k (for E' only)
//   T3  hb_stage_kernel       one decimation-in-time stage in place: (a, b) <- (a + t b, a - t b), t the stage twiddle; one launch per
//                             stage, log2 N of them; natural order out
//   T4  batch_to_affine_kernel (msm_impl.cuh)
//   G1-G3  column gather of C (colgather_impl.cuh over G1Terms): column-major order, one lane per column of at most
//       COLGATHER_LANE_MAX entries, a workgroup per chunk of a longer column and a wave per such column; unit coefficients are
//       plain (mixed) additions
//   G4  hb_fold_kernel        slot i of the folded L' vector: l_ext[i] - D'_i (instance slots hold infinity: -D'_i)
#pragma once
#include "common.h"
#include "msm_impl.cuh"
#include "witness_impl.cuh"
#include "colgather_impl.cuh"
#include "setup_impl.cuh"

namespace ark355 {

constexpr uint32_t HB_THREADS = 128;

// k * P over a little-endian canonical scalar, fixed 4-bit windows: every lane of a wave does the same sequence of doublings and
// (almost always) an addition per window, whatever its scalar
template <class F>
ARK_D XYZZ<F> hb_mul(const XYZZ<F>& p, const uint32_t* k, int nlimbs) {
  if (p.is_inf()) return p;
  XYZZ<F> tab[16];
  tab[0] = XYZZ<F>::inf();
  tab[1] = p;
  for (int i = 2; i < 16; i++) tab[i] = (i & 1) ? xyzz_add(tab[i - 1], p) : xyzz_dbl(tab[i >> 1]);
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int i = nlimbs * 8 - 1; i >= 0; i--) {
    for (int d = 0; d < 4; d++) acc = xyzz_dbl(acc);
    const uint32_t dg = (k[i >> 3] >> ((uint32_t)(i & 7) * 4u)) & 15u;
    if (dg) acc = xyzz_add(acc, tab[dg]);
  }
  return acc;
}
template <class F, class Fr>
ARK_D XYZZ<F> hb_mul_fr(const XYZZ<F>& p, const Fr& mont) {
  const Fr c = Fr::from_mont(mont);
  return hb_mul(p, c.l, Fr::N);
}

// T1
template <class F, class Fr>
__global__ void __launch_bounds__(HB_THREADS)
hb_load_kernel(const Affine<F>* __restrict__ h, uint32_t cnt, uint32_t n, uint32_t log_n, Fr c0, XYZZ<F>* __restrict__ out) {
  const uint64_t k64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k64 >= n) return;
  const uint32_t k = (uint32_t)k64;
  XYZZ<F> q = XYZZ<F>::inf();
  if (k < cnt) q = hb_mul_fr(XYZZ<F>::from_affine(h[k]), c0);
  out[bitrev_bits(k, log_n)] = q;
}

// T2: x[bitrev(k)] *= base^k
template <class F, class Fr>
__global__ void __launch_bounds__(HB_THREADS)
hb_shift_kernel(XYZZ<F>* __restrict__ x, uint32_t n, uint32_t log_n, Fr base) {
  const uint64_t k64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k64 >= n || k64 == 0) return;
  const uint32_t k = (uint32_t)k64;
  const uint32_t at = bitrev_bits(k, log_n);
  x[at] = hb_mul_fr(x[at], fr_pow(base, (uint64_t)k));
}

// T3: stage s (half = 2^s) of the in-place decimation-in-time transform; w_stage is the primitive 2^(s+1)-th root
template <class F, class Fr>
__global__ void __launch_bounds__(HB_THREADS)
hb_stage_kernel(XYZZ<F>* __restrict__ x, uint32_t pairs, uint32_t s, Fr w_stage) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t64 >= pairs) return;
  const uint32_t t = (uint32_t)t64;
  const uint32_t half = 1u << s, j = t & (half - 1u);
  const uint32_t i0 = ((t >> s) << (s + 1u)) + j, i1 = i0 + half;
  const XYZZ<F> a = x[i0];
  XYZZ<F> b = x[i1];
  if (j != 0) b = hb_mul_fr(b, fr_pow(w_stage, (uint64_t)j));
  x[i0] = xyzz_add(a, b);
  x[i1] = xyzz_add(a, XYZZ<F>::neg(b));
}

static inline uint32_t hb_grid(uint64_t lanes) { return (uint32_t)((lanes + HB_THREADS - 1) / HB_THREADS); }

// d_h: the N - 1 affine points of h_query (device).  d_E / d_U (either may be null): N affine points each, natural order.
template <class Curve>
static void hbasis_transforms(const void* d_h, uint32_t log_n, hipStream_t st, void* d_E, void* d_U) {
  using Fr = typename Curve::Fr;
  using Fq = typename Curve::Fq;
  using P = typename Fr::Params;
  ARK_REQUIRE(log_n >= 1 && log_n <= 23 && log_n <= (uint32_t)P::TWO_ADICITY, ARK355_EINVAL, "group transform: 2^1 .. 2^23 points");
  const uint32_t N = 1u << log_n;
  const Fr g = fr_from_params<Fr>(&P::gen);
  Fr nn = Fr::zero();
  nn.l[0] = N;
  const Fr c0 = Fr::inv(Fr::mul(Fr::to_mont(nn), Fr::sub(fr_pow2k(g, log_n), Fr::one())));
  const Fr g_inv = Fr::inv(g), w_inv = ntt_root<Fr>(log_n, true);
  DevBuf q((size_t)N * sizeof(XYZZ<Fq>)), work;
  ARK_LAUNCH((hb_load_kernel<Fq, Fr>), dim3(hb_grid(N)), dim3(HB_THREADS), 0, st, (const Affine<Fq>*)d_h, N - 1, N, log_n, c0,
             q.as<XYZZ<Fq>>());
  ARK_CHECK_LAUNCH();
  auto transform = [&](XYZZ<Fq>* x, void* d_out) {
    for (uint32_t s = 0; s < log_n; s++) {
      ARK_LAUNCH((hb_stage_kernel<Fq, Fr>), dim3(hb_grid(N / 2)), dim3(HB_THREADS), 0, st, x, N / 2, s, fr_pow2k(w_inv, log_n - s - 1));
      ARK_CHECK_LAUNCH();
    }
    ARK_LAUNCH((batch_to_affine_kernel<Fq>), dim3(((N + PRE_K - 1) / PRE_K + MSM_THREADS - 1) / MSM_THREADS), dim3(MSM_THREADS), 0, st,
               (const XYZZ<Fq>*)x, (Affine<Fq>*)d_out, N);
    ARK_CHECK_LAUNCH();
  };
  if (d_U) {
    XYZZ<Fq>* x = q.as<XYZZ<Fq>>();
    if (d_E) {           // (the scaled points are needed once more)
      work.alloc((size_t)N * sizeof(XYZZ<Fq>));
      ARK_CHECK_HIP(hipMemcpyAsync(work.p, q.p, (size_t)N * sizeof(XYZZ<Fq>), hipMemcpyDeviceToDevice, st));
      x = work.as<XYZZ<Fq>>();
    }
    transform(x, d_U);
  }
  if (d_E) {
    ARK_LAUNCH((hb_shift_kernel<Fq, Fr>), dim3(hb_grid(N)), dim3(HB_THREADS), 0, st, q.as<XYZZ<Fq>>(), N, log_n, g_inv);
    ARK_CHECK_LAUNCH();
    transform(q.as<XYZZ<Fq>>(), d_E);
  }
  ARK_CHECK_HIP(hipStreamSynchronize(st));            // the scratch is freed on return
}

// ---- column gather ----------------------------------------------------------------------------------------------------------
// the terms of colgather_impl.cuh over G1: coefficient * U_row added to an XYZZ sum (cidx 0 = the coefficient one: a mixed addition)
template <class Curve>
struct G1Terms {
  using Fr = typename Curve::Fr;
  using F = typename Curve::Fq;
  using Value = XYZZ<F>;
  using Src = Affine<F>;
  static constexpr uint32_t GATHER_THREADS = HB_THREADS;
  static ARK_D Value zero() { return Value::inf(); }
  static ARK_D Value add(const Value& a, const Value& b) { return xyzz_add(a, b); }
  static ARK_D void term(Value& acc, const uint2 e, const Src* __restrict__ U, const Fr* __restrict__ pool) {
    const Src u = U[e.x];
    if (e.y == 0) xyzz_madd_ni(acc, u);
    else acc = xyzz_add(acc, hb_mul_fr(Value::from_affine(u), pool[e.y]));
  }
  static ARK_D Value wave_sum(const Value& x) { return wave_reduce_sum(x); }
};

// G4: out[i] = l[i] - D[i] for i < cols, l[i] beyond (the four tail slots of l_ext)
template <class F>
__global__ void __launch_bounds__(HB_THREADS)
hb_fold_kernel(const Affine<F>* __restrict__ l, const XYZZ<F>* __restrict__ D, uint32_t cols, uint32_t total, XYZZ<F>* __restrict__ out) {
  const uint64_t i64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i64 >= total) return;
  const uint32_t i = (uint32_t)i64;
  XYZZ<F> v = XYZZ<F>::from_affine(l[i]);
  if (i < cols) v = xyzz_add(v, XYZZ<F>::neg(D[i]));
  out[i] = v;
}

// D_i = sum_j C[j][i] U_j for the m columns of the resident C (XYZZ, device).  d_U: N affine points.  One host wait reads the
// heavy-column counter (8 bytes); all scratch of the gather is gone on return.
template <class Curve>
static void hbasis_gather(const R1csDev& r1, const void* d_U, hipStream_t st, void* d_D) {
  using Fr = typename Curve::Fr;
  using Fq = typename Curve::Fq;
  const uint64_t n = r1.n, m = r1.m, nnz = r1.nnz[2];
  ARK_REQUIRE(m + 1 < (1ull << 32) && nnz < (1ull << 32) && n < (1ull << 32), ARK355_EINVAL, "instance too large for the column gather");
  ColGatherIn in;
  in.mats = r1.mats.as<Gr1csMat>() + 2;                 // C alone
  in.t = 1;
  in.n = (uint32_t)n;
  in.m = (uint32_t)m;
  in.nnz = in.max_nnz = nnz;
  ColGatherScratch cs;
  colgather_reserve(cs, m, nnz, COLGATHER_LANE_MAX, sizeof(XYZZ<Fq>));
  colgather_run<G1Terms<Curve>>(in, (const Affine<Fq>*)d_U, r1.pool.as<const Fr>(), (XYZZ<Fq>*)d_D, cs, COLGATHER_LANE_MAX, st);
  ARK_CHECK_HIP(hipStreamSynchronize(st));              // the scratch is freed on return
}

// The two base vectors of a bound key (affine, device): E' (N points) and the folded L' vector (m + 4 points, aligned with zx).
// d_h: h_query (N - 1 affine points); d_l: l_ext (m + 4 affine points: ell infinities, l_query, delta_1, three infinities).
template <class Curve>
static void hbasis_build(const R1csDev& r1, const void* d_h, const void* d_l, hipStream_t st, DevBuf& out_E, DevBuf& out_L) {
  using Fq = typename Curve::Fq;
  const uint64_t N = r1.N, m = r1.m;
  out_E.alloc(N * sizeof(Affine<Fq>));
  DevBuf d_D(m * sizeof(XYZZ<Fq>));
  {
    DevBuf d_U(N * sizeof(Affine<Fq>));
    hbasis_transforms<Curve>(d_h, r1.log_n, st, out_E.p, d_U.p);
    hbasis_gather<Curve>(r1, d_U.p, st, d_D.p);
  }
  const uint32_t total = (uint32_t)(m + 4);
  DevBuf d_x((size_t)total * sizeof(XYZZ<Fq>));
  out_L.alloc((size_t)total * sizeof(Affine<Fq>));
  ARK_LAUNCH((hb_fold_kernel<Fq>), dim3(hb_grid(total)), dim3(HB_THREADS), 0, st, (const Affine<Fq>*)d_l, d_D.as<const XYZZ<Fq>>(), (uint32_t)m,
             total, d_x.as<XYZZ<Fq>>());
  ARK_CHECK_LAUNCH();
  ARK_LAUNCH((batch_to_affine_kernel<Fq>), dim3(((total + PRE_K - 1) / PRE_K + MSM_THREADS - 1) / MSM_THREADS), dim3(MSM_THREADS), 0, st,
             d_x.as<const XYZZ<Fq>>(), out_L.as<Affine<Fq>>(), total);
  ARK_CHECK_LAUNCH();
  ARK_CHECK_HIP(hipStreamSynchronize(st));
}

}  // namespace ark355
