// Groth16 generator on the device (circuit_specific_setup, the reference's snark/src/lib.rs:43-46; upstream
// `generate_parameters_with_qap` / `R1CSToQAP::instance_map_with_evaluation`, SURVEY.md Appendix A "Setup"): the scalar
// stages of ark355_setup, from the resident CSR matrices (R1csDev) and the five trapdoor elements to the canonical scalar
// vectors the fixed-base kernels of api_impl.cuh multiply out.  Same values as the host generator Api::setup_scalars --
// field arithmetic is exact, so the order in which a column is summed does not matter.
//
//   S1  Lagrange coefficients  L_k(tau) = Z(tau)/N * w^k / (tau - w^k): a lane owns SETUP_RUN consecutive k, one
//       Montgomery-trick batch inversion per lane.  tau INSIDE the domain (Z(tau) = 0) never reaches that kernel: the host
//       detects it and launches the indicator kernel L_k = [w^k == tau] instead.
//   S2  column gather  u_j = sum_i L_i A[i][j], v_j, w_j over the three matrices side by side: colgather_impl.cuh over FrTerms
//       (column-major order, one lane per column of at most COLGATHER_LANE_MAX entries, a heavy list for the longer ones), the
//       same kernels that serve columns_impl.cuh.  Field arithmetic is exact: the order of a column's additions is free.
//   S3  the input-consistency rows of A, u_j += L_{n+j} for j < ell, are added where u_j is read next: in S4.
//   S4  combination  gamma_abc_j = (beta u_j + alpha v_j + w_j) / gamma (j < ell), l_j = (..) / delta (j >= ell), and the
//       Montgomery -> canonical conversion of u, v, w; h_i = Z(tau)/delta * tau^i as a running product per lane run.
#pragma once
#include <algorithm>
#include "common.h"
#include "msm_impl.cuh"
#include "witness_impl.cuh"
#include "colgather_impl.cuh"

namespace ark355 {

constexpr uint32_t SETUP_THREADS = 256;
constexpr uint32_t SETUP_RUN = 8;                         // domain points per lane of S1: one inversion per eight coefficients
constexpr uint32_t SETUP_H_RUN = 16;                      // powers of tau per lane of the h kernel

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

// S3 + S4: canonical u, v, w (m each), l (m - ell) and gamma_abc (ell) from the Montgomery column sums and L (n + ell <= N)
template <class Fr>
__global__ void __launch_bounds__(SETUP_THREADS)
setup_combine_kernel(const Fr* __restrict__ uvw, const Fr* __restrict__ L, uint64_t n, uint32_t m, uint32_t ell, Fr alpha, Fr beta,
                     Fr gamma_inv, Fr delta_inv, Fr* __restrict__ cu, Fr* __restrict__ cv, Fr* __restrict__ cw, Fr* __restrict__ cl,
                     Fr* __restrict__ cgabc) {
  const uint64_t j64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j64 >= m) return;
  const uint32_t j = (uint32_t)j64;
  Fr u = uvw[j];
  const Fr v = uvw[(uint64_t)m + j], w = uvw[2ull * m + j];
  const bool inst = j < ell;                              // one selection, not two branches: fewer registers, all eight waves
  if (inst) u = Fr::add(u, L[n + j]);                     // the input-consistency rows of A
  const Fr abc = Fr::add(Fr::add(Fr::mul(beta, u), Fr::mul(alpha, v)), w);
  Fr* dst = inst ? cgabc + j : cl + (j - ell);
  *dst = Fr::from_mont(Fr::mul(abc, inst ? gamma_inv : delta_inv));
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

// L_i(tau) for i < N = 2^log_n into d_L on `st` (queued); tau in Montgomery form.  tau inside H_N gives the indicator vector.
// Returns Z(tau) = tau^N - 1.
template <class Curve>
static typename Curve::Fr lagrange_run(uint32_t log_n, const typename Curve::Fr& tau, void* d_L, hipStream_t st) {
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
  return zt;
}

// td: tau, alpha, beta, gamma, delta in Montgomery form (gamma, delta non-zero).  Everything is queued on `st`; the one
// host wait before the end is the gather's (the heavy-column counter, 8 bytes).  All scratch of the gather is gone on return.
template <class Curve>
static void setup_scalars_dev(const R1csDev& r1, const typename Curve::Fr td[5], bool want_h, SetupScalarsDev& out,
                              hipStream_t st) {
  using Fr = typename Curve::Fr;
  const uint64_t n = r1.n, ell = r1.ell, m = r1.m, N = r1.N;
  ColGatherIn in;
  in.mats = r1.mats.as<Gr1csMat>();
  in.t = 3;
  in.n = (uint32_t)n;
  in.m = (uint32_t)m;
  for (int k = 0; k < 3; k++) {
    in.nnz += r1.nnz[k];
    in.max_nnz = std::max(in.max_nnz, r1.nnz[k]);
  }
  ARK_REQUIRE(3 * m + 1 < (1ull << 32) && in.nnz < (1ull << 32) && n < (1ull << 32), ARK355_EINVAL,
              "instance too large for the device generator (3 (ell + w) and the non-zeros of A, B, C together must stay below 2^32)");
  const Fr tau = td[0], alpha = td[1], beta = td[2];
  const Fr gamma_inv = Fr::inv(td[3]), delta_inv = Fr::inv(td[4]);

  DevBuf d_uvw((size_t)in.cols() * sizeof(Fr)), d_L(N * sizeof(Fr));
  const Fr zt = lagrange_run<Curve>(r1.log_n, tau, d_L.p, st);
  {
    ColGatherScratch cs;
    colgather_reserve(cs, in.cols(), in.nnz, COLGATHER_LANE_MAX, sizeof(Fr));
    colgather_run<FrTerms<Fr>>(in, d_L.as<const Fr>(), r1.pool.as<const Fr>(), d_uvw.as<Fr>(), cs, COLGATHER_LANE_MAX, st);
    ARK_CHECK_HIP(hipStreamSynchronize(st));            // the scratch is freed here
  }

  out.u.alloc(m * sizeof(Fr));
  out.v.alloc(m * sizeof(Fr));
  out.w.alloc(m * sizeof(Fr));
  out.l.alloc(r1.w * sizeof(Fr));
  out.gabc.alloc(ell * sizeof(Fr));
  ARK_LAUNCH((setup_combine_kernel<Fr>), dim3(setup_grid(m)), dim3(SETUP_THREADS), 0, st, d_uvw.as<const Fr>(), d_L.as<const Fr>(), n,
             (uint32_t)m, (uint32_t)ell, alpha, beta, gamma_inv, delta_inv, out.u.as<Fr>(), out.v.as<Fr>(), out.w.as<Fr>(),
             out.l.as<Fr>(), out.gabc.as<Fr>());
  ARK_CHECK_LAUNCH();
  if (want_h) {
    out.h.alloc((N - 1) * sizeof(Fr));
    if (N > 1) {
      ARK_LAUNCH((setup_h_kernel<Fr>), dim3(setup_grid((N - 1 + SETUP_H_RUN - 1) / SETUP_H_RUN)), dim3(SETUP_THREADS), 0, st,
                 out.h.as<Fr>(), N - 1, tau, Fr::mul(zt, delta_inv));
      ARK_CHECK_LAUNCH();
    }
  }
  ARK_CHECK_HIP(hipStreamSynchronize(st));              // d_uvw and d_L are freed on return
}

}  // namespace ark355
