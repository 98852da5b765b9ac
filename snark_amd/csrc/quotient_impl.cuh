// Quotient polynomial of any GR1CS predicate on the device: the step between the assignment of a resident system and the MSMs
// of a prover that is not Groth16 (the GM17-style provers behind sr1cs/mod.rs consume x0^2 - x1; a custom predicate of
// predicate/polynomial_constraint.rs any polynomial).
//
// With n rows, N = 2^log_domain >= max(n, 2), m_k the interpolation of M_k z over H_N (rows n .. N-1 are zero rows), d the total
// degree of P, D = 1 for d <= 2 and next_pow2(d - 1) otherwise:
//     h = the polynomial of degree < D N that agrees with P(m_0, .., m_{t-1}) / (X^N - 1) on the coset g H_{DN}.
// P(m_0, ..) has degree <= d (N - 1); for an assignment that satisfies all N rows X^N - 1 divides it and the quotient, of degree
// <= (d - 1) N - d < D N, is what comes out.  For any other assignment h is still the value the sentence above defines
// (witness_impl.cuh makes the same promise for a b - c).
//
//   gr1cs_spmv_padded_kernel   M_k z for the t matrices (grid.y) straight into t vectors of N elements, zero from row n up, at
//                              the uniform stride of ntt_inverse_then_coset (vector k at 2 k L, its ping-pong partner at
//                              (2 k + 1) L, L = D N)
//   D = 1                      ONE ntt_inverse_then_coset with batch = t: the fused seam and the log_n < 3 path are kept
//   D > 1                      per vector: ntt_run inverse of size N, zero-extension to L, ntt_run coset of size L
//   gr1cs_quotient_kernel      one lane per point i < L: the polynomial program gr1cs_pred_kernel reads, its factors loaded from
//                              vec[var][i] (coalesced; the variable is wave-uniform, so no LDS and no per-lane array), times
//                              zinv[i & (D - 1)]: point i of the coset is g w_{DN}^i, where X^N - 1 = g^N w_D^i - 1 takes D values
//   ntt_run inverse coset of size L: its result buffer is h.
// Seven transforms for t = 3, D = 1, where witness_map_run runs six and never interprets a program: that map stays the route of
// the Groth16 prover.
#pragma once
#include <map>
#include "common.h"
#include "ntt_impl.cuh"
#include "gr1cs_impl.cuh"

namespace ark355 {

struct QuotientDims {
  uint64_t degree = 0;
  uint32_t log_domain = 0, log_ext = 0;
  uint64_t h_len = 0;                  // 0 unless the dimensions are accepted
};

// grow-only scratch of a context: 2 t vectors of D N Fr, and the D constants per (curve, log_domain, log_ext)
struct QuotientScratch {
  DevBuf vecs;
  std::map<uint32_t, DevBuf> zinv;
};

// The dimensions and what refuses them; no HIP call.  degree, log_domain and log_ext are written whenever they are defined, so
// a refusal still reports the 64-bit degree it refused.
static inline int32_t quotient_dims(const Gr1csPred& P, uint32_t log_n, uint32_t two_adicity, QuotientDims* q, std::string* why) {
  q->degree = P.degree;
  uint32_t log_ext = 0;
  if (P.degree > 2)
    while ((1ull << log_ext) < P.degree - 1) log_ext++;          // degree < 2^42: 1024 factors of 32-bit exponents
  q->log_ext = log_ext;
  uint32_t log_domain = log_n;
  if (log_n == 0) {
    log_domain = 1;
    while ((1ull << log_domain) < P.n) log_domain++;
  }
  q->log_domain = log_domain;
  if (log_domain > two_adicity) {
    *why = "the evaluation domain exceeds the largest radix-2 domain of Fr";
    return ARK355_E_POLY_DEGREE_TOO_LARGE;
  }
  if ((1ull << log_domain) < P.n) {
    *why = "2^log_n is below the predicate's row count";
    return ARK355_EINVAL;
  }
  if (log_domain + log_ext > two_adicity) {
    *why = "degree " + std::to_string(P.degree) + " on 2^" + std::to_string(log_domain) +
           " points: the extended domain exceeds the largest radix-2 domain of Fr";
    return ARK355_E_POLY_DEGREE_TOO_LARGE;
  }
  q->h_len = 1ull << (log_domain + log_ext);
  return ARK355_OK;
}

template <class Fr>
__global__ void __launch_bounds__(256)
gr1cs_spmv_padded_kernel(const Gr1csMat* __restrict__ mats, const Fr* __restrict__ pool, const Fr* __restrict__ z, uint64_t n,
                         uint64_t N, uint64_t stride, Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Fr v = Fr::zero();
  if (i < n) v = gr1cs_row_dot<Fr>(mats[blockIdx.y], pool, z, i);
  out[(uint64_t)blockIdx.y * stride + i] = v;
}

// out[i] = P(vec[0][i], .., vec[t-1][i]) * zinv[i & ext_mask]; vec[k] = vec + k * stride.  The loops over terms, factors and
// exponent bits are wave-uniform (the program sits behind a kernel-argument pointer), a factor is one coalesced 32-byte load per
// lane; out aliases no vec[k].
template <class Fr>
__global__ void __launch_bounds__(256)
gr1cs_quotient_kernel(const Fr* __restrict__ vec, uint64_t stride, const uint32_t* __restrict__ prog, const Fr* __restrict__ pool,
                      const Fr* __restrict__ zinv, uint32_t ext_mask, uint64_t count, Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  Fr acc = Fr::zero();
  const uint32_t n_terms = prog[0];
  uint32_t pc = 1;
  for (uint32_t t = 0; t < n_terms; t++) {
    const uint32_t ci = prog[pc], n_factors = prog[pc + 1];
    pc += 2;
    bool have = false;
    Fr prod = Fr::zero();
    for (uint32_t f = 0; f < n_factors; f++) {
      const uint32_t var = prog[pc], e = prog[pc + 1];
      pc += 2;
      if (e == 0) continue;                // x^0 = 1
      const Fr pw = gr1cs_pow<Fr>(vec[(uint64_t)var * stride + i], e);
      prod = have ? Fr::mul(prod, pw) : pw;
      have = true;
    }
    Fr term = pool[ci];                    // a term without factors is the constant term
    if (have) term = ci ? Fr::mul(prod, term) : prod;
    acc = Fr::add(acc, term);
  }
  out[i] = Fr::mul(acc, zinv[i & ext_mask]);
}

// zinv[s] = (g^N w_D^s - 1)^-1 for s < D, with the library's field code on the host and one inversion for all of them
// (r1cs_upload_zinv is the case D = 1); cached per (curve, log_domain, log_ext)
template <class Curve>
static const typename Curve::Fr* quotient_zinv(QuotientScratch& qs, uint32_t log_domain, uint32_t log_ext) {
  using Fr = typename Curve::Fr;
  using P = typename Fr::Params;
  const uint32_t key = ((uint32_t)Curve::ID << 16) | (log_domain << 8) | log_ext;
  auto it = qs.zinv.find(key);
  if (it != qs.zinv.end()) return it->second.template as<Fr>();
  const uint64_t D = 1ull << log_ext;
  const Fr gn = fr_pow2k(fr_from_params<Fr>(&P::gen), log_domain);
  const Fr w = ntt_root<Fr>(log_ext, false);
  std::vector<Fr> val(D), pre(D);
  Fr cur = gn, run = Fr::one();
  for (uint64_t s = 0; s < D; s++) {       // g^N w_D^s = 1 would make g^(D N) = 1: g generates the whole group
    val[s] = Fr::sub(cur, Fr::one());
    pre[s] = run;
    run = Fr::mul(run, val[s]);
    cur = Fr::mul(cur, w);
  }
  Fr inv = Fr::inv(run);
  for (uint64_t s = D; s-- > 0;) {
    const Fr v = val[s];
    val[s] = Fr::mul(inv, pre[s]);
    inv = Fr::mul(inv, v);
  }
  DevBuf d(D * sizeof(Fr));
  ARK_CHECK_HIP(hipMemcpy(d.p, val.data(), D * sizeof(Fr), hipMemcpyHostToDevice));
  return qs.zinv.emplace(key, std::move(d)).first->second.template as<Fr>();
}

// z (device) -> h (device, q.h_len Fr, Montgomery): returns where it sits inside the scratch; everything on `st`
template <class Curve>
static void* quotient_run(ark355_ctx* ctx, const Gr1csDev& g, const Gr1csPred& P, const QuotientDims& q, const void* d_z,
                          QuotientScratch& qs, hipStream_t st) {
  using Fr = typename Curve::Fr;
  const uint32_t t = P.arity, log_len = q.log_domain + q.log_ext;
  const uint64_t N = 1ull << q.log_domain, L = q.h_len, stride = 2 * L;
  qs.vecs.ensure((size_t)stride * t * sizeof(Fr));
  const Fr* zinv = quotient_zinv<Curve>(qs, q.log_domain, q.log_ext);
  Fr* base = qs.vecs.as<Fr>();
  ARK_LAUNCH((gr1cs_spmv_padded_kernel<Fr>), dim3((uint32_t)((N + 255) / 256), t), dim3(256), 0, st,
             (const Gr1csMat*)P.mats.as<Gr1csMat>(), (const Fr*)g.pool.as<Fr>(), (const Fr*)d_z, P.n, N, stride, base);
  ARK_CHECK_LAUNCH();
  Fr* res0 = nullptr;
  if (q.log_ext == 0) {
    res0 = (Fr*)ntt_inverse_then_coset<Curve>(ctx, base, base + L, q.log_domain, st, t, stride);
  } else {
    for (uint32_t k = 0; k < t; k++) {
      Fr* cur = base + (uint64_t)k * stride;
      Fr* oth = cur + L;
      Fr* coef = (Fr*)ntt_run<Curve>(ctx, cur, oth, q.log_domain, /*inverse=*/true, /*coset=*/false, st);
      ARK_CHECK_HIP(hipMemsetAsync(coef + N, 0, (size_t)(L - N) * sizeof(Fr), st));
      Fr* res = (Fr*)ntt_run<Curve>(ctx, coef, coef == cur ? oth : cur, log_len, /*inverse=*/false, /*coset=*/true, st);
      if (k == 0) res0 = res;
      ARK_REQUIRE(res == res0 + (uint64_t)k * stride, ARK355_EINVAL, "quotient: the vectors left the uniform stride");
    }
  }
  Fr* free0 = res0 == base ? base + L : base;          // the partner of vector 0: the pointwise result, then ping-pong
  ARK_LAUNCH((gr1cs_quotient_kernel<Fr>), dim3((uint32_t)((L + 255) / 256)), dim3(256), 0, st, (const Fr*)res0, stride,
             (const uint32_t*)P.prog.as<uint32_t>(), (const Fr*)g.pool.as<Fr>(), zinv, (uint32_t)((1ull << q.log_ext) - 1), L, free0);
  ARK_CHECK_LAUNCH();
  return ntt_run<Curve>(ctx, free0, res0, log_len, /*inverse=*/true, /*coset=*/true, st);
}

}  // namespace ark355
