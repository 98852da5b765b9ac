// Per-curve implementation of the C ABI (explicitly instantiated in ark355_bls.hip / ark355_bn.hip).
#pragma once
#include <chrono>
#include <functional>
#include <thread>
#include "common.h"
#include "groth16_impl.cuh"
#include "gr1cs_impl.cuh"
#include "sr1cs_impl.cuh"
#include "quotient_impl.cuh"
#include "columns_impl.cuh"
#include "poly_impl.cuh"
#include "evals_impl.cuh"
#include "mle_impl.cuh"
#include "mle_open_impl.cuh"
#include "msm_batch_impl.cuh"
#include "sumcheck_impl.cuh"
#include "lcmap_impl.cuh"
#include "setup_impl.cuh"
#include "wire_impl.cuh"
#include "verify_impl.cuh"

namespace ark355 {

struct BasesDev {
  int curve = 0, group = 1;
  int device = -1;       // where the tables are resident (set by ark355_bases_load)
  uint64_t n = 0;
  PrecompTable tab;      // per-window tables of the resident bases
};

// ---- fixed-base multiplication (setup: the generator's five query vectors are k_i * G) -----------------------------
// Windowed: T[w][d-1] = d * 2^(8w) * base for d = 1..255, w < 32 (8 160 affine points, built once per call on the
// device), then every scalar costs 32 mixed additions instead of the ~383 group operations of double-and-add, and the
// results are normalised 16 at a time with one inversion (batch_to_affine_kernel).  The first version (one lane per
// scalar, double-and-add, an inversion each) spilled 2.9 KB per lane and took most of the 9 s of bench.py's preparation.
constexpr uint32_t FB_WBITS = 8, FB_WINDOWS = 32, FB_ROW = (1u << FB_WBITS) - 1u;

// row w of the table in XYZZ form: lane d-1 computes d * (2^(8w) base) by double-and-add over the 8-bit d
template <class F>
__global__ void __launch_bounds__(256)
fixed_base_table_kernel(const Affine<F>* __restrict__ base, XYZZ<F>* __restrict__ table) {
  const uint32_t w = blockIdx.x, d = threadIdx.x + 1;
  if (d > FB_ROW) return;
  XYZZ<F> p = XYZZ<F>::from_affine(*base);
  for (uint32_t i = 0; i < w * FB_WBITS; i++) p = xyzz_dbl(p);
  uint32_t k = d;
  table[w * FB_ROW + (d - 1)] = xyzz_mul_scalar(p, &k, 1);
}

// a handful of scalars (the alpha/beta/gamma/delta points of a key, closed-form checks): one lane each, double-and-add --
// building the 8 160-point table first would cost more than it saves
template <class F, class Fr>
__global__ void __launch_bounds__(128)
fixed_base_small_kernel(const Affine<F>* __restrict__ base, const Fr* __restrict__ scalars, uint64_t n,
                        XYZZ<F>* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr k = scalars[i];
  out[i] = xyzz_mul_scalar(XYZZ<F>::from_affine(*base), k.l, Fr::N);
}

template <class F, class Fr>
__global__ void __launch_bounds__(128)
fixed_base_mul_kernel(const Affine<F>* __restrict__ table, const Fr* __restrict__ scalars, uint64_t n,
                      XYZZ<F>* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr k = scalars[i];
  XYZZ<F> acc = XYZZ<F>::inf();
  for (uint32_t w = 0; w < FB_WINDOWS; w++) {
    const uint32_t d = (k.l[w >> 2] >> ((w & 3u) * 8u)) & 0xFFu;
    if (d) xyzz_madd_ni(acc, table[w * FB_ROW + (d - 1)]);
  }
  out[i] = acc;
}

// canonical values of n Montgomery images (the device-scalar entry of the fixed-base multiplication)
template <class Fr>
__global__ void __launch_bounds__(256)
fr_from_mont_kernel(const Fr* __restrict__ in, uint64_t n, Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr one = Fr::zero();                     // the integer 1: x R * 1 / R = x.  Fr::from_mont calls the out-of-line multiplication,
  one.l[0] = 1;                            // whose operands travel through 48 bytes of stack per lane; inlined there is none
  out[i] = Fr::mul(in[i], one);
}

struct GenericScratch {
  MsmSort sort;
  MsmBuckets bk;
  DevBuf a, b, c;
  DevBuf rows;       // the 28-bit rows of a one-shot MSM's bases (msm_host)
  PairingScratch pair;   // the device routes of the pairing entries (verify_impl.cuh)
};

template <class Curve>
struct Api {
  using Fr = typename Curve::Fr;
  using Fq = typename Curve::Fq;
  using Fq2 = typename Curve::Fq2;
  using W = Wire<Curve>;

  static void sizes(uint32_t what[4]) {
    what[0] = sizeof(Fr);
    what[1] = sizeof(Fq);
    what[2] = sizeof(Affine<Fq>);
    what[3] = sizeof(Affine<Fq2>);
  }

  static PkDev* pk_load(const TunePolicy& pol, const ark355_pk_desc* d, hipStream_t st, uint32_t shard_index = 0,
                        uint32_t shard_count = 1) {
    return pk_upload<Curve>(pol, d, st, shard_index, shard_count);
  }

  static R1csDev* r1cs_load(uint64_t n, uint64_t ell, uint64_t w, const uint64_t* const rp[3],
                            const uint32_t* const col[3], const uint8_t* const coeff[3]) {
    return r1cs_upload<Curve>(n, ell, w, rp, col, coeff);
  }

  static void prove(ark355_ctx* ctx, ProverScratch& sc, PkDev& pk, const R1csDev& r1, const void* z,
                    bool on_dev, const uint8_t* r, const uint8_t* s, ark355_proof_raw* out, uint8_t* partials = nullptr,
                    CommDev* cm = nullptr, int shard_mode = 0) {
    prove_run<Curve>(ctx, sc, pk, r1, z, on_dev, r, s, out, partials, cm, shard_mode);
  }
  static void combine(const uint8_t* partials, uint64_t count, const uint8_t* r, const uint8_t* s, ark355_proof_raw* out) {
    combine_partials_host<Curve>(partials, count, r, s, out);
  }
  static size_t partial_size() { return 4 * sizeof(XYZZ<Fq>) + sizeof(XYZZ<Fq2>); }

  // the two group transforms of hbasis_impl.cuh on host vectors (tests, diagnostics): h_query is N - 1 raw affine points, out_e /
  // out_u N each (either may be null)
  static void hbasis_transform(ark355_ctx* ctx, const uint8_t* h_query, uint32_t log_n, uint8_t* out_e, uint8_t* out_u) {
    constexpr size_t G1 = sizeof(Affine<Fq>);
    ARK_REQUIRE(log_n >= 1 && log_n <= 23, ARK355_EINVAL, "group transform: 2^1 .. 2^23 points");
    const uint64_t N = 1ull << log_n;
    hipStream_t st = ctx->stream;
    DevBuf d_h((N - 1) * G1), d_e, d_u;
    ARK_CHECK_HIP(hipMemcpy(d_h.p, h_query, (N - 1) * G1, hipMemcpyHostToDevice));
    if (out_e) d_e.alloc(N * G1);
    if (out_u) d_u.alloc(N * G1);
    hbasis_transforms<Curve>(d_h.p, log_n, st, out_e ? d_e.p : nullptr, out_u ? d_u.p : nullptr);
    if (out_e) ARK_CHECK_HIP(hipMemcpy(out_e, d_e.p, N * G1, hipMemcpyDeviceToHost));
    if (out_u) ARK_CHECK_HIP(hipMemcpy(out_u, d_u.p, N * G1, hipMemcpyDeviceToHost));
  }
  // the column gather D_i = sum_j C[j][i] U_j of hbasis_impl.cuh: u is N raw affine points, out_d gets ell + w
  static void hbasis_gather_host(ark355_ctx* ctx, const R1csDev& r1, const uint8_t* u, uint8_t* out_d) {
    constexpr size_t G1 = sizeof(Affine<Fq>);
    ARK_REQUIRE(r1.curve == Curve::ID, ARK355_EINVAL, "curve mismatch");
    hipStream_t st = ctx->stream;
    const uint32_t m = (uint32_t)r1.m;
    DevBuf d_u(r1.N * G1), d_D((size_t)m * sizeof(XYZZ<Fq>)), d_aff((size_t)m * G1);
    ARK_CHECK_HIP(hipMemcpy(d_u.p, u, r1.N * G1, hipMemcpyHostToDevice));
    hbasis_gather<Curve>(r1, d_u.p, st, d_D.p);
    ARK_LAUNCH((batch_to_affine_kernel<Fq>), dim3(((m + PRE_K - 1) / PRE_K + MSM_THREADS - 1) / MSM_THREADS), dim3(MSM_THREADS), 0, st,
               d_D.as<const XYZZ<Fq>>(), d_aff.as<Affine<Fq>>(), m);
    ARK_CHECK_LAUNCH();
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    ARK_CHECK_HIP(hipMemcpy(out_d, d_aff.p, (size_t)m * G1, hipMemcpyDeviceToHost));
  }

  static void witness_map(ark355_ctx* ctx, ProverScratch& sc, const R1csDev& r1, const uint8_t* z, uint8_t* h_out) {
    hipStream_t st = ctx->stream;
    sc.zx.ensure((r1.m + 4) * sizeof(Fr));
    ARK_CHECK_HIP(hipMemcpyAsync(sc.zx.p, z, r1.m * sizeof(Fr), hipMemcpyHostToDevice, st));
    void* d_h = witness_map_run<Curve>(ctx, r1, sc.zx.p, sc.ws, st);
    ARK_CHECK_HIP(hipMemcpyAsync(h_out, d_h, r1.N * sizeof(Fr), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  static void witness_map_dist_sim(ark355_ctx* ctx, ProverScratch& sc, const R1csDev& r1, const uint8_t* z, uint32_t world,
                                   uint8_t* h_out) {
    hipStream_t st = ctx->stream;
    sc.zx.ensure((r1.m + 4) * sizeof(Fr));
    ARK_CHECK_HIP(hipMemcpyAsync(sc.zx.p, z, r1.m * sizeof(Fr), hipMemcpyHostToDevice, st));
    DevBuf h(r1.N * sizeof(Fr));
    ark355::witness_map_dist_sim<Curve>(ctx, r1, sc.zx.p, world, h.p, st);
    ARK_CHECK_HIP(hipMemcpyAsync(h_out, h.p, r1.N * sizeof(Fr), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  static void mat_vec(ark355_ctx* ctx, ProverScratch& sc, const R1csDev& r1, const uint8_t* z, uint8_t* az,
                      uint8_t* bz, uint8_t* cz, int64_t* first_bad) {
    hipStream_t st = ctx->stream;
    sc.zx.ensure((r1.m + 4) * sizeof(Fr));
    ARK_CHECK_HIP(hipMemcpyAsync(sc.zx.p, z, r1.m * sizeof(Fr), hipMemcpyHostToDevice, st));
    spmv_run<Curve>(r1, sc.zx.p, sc.ws, st);
    if (az) ARK_CHECK_HIP(hipMemcpyAsync(az, sc.ws.buf[0].p, r1.n * sizeof(Fr), hipMemcpyDeviceToHost, st));
    if (bz) ARK_CHECK_HIP(hipMemcpyAsync(bz, sc.ws.buf[2].p, r1.n * sizeof(Fr), hipMemcpyDeviceToHost, st));
    if (cz) ARK_CHECK_HIP(hipMemcpyAsync(cz, sc.ws.buf[4].p, r1.n * sizeof(Fr), hipMemcpyDeviceToHost, st));
    if (first_bad) {
      sc.ws.first_bad.ensure(8);
      ARK_CHECK_HIP(hipMemsetAsync(sc.ws.first_bad.p, 0xFF, 8, st));
      if (r1.n) {
        const uint32_t grid = (uint32_t)((r1.n + 255) / 256);
        ARK_LAUNCH((r1cs_check_kernel<Fr>), dim3(grid), dim3(256), 0, st, sc.ws.buf[0].as<Fr>(),
                   sc.ws.buf[2].as<Fr>(), sc.ws.buf[4].as<Fr>(), r1.n, sc.ws.first_bad.as<unsigned long long>());
        ARK_CHECK_LAUNCH();
      }
      unsigned long long fb = 0;
      ARK_CHECK_HIP(hipMemcpyAsync(&fb, sc.ws.first_bad.p, 8, hipMemcpyDeviceToHost, st));
      ARK_CHECK_HIP(hipStreamSynchronize(st));
      *first_bad = (fb == ~0ull) ? -1 : (int64_t)fb;
    }
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // ---- GR1CS (gr1cs_impl.cuh) ------------------------------------------------------------------------------------
  static Gr1csDev* gr1cs_load(uint64_t ell, uint64_t w, const ark355_predicate_desc* preds, uint32_t n_preds) {
    return gr1cs_upload<Curve>(ell, w, preds, n_preds);
  }
  static void* gr1cs_stage_z(ark355_ctx* ctx, ProverScratch& sc, const Gr1csDev& g, const uint8_t* z) {
    sc.zx.ensure((g.m + 4) * sizeof(Fr));
    ARK_CHECK_HIP(hipMemcpyAsync(sc.zx.p, z, g.m * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return sc.zx.p;
  }
  // *predicate = the caller's index of the first failing predicate in label order, *constraint = its first failing row
  static void gr1cs_check(ark355_ctx* ctx, ProverScratch& sc, const Gr1csDev& g, const uint8_t* z, int64_t* predicate,
                          int64_t* constraint) {
    hipStream_t st = ctx->stream;
    void* d_z = gr1cs_stage_z(ctx, sc, g, z);
    sc.ws.first_bad.ensure(8);
    gr1cs_check_run<Curve>(g, d_z, sc.ws.first_bad.as<unsigned long long>(), st);
    unsigned long long key = 0;
    ARK_CHECK_HIP(hipMemcpyAsync(&key, sc.ws.first_bad.p, 8, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    *predicate = -1;
    *constraint = -1;
    if (key == ~0ull) return;
    const uint32_t rank = (uint32_t)(key >> GR1CS_ROW_BITS);
    for (size_t p = 0; p < g.preds.size(); p++)
      if (g.preds[p].rank == rank) *predicate = (int64_t)p;
    *constraint = (int64_t)(key & ((1ull << GR1CS_ROW_BITS) - 1));
  }
  static void gr1cs_mat_vec(ark355_ctx* ctx, ProverScratch& sc, GenericScratch& gs, const Gr1csDev& g, uint32_t p,
                            const uint8_t* z, uint8_t* out, bool eval) {
    hipStream_t st = ctx->stream;
    const Gr1csPred& P = g.preds[p];
    if (!P.n) return;
    void* d_z = gr1cs_stage_z(ctx, sc, g, z);
    const size_t bytes = (size_t)(eval ? 1 : P.arity) * P.n * sizeof(Fr);
    gs.a.ensure(bytes);
    if (eval) gr1cs_eval_run<Curve>(g, P, d_z, gs.a.p, st);
    else gr1cs_spmv_run<Curve>(g, P, d_z, gs.a.p, st);
    ARK_CHECK_HIP(hipMemcpyAsync(out, gs.a.p, bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }
  static R1csDev* gr1cs_r1cs(ark355_ctx* ctx, const Gr1csDev& g) { return gr1cs_to_r1cs<Curve>(g, ctx->stream); }

  static void gr1cs_matrix(ark355_ctx* ctx, GenericScratch& gs, const Gr1csDev& g, uint32_t p, uint32_t which, uint64_t* row_ptr,
                           uint32_t* col, uint8_t* coeff) {
    ark355::gr1cs_matrix<Curve>(g, g.preds[p], which, row_ptr, col, coeff, gs.a, ctx->stream);
  }
  // ---- finalize() on the device (lcmap_impl.cuh) -----------------------------------------------------------------
  static Gr1csDev* gr1cs_from_lcs(ark355_ctx* ctx, const ark355_lc_system_desc& s, const ark355_predicate_lcs_desc* preds,
                                  uint32_t n_preds) {
    return lcs_finalize<Curve>(s, preds, n_preds, (uint32_t)std::max(ctx->policy.lcs_row_lds_max, 1), ctx->stream);
  }

  // ---- Square R1CS (sr1cs_impl.cuh) ------------------------------------------------------------------------------
  static Sr1csDev* sr1cs_from_r1cs(ark355_ctx* ctx, const R1csDev& r1) { return sr1cs_build<Curve>(r1, ctx->device, ctx->stream); }
  static void sr1cs_matrix(ark355_ctx* ctx, GenericScratch& gs, const Sr1csDev& s, int which, uint64_t* row_ptr, uint32_t* col,
                           uint8_t* coeff) {
    ark355::sr1cs_matrix<Curve>(s, which, row_ptr, col, coeff, gs.a, ctx->stream);
  }
  static void sr1cs_assignment(ark355_ctx* ctx, ProverScratch& sc, GenericScratch& gs, const Sr1csDev& s, const void* z, void* z_out,
                               bool on_dev) {
    ark355::sr1cs_assignment<Curve>(s, z, z_out, on_dev, sc.zx, gs.a, ctx->stream);
  }

  // ---- quotient of a predicate (quotient_impl.cuh) -----------------------------------------------------------------
  static int32_t gr1cs_quotient_dims(const Gr1csPred& P, uint32_t log_n, QuotientDims* q, std::string* why) {
    return quotient_dims(P, log_n, (uint32_t)Fr::Params::TWO_ADICITY, q, why);
  }
  // z and h_out both on the host or both on the device; returns when h_out is complete
  static void gr1cs_quotient(ark355_ctx* ctx, ProverScratch& sc, QuotientScratch& qs, const Gr1csDev& g, uint32_t p,
                             const QuotientDims& q, const void* z, bool on_dev, void* h_out) {
    hipStream_t st = ctx->stream;
    const void* d_z = on_dev ? z : gr1cs_stage_z(ctx, sc, g, (const uint8_t*)z);
    void* d_h = quotient_run<Curve>(ctx, g, g.preds[p], q, d_z, qs, st);
    ARK_CHECK_HIP(hipMemcpyAsync(h_out, d_h, q.h_len * sizeof(Fr), on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // ---- column polynomials of a predicate at a point (columns_impl.cuh) ----------------------------------------------
  static uint32_t two_adicity() { return (uint32_t)Fr::Params::TWO_ADICITY; }
  // a canonical 32-byte little-endian integer below r -> its Montgomery image; false for a value >= r
  static bool fr_from_canonical(const uint8_t* bytes, Fr* mont) {
    Fr c;
    memcpy(c.l, bytes, sizeof(Fr));
    if (!fr_canonical(c)) return false;
    *mont = Fr::to_mont(c);
    return true;
  }
  static int32_t gr1cs_columns_dims(const Gr1csDev& g, const Gr1csPred& P, bool with_domain, uint32_t log_n, ColumnsDims* d,
                                    std::string* why) {
    return columns_dims(g, P, with_domain, log_n, two_adicity(), d, why);
  }
  // out[i] = L_i(tau) for i < 2^log_n, in host or in device memory; returns when out is complete
  static void lagrange(ark355_ctx* ctx, ColumnsScratch& cs, uint32_t log_n, const Fr& tau, void* out, bool on_dev) {
    hipStream_t st = ctx->stream;
    const size_t bytes = sizeof(Fr) << log_n;
    if (!on_dev) cs.lag.ensure(bytes);
    void* d_L = on_dev ? out : cs.lag.p;
    lagrange_run<Curve>(log_n, tau, d_L, st);
    if (!on_dev) ARK_CHECK_HIP(hipMemcpyAsync(out, d_L, bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }
  // tau == nullptr: out = M_k^T y for the caller's y; otherwise y = (L_i(tau))_i over 2^d.log_domain points, computed into the
  // scratch.  y and out both on the host or both on the device; every allocation happens before the first launch.
  static void gr1cs_columns(ark355_ctx* ctx, ColumnsScratch& cs, const Gr1csDev& g, uint32_t p, const ColumnsDims& d, const void* y,
                            const Fr* tau, bool on_dev, void* out) {
    hipStream_t st = ctx->stream;
    const Gr1csPred& P = g.preds[p];
    const uint32_t lane_max = cols_lane_max(ctx->policy.cols_lane_max);
    const size_t out_bytes = (size_t)d.cols * sizeof(Fr);
    columns_reserve<Fr>(cs, d, lane_max);
    if (tau && d.nnz) cs.lag.ensure(sizeof(Fr) << d.log_domain);
    if (!on_dev) {
      cs.out.ensure(out_bytes);
      if (!tau && d.nnz) cs.y.ensure((size_t)d.n * sizeof(Fr));
    }
    const void* d_y = y;
    if (tau) {
      if (d.nnz) lagrange_run<Curve>(d.log_domain, *tau, cs.lag.p, st);
      d_y = cs.lag.p;
    } else if (!on_dev && d.nnz) {
      ARK_CHECK_HIP(hipMemcpyAsync(cs.y.p, y, (size_t)d.n * sizeof(Fr), hipMemcpyHostToDevice, st));
      d_y = cs.y.p;
    }
    void* d_out = on_dev ? out : cs.out.p;
    columns_run<Curve>(g, P, d, d_y, d_out, cs, lane_max, st);
    if (!on_dev && out_bytes) ARK_CHECK_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // ---- polynomial openings (poly_impl.cuh): the refusals are capi.hip's; every allocation happens before the first launch --
  // out[k] = p_k(x); coeffs and out both on the host or both on the device; returns when out is complete
  static void poly_eval(ark355_ctx* ctx, PolyScratch& ps, const void* coeffs, uint64_t len, uint64_t count, const Fr& x, void* out,
                        bool on_dev) {
    hipStream_t st = ctx->stream;
    if (!count) return;
    const PolyPlan plan = poly_plan(len, count, poly_lane_coeffs(ctx->policy.poly_lane_coeffs));
    const size_t bytes = (size_t)count * len * sizeof(Fr), out_bytes = (size_t)count * sizeof(Fr);
    poly_reserve<Fr>(ps, plan, count, false);
    if (!on_dev) {
      ps.in.ensure(bytes);
      ps.small.ensure(out_bytes);
      if (bytes) ARK_CHECK_HIP(hipMemcpyAsync(ps.in.p, coeffs, bytes, hipMemcpyHostToDevice, st));
    }
    void* d_out = on_dev ? out : ps.small.p;
    poly_eval_run<Curve>(on_dev ? coeffs : ps.in.p, count, plan, x, d_out, ps, st);
    if (!on_dev) ARK_CHECK_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }
  // q[k] = (p_k - p_k(x)) / (X - x), rem[k] = p_k(x) (rem may be null); the host variant divides in place on its staging
  static void poly_div_linear(ark355_ctx* ctx, PolyScratch& ps, const void* coeffs, uint64_t len, uint64_t count, const Fr& x,
                              void* q, void* rem, bool on_dev) {
    hipStream_t st = ctx->stream;
    if (!count) return;
    const PolyPlan plan = poly_plan(len, count, poly_lane_coeffs(ctx->policy.poly_lane_coeffs));
    const size_t bytes = (size_t)count * len * sizeof(Fr), rem_bytes = (size_t)count * sizeof(Fr);
    if (!len) {                                          // nothing to divide: only the remainder, zero, is written
      if (!rem) return;
      if (on_dev) {
        ARK_CHECK_HIP(hipMemsetAsync(rem, 0, rem_bytes, st));
        ARK_CHECK_HIP(hipStreamSynchronize(st));
      } else {
        memset(rem, 0, rem_bytes);
      }
      return;
    }
    poly_reserve<Fr>(ps, plan, count, !rem || !on_dev);
    if (!on_dev) {
      ps.in.ensure(bytes);
      ARK_CHECK_HIP(hipMemcpyAsync(ps.in.p, coeffs, bytes, hipMemcpyHostToDevice, st));
    }
    void* d_q = on_dev ? q : ps.in.p;
    void* d_rem = on_dev ? rem : ps.rem.p;
    poly_div_run<Curve>(on_dev ? coeffs : ps.in.p, count, plan, x, d_q, d_rem, ps, st);
    if (!on_dev) {
      ARK_CHECK_HIP(hipMemcpyAsync(q, d_q, bytes, hipMemcpyDeviceToHost, st));
      if (rem) ARK_CHECK_HIP(hipMemcpyAsync(rem, d_rem, rem_bytes, hipMemcpyDeviceToHost, st));
    }
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }
  // out = sum_k scalars[k] polys[k]; scalars: count Montgomery images on the host; the host variant combines in place on its staging
  static void poly_lincomb(ark355_ctx* ctx, PolyScratch& ps, const void* polys, uint64_t len, uint64_t count, const Fr* scalars,
                           void* out, bool on_dev) {
    hipStream_t st = ctx->stream;
    if (!len) return;
    const size_t bytes = (size_t)count * len * sizeof(Fr), out_bytes = (size_t)len * sizeof(Fr);
    ps.tab.ensure(std::max((size_t)count, (size_t)POLY_MAX_LEVELS * POLY_TAB_STRIDE) * sizeof(Fr));
    if (!on_dev) {
      ps.in.ensure(std::max(bytes, out_bytes));
      if (bytes) ARK_CHECK_HIP(hipMemcpyAsync(ps.in.p, polys, bytes, hipMemcpyHostToDevice, st));
    }
    void* d_out = on_dev ? out : ps.in.p;
    poly_lincomb_run<Curve>(on_dev ? polys : ps.in.p, len, count, scalars, d_out, ps, st);
    if (!on_dev) ARK_CHECK_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // ---- openings in the evaluation basis (evals_impl.cuh): the refusals are capi.hip's; every allocation happens before the first launch
  // out[k] = p_k(x) from the values of p_k over the domain; evals and out both on the host or both on the device
  static void evals_eval(ark355_ctx* ctx, EvalsScratch& es, const void* evals, uint32_t log_n, uint64_t count, bool coset, const Fr& x,
                         void* out, bool on_dev) {
    hipStream_t st = ctx->stream;
    if (!count) return;
    const EvalsPlan plan = evals_plan(log_n, count, evals_lane_points(ctx->policy.evals_lane_points));
    const EvalsPoint<Fr> pt = evals_point<Fr>(log_n, coset, x);
    const size_t bytes = (size_t)count * plan.N * sizeof(Fr), out_bytes = (size_t)count * sizeof(Fr);
    evals_reserve<Fr>(es, plan, count, false);
    if (!on_dev) {
      es.in.ensure(bytes);
      es.small.ensure(out_bytes);
      ARK_CHECK_HIP(hipMemcpyAsync(es.in.p, evals, bytes, hipMemcpyHostToDevice, st));
    }
    if (!pt.inside) evals_upload_tables<Fr>(es, plan, pt, st);
    void* d_out = on_dev ? out : es.small.p;
    evals_eval_run<Curve>(on_dev ? evals : es.in.p, count, plan, pt, d_out, es, st);
    if (!on_dev) ARK_CHECK_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }
  // q[k][i] = q_k(a_i) for q_k = (p_k - p_k(x)) / (X - x), rem[k] = p_k(x) (rem may be null); the host variant divides in place on
  // its staging
  static void evals_div_linear(ark355_ctx* ctx, EvalsScratch& es, const void* evals, uint32_t log_n, uint64_t count, bool coset,
                               const Fr& x, void* q, void* rem, bool on_dev) {
    hipStream_t st = ctx->stream;
    if (!count) return;
    const EvalsPlan plan = evals_plan(log_n, count, evals_lane_points(ctx->policy.evals_lane_points));
    const EvalsPoint<Fr> pt = evals_point<Fr>(log_n, coset, x);
    const size_t bytes = (size_t)count * plan.N * sizeof(Fr), rem_bytes = (size_t)count * sizeof(Fr);
    evals_reserve<Fr>(es, plan, count, !rem || !on_dev);
    if (!on_dev) {
      es.in.ensure(bytes);
      ARK_CHECK_HIP(hipMemcpyAsync(es.in.p, evals, bytes, hipMemcpyHostToDevice, st));
    }
    evals_upload_tables<Fr>(es, plan, pt, st);
    void* d_q = on_dev ? q : es.in.p;
    void* d_rem = on_dev ? rem : es.rem.p;
    evals_div_run<Curve>(on_dev ? evals : es.in.p, count, plan, pt, d_q, d_rem, es, st);
    if (!on_dev) {
      ARK_CHECK_HIP(hipMemcpyAsync(q, d_q, bytes, hipMemcpyDeviceToHost, st));
      if (rem) ARK_CHECK_HIP(hipMemcpyAsync(rem, d_rem, rem_bytes, hipMemcpyDeviceToHost, st));
    }
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }
  // d_out[k][i] = (M_k z)_i for i < n and zero for n <= i < N = 2^q.log_domain: the values of m_k over H_N, matrix-major
  static void gr1cs_mat_vec_dev(ark355_ctx* ctx, const Gr1csDev& g, uint32_t p, const QuotientDims& q, const void* d_z, void* d_out) {
    hipStream_t st = ctx->stream;
    const Gr1csPred& P = g.preds[p];
    if (!P.arity) return;
    const uint64_t N = 1ull << q.log_domain;
    ARK_LAUNCH((gr1cs_spmv_padded_kernel<Fr>), dim3((uint32_t)((N + 255) / 256), P.arity), dim3(256), 0, st,
               (const Gr1csMat*)P.mats.template as<Gr1csMat>(), (const Fr*)g.pool.template as<Fr>(), (const Fr*)d_z, P.n, N, N, (Fr*)d_out);
    ARK_CHECK_LAUNCH();
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // ---- multilinear extensions (mle_impl.cuh): the refusals are capi.hip's; every allocation happens before the first launch
  // out[i] = eq(pt, i), 2^v Fr; pt: v Montgomery elements on the host
  static void mle_eq(ark355_ctx* ctx, MleScratch& ms, uint32_t v, const Fr* pt, void* out, bool on_dev) {
    hipStream_t st = ctx->stream;
    const size_t bytes = sizeof(Fr) << v;
    ms.pt.ensure((size_t)(2 * v + 2) * sizeof(Fr));
    if (!on_dev) ms.out.ensure(bytes);
    Fr* d_out = on_dev ? (Fr*)out : ms.out.template as<Fr>();
    mle_eq_run<Fr>(v, pt, d_out, ms, st);
    if (!on_dev) ARK_CHECK_HIP(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }
  // variables 0 .. k-1 of `count` tables of 2^v fixed to pt[0 .. k): count x 2^(v-k) Fr; k = v is eval
  static void mle_fix(ark355_ctx* ctx, MleScratch& ms, const void* evals, uint32_t v, uint64_t count, const Fr* pt, uint32_t k, void* out,
                      bool on_dev) {
    hipStream_t st = ctx->stream;
    if (!count) return;
    const size_t bytes = (size_t)(count << v) * sizeof(Fr), out_bytes = (size_t)(count << (v - k)) * sizeof(Fr);
    mle_fix_reserve<Fr>(ms, v, count, k);
    if (!on_dev) {
      ms.in.ensure(bytes);
      ms.out.ensure(out_bytes);
      ARK_CHECK_HIP(hipMemcpyAsync(ms.in.p, evals, bytes, hipMemcpyHostToDevice, st));
    }
    Fr* d_out = on_dev ? (Fr*)out : ms.out.template as<Fr>();
    mle_fix_run<Fr>(on_dev ? (const Fr*)evals : (const Fr*)ms.in.template as<Fr>(), v, count, pt, k, d_out, ms,
                    sumcheck_lane_pairs(ctx->policy.sumcheck_lane_pairs), st);
    if (!on_dev) ARK_CHECK_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // ---- multilinear openings (mle_open_impl.cuh).  Declared here and defined behind the struct: a member defined in the class is
  // inline, and capi.hip -- which only declares the explicit instantiations -- would compile its kernels a second time
  // the quotient tables of `count` tables of 2^v at pt: count x 2^v Fr at q, the count values at rem (may be nullptr)
  static void mle_quotients(ark355_ctx* ctx, MleScratch& ms, const void* evals, uint32_t v, uint64_t count, const Fr* pt, void* q, void* rem,
                            bool on_dev);
  // the PST opening of one table in device memory: the quotients into the context's scratch, then one MSM a level against
  // bases[j] (msm_generic, Montgomery scalars); v affine points at proofs, the value at value_out
  static void mle_open_dev(ark355_ctx* ctx, MleScratch& ms, MsmBatchScratch& bs, GenericScratch& g, const BasesDev* const* bases,
                           const void* d_evals, uint32_t v, const Fr* pt, uint8_t* proofs, uint8_t* value_out);

  // ---- batched short MSMs (msm_batch_impl.cuh); declared here and defined behind the struct for the same reason
  // `count` independent MSMs over handles of ONE group: out[s] = sum_{i < n[s]} scalars_s[i] bases[s][i], affine, back to back.
  // Segments of 1 .. MSM_BATCH_SMALL_MAX scalars leave as one batch, the others run through msm_dev one after another.
  static void msm_batch_dev(ark355_ctx* ctx, MsmBatchScratch& bs, GenericScratch& g, const BasesDev* const* bases, const void* const* d_scalars,
                            const uint64_t* n, uint64_t count, int mont, uint8_t* out);
  template <class F>
  static void msm_batch_t(ark355_ctx* ctx, MsmBatchScratch& bs, GenericScratch& g, const BasesDev* const* bases, const void* const* d_scalars,
                          const uint64_t* n, uint64_t count, int mont, uint8_t* out);

  // ---- sum-check of a predicate (sumcheck_impl.cuh): the order of the calls is checked by capi.hip
  static SumcheckDev* sumcheck_begin(ark355_ctx* ctx, const Gr1csDev& g, uint32_t p, const void* d_tables, const void* d_weight,
                                     uint32_t num_vars) {
    return ark355::sumcheck_begin<Curve>(ctx->device, g, p, d_tables, d_weight, num_vars);
  }
  static void sumcheck_round(ark355_ctx* ctx, SumcheckDev& sc, const Fr& r, void* out) {
    ark355::sumcheck_round<Curve>(sc, r, sumcheck_lane_pairs(ctx->policy.sumcheck_lane_pairs), out, ctx->stream);
  }
  static void sumcheck_finish(ark355_ctx* ctx, SumcheckDev& sc, const Fr& r, void* out) {
    ark355::sumcheck_finish<Curve>(sc, r, out, ctx->stream);
  }

  static void ntt_host(ark355_ctx* ctx, GenericScratch& g, uint8_t* data, uint32_t log_n, bool inverse, bool coset) {
    hipStream_t st = ctx->stream;
    const size_t bytes = sizeof(Fr) << log_n;
    g.a.ensure(bytes);
    g.b.ensure(bytes);
    ARK_CHECK_HIP(hipMemcpyAsync(g.a.p, data, bytes, hipMemcpyHostToDevice, st));
    void* res = ntt_run<Curve>(ctx, g.a.p, g.b.p, log_n, inverse, coset, st);
    ARK_CHECK_HIP(hipMemcpyAsync(data, res, bytes, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  static void ntt_dev(ark355_ctx* ctx, void* d_data, void* d_scratch, uint32_t log_n, bool inverse, bool coset,
                      hipStream_t st) {
    const size_t bytes = sizeof(Fr) << log_n;
    void* res = ntt_run<Curve>(ctx, d_data, d_scratch, log_n, inverse, coset, st);
    if (res != d_data) ARK_CHECK_HIP(hipMemcpyAsync(d_data, res, bytes, hipMemcpyDeviceToDevice, st));
  }

  // d_rows: 28-bit rows in the format `packed`; tab: the window tables they are, nullptr for the re-encoded bases of a one-shot
  // MSM (msm_plan without tables: every window its own bucket set)
  template <class F>
  static void msm_generic(ark355_ctx* ctx, GenericScratch& g, const void* d_rows, bool packed, const void* d_scalars,
                          uint64_t n, int mont, uint8_t* out, bool want_affine, const PrecompTable* tab = nullptr) {
    hipStream_t st = ctx->stream;
    hipEvent_t e0, e1;
    ARK_CHECK_HIP(hipEventCreate(&e0));
    ARK_CHECK_HIP(hipEventCreate(&e1));
    try {
      msm_sort<Fr>(ctx, g.sort, d_scalars, n, mont, st, tab);
      // what the tails leave on the device: c partial sums per bucket set
      const uint32_t parts = msm_parts_count(g.sort.plan);
      g.c.ensure((size_t)parts * sizeof(XYZZ<F>));
      XYZZ<F>* d_res = g.c.as<XYZZ<F>>();
      msm_accumulate_phase<F>(ctx, g.sort, g.bk, d_rows, packed, st, 0, n ? e0 : nullptr, n ? e1 : nullptr);
      msm_reduce_phase<F>(ctx, g.sort, g.bk, d_res, st);
      // The last 2c group operations per bucket set (Horner over the bit sums) and the one inversion of the normalisation run
      // in the library's host-compiled field code: ~1 us per group operation against ~12 us for a device lane, tens of
      // microseconds for the inversion against ~1 ms.
      std::vector<XYZZ<F>> h_parts(parts);
      ARK_CHECK_HIP(hipMemcpyAsync(h_parts.data(), d_res, (size_t)parts * sizeof(XYZZ<F>), hipMemcpyDeviceToHost, st));
      ARK_CHECK_HIP(hipStreamSynchronize(st));
      const XYZZ<F> h_res = msm_parts_finish<F>(h_parts.data(), g.sort.plan);
      if (want_affine) {
        const Affine<F> a = xyzz_to_affine(h_res);
        memcpy(out, &a, sizeof(a));
      } else {
        memcpy(out, &h_res, sizeof(h_res));
      }
      float ms = 0;
      if (n) (void)hipEventElapsedTime(&ms, e0, e1);
      ctx->acc_ms = ms;
      ctx->acc_launches = n ? 1 : 0;
      ctx->acc_points = (uint64_t)g.sort.plan.windows * n;
    } catch (...) {
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }

  // One-shot MSM over the caller's bases: uploaded and re-encoded to 28-bit rows in the format a key of this curve gets
  // (table_pack_default), then the accumulation and tails of the resident keys over the plan without tables.
  template <class F>
  static void msm_host_t(ark355_ctx* ctx, GenericScratch& g, const uint8_t* bases, const uint8_t* scalars, uint64_t n,
                         uint8_t* out) {
    hipStream_t st = ctx->stream;
    const bool pack = table_pack_default<Fq>(ctx->policy);
    g.a.ensure(n * sizeof(Affine<F>));
    g.b.ensure(n * sizeof(Fr));
    g.rows.ensure(n * table_row_bytes<F>(pack));
    if (n) {
      ARK_CHECK_HIP(hipMemcpyAsync(g.a.p, bases, n * sizeof(Affine<F>), hipMemcpyHostToDevice, st));
      ARK_CHECK_HIP(hipMemcpyAsync(g.b.p, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, st));
      rows_to28<F>(g.a.as<Affine<F>>(), g.rows.p, n, pack, st);
    }
    msm_generic<F>(ctx, g, g.rows.p, pack, g.b.p, n, 0, out, true);
  }

  static void msm_host(ark355_ctx* ctx, GenericScratch& g, int group, const uint8_t* bases, const uint8_t* scalars,
                       uint64_t n, uint8_t* out) {
    if (group == 1) msm_host_t<Fq>(ctx, g, bases, scalars, n, out);
    else msm_host_t<Fq2>(ctx, g, bases, scalars, n, out);
  }

  static BasesDev* bases_load(const TunePolicy& pol, int group, const uint8_t* bases, uint64_t n, hipStream_t st) {
    auto* b = new BasesDev();
    try {
      b->curve = Curve::ID;
      b->group = group;
      b->n = n;
      const size_t psz = group == 1 ? sizeof(Affine<Fq>) : sizeof(Affine<Fq2>);
      DevBuf stage((n ? n : 1) * psz);
      if (n) ARK_CHECK_HIP(hipMemcpy(stage.p, bases, n * psz, hipMemcpyHostToDevice));
      const TableNeed need{n, 0, group == 2};
      std::string why;
      bool packed = false;
      const uint32_t ws = table_stride_plan<Fq, Fq2, Fr>(pol, &need, 1, table_budget_bytes(pol, (size_t)2 * 16 * 17 * n, true), &why, &packed);
      if (ws == 0) throw HipError{ARK355_ENOMEM, "base set: " + why};
      if (group == 1) precomp_build<Fq, Fr>(pol, b->tab, stage.p, n, st, 0, ws, 0, packed ? 1 : 0);
      else precomp_build<Fq2, Fr>(pol, b->tab, stage.p, n, st, 0, ws, 0, packed ? 1 : 0);
    } catch (...) {
      delete b;
      throw;
    }
    return b;
  }

  static void msm_dev(ark355_ctx* ctx, GenericScratch& g, const BasesDev& b, const void* d_scalars, uint64_t n, int mont,
                      uint8_t* out, bool want_affine) {
    ARK_REQUIRE(n <= b.n, ARK355_EINVAL, "more scalars than bases");
    if (b.group == 1) msm_generic<Fq>(ctx, g, b.tab.table.p, b.tab.packed, d_scalars, n, mont, out, want_affine, &b.tab);
    else msm_generic<Fq2>(ctx, g, b.tab.table.p, b.tab.packed, d_scalars, n, mont, out, want_affine, &b.tab);
  }

  // ark355_diag_msm_sort: the sort stage of an MSM on its own -- the scalars go up, msm_sort_plan / msm_sort_run (the very
  // functions every MSM and proof calls) run on the context's stream over its scratch, and everything the sort leaves on the
  // device comes back.  b == nullptr: the plan of a one-shot MSM.  plan and *total are written before a capacity is refused.
  static void diag_msm_sort(ark355_ctx* ctx, GenericScratch& g, const BasesDev* b, const uint8_t* scalars, uint64_t n, int mont,
                            uint32_t* plan, uint32_t* counts, uint32_t* offsets, uint64_t bucket_capacity, uint32_t* sorted_keys,
                            uint32_t* sorted_vals, uint64_t entry_capacity, uint32_t* total) {
    hipStream_t st = ctx->stream;
    if (b) ARK_REQUIRE(b->curve == Curve::ID, ARK355_EINVAL, "sort diagnostic: the base set belongs to another curve");
    ARK_REQUIRE((counts == nullptr) == (offsets == nullptr) && (sorted_keys == nullptr) == (sorted_vals == nullptr), ARK355_EINVAL,
                "sort diagnostic: counts / offsets and sorted_keys / sorted_vals come in pairs");
    const PrecompTable* tab = b ? &b->tab : nullptr;
    g.b.ensure(n * sizeof(Fr));
    if (n) ARK_CHECK_HIP(hipMemcpyAsync(g.b.p, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, st));
    msm_sort_plan<Fr>(ctx, g.sort, n, st, tab);
    msm_sort_run<Fr>(ctx, g.sort, g.b.p, n, mont, st, tab);
    const MsmPlan& p = g.sort.plan;
    uint32_t tot = 0;
    ARK_CHECK_HIP(hipMemcpyAsync(&tot, g.sort.total.p, 4, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    plan[0] = p.c;
    plan[1] = p.windows;
    plan[2] = p.wstride;
    plan[3] = p.key_windows;
    plan[4] = p.total_buckets;
    plan[5] = p.negate_high ? 1u : 0u;
    plan[6] = tab ? (uint32_t)tab->n : 0u;
    plan[7] = msm_sort_one_pass(p) ? 1u : 0u;
    *total = tot;
    ARK_REQUIRE((uint64_t)tot <= (uint64_t)p.windows * n, ARK355_EINVAL, "sort diagnostic: more entries than digits");
    if (counts) {
      ARK_REQUIRE(bucket_capacity >= p.total_buckets, ARK355_EINVAL, "sort diagnostic: bucket_capacity below the plan's buckets");
      ARK_CHECK_HIP(hipMemcpy(counts, g.sort.counts.p, (size_t)p.total_buckets * 4, hipMemcpyDeviceToHost));
      ARK_CHECK_HIP(hipMemcpy(offsets, g.sort.offsets.p, (size_t)p.total_buckets * 4, hipMemcpyDeviceToHost));
    }
    if (sorted_keys) {
      ARK_REQUIRE(entry_capacity >= tot, ARK355_EINVAL, "sort diagnostic: entry_capacity below the number of entries");
      if (tot) {
        ARK_CHECK_HIP(hipMemcpy(sorted_keys, g.sort.sorted_keys.p, (size_t)tot * 4, hipMemcpyDeviceToHost));
        ARK_CHECK_HIP(hipMemcpy(sorted_vals, g.sort.sorted_vals.p, (size_t)tot * 4, hipMemcpyDeviceToHost));
      }
    }
  }

  template <class F>
  static void xyzz_sum_t(ark355_ctx* ctx, GenericScratch& g, const uint8_t* partials, uint64_t count, uint8_t* out) {
    hipStream_t st = ctx->stream;
    g.a.ensure(count * sizeof(XYZZ<F>) + sizeof(XYZZ<F>) + sizeof(Affine<F>));
    XYZZ<F>* d_in = g.a.as<XYZZ<F>>();
    XYZZ<F>* d_sum = d_in + count;
    if (count) ARK_CHECK_HIP(hipMemcpyAsync(d_in, partials, count * sizeof(XYZZ<F>), hipMemcpyHostToDevice, st));
    ARK_LAUNCH((xyzz_sum_kernel<F>), dim3(1), dim3(64), 0, st, (const XYZZ<F>*)d_in, (uint32_t)count, d_sum);
    ARK_CHECK_LAUNCH();
    XYZZ<F> h_sum;
    ARK_CHECK_HIP(hipMemcpyAsync(&h_sum, d_sum, sizeof(XYZZ<F>), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    const Affine<F> a = xyzz_to_affine(h_sum);      // host-side normalisation (see msm_generic)
    memcpy(out, &a, sizeof(a));
  }

  static void xyzz_sum(ark355_ctx* ctx, GenericScratch& g, int group, const uint8_t* partials, uint64_t count,
                       uint8_t* out) {
    if (group == 1) xyzz_sum_t<Fq>(ctx, g, partials, count, out);
    else xyzz_sum_t<Fq2>(ctx, g, partials, count, out);
  }

  // The affine window table of `d_base` (FB_WINDOWS x FB_ROW rows) on `st`; d_tx is scratch of as many XYZZ rows.
  template <class F>
  static void fixed_base_table(const Affine<F>* d_base, XYZZ<F>* d_tx, Affine<F>* d_ta, hipStream_t st) {
    static_assert(Fr::N * 4 == FB_WINDOWS, "one 8-bit window per scalar byte");
    const uint32_t rows = FB_WINDOWS * FB_ROW;
    ARK_LAUNCH((fixed_base_table_kernel<F>), dim3(FB_WINDOWS), dim3(256), 0, st, d_base, d_tx);
    ARK_CHECK_LAUNCH();
    ARK_LAUNCH((batch_to_affine_kernel<F>), dim3(((rows + PRE_K - 1) / PRE_K + MSM_THREADS - 1) / MSM_THREADS),
               dim3(MSM_THREADS), 0, st, (const XYZZ<F>*)d_tx, d_ta, rows);
    ARK_CHECK_LAUNCH();
  }
  // d_out[i] = d_scalars[i] * base for n resident canonical scalars: through the table when there is one (d_ta), else one
  // double-and-add per lane.  d_xyzz: scratch of n XYZZ points.
  template <class F>
  static void fixed_base_mul_dev(const Affine<F>* d_base, const Affine<F>* d_ta, const Fr* d_scalars, uint64_t n,
                                 XYZZ<F>* d_xyzz, Affine<F>* d_out, hipStream_t st) {
    if (!n) return;
    ARK_REQUIRE(n < (1ull << 32), ARK355_EINVAL, "too many scalars");
    if (d_ta) {
      ARK_LAUNCH((fixed_base_mul_kernel<F, Fr>), dim3((uint32_t)((n + 127) / 128)), dim3(128), 0, st, d_ta, d_scalars, n, d_xyzz);
    } else {
      ARK_LAUNCH((fixed_base_small_kernel<F, Fr>), dim3((uint32_t)((n + 127) / 128)), dim3(128), 0, st, d_base, d_scalars, n, d_xyzz);
    }
    ARK_CHECK_LAUNCH();
    ARK_LAUNCH((batch_to_affine_kernel<F>), dim3((uint32_t)(((n + PRE_K - 1) / PRE_K + MSM_THREADS - 1) / MSM_THREADS)),
               dim3(MSM_THREADS), 0, st, (const XYZZ<F>*)d_xyzz, d_out, (uint32_t)n);
    ARK_CHECK_LAUNCH();
  }
  // a handful of scalars go without the table: building its 8 160 points would cost more than it saves
  static constexpr uint64_t FB_TABLE_MIN = 512;

  // scalars: n canonical values on the host, or (on_dev) n values in device memory, Montgomery images when mont
  template <class F>
  static void fixed_base_t(ark355_ctx* ctx, GenericScratch& g, const uint8_t* base, const void* scalars, uint64_t n,
                           uint8_t* out, bool on_dev = false, bool mont = false) {
    hipStream_t st = ctx->stream;
    const uint32_t rows = FB_WINDOWS * FB_ROW;
    DevBuf d_base(sizeof(Affine<F>)), d_tx((size_t)rows * sizeof(XYZZ<F>)), d_ta((size_t)rows * sizeof(Affine<F>));
    if (!on_dev || mont) g.b.ensure(n * sizeof(Fr));
    g.a.ensure((n ? n : 1) * sizeof(XYZZ<F>));
    g.c.ensure((n ? n : 1) * sizeof(Affine<F>));
    ARK_CHECK_HIP(hipMemcpyAsync(d_base.p, base, sizeof(Affine<F>), hipMemcpyHostToDevice, st));
    if (n) {
      ARK_REQUIRE(n < (1ull << 32), ARK355_EINVAL, "too many scalars");
      const Fr* d_k = g.b.as<Fr>();
      if (!on_dev) {
        ARK_CHECK_HIP(hipMemcpyAsync(g.b.p, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, st));
      } else if (mont) {
        ARK_LAUNCH((fr_from_mont_kernel<Fr>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, (const Fr*)scalars, n, g.b.as<Fr>());
        ARK_CHECK_LAUNCH();
      } else {
        d_k = (const Fr*)scalars;
      }
      const bool table = n >= FB_TABLE_MIN;
      if (table) fixed_base_table<F>(d_base.as<Affine<F>>(), d_tx.as<XYZZ<F>>(), d_ta.as<Affine<F>>(), st);
      fixed_base_mul_dev<F>(d_base.as<Affine<F>>(), table ? d_ta.as<Affine<F>>() : nullptr, d_k, n, g.a.as<XYZZ<F>>(),
                            g.c.as<Affine<F>>(), st);
      ARK_CHECK_HIP(hipMemcpyAsync(out, g.c.p, n * sizeof(Affine<F>), hipMemcpyDeviceToHost, st));
    }
    ARK_CHECK_HIP(hipStreamSynchronize(st));       // the table buffers are freed on return
  }

  static void fixed_base(ark355_ctx* ctx, GenericScratch& g, int group, const uint8_t* base, const uint8_t* scalars,
                         uint64_t n, uint8_t* out) {
    if (group == 1) fixed_base_t<Fq>(ctx, g, base, scalars, n, out);
    else fixed_base_t<Fq2>(ctx, g, base, scalars, n, out);
  }
  static void fixed_base_dev(ark355_ctx* ctx, GenericScratch& g, int group, const uint8_t* base, const void* d_scalars, uint64_t n,
                             bool mont, uint8_t* out) {
    if (group == 1) fixed_base_t<Fq>(ctx, g, base, d_scalars, n, out, true, mont);
    else fixed_base_t<Fq2>(ctx, g, base, d_scalars, n, out, true, mont);
  }

  // ---- Groth16 generator scalars on the host (the library's own field code, std::thread) ------------------------------
  // Upstream `generate_parameters_with_qap` / `R1CSToQAP::instance_map_with_evaluation` (SURVEY.md Appendix A "Setup"):
  //   L_k(tau) = Z(tau)/N * w^k / (tau - w^k);  u_j = sum_k L_k A[k][j] (+ L_{n+j} for j < ell), v_j, w_j likewise;
  //   l_j = (beta u_j + alpha v_j + w_j) / delta (witness columns), gamma_abc_j = (...) / gamma (instance columns),
  //   h_i = Z(tau) tau^i / delta.  All outputs canonical 32-byte little-endian; the fixed-base multiplications that turn
  // them into the key's query vectors are ark355_fixed_base_mul's job.
  static void setup_scalars(uint64_t n, uint64_t ell, uint64_t w, const uint64_t* const rp[3], const uint32_t* const col[3],
                            const uint8_t* const coeff[3], const uint8_t* trapdoor, uint8_t* out_u, uint8_t* out_v,
                            uint8_t* out_w, uint8_t* out_l, uint8_t* out_gabc, uint8_t* out_h) {
    using P = typename Fr::Params;
    ARK_REQUIRE(ell >= 1, ARK355_EINVAL, "num_instance must include the constant One");
    const uint64_t m = ell + w;
    // the three CSR matrices come from the caller: monotone row pointers, columns inside [0, ell + w)
    for (int k = 0; k < 3; k++) {
      ARK_REQUIRE(rp[k][0] == 0, ARK355_EINVAL, "CSR row_ptr must start at 0");
      for (uint64_t i = 0; i < n; i++) ARK_REQUIRE(rp[k][i] <= rp[k][i + 1], ARK355_EINVAL, "CSR row_ptr is not monotone");
      const uint64_t nnz = rp[k][n];
      for (uint64_t t = 0; t < nnz; t++) ARK_REQUIRE(col[k][t] < m, ARK355_EINVAL, "CSR column index out of range");
    }
    uint32_t lg = 0;
    while ((1ull << lg) < n + ell) lg++;
    ARK_REQUIRE(lg <= (uint32_t)P::TWO_ADICITY, ARK355_E_POLY_DEGREE_TOO_LARGE, "n + ell exceeds the largest radix-2 domain of Fr");
    const uint64_t N = 1ull << lg;
    Fr td[5];
    for (int i = 0; i < 5; i++) {
      Fr c;
      memcpy(c.l, trapdoor + 32 * i, sizeof(Fr));
      td[i] = Fr::to_mont(c);
    }
    const Fr tau = td[0], alpha = td[1], beta = td[2], gamma = td[3], delta = td[4];
    const Fr omega = ntt_root<Fr>(lg, false);
    const Fr zt = Fr::sub(fr_pow_u64(tau, N), Fr::one());
    // tau inside the evaluation domain (Z(tau) = 0; probability N / r for an honest trapdoor, but a legal input): the
    // Lagrange coefficients degenerate to an indicator, L_k(tau) = [w^k == tau], as `evaluate_all_lagrange_coefficients`
    // upstream returns them; h_i = Z(tau) tau^i / delta = 0.
    const bool tau_in_domain = zt.is_zero();
    Fr nn = Fr::zero();
    nn.l[0] = (uint32_t)N;
    nn.l[1] = (uint32_t)(N >> 32);
    const Fr cN = Fr::mul(zt, Fr::inv(Fr::to_mont(nn)));
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 4;
    if (nt > 32) nt = 32;
    auto parallel = [&](uint64_t count, const std::function<void(uint64_t, uint64_t)>& fn) {
      const uint64_t chunk = (count + nt - 1) / nt;
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nt; t++) {
        const uint64_t a = t * chunk, b = std::min<uint64_t>(count, a + chunk);
        if (a < b) th.emplace_back(fn, a, b);
      }
      for (auto& x : th) x.join();
    };
    std::vector<Fr> L(N), wk(N);
    if (tau_in_domain) {
      parallel(N, [&](uint64_t a, uint64_t b) {
        Fr p = fr_pow_u64(omega, a);
        for (uint64_t k = a; k < b; k++) {
          L[k] = (p == tau) ? Fr::one() : Fr::zero();
          p = Fr::mul(p, omega);
        }
      });
    } else
    parallel(N, [&](uint64_t a, uint64_t b) {
      Fr p = fr_pow_u64(omega, a), acc = Fr::one();
      for (uint64_t k = a; k < b; k++) {            // prefix products of the denominators of this chunk
        wk[k] = p;
        acc = Fr::mul(acc, Fr::sub(tau, p));
        L[k] = acc;
        p = Fr::mul(p, omega);
      }
      Fr inv = Fr::inv(acc);
      for (uint64_t k = b; k-- > a;) {
        const Fr iv = k > a ? Fr::mul(inv, L[k - 1]) : inv;
        inv = Fr::mul(inv, Fr::sub(tau, wk[k]));
        L[k] = Fr::mul(Fr::mul(iv, wk[k]), cN);
      }
    });
    std::vector<Fr> uvw[3];
    for (auto& x : uvw) x.assign(m, Fr::zero());
    for (uint64_t i = 0; i < ell; i++) uvw[0][i] = L[n + i];
    {
      const Fr one = Fr::one();
      std::vector<std::thread> th;
      for (int k = 0; k < 3; k++)
        th.emplace_back([&, k] {
          for (uint64_t i = 0; i < n; i++)
            for (uint64_t t = rp[k][i]; t < rp[k][i + 1]; t++) {
              Fr c;
              memcpy(c.l, coeff[k] + t * sizeof(Fr), sizeof(Fr));
              Fr& dst = uvw[k][col[k][t]];
              dst = Fr::add(dst, c == one ? L[i] : Fr::mul(L[i], c));
            }
        });
      for (auto& x : th) x.join();
    }
    const Fr gi = Fr::inv(gamma), di = Fr::inv(delta);
    auto put = [](uint8_t* dst, uint64_t i, const Fr& mont) {
      const Fr c = Fr::from_mont(mont);
      memcpy(dst + 32 * i, c.l, sizeof(Fr));
    };
    parallel(m, [&](uint64_t a, uint64_t b) {
      for (uint64_t i = a; i < b; i++) {
        const Fr abc = Fr::add(Fr::add(Fr::mul(beta, uvw[0][i]), Fr::mul(alpha, uvw[1][i])), uvw[2][i]);
        if (i < ell) put(out_gabc, i, Fr::mul(abc, gi));
        else put(out_l, i - ell, Fr::mul(abc, di));
        put(out_u, i, uvw[0][i]);
        put(out_v, i, uvw[1][i]);
        put(out_w, i, uvw[2][i]);
      }
    });
    const Fr h0 = Fr::mul(zt, di);
    parallel(N - 1, [&](uint64_t a, uint64_t b) {
      Fr p = Fr::mul(fr_pow_u64(tau, a), h0);
      for (uint64_t i = a; i < b; i++) {
        put(out_h, i, p);
        p = Fr::mul(p, tau);
      }
    });
  }

  // ---- Groth16 generator on the device (ark355_setup) ------------------------------------------------------------------
  // The scalar stages are setup_impl.cuh; here: argument checks, one window table per group and per call, a fixed-base
  // multiplication per requested vector from the resident canonical scalars (v feeds b_g1_query and b_g2_query), and the
  // hand-over of the device vectors to pk_upload (the pk_load_bytes pattern).  Returns nullptr when want_pk is false.
  static bool fr_canonical(const Fr& c) {
    for (int i = Fr::N - 1; i >= 0; i--) {
      const uint32_t q = Fr::Params::mod(i);
      if (c.l[i] < q) return true;
      if (c.l[i] > q) return false;
    }
    return false;
  }
  static bool base_on_curve(const Affine<Fq>& p) {
    return W::is_reduced(p.x) && W::is_reduced(p.y) && Fq::sqr(p.y) == W::curve_rhs(p.x);
  }
  static bool base_on_curve(const Affine<Fq2>& p) {
    return W::is_reduced(p.x.c0) && W::is_reduced(p.x.c1) && W::is_reduced(p.y.c0) && W::is_reduced(p.y.c1) &&
           Fq2::sqr(p.y) == W::curve_rhs(p.x);
  }

  // One group's share of a setup call: the base, its window table (when the call multiplies out FB_TABLE_MIN scalars or
  // more in this group) and the XYZZ scratch of the longest vector.
  template <class F>
  struct SetupGroup {
    DevBuf base, table, xyzz;
    bool has_table = false;
    hipStream_t st = nullptr;
    void init(const Affine<F>& h_base, uint64_t total, uint64_t longest, hipStream_t stream) {
      st = stream;
      base.alloc(sizeof(Affine<F>));
      ARK_CHECK_HIP(hipMemcpyAsync(base.p, &h_base, sizeof(Affine<F>), hipMemcpyHostToDevice, st));
      xyzz.alloc((longest ? longest : 1) * sizeof(XYZZ<F>));
      has_table = total >= FB_TABLE_MIN;
      if (has_table) {
        const uint32_t rows = FB_WINDOWS * FB_ROW;
        DevBuf tx((size_t)rows * sizeof(XYZZ<F>));
        table.alloc((size_t)rows * sizeof(Affine<F>));
        fixed_base_table<F>(base.as<Affine<F>>(), tx.as<XYZZ<F>>(), table.as<Affine<F>>(), st);
        ARK_CHECK_HIP(hipStreamSynchronize(st));          // tx is freed here
      }
    }
    void mul(const DevBuf& scalars, uint64_t n, DevBuf& out) {
      out.alloc((n ? n : 1) * sizeof(Affine<F>));
      fixed_base_mul_dev<F>(base.as<Affine<F>>(), has_table ? table.as<Affine<F>>() : nullptr, scalars.as<Fr>(), n,
                            xyzz.as<XYZZ<F>>(), out.as<Affine<F>>(), st);
    }
  };

  static PkDev* setup(ark355_ctx* ctx, const R1csDev& r1, const uint8_t* g1_base, const uint8_t* g2_base,
                      const uint8_t* trapdoor, const ark355_setup_out* out, bool want_pk) {
    ARK_REQUIRE(r1.curve == Curve::ID, ARK355_EINVAL, "curve mismatch");
    hipStream_t st = ctx->stream;
    static const char* const td_name[5] = {"tau", "alpha", "beta", "gamma", "delta"};
    Fr tdc[5], td[5];
    for (int i = 0; i < 5; i++) {
      memcpy(tdc[i].l, trapdoor + 32 * i, sizeof(Fr));
      if (!fr_canonical(tdc[i])) throw HipError{ARK355_EINVAL, std::string("trapdoor element ") + td_name[i] + " is not below r"};
      td[i] = Fr::to_mont(tdc[i]);
    }
    ARK_REQUIRE(!td[3].is_zero(), ARK355_EINVAL, "trapdoor element gamma is zero: it has no inverse");
    ARK_REQUIRE(!td[4].is_zero(), ARK355_EINVAL, "trapdoor element delta is zero: it has no inverse");
    Affine<Fq> b1;
    Affine<Fq2> b2;
    memcpy(&b1, g1_base, sizeof(b1));
    memcpy(&b2, g2_base, sizeof(b2));
    ARK_REQUIRE(base_on_curve(b1), ARK355_EINVAL, "g1_base is not a point of the G1 curve");
    ARK_REQUIRE(base_on_curve(b2), ARK355_EINVAL, "g2_base is not a point of the G2 curve");

    static const ark355_setup_out none{};
    const ark355_setup_out& o = out ? *out : none;
    const uint64_t ell = r1.ell, w = r1.w, m = r1.m, hn = r1.N - 1;
    // work nobody asked for is skipped
    const bool need_a = want_pk || o.a_query, need_b1 = want_pk || o.b_g1_query, need_b2 = want_pk || o.b_g2_query;
    const bool need_h = want_pk || o.h_query, need_l = want_pk || o.l_query, need_gabc = o.gamma_abc_g1 != nullptr;
    const bool need_s1 = want_pk || o.alpha_g1 || o.beta_g1 || o.delta_g1;
    const bool need_s2 = want_pk || o.beta_g2 || o.gamma_g2 || o.delta_g2;

    SetupScalarsDev sc;
    setup_scalars_dev<Curve>(r1, td, need_h, sc, st);
    if (o.u) ARK_CHECK_HIP(hipMemcpyAsync(o.u, sc.u.p, m * sizeof(Fr), hipMemcpyDeviceToHost, st));
    if (o.v) ARK_CHECK_HIP(hipMemcpyAsync(o.v, sc.v.p, m * sizeof(Fr), hipMemcpyDeviceToHost, st));
    if (o.w) ARK_CHECK_HIP(hipMemcpyAsync(o.w, sc.w.p, m * sizeof(Fr), hipMemcpyDeviceToHost, st));

    DevBuf d_a, d_b1, d_b2, d_h, d_l, d_gabc, d_s1, d_s2;
    Affine<Fq> h_s1[3] = {};           // alpha, beta, delta
    Affine<Fq2> h_s2[3] = {};          // beta, gamma, delta
    const uint64_t total1 = (need_a ? m : 0) + (need_b1 ? m : 0) + (need_h ? hn : 0) + (need_l ? w : 0) + (need_gabc ? ell : 0) +
                            (need_s1 ? 3 : 0);
    if (total1) {
      SetupGroup<Fq> g;
      g.init(b1, total1, std::max<uint64_t>(std::max(m, hn), 3), st);
      if (need_a) g.mul(sc.u, m, d_a);
      if (need_b1) g.mul(sc.v, m, d_b1);
      if (need_h) g.mul(sc.h, hn, d_h);
      if (need_l) g.mul(sc.l, w, d_l);
      if (need_gabc) g.mul(sc.gabc, ell, d_gabc);
      if (need_s1) {
        const Fr ks[3] = {tdc[1], tdc[2], tdc[4]};
        DevBuf d_ks(sizeof(ks));
        ARK_CHECK_HIP(hipMemcpyAsync(d_ks.p, ks, sizeof(ks), hipMemcpyHostToDevice, st));
        g.mul(d_ks, 3, d_s1);
        ARK_CHECK_HIP(hipMemcpyAsync(h_s1, d_s1.p, sizeof(h_s1), hipMemcpyDeviceToHost, st));
        ARK_CHECK_HIP(hipStreamSynchronize(st));          // ks and d_ks go out of scope
      }
      ARK_CHECK_HIP(hipStreamSynchronize(st));            // the group's table and scratch are freed here
    }
    const uint64_t total2 = (need_b2 ? m : 0) + (need_s2 ? 3 : 0);
    if (total2) {
      SetupGroup<Fq2> g;
      g.init(b2, total2, std::max<uint64_t>(need_b2 ? m : 0, 3), st);
      if (need_b2) g.mul(sc.v, m, d_b2);
      if (need_s2) {
        const Fr ks[3] = {tdc[2], tdc[3], tdc[4]};
        DevBuf d_ks(sizeof(ks));
        ARK_CHECK_HIP(hipMemcpyAsync(d_ks.p, ks, sizeof(ks), hipMemcpyHostToDevice, st));
        g.mul(d_ks, 3, d_s2);
        ARK_CHECK_HIP(hipMemcpyAsync(h_s2, d_s2.p, sizeof(h_s2), hipMemcpyDeviceToHost, st));
        ARK_CHECK_HIP(hipStreamSynchronize(st));
      }
      ARK_CHECK_HIP(hipStreamSynchronize(st));
    }
    sc = SetupScalarsDev();                                 // the scalars are multiplied out

    constexpr size_t G1 = sizeof(Affine<Fq>), G2 = sizeof(Affine<Fq2>);
    if (o.alpha_g1) memcpy(o.alpha_g1, &h_s1[0], G1);
    if (o.beta_g1) memcpy(o.beta_g1, &h_s1[1], G1);
    if (o.delta_g1) memcpy(o.delta_g1, &h_s1[2], G1);
    if (o.beta_g2) memcpy(o.beta_g2, &h_s2[0], G2);
    if (o.gamma_g2) memcpy(o.gamma_g2, &h_s2[1], G2);
    if (o.delta_g2) memcpy(o.delta_g2, &h_s2[2], G2);
    // requested vectors: from the staging buffers to the caller's memory
    auto give = [&](uint8_t* dst, const DevBuf& src, size_t bytes) {
      if (dst && bytes) ARK_CHECK_HIP(hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, st));
    };
    give(o.gamma_abc_g1, d_gabc, ell * G1);
    give(o.a_query, d_a, m * G1);
    give(o.b_g1_query, d_b1, m * G1);
    give(o.b_g2_query, d_b2, m * G2);
    give(o.h_query, d_h, hn * G1);
    give(o.l_query, d_l, w * G1);
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    if (!want_pk) return nullptr;
    d_gabc.release();
    ark355_pk_desc d{};
    d.num_instance = ell;
    d.num_witness = w;
    d.domain_size = r1.N;
    d.a_query = d_a.as<uint8_t>();            // device pointers: pk_upload copies with hipMemcpyDefault
    d.b_g1_query = d_b1.as<uint8_t>();
    d.b_g2_query = d_b2.as<uint8_t>();
    d.h_query = d_h.as<uint8_t>();
    d.l_query = d_l.as<uint8_t>();
    d.alpha_g1 = reinterpret_cast<const uint8_t*>(&h_s1[0]);
    d.beta_g1 = reinterpret_cast<const uint8_t*>(&h_s1[1]);
    d.delta_g1 = reinterpret_cast<const uint8_t*>(&h_s1[2]);
    d.beta_g2 = reinterpret_cast<const uint8_t*>(&h_s2[0]);
    d.delta_g2 = reinterpret_cast<const uint8_t*>(&h_s2[2]);
    return pk_upload<Curve>(ctx->policy, &d, st);
  }

  // ---- pairings and verification (verify_impl.cuh) -----------------------------------------------------------------------
  static void multi_pairing(ark355_ctx* ctx, GenericScratch& g, const uint8_t* g1, const uint8_t* g2, uint64_t n, uint8_t* out_gt,
                            int32_t* is_one) {
    Verify<Curve>{ctx, g.pair, g.c}.multi_pairing(g1, g2, n, out_gt, is_one);
  }
  static void pairing_groups(ark355_ctx* ctx, GenericScratch& g, const uint8_t* g1, const uint8_t* g2, uint64_t groups,
                             uint32_t group_len, uint8_t* out_gt, uint8_t* is_one) {
    Verify<Curve>{ctx, g.pair, g.c}.pairing_groups(g1, g2, groups, group_len, out_gt, is_one);
  }
  static void verify_each(ark355_ctx* ctx, GenericScratch& g, const ark355_vk_desc* vk, const ark355_proof_raw* proofs,
                          const uint8_t* inputs, uint64_t count, uint8_t* ok) {
    Verify<Curve>{ctx, g.pair, g.c}.verify_each(vk, proofs, inputs, count, ok);
  }
  static bool verify_batch(ark355_ctx* ctx, GenericScratch& g, const ark355_vk_desc* vk, const ark355_proof_raw* proofs,
                           const uint8_t* inputs, const uint8_t* rho, uint64_t count) {
    return Verify<Curve>{ctx, g.pair, g.c}.verify_batch(
        vk, proofs, inputs, rho, count, [&](const uint8_t* bases, const uint8_t* scalars, uint64_t n, Affine<Fq>* out) {
          msm_host(ctx, g, 1, bases, scalars, n, reinterpret_cast<uint8_t*>(out));
        });
  }

  // ---- the processed verifying key (verify_impl.cuh) -------------------------------------------------------------------
  static PvkDev* vk_process(ark355_ctx* ctx, GenericScratch& g, const ark355_vk_desc* vk) {
    return Verify<Curve>{ctx, g.pair, g.c}.vk_process(vk);
  }
  static void pvk_pairings(ark355_ctx* ctx, GenericScratch& g, const PvkDev& pvk, int which, const uint8_t* g1, uint64_t n,
                           uint8_t* out_gt, uint8_t* is_one) {
    Verify<Curve>{ctx, g.pair, g.c}.pvk_pairings(pvk, which, g1, n, out_gt, is_one);
  }
  static void verify_each_pvk(ark355_ctx* ctx, GenericScratch& g, const PvkDev& pvk, const ark355_proof_raw* proofs,
                              const uint8_t* inputs, uint64_t count, uint8_t* ok) {
    Verify<Curve>{ctx, g.pair, g.c}.verify_each_pvk(pvk, proofs, inputs, count, ok);
  }
  static void verify_each_bytes(ark355_ctx* ctx, GenericScratch& g, const PvkDev& pvk, const uint8_t* proofs, uint64_t count,
                                bool compressed, int validate, const uint8_t* inputs, uint8_t* ok, uint8_t* status) {
    Verify<Curve>{ctx, g.pair, g.c}.verify_each_bytes(pvk, proofs, count, compressed, validate, inputs, ok, status);
  }
  static void proofs_from_bytes(ark355_ctx* ctx, GenericScratch& g, const uint8_t* in, uint64_t count, bool compressed, int validate,
                                ark355_proof_raw* out, uint8_t* status) {
    Verify<Curve>{ctx, g.pair, g.c}.proofs_from_bytes(in, count, compressed, validate, out, status);
  }
  static void points_check(ark355_ctx* ctx, GenericScratch& g, int group, const uint8_t* raw, uint64_t n, int method,
                           uint8_t* status) {
    Verify<Curve>{ctx, g.pair, g.c}.points_check(group, raw, n, method, status);
  }
  static bool verify_batch_pvk(ark355_ctx* ctx, GenericScratch& g, const PvkDev& pvk, const ark355_proof_raw* proofs,
                               const uint8_t* inputs, const uint8_t* rho, uint64_t count) {
    return Verify<Curve>{ctx, g.pair, g.c}.verify_batch_pvk(
        pvk, proofs, inputs, rho, count, [&](const uint8_t* bases, const uint8_t* scalars, uint64_t n, Affine<Fq>* out) {
          msm_host(ctx, g, 1, bases, scalars, n, reinterpret_cast<uint8_t*>(out));
        });
  }

  // ---- ark-serialize wire formats (wire_impl.cuh) ------------------------------------------------------------------
  static size_t point_size(int group, bool compressed) { return group == 1 ? W::g1_size(compressed) : W::g2_size(compressed); }
  static size_t raw_size(int group) { return group == 1 ? sizeof(Affine<Fq>) : sizeof(Affine<Fq2>); }

  // d_in: device byte stream of n encoded points -> d_out: n raw affine images (device).  Throws on a bad point.
  static void decode_dev(int group, const uint8_t* d_in, uint64_t n, bool compressed, int validate, void* d_out,
                         DevBuf& errbuf, hipStream_t st, const char* what) {
    if (n == 0) return;
    errbuf.ensure(8);
    ARK_CHECK_HIP(hipMemsetAsync(errbuf.p, 0, 8, st));
    const dim3 grid((uint32_t)((n + 127) / 128));
    if (group == 1)
      ARK_LAUNCH((wire_decode_kernel<Curve, 1>), grid, dim3(128), 0, st, d_in, n, compressed ? 1 : 0, validate, d_out,
                 errbuf.as<unsigned long long>());
    else
      ARK_LAUNCH((wire_decode_kernel<Curve, 2>), grid, dim3(128), 0, st, d_in, n, compressed ? 1 : 0, validate, d_out,
                 errbuf.as<unsigned long long>());
    ARK_CHECK_LAUNCH();
    unsigned long long e = 0;
    ARK_CHECK_HIP(hipMemcpyAsync(&e, errbuf.p, 8, hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
    if (e != 0)
      throw HipError{ARK355_EINVAL, std::string(what) + "[" + std::to_string((e >> 4) - 1) + "]: " + wire_status_name((int)(e & 15))};
  }

  static void points_decode(ark355_ctx* ctx, GenericScratch& g, int group, const uint8_t* in, uint64_t n, bool compressed,
                            int validate, uint8_t* out_raw) {
    hipStream_t st = ctx->stream;
    if (n == 0) return;
    g.a.ensure(n * point_size(group, compressed));
    g.b.ensure(n * raw_size(group));
    ARK_CHECK_HIP(hipMemcpyAsync(g.a.p, in, n * point_size(group, compressed), hipMemcpyHostToDevice, st));
    decode_dev(group, g.a.as<uint8_t>(), n, compressed, validate, g.b.p, g.c, st, "point");
    ARK_CHECK_HIP(hipMemcpyAsync(out_raw, g.b.p, n * raw_size(group), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  static void points_encode(ark355_ctx* ctx, GenericScratch& g, int group, const uint8_t* in_raw, uint64_t n,
                            bool compressed, uint8_t* out) {
    hipStream_t st = ctx->stream;
    if (n == 0) return;
    g.a.ensure(n * raw_size(group));
    g.b.ensure(n * point_size(group, compressed));
    ARK_CHECK_HIP(hipMemcpyAsync(g.a.p, in_raw, n * raw_size(group), hipMemcpyHostToDevice, st));
    const dim3 grid((uint32_t)((n + 127) / 128));
    if (group == 1)
      ARK_LAUNCH((wire_encode_kernel<Curve, 1>), grid, dim3(128), 0, st, (const void*)g.a.p, n, compressed ? 1 : 0, g.b.as<uint8_t>());
    else
      ARK_LAUNCH((wire_encode_kernel<Curve, 2>), grid, dim3(128), 0, st, (const void*)g.a.p, n, compressed ? 1 : 0, g.b.as<uint8_t>());
    ARK_CHECK_LAUNCH();
    ARK_CHECK_HIP(hipMemcpyAsync(out, g.b.p, n * point_size(group, compressed), hipMemcpyDeviceToHost, st));
    ARK_CHECK_HIP(hipStreamSynchronize(st));
  }

  // Proof = a || b || c (three points: host code)
  static void proof_to_bytes(const ark355_proof_raw* p, bool compressed, uint8_t* out) {
    Affine<Fq> a, c;
    Affine<Fq2> b;
    memcpy(&a, p->a, sizeof(a));
    memcpy(&b, p->b, sizeof(b));
    memcpy(&c, p->c, sizeof(c));
    W::g1_encode(a, compressed, out);
    W::g2_encode(b, compressed, out + W::g1_size(compressed));
    W::g1_encode(c, compressed, out + W::g1_size(compressed) + W::g2_size(compressed));
  }
  static void proof_from_bytes(const uint8_t* in, uint64_t len, bool compressed, int validate, ark355_proof_raw* out) {
    ARK_REQUIRE(len == 2 * W::g1_size(compressed) + W::g2_size(compressed), ARK355_EINVAL, "bad proof length");
    Affine<Fq> a, c;
    Affine<Fq2> b;
    int st = W::g1_decode(in, compressed, validate, &a);
    if (st == WIRE_OK) st = W::g2_decode(in + W::g1_size(compressed), compressed, validate, &b);
    if (st == WIRE_OK) st = W::g1_decode(in + W::g1_size(compressed) + W::g2_size(compressed), compressed, validate, &c);
    if (st != WIRE_OK) throw HipError{ARK355_EINVAL, std::string("proof: ") + wire_status_name(st)};
    memset(out, 0, sizeof(*out));
    memcpy(out->a, &a, sizeof(a));
    memcpy(out->b, &b, sizeof(b));
    memcpy(out->c, &c, sizeof(c));
  }

  // ark_groth16::ProvingKey<E> stream (vk {alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1}, beta_g1, delta_g1,
  // a_query, b_g1_query, b_g2_query, h_query, l_query; Vec = u64 LE length + elements) -> resident key.  The host walks
  // the structure, the device decodes the points.
  static PkDev* pk_load_bytes(ark355_ctx* ctx, const uint8_t* bytes, uint64_t len, bool compressed, int validate) {
    hipStream_t st = ctx->stream;
    const size_t s1 = W::g1_size(compressed), s2 = W::g2_size(compressed);
    uint64_t off = 0;
    auto need = [&](uint64_t k) { ARK_REQUIRE(k <= len && off <= len - k, ARK355_EINVAL, "truncated proving key"); };
    struct Span {
      uint64_t off = 0, n = 0;
      int group = 1;
    };
    auto single = [&](int group) {
      Span sp;
      sp.group = group;
      sp.off = off;
      sp.n = 1;
      need(group == 1 ? s1 : s2);
      off += group == 1 ? s1 : s2;
      return sp;
    };
    auto vec = [&](int group) {
      need(8);
      uint64_t n = 0;
      memcpy(&n, bytes + off, 8);
      off += 8;
      const uint64_t sz = group == 1 ? s1 : s2;
      ARK_REQUIRE(n <= (len - off) / sz, ARK355_EINVAL, "vector length exceeds the stream");
      Span sp;
      sp.group = group;
      sp.off = off;
      sp.n = n;
      off += n * sz;
      return sp;
    };
    const Span alpha = single(1), beta2 = single(2), gamma2 = single(2), delta2 = single(2), gabc = vec(1);
    const Span beta1 = single(1), delta1 = single(1), aq = vec(1), b1q = vec(1), b2q = vec(2), hq = vec(1), lq = vec(1);
    ARK_REQUIRE(off == len, ARK355_EINVAL, "trailing bytes in proving key");
    const uint64_t ell = gabc.n, m = aq.n, w = lq.n, N = hq.n + 1;
    ARK_REQUIRE(ell >= 1 && m == ell + w && b1q.n == m && b2q.n == m && (N & (N - 1)) == 0, ARK355_EINVAL,
                "proving key: inconsistent query lengths");
    DevBuf d_bytes(len), d_err;
    ARK_CHECK_HIP(hipMemcpyAsync(d_bytes.p, bytes, len, hipMemcpyHostToDevice, st));
    auto decode_vec = [&](const Span& sp, DevBuf& out, const char* what) {
      out.alloc((sp.n ? sp.n : 1) * raw_size(sp.group));
      decode_dev(sp.group, d_bytes.as<uint8_t>() + sp.off, sp.n, compressed, validate, out.p, d_err, st, what);
    };
    DevBuf d_a, d_b1, d_b2, d_h, d_l;
    {
      // the verifying key's gamma_abc_g1 and gamma_g2 are no part of the resident key: decoded for the verdict only, so
      // that a bad point anywhere in the stream is refused as upstream's deserialiser refuses it
      DevBuf d_gabc;
      decode_vec(gabc, d_gabc, "gamma_abc_g1");
    }
    decode_vec(aq, d_a, "a_query");
    decode_vec(b1q, d_b1, "b_g1_query");
    decode_vec(b2q, d_b2, "b_g2_query");
    decode_vec(hq, d_h, "h_query");
    decode_vec(lq, d_l, "l_query");
    Affine<Fq> h_alpha, h_beta1, h_delta1;
    Affine<Fq2> h_beta2, h_gamma2, h_delta2;
    auto dec1 = [&](const Span& sp, Affine<Fq>* o, const char* what) {
      const int e = W::g1_decode(bytes + sp.off, compressed, validate, o);
      if (e != WIRE_OK) throw HipError{ARK355_EINVAL, std::string(what) + ": " + wire_status_name(e)};
    };
    auto dec2 = [&](const Span& sp, Affine<Fq2>* o, const char* what) {
      const int e = W::g2_decode(bytes + sp.off, compressed, validate, o);
      if (e != WIRE_OK) throw HipError{ARK355_EINVAL, std::string(what) + ": " + wire_status_name(e)};
    };
    dec1(alpha, &h_alpha, "alpha_g1");
    dec1(beta1, &h_beta1, "beta_g1");
    dec1(delta1, &h_delta1, "delta_g1");
    dec2(beta2, &h_beta2, "beta_g2");
    dec2(gamma2, &h_gamma2, "gamma_g2");
    dec2(delta2, &h_delta2, "delta_g2");
    ark355_pk_desc d{};
    d.num_instance = ell;
    d.num_witness = w;
    d.domain_size = N;
    d.a_query = d_a.as<uint8_t>();            // device pointers: pk_upload copies with hipMemcpyDefault
    d.b_g1_query = d_b1.as<uint8_t>();
    d.b_g2_query = d_b2.as<uint8_t>();
    d.h_query = d_h.as<uint8_t>();
    d.l_query = d_l.as<uint8_t>();
    d.alpha_g1 = reinterpret_cast<const uint8_t*>(&h_alpha);
    d.beta_g1 = reinterpret_cast<const uint8_t*>(&h_beta1);
    d.delta_g1 = reinterpret_cast<const uint8_t*>(&h_delta1);
    d.beta_g2 = reinterpret_cast<const uint8_t*>(&h_beta2);
    d.delta_g2 = reinterpret_cast<const uint8_t*>(&h_delta2);
    return pk_upload<Curve>(ctx->policy, &d, st);
  }
};

// ---- multilinear openings (mle_open_impl.cuh): the two members Api declares without a body
// the quotient tables of `count` tables of 2^v at pt: count x 2^v Fr at q, the count values at rem (may be nullptr)
template <class Curve>
void Api<Curve>::mle_quotients(ark355_ctx* ctx, MleScratch& ms, const void* evals, uint32_t v, uint64_t count, const Fr* pt, void* q, void* rem,
                               bool on_dev) {
  hipStream_t st = ctx->stream;
  if (!count) return;
  const uint32_t E = mle_open_lane_entries(ctx->policy.mle_open_lane_entries);
  const size_t bytes = (size_t)(count << v) * sizeof(Fr), rem_bytes = (size_t)count * sizeof(Fr);
  mle_open_reserve<Fr>(ms, v, count, E);
  if (!on_dev) {
    ms.in.ensure(bytes);
    ms.q.ensure(bytes);
    if (rem) ms.rem.ensure(rem_bytes);
    ARK_CHECK_HIP(hipMemcpyAsync(ms.in.p, evals, bytes, hipMemcpyHostToDevice, st));
  }
  Fr* d_q = on_dev ? (Fr*)q : ms.q.template as<Fr>();
  Fr* d_rem = on_dev ? (Fr*)rem : (rem ? ms.rem.template as<Fr>() : nullptr);
  mle_open_run<Fr>(on_dev ? (const Fr*)evals : (const Fr*)ms.in.template as<Fr>(), v, count, pt, d_q, d_rem, ms, E, st);
  if (!on_dev) {
    ARK_CHECK_HIP(hipMemcpyAsync(q, d_q, bytes, hipMemcpyDeviceToHost, st));
    if (rem) ARK_CHECK_HIP(hipMemcpyAsync(rem, d_rem, rem_bytes, hipMemcpyDeviceToHost, st));
  }
  ARK_CHECK_HIP(hipStreamSynchronize(st));
}
// ---- batched short MSMs (msm_batch_impl.cuh)
template <class Curve>
template <class F>
void Api<Curve>::msm_batch_t(ark355_ctx* ctx, MsmBatchScratch& bs, GenericScratch& g, const BasesDev* const* bases, const void* const* d_scalars,
                             const uint64_t* n, uint64_t count, int mont, uint8_t* out) {
  hipStream_t st = ctx->stream;
  const uint64_t small_max = msm_batch_small_max(ctx->policy.msm_batch_small_max);
  auto* res = reinterpret_cast<Affine<F>*>(out);
  // the short route: every segment of 1 .. small_max scalars, in one launch sequence
  std::vector<MsmBatchSeg> segs;
  std::vector<uint64_t> who;
  uint64_t digits_total = 0, parts_total = 0;
  for (uint64_t s = 0; s < count; s++) {
    if (n[s] < 1 || n[s] > small_max) continue;
    const PrecompTable& tab = bases[s]->tab;
    const MsmPlan& p = tab.plan;
    MsmBatchSeg sg;
    sg.rows = tab.table.p;
    sg.scalars = d_scalars[s];
    sg.dig_off = digits_total;
    sg.out_off = (uint32_t)parts_total;
    sg.n = (uint32_t)n[s];
    sg.c = p.c;
    sg.windows = p.windows;
    sg.wstride = p.wstride;
    sg.row_stride = (uint32_t)tab.n;
    sg.packed = tab.packed ? 1u : 0u;
    sg.digit_flags = msm_digit_flags(p);
    digits_total += (uint64_t)p.windows * n[s];
    parts_total += msm_parts_count(p);
    segs.push_back(sg);
    who.push_back(s);
  }
  ARK_REQUIRE(parts_total < (1ull << 31), ARK355_EINVAL, "batched MSM: too many partial sums");
  if (!segs.empty()) {
    std::vector<XYZZ<F>> h_parts;
    msm_batch_short_run<F, Fr>(bs, segs, digits_total, (uint32_t)parts_total, mont, h_parts, st);
    // Horner over the bit sums of each segment (msm_parts_finish, as msm_generic), then one inversion for all of them
    std::vector<XYZZ<F>> sums(segs.size());
    for (size_t t = 0; t < segs.size(); t++) sums[t] = msm_parts_finish<F>(h_parts.data() + segs[t].out_off, bases[who[t]]->tab.plan);
    std::vector<Affine<F>> aff(segs.size());
    xyzz_batch_to_affine_host<F>(sums.data(), sums.size(), aff.data());
    for (size_t t = 0; t < segs.size(); t++) res[who[t]] = aff[t];
  }
  // every other segment: the empty ones are the point at infinity, the long ones run as ark355_msm_dev runs them
  for (uint64_t s = 0; s < count; s++) {
    if (n[s] == 0) res[s] = Affine<F>::inf();
    else if (n[s] > small_max) msm_dev(ctx, g, *bases[s], d_scalars[s], n[s], mont, out + (size_t)s * sizeof(Affine<F>), true);
  }
}
template <class Curve>
void Api<Curve>::msm_batch_dev(ark355_ctx* ctx, MsmBatchScratch& bs, GenericScratch& g, const BasesDev* const* bases, const void* const* d_scalars,
                               const uint64_t* n, uint64_t count, int mont, uint8_t* out) {
  if (!count) return;
  if (bases[0]->group == 1) msm_batch_t<Fq>(ctx, bs, g, bases, d_scalars, n, count, mont, out);
  else msm_batch_t<Fq2>(ctx, bs, g, bases, d_scalars, n, count, mont, out);
}

// the PST opening of one table in device memory: the quotients into the context's scratch, then the MSMs of all levels against
// bases[j] as ONE batch (msm_batch_dev, Montgomery scalars: the short levels in one launch sequence, the long ones through
// msm_generic one after another); v affine points at proofs, the value at value_out
template <class Curve>
void Api<Curve>::mle_open_dev(ark355_ctx* ctx, MleScratch& ms, MsmBatchScratch& bs, GenericScratch& g, const BasesDev* const* bases,
                              const void* d_evals, uint32_t v, const Fr* pt, uint8_t* proofs, uint8_t* value_out) {
  hipStream_t st = ctx->stream;
  const uint32_t E = mle_open_lane_entries(ctx->policy.mle_open_lane_entries);
  const uint64_t N = 1ull << v;
  mle_open_reserve<Fr>(ms, v, 1, E);
  ms.q.ensure((size_t)N * sizeof(Fr));
  ms.rem.ensure(sizeof(Fr));
  mle_open_run<Fr>((const Fr*)d_evals, v, 1, pt, ms.q.template as<Fr>(), ms.rem.template as<Fr>(), ms, E, st);
  ARK_CHECK_HIP(hipMemcpyAsync(value_out, ms.rem.p, sizeof(Fr), hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  std::vector<const void*> scalars(v);
  std::vector<uint64_t> lens(v);
  for (uint32_t j = 0; j < v; j++) {
    scalars[j] = ms.q.template as<Fr>() + mle_open_level_offset(N, j);
    lens[j] = N >> (j + 1);
  }
  msm_batch_dev(ctx, bs, g, bases, scalars.data(), lens.data(), v, 1, proofs);
}

}  // namespace ark355
