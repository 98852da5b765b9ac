// Openings in the evaluation basis: evaluate at a point and divide by X - x without a transform.  A prover that holds a
// Lagrange-basis key (ark355_lagrange_fr_dev -> ark355_fixed_base_mul_dev) commits to the values of a polynomial over its domain
// and opens from the same values.  With N = 2^log_n, w the N-th root of ark355_ntt_fr, s = 1 (coset = 0) or the coset generator g
// (coset != 0), a_i = s w^i and e[k][i] = p_k(a_i) for `count` polynomials of degree < N lying back to back:
//     eval        y[k]    = p_k(x)                                     barycentric formula
//     div_linear  q[k][i] = q_k(a_i) for q_k = (p_k - y_k) / (X - x),  rem[k] = y[k]
// For x outside the domain, with D_i = a_i - x:
//     y = (x'^N - 1)/N sum_i e_i w^i / (x' - w^i),  x' = x / s
//       = (1 - x'^N)/N (sum_i e_i + x sum_i e_i / D_i)                 because a_i / D_i = 1 + x / D_i
//     q_i = (e_i - y) / D_i
// so both entries need the same N inverses 1 / D_i, which do not depend on the polynomial.  For x = a_j: y = e_j, D_j is replaced
// by one BEFORE it enters any product (e_j - y = 0 makes that point's q zero for the moment), and
//     q_j = - sum_{i != j} q_i w^(i-j) = -(1/x) sum_i q_i a_i          (a_j = x is not zero)
// because q has degree <= N - 2 and so sum_i q_i w^i = 0 over the domain.
//
// Decomposition (gfx950, wave64, workgroups of 256 lanes).  A lane owns E consecutive points (policy EVALS_LANE_POINTS, 8 by
// default), a workgroup 256 E, `count` is a loop inside the lane: the inverses are computed once for all polynomials.
//   inverses   evals_lane_inverses   a_first from the tables (one multiplication per 6 bits of the wave's index), the prefix
//                           products of the lane's E denominators, the product of the wave's 64 lane products by a butterfly of
//                           six shuffles, the four wave products through LDS, ONE inversion per workgroup (wave 0 computes it, the
//                           other waves wait at a barrier), back through the wave products and down the butterfly to the inverse of
//                           the lane's own product, then two multiplications a point.  One inversion per 256 E points where
//                           setup_lagrange_kernel pays one per 8 -- and a wave pays for an inversion what a lane does.
//   E1  evals_eval_kernel   partial[k][g] = sum over workgroup g of e_i + x e_i / D_i: six shuffle steps, the four wave values
//                           through LDS (two buffers, one barrier a polynomial)
//   E2  evals_sum_kernel    a plain chunked sum (2048 values a workgroup, its own kernel: poly_chunk_kernel would need a table of
//                           ones), run on its own output until one value a polynomial is left; the last level multiplies by
//                           (1 - x'^N)/N, or by -1/x and stores at [k][j]
//   E3  evals_quot_kernel   (div_linear) recomputes the inverses once y is complete and writes q pointwise; for x = a_j it also
//                           leaves the partial sums of q_i a_i for E2
//   E0  evals_pick_kernel   x = a_j: finds j by comparing a_i with x (as setup_indicator_kernel does), y[k] = e[k][j], j into the
//                           scratch for E2
// Every lane loads its E values of a polynomial BEFORE it stores its E quotients and reads no other lane's input: q_out == evals
// is legal.  Every output element is written exactly once (q[k][j] a second time, by a later launch of the same stream); no
// atomics; no host wait between the launches.
//
// Scratch of one call (EvalsScratch, grow-only, owned by the context; G = ceil(N / (256 E)), G_{l+1} = ceil(G_l / 2048)):
//     32 count (G + G_2 + ..)    partials                   32 * 384   tables            8   the index j
//     32 count                   the remainder nobody asked for
//     32 count N (+ 32 count)    staging of the host variants (div_linear runs in place on it)
#pragma once
#include <string>
#include <vector>
#include "common.h"
#include "field.cuh"
#include "fr_wave.cuh"
#include "ntt_impl.cuh"
#include "setup_impl.cuh"

namespace ark355 {

constexpr uint32_t EVALS_THREADS = 256;
constexpr uint32_t EVALS_LANE_POINTS_DEFAULT = 8, EVALS_LANE_POINTS_MAX = 8;
constexpr uint32_t EVALS_SUM_RUN = 8;                     // E2: values a lane adds; a workgroup sums 256 * 8 = 2048
constexpr uint32_t EVALS_SUM_CHUNK = EVALS_THREADS * EVALS_SUM_RUN;
constexpr uint32_t EVALS_MAX_LEVELS = 4;                  // G <= 2^24 -> 2^13 -> 4 -> 1
constexpr uint32_t EVALS_TAB_DIGITS = 5;                  // 6-bit digits of a wave's index: at most 2^26 waves (N = 2^32, E = 1)
constexpr uint32_t EVALS_TAB_ELEMS = 64 * (1 + EVALS_TAB_DIGITS);
constexpr uint32_t EVALS_PICK_RUN = 8;                    // E0: points a lane compares

// policy EVALS_LANE_POINTS -> the points a lane owns: <= 0 selects the default, anything else is clamped to 1 .. 8
static inline uint32_t evals_lane_points(int32_t policy) {
  if (policy <= 0) return EVALS_LANE_POINTS_DEFAULT;
  return (uint32_t)policy > EVALS_LANE_POINTS_MAX ? EVALS_LANE_POINTS_MAX : (uint32_t)policy;
}

// grow-only scratch of a context
struct EvalsScratch {
  DevBuf part;                       // partials of every level
  DevBuf tab;                        // tables of a_first
  DevBuf idx;                        // the index j of x = a_j
  DevBuf rem;                        // the remainder of a div_linear whose caller passed no rem_out
  DevBuf in, small;                  // staging of the host variants
  std::vector<unsigned char> host;   // host image of `tab`: alive until the call's last wait
};

// The launches of one call: len[0] = G workgroups of E1 / E3, len[l + 1] = ceil(len[l] / 2048) down to 1 (always at least one
// launch of E2: it applies the factor); off[l] = where level l's partials start inside the scratch, in Fr.  No HIP call.
struct EvalsPlan {
  uint32_t E = EVALS_LANE_POINTS_DEFAULT, log_n = 0, levels = 0, tab_digits = 0;
  uint64_t N = 1;
  uint64_t len[EVALS_MAX_LEVELS + 1] = {0, 0, 0, 0, 0};
  uint64_t off[EVALS_MAX_LEVELS + 1] = {0, 0, 0, 0, 0};
  uint64_t scratch_elems = 0;
};

static inline EvalsPlan evals_plan(uint32_t log_n, uint64_t count, uint32_t E) {
  EvalsPlan p;
  p.log_n = log_n;
  p.N = 1ull << log_n;
  if (E == 1 && p.N > 0xFFFFFF00ull) E = 2;               // a grid of 2^24 workgroups of 256 lanes would not launch
  p.E = E;
  const uint64_t K = (uint64_t)EVALS_THREADS * E;
  p.len[0] = (p.N + K - 1) / K;
  do {
    p.len[p.levels + 1] = (p.len[p.levels] + EVALS_SUM_CHUNK - 1) / EVALS_SUM_CHUNK;
    p.levels++;
  } while (p.len[p.levels] > 1 && p.levels < EVALS_MAX_LEVELS);
  for (uint32_t l = 0; l < p.levels; l++) {
    p.off[l] = p.scratch_elems;
    p.scratch_elems += count * p.len[l];
  }
  const uint64_t waves = p.len[0] * (EVALS_THREADS / 64);
  while (p.tab_digits < EVALS_TAB_DIGITS && ((waves - 1) >> (6 * p.tab_digits))) p.tab_digits++;
  return p;
}

// What the host knows about the point: everything in Montgomery form
template <class Fr>
struct EvalsPoint {
  Fr x, s, omega;
  bool inside = false;               // x = a_j for some j
  Fr fac_eval;                       // (1 - x'^N) / N
  Fr fac_fix;                        // -1 / x (inside only)
};

template <class Fr>
static EvalsPoint<Fr> evals_point(uint32_t log_n, bool coset, const Fr& x) {
  using P = typename Fr::Params;
  static const Fr half = Fr::inv(Fr::add(Fr::one(), Fr::one()));
  EvalsPoint<Fr> pt;
  pt.x = x;
  pt.s = coset ? fr_from_params<Fr>(&P::gen) : Fr::one();
  pt.omega = ntt_root<Fr>(log_n, false);
  const Fr xs = coset ? Fr::mul(x, fr_from_params<Fr>(&P::gen_inv)) : x;
  const Fr zt = Fr::sub(Fr::one(), fr_pow2k(xs, log_n));
  pt.inside = zt.is_zero();
  pt.fac_eval = Fr::mul(zt, fr_pow_u64(half, log_n));
  pt.fac_fix = pt.inside ? Fr::neg(Fr::inv(x)) : Fr::zero();
  return pt;
}

// tab[l] = s w^(l E) for l < 64; digit t: tab[64 + 64 t + i] = w^(64 E 64^t i) for i < 64
template <class Fr>
static void evals_tables(EvalsScratch& es, const EvalsPlan& plan, const EvalsPoint<Fr>& pt) {
  es.host.resize((size_t)64 * (1 + plan.tab_digits) * sizeof(Fr));
  Fr* t = reinterpret_cast<Fr*>(es.host.data());
  const Fr wE = fr_pow_u64(pt.omega, plan.E);
  Fr cur = pt.s;
  for (uint32_t l = 0; l < 64; l++) {
    t[l] = cur;
    cur = Fr::mul(cur, wE);
  }
  Fr base = fr_pow2k(wE, 6);
  for (uint32_t d = 0; d < plan.tab_digits; d++) {
    Fr* td = t + 64 + 64 * d;
    cur = Fr::one();
    for (uint32_t i = 0; i < 64; i++) {
      td[i] = cur;
      cur = Fr::mul(cur, base);
    }
    base = cur;                                           // base^64
  }
}

// One element as two 16-byte loads (the vectors of the C ABI are 32-byte aligned like every Fr array of the library, and Fr itself
// carries only the alignment of its limbs, which leaves the compiler eight single loads wherever the pointer may alias a store)
template <class Fr>
ARK_D Fr evals_load(const Fr* p) {
  static_assert(Fr::N == 8, "an Fr is two uint4");
  const uint4* s = reinterpret_cast<const uint4*>(p);
  const uint4 a = s[0], b = s[1];
  Fr o;
  o.l[0] = a.x; o.l[1] = a.y; o.l[2] = a.z; o.l[3] = a.w;
  o.l[4] = b.x; o.l[5] = b.y; o.l[6] = b.z; o.l[7] = b.w;
  return o;
}
template <class Fr>
ARK_D void evals_store(Fr* p, const Fr& v) {
  uint4* d = reinterpret_cast<uint4*>(p);
  d[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  d[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// Fr::inv and fr_pow with their multiplications inlined: the out-of-line Fr::mul_ni they call takes its operands through the
// stack, and the kernels of this file keep no scratch memory.  Same operations in the same order: the same bytes.
template <class Fr>
ARK_D Fr evals_inv(const Fr& a) {
  using P = typename Fr::Params;
  Fr result = a;
  bool started = false;
#pragma unroll 1
  for (int i = Fr::N - 1; i >= 0; i--) {
    const uint32_t w = P::pm2(i);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      if (started) result = Fr::sqr(result);
      if ((w >> b) & 1) {
        if (started) result = Fr::mul(result, a);
        started = true;
      }
    }
  }
  return result;
}
template <class Fr>
ARK_D Fr evals_pow(Fr x, uint64_t e) {
  Fr r = Fr::one();
#pragma unroll 1
  while (e) {
    if (e & 1) r = Fr::mul(r, x);
    x = Fr::sqr(x);
    e >>= 1;
  }
  return r;
}

// d[e] = a_(first+e) - x, or one where that is zero or first + e >= N; iv[e] = 1 / d[e].  Every lane of the workgroup takes part
// (two barriers); wprod: LDS for the four wave products and the inverse of their product.
template <class Fr, int E>
ARK_D void evals_lane_inverses(const Fr* __restrict__ tab, uint32_t tab_digits, const Fr& x, const Fr& omega, uint64_t first,
                               uint64_t N, uint32_t (*wprod)[Fr::N], Fr (&d)[E], Fr (&iv)[E]) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t W = (uint64_t)blockIdx.x * (EVALS_THREADS / 64) + (threadIdx.x >> 6);
  Fr a = tab[lane];
  for (uint32_t t = 0; t < tab_digits; t++) {             // wave-uniform
    const uint32_t i = (uint32_t)(W >> (6 * t)) & 63u;
    if (i) a = Fr::mul(a, tab[64 + 64 * t + i]);
  }
  Fr acc = Fr::one();
#pragma unroll
  for (int e = 0; e < E; e++) {
    Fr t = Fr::sub(a, x);
    if (first + e >= N || t.is_zero()) t = Fr::one();     // the zero must not enter any product
    d[e] = t;
    acc = e ? Fr::mul(acc, t) : t;
    iv[e] = acc;                                          // prefix products
    if (e + 1 < E) a = Fr::mul(a, omega);
  }
  Fr o[6];
#pragma unroll
  for (int s = 0; s < 6; s++) {                           // acc = the product of the 2^(s+1) lanes around this one
    o[s] = fr_shfl_xor(acc, 1u << s);
    acc = Fr::mul(acc, o[s]);
  }
  // acc = the wave's product, in all 64 lanes.  ONE inversion a workgroup: wave 0 inverts the product of the four wave products while
  // the other waves wait at the barrier and leave their SIMDs to other workgroups
  const uint32_t wave = threadIdx.x >> 6;
  constexpr uint32_t WAVES = EVALS_THREADS / 64;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < Fr::N; i++) wprod[wave][i] = acc.l[i];
  }
  __syncthreads();
  if (wave == 0) {
    Fr t = acc;
    for (uint32_t w = 1; w < WAVES; w++) {
      Fr u;
#pragma unroll
      for (int i = 0; i < Fr::N; i++) u.l[i] = wprod[w][i];
      t = Fr::mul(t, u);
    }
    t = evals_inv(t);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < Fr::N; i++) wprod[WAVES][i] = t.l[i];
    }
  }
  __syncthreads();
  Fr inv;
#pragma unroll
  for (int i = 0; i < Fr::N; i++) inv.l[i] = wprod[WAVES][i];
  for (uint32_t w = 0; w < WAVES; w++) {                  // wave-uniform: times the other waves' products
    if (w == wave) continue;
    Fr u;
#pragma unroll
    for (int i = 0; i < Fr::N; i++) u.l[i] = wprod[w][i];
    inv = Fr::mul(inv, u);
  }
#pragma unroll
  for (int s = 5; s >= 0; s--) inv = Fr::mul(inv, o[s]);  // 1 / (this lane's product)
#pragma unroll
  for (int e = E - 1; e > 0; e--) {
    const Fr t = Fr::mul(inv, iv[e - 1]);
    inv = Fr::mul(inv, d[e]);
    iv[e] = t;
  }
  iv[0] = inv;
}

// E1: workgroup g -> part[k gridDim.x + g] = sum_{i in g} e[k][i] (1 + x / D_i) for every k < count
template <class Fr, int E>
__global__ void __launch_bounds__(EVALS_THREADS)
evals_eval_kernel(const Fr* __restrict__ in, uint64_t N, uint32_t count, const Fr* __restrict__ tab, uint32_t tab_digits, Fr x, Fr omega,
                  Fr* __restrict__ part) {
  __shared__ uint32_t wave_val[2][EVALS_THREADS / 64][Fr::N];
  const uint64_t first = ((uint64_t)blockIdx.x * EVALS_THREADS + threadIdx.x) * E;
  __shared__ uint32_t wprod[EVALS_THREADS / 64 + 1][Fr::N];
  Fr d[E], iv[E];
  evals_lane_inverses<Fr, E>(tab, tab_digits, x, omega, first, N, wprod, d, iv);
  for (uint32_t k = 0; k < count; k++) {
    const Fr* p = in + (uint64_t)k * N;
#pragma unroll
    for (int e = 0; e < E; e++) {
      d[e] = Fr::zero();
      if (first + e < N) d[e] = evals_load(p + first + e);
    }
    Fr s1 = d[0], s2 = Fr::mul(d[0], iv[0]);
#pragma unroll
    for (int e = 1; e < E; e++) {
      s1 = Fr::add(s1, d[e]);
      s2 = Fr::add(s2, Fr::mul(d[e], iv[e]));
    }
    fr_group_sum<Fr>(Fr::add(s1, Fr::mul(s2, x)), wave_val[k & 1], EVALS_THREADS / 64, part + (uint64_t)k * gridDim.x + blockIdx.x);
  }
}

// E3: q[k][i] = (e[k][i] - y[k]) / D_i; SUM (x = a_j): also part[k gridDim.x + g] = sum_{i in g} q[k][i] a_i.  q == in is legal.
template <class Fr, int E, bool SUM>
__global__ void __launch_bounds__(EVALS_THREADS)
evals_quot_kernel(const Fr* in, uint64_t N, uint32_t count, const Fr* __restrict__ tab, uint32_t tab_digits, Fr x, Fr omega,
                  const Fr* __restrict__ y, Fr* q, Fr* __restrict__ part) {
  __shared__ uint32_t wave_val[2][EVALS_THREADS / 64][Fr::N];
  const uint64_t first = ((uint64_t)blockIdx.x * EVALS_THREADS + threadIdx.x) * E;
  __shared__ uint32_t wprod[EVALS_THREADS / 64 + 1][Fr::N];
  Fr d[E], iv[E];
  evals_lane_inverses<Fr, E>(tab, tab_digits, x, omega, first, N, wprod, d, iv);
  for (uint32_t k = 0; k < count; k++) {
    const Fr* p = in + (uint64_t)k * N;
    Fr* o = q + (uint64_t)k * N;
    const Fr yk = y[k];
    Fr v[E];
#pragma unroll
    for (int e = 0; e < E; e++) {                         // whole elements, selected afterwards: every load before the first store
      v[e] = yk;
      if (first + e < N) v[e] = evals_load(p + first + e);
    }
    Fr acc = Fr::zero();
#pragma unroll
    for (int e = 0; e < E; e++) {
      const Fr t = Fr::mul(Fr::sub(v[e], yk), iv[e]);     // behind the end: zero
      if (first + e < N) evals_store(o + first + e, t);
      if (SUM) acc = Fr::add(acc, Fr::mul(t, Fr::add(d[e], x)));   // a_i = D_i + x; where D was replaced, t is zero
    }
    if (SUM) fr_group_sum<Fr>(acc, wave_val[k & 1], EVALS_THREADS / 64, part + (uint64_t)k * gridDim.x + blockIdx.x);
  }
}

// E2: workgroup (c, k) -> the sum of in[k len + i] for the i of chunk c.  fin = 0: out[k gridDim.x + c]; fin = 1 (one chunk):
// times factor; fin = 2 (one chunk): times factor into out[k N + *j]
template <class Fr>
__global__ void __launch_bounds__(EVALS_THREADS)
evals_sum_kernel(const Fr* __restrict__ in, uint64_t len, Fr factor, uint32_t fin, const unsigned long long* __restrict__ j, uint64_t N,
                 Fr* __restrict__ out) {
  __shared__ uint32_t wave_val[EVALS_THREADS / 64][Fr::N];
  const Fr* p = in + (uint64_t)blockIdx.y * len;
  const uint64_t base = (uint64_t)blockIdx.x * EVALS_SUM_CHUNK + threadIdx.x;
  Fr acc = Fr::zero();
#pragma unroll
  for (uint32_t r = 0; r < EVALS_SUM_RUN; r++) {
    const uint64_t i = base + (uint64_t)r * EVALS_THREADS;
    if (i < len) acc = Fr::add(acc, p[i]);
  }
  Fr total;
  fr_group_sum<Fr>(acc, wave_val, EVALS_THREADS / 64, &total);
  if (threadIdx.x == 0) {
    if (fin) total = Fr::mul(total, factor);
    if (fin == 2) {
      const uint64_t at = (uint64_t)*j;                   // written by E0 of the same call; never trusted as an index
      if (at < N) out[(uint64_t)blockIdx.y * N + at] = total;
    } else {
      out[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
    }
  }
}

// E0 (x = a_j): out[k] = in[k N + j] for every k < count and *j_out = j
template <class Fr>
__global__ void __launch_bounds__(EVALS_THREADS)
evals_pick_kernel(const Fr* __restrict__ in, uint64_t N, uint32_t count, Fr x, Fr s, Fr omega, Fr* __restrict__ out,
                  unsigned long long* __restrict__ j_out) {
  const uint64_t first = ((uint64_t)blockIdx.x * EVALS_THREADS + threadIdx.x) * EVALS_PICK_RUN;
  if (first >= N) return;
  const uint32_t cnt = first + EVALS_PICK_RUN <= N ? EVALS_PICK_RUN : (uint32_t)(N - first);
  Fr p = Fr::mul(s, evals_pow(omega, first));
  for (uint32_t e = 0; e < cnt; e++) {
    if (p == x) {
      *j_out = first + e;
      for (uint32_t k = 0; k < count; k++) out[k] = in[(uint64_t)k * N + first + e];
    }
    p = Fr::mul(p, omega);
  }
}

// every buffer of one eval / div_linear at its size for this call: the one place that may allocate, before the first launch
template <class Fr>
static void evals_reserve(EvalsScratch& es, const EvalsPlan& plan, uint64_t count, bool own_rem) {
  es.part.ensure((size_t)plan.scratch_elems * sizeof(Fr));
  es.tab.ensure((size_t)EVALS_TAB_ELEMS * sizeof(Fr));
  es.idx.ensure(sizeof(unsigned long long));
  if (own_rem) es.rem.ensure((size_t)count * sizeof(Fr));
}

// E2 on the partials of level 0 down to one value a polynomial, the last launch with (factor, fin) into d_out
template <class Fr>
static void evals_sum_levels(const EvalsPlan& plan, uint64_t count, EvalsScratch& es, const Fr& factor, uint32_t fin, Fr* d_out,
                             hipStream_t st) {
  for (uint32_t l = 0; l < plan.levels; l++) {
    const bool last = l + 1 == plan.levels;
    const Fr* in = es.part.as<Fr>() + plan.off[l];
    Fr* out = last ? d_out : es.part.as<Fr>() + plan.off[l + 1];
    const dim3 grid((uint32_t)plan.len[l + 1], (uint32_t)count);
    ARK_LAUNCH((evals_sum_kernel<Fr>), grid, dim3(EVALS_THREADS), 0, st, in, plan.len[l], factor, last ? fin : 0u,
               (const unsigned long long*)es.idx.as<unsigned long long>(), plan.N, out);
    ARK_CHECK_LAUNCH();
  }
}

template <class Fr>
static void evals_upload_tables(EvalsScratch& es, const EvalsPlan& plan, const EvalsPoint<Fr>& pt, hipStream_t st) {
  evals_tables<Fr>(es, plan, pt);
  ARK_CHECK_HIP(hipMemcpyAsync(es.tab.p, es.host.data(), es.host.size(), hipMemcpyHostToDevice, st));
}

// d_out[k] = p_k(x) for k < count on `st` (queued, not waited for); es was reserved by evals_reserve with the same plan; for a
// point outside the domain the tables are in place (evals_upload_tables)
template <class Curve>
static void evals_eval_run(const void* d_evals, uint64_t count, const EvalsPlan& plan, const EvalsPoint<typename Curve::Fr>& pt,
                           void* d_out, EvalsScratch& es, hipStream_t st) {
  using Fr = typename Curve::Fr;
  if (!count) return;
  if (pt.inside) {
    const uint64_t lanes = (plan.N + EVALS_PICK_RUN - 1) / EVALS_PICK_RUN;
    ARK_LAUNCH((evals_pick_kernel<Fr>), dim3((uint32_t)((lanes + EVALS_THREADS - 1) / EVALS_THREADS)), dim3(EVALS_THREADS), 0, st,
               (const Fr*)d_evals, plan.N, (uint32_t)count, pt.x, pt.s, pt.omega, (Fr*)d_out, es.idx.as<unsigned long long>());
    ARK_CHECK_LAUNCH();
    return;
  }
  ARK_BY_E(plan.E, ARK_LAUNCH((evals_eval_kernel<Fr, PE>), dim3((uint32_t)plan.len[0]), dim3(EVALS_THREADS), 0, st,
                              (const Fr*)d_evals, plan.N, (uint32_t)count, (const Fr*)es.tab.as<Fr>(), plan.tab_digits, pt.x,
                              pt.omega, es.part.as<Fr>()));
  ARK_CHECK_LAUNCH();
  evals_sum_levels<Fr>(plan, count, es, pt.fac_eval, 1u, (Fr*)d_out, st);
}

// d_q (count x N) and d_rem (count; nullptr: the scratch's) on `st` (queued); d_q == d_evals is legal
template <class Curve>
static void evals_div_run(const void* d_evals, uint64_t count, const EvalsPlan& plan, const EvalsPoint<typename Curve::Fr>& pt,
                          void* d_q, void* d_rem, EvalsScratch& es, hipStream_t st) {
  using Fr = typename Curve::Fr;
  if (!count) return;
  if (!d_rem) d_rem = es.rem.p;
  evals_eval_run<Curve>(d_evals, count, plan, pt, d_rem, es, st);
  const dim3 grid((uint32_t)plan.len[0]);
  if (pt.inside) {
    ARK_BY_E(plan.E, ARK_LAUNCH((evals_quot_kernel<Fr, PE, true>), grid, dim3(EVALS_THREADS), 0, st, (const Fr*)d_evals, plan.N,
                                (uint32_t)count, (const Fr*)es.tab.as<Fr>(), plan.tab_digits, pt.x, pt.omega, (const Fr*)d_rem,
                                (Fr*)d_q, es.part.as<Fr>()));
    ARK_CHECK_LAUNCH();
    evals_sum_levels<Fr>(plan, count, es, pt.fac_fix, 2u, (Fr*)d_q, st);
  } else {
    ARK_BY_E(plan.E, ARK_LAUNCH((evals_quot_kernel<Fr, PE, false>), grid, dim3(EVALS_THREADS), 0, st, (const Fr*)d_evals, plan.N,
                                (uint32_t)count, (const Fr*)es.tab.as<Fr>(), plan.tab_digits, pt.x, pt.omega, (const Fr*)d_rem,
                                (Fr*)d_q, es.part.as<Fr>()));
    ARK_CHECK_LAUNCH();
  }
}

}  // namespace ark355
