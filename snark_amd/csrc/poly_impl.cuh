// Polynomial openings on the device: evaluate at a point, divide by X - x, combine.  What a KZG-style prover does with a
// Fiat-Shamir challenge x after it has committed: for `count` polynomials of `len` coefficients lying back to back
// (polynomial k at element k len, coeffs[k][j] the coefficient of X^j; Fr values are Montgomery images, outputs fully reduced)
//     eval        out[k]  = sum_j coeffs[k][j] x^j                                  ark-poly  DensePolynomial::evaluate
//     div_linear  q[k][j] = sum_{i > j} coeffs[k][i] x^(i-j-1),  rem[k] = p_k(x)    ark-poly-commit  KZG10::compute_witness_polynomial
//                 so that p_k(X) = q_k(X) (X - x) + rem_k coefficient by coefficient, for any p and any x, a root or not
//     lincomb     out[j]  = sum_k scalars[k] polys[k][j]                            ark-poly  DensePolynomial: Add, Mul<F>
// The reference tree holds the traits and the relations only and has no counterpart.
//
// Decomposition (gfx950, wave64, workgroups of 256 lanes).  A lane owns E consecutive coefficients (policy POLY_LANE_COEFFS,
// 8 by default), a workgroup one chunk of K = 256 E, grid.y is the polynomial: one launch serves all `count` polynomials.
//   P1  poly_chunk_kernel   partial[k][c] = sum_{i in chunk c} coeffs[k][i] x^(i - c K): Horner over the lane's E coefficients,
//                           v_lo + x^(E 2^s) v_hi over six shuffle steps, the four wave values through 128 bytes of LDS.
//       The partials of one polynomial are a polynomial in Y = x^K whose value at Y is p(x): P1 runs on its own output until
//       one value per polynomial is left (at most four levels for len < 2^32 at E = 1, three at E = 8).  That is eval, and the
//       remainder of div_linear.
//   P3  poly_apply_kernel   (div_linear only)  With S_j = sum_{i >= j} c_i x^(i-j):  q[j] = S_{j+1} and S_j = c_j + x S_{j+1}.
//                           The value a chunk needs from behind its end, carry_c = S_{(c+1) K}, is exactly the quotient of the
//                           partials by (Y' - Y) at position c: the same kernel runs from the top level down, each level's
//                           quotient being the carries of the level below.  Inside a chunk: Horner per lane, an inclusive
//                           suffix scan over the wave by shuffles (six steps with the same powers), the wave totals through
//                           LDS, the chunk carry times x^(E (63 - lane)) from the table, then E single multiplications.
//       Every lane loads its E coefficients into registers BEFORE it stores its E quotients and reads no other lane's input
//       from global memory: that is why q_out == coeffs (in place) is legal, and the levels above the first always run in place
//       on their partials.
//   lincomb  poly_lincomb_kernel   one lane per output element, `count` is a loop; a scalar 0 skips its polynomial and a scalar 1
//                           its multiplication (the `pool index 0` idiom of columns_impl.cuh).  A lane reads polys[k][j] for its
//                           own j only, so out == polys (in place on polynomial 0) is legal.
// Every output element is written exactly once; no atomics; no host wait between the levels -- the caller waits once, at the end.
//
// Powers.  The chunk is a power of two only for E = 1, 2, 4, 8, so the point of every level, X_l = x^(K^l), and its table
// X_l, (X_l^E)^i for i = 0 .. 64 (66 Fr a level) are computed per call on the host with the library's own field code (about
// 70 multiplications a level) and copied into the scratch ahead of the first launch.  lincomb's scalars are converted to
// Montgomery form there as well, once per call.
//
// Scratch of one call (PolyScratch, grow-only, owned by the context, bytes; L_1 = ceil(len / K), L_{l+1} = ceil(L_l / K)):
//     32 count (L_1 + L_2 + ..)   partials, overwritten in place by the carries (nothing for len <= K)
//     32 * 66 * 4                 power tables          32 count   lincomb's scalars / the remainder nobody asked for
//     32 count len (+ 32 count)   staging of the host variants (div_linear and lincomb run in place on it)
#pragma once
#include <string>
#include <vector>
#include "common.h"
#include "field.cuh"
#include "fr_wave.cuh"
#include "ntt_impl.cuh"

namespace ark355 {

constexpr uint32_t POLY_THREADS = 256;
constexpr uint32_t POLY_LANE_COEFFS_DEFAULT = 8, POLY_LANE_COEFFS_MAX = 8;
constexpr uint32_t POLY_MAX_LEVELS = 4;                  // len < 2^32 at the smallest chunk (256): 2^24, 2^16, 2^8, 1
constexpr uint32_t POLY_TAB_STRIDE = 66;                 // a level's table: X, then (X^E)^i for i = 0 .. 64
constexpr uint32_t POLY_MAX_COUNT = 1024;                // ARK355_POLY_MAX_COUNT
constexpr uint64_t POLY_MAX_ELEMS = 1ull << 40;          // count * len: all indices are 64-bit; 2^40 Fr are 32 TiB

// policy POLY_LANE_COEFFS -> the coefficients a lane owns: <= 0 selects the default, anything else is clamped to 1 .. 8
static inline uint32_t poly_lane_coeffs(int32_t policy) {
  if (policy <= 0) return POLY_LANE_COEFFS_DEFAULT;
  return (uint32_t)policy > POLY_LANE_COEFFS_MAX ? POLY_LANE_COEFFS_MAX : (uint32_t)policy;
}

// grow-only scratch of a context
struct PolyScratch {
  DevBuf levels;                     // partials / carries of the levels above the first
  DevBuf tab;                        // power tables of the levels, or lincomb's scalars
  DevBuf rem;                        // the remainder of a div_linear whose caller passed no rem_out
  DevBuf in, small;                  // staging of the host variants: the polynomials, and eval's / the remainder's count Fr
  std::vector<unsigned char> host;   // host image of `tab`: alive until the call's last wait
};

// The levels of one call: len[0] = len, len[l + 1] = ceil(len[l] / K) down to 1; off[l] = where level l's partials start
// inside the scratch (in Fr, levels 1 .. levels - 1).  No HIP call.
struct PolyPlan {
  uint32_t E = POLY_LANE_COEFFS_DEFAULT, levels = 0;
  uint64_t len[POLY_MAX_LEVELS + 1] = {0, 0, 0, 0, 0};
  uint64_t off[POLY_MAX_LEVELS + 1] = {0, 0, 0, 0, 0};
  uint64_t scratch_elems = 0;
};

static inline PolyPlan poly_plan(uint64_t len, uint64_t count, uint32_t E) {
  PolyPlan p;
  if (E == 1 && len > 0xFFFFFF00ull) E = 2;              // a grid of 2^24 workgroups of 256 lanes would not launch
  p.E = E;
  p.len[0] = len;
  if (!len || !count) return p;
  const uint64_t K = (uint64_t)POLY_THREADS * E;
  uint64_t cur = len;
  do {
    cur = (cur + K - 1) / K;
    p.levels++;
    p.len[p.levels] = cur;
  } while (cur > 1 && p.levels < POLY_MAX_LEVELS);
  for (uint32_t l = 1; l < p.levels; l++) {
    p.off[l] = p.scratch_elems;
    p.scratch_elems += count * p.len[l];
  }
  return p;
}

// the lane's E coefficients (zero behind the end) and their value sum_e a[e] X^e
template <class Fr, int E>
ARK_D Fr poly_lane_load(const Fr* p, uint64_t base, uint64_t len, const Fr& X, Fr (&a)[E]) {
#pragma unroll
  for (int e = 0; e < E; e++) a[e] = base + e < len ? p[base + e] : Fr::zero();
  Fr v = a[E - 1];
#pragma unroll
  for (int e = E - 2; e >= 0; e--) v = Fr::add(Fr::mul(v, X), a[e]);
  return v;
}

// P1: workgroup (c, k) -> out[k gridDim.x + c] = sum_{i in chunk c} in[k len + i] X^(i - c K)
template <class Fr, int E>
__global__ void __launch_bounds__(POLY_THREADS)
poly_chunk_kernel(const Fr* __restrict__ in, uint64_t len, const Fr* __restrict__ tab, Fr* __restrict__ out) {
  __shared__ uint32_t wave_val[POLY_THREADS / 64][Fr::N];
  const uint32_t tid = threadIdx.x;
  const Fr* p = in + (uint64_t)blockIdx.y * len;
  const uint64_t base = ((uint64_t)blockIdx.x * POLY_THREADS + tid) * E;
  Fr a[E];
  Fr v = poly_lane_load<Fr, E>(p, base, len, tab[0], a);
  for (uint32_t s = 0; s < 6; s++) {                     // lane 0 ends with sum_t v_t (X^E)^t over its wave
    const Fr o = fr_shfl_down(v, 1u << s);
    v = Fr::add(v, Fr::mul(o, tab[1 + (1u << s)]));
  }
  if ((tid & 63u) == 0) {
#pragma unroll
    for (int i = 0; i < Fr::N; i++) wave_val[tid >> 6][i] = v.l[i];
  }
  __syncthreads();
  if (tid == 0) {
    const Fr XW = tab[1 + 64];                           // X^(64 E): from one wave to the next
    Fr acc = Fr::zero();
    for (uint32_t w = POLY_THREADS / 64; w-- > 1;) {
      Fr o;
#pragma unroll
      for (int i = 0; i < Fr::N; i++) o.l[i] = wave_val[w][i];
      acc = Fr::mul(Fr::add(acc, o), XW);
    }
    out[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = Fr::add(acc, v);
  }
}

// P3: workgroup (c, k) -> out[k len + j] = S_{j+1} for the j of chunk c, S_j = sum_{i >= j} in[k len + i] X^(i-j); carry
// (gridDim.x a polynomial, or nullptr at the top level: all zero) holds S at the chunks' ends.  out == in is legal.
template <class Fr, int E>
__global__ void __launch_bounds__(POLY_THREADS)
poly_apply_kernel(const Fr* in, uint64_t len, const Fr* __restrict__ carry, const Fr* __restrict__ tab, Fr* out) {
  __shared__ uint32_t wave_val[POLY_THREADS / 64][Fr::N];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const Fr* p = in + (uint64_t)blockIdx.y * len;
  Fr* q = out + (uint64_t)blockIdx.y * len;
  const uint64_t base = ((uint64_t)blockIdx.x * POLY_THREADS + tid) * E;
  const Fr X = tab[0];
  Fr a[E];
  Fr t = poly_lane_load<Fr, E>(p, base, len, X, a);
  for (uint32_t s = 0; s < 6; s++) {                     // t = sum_{u >= lane, same wave} v_u (X^E)^(u - lane)
    const Fr o = fr_shfl_down(t, 1u << s);
    const Fr n = Fr::add(t, Fr::mul(o, tab[1 + (1u << s)]));
    if (lane + (1u << s) < 64u) t = n;
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < Fr::N; i++) wave_val[wave][i] = t.l[i];
  }
  __syncthreads();
  Fr r = carry ? carry[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] : Fr::zero();
  const Fr XW = tab[1 + 64];
  for (uint32_t w = POLY_THREADS / 64 - 1; w > wave; w--) {        // r = S at the end of this wave
    Fr o;
#pragma unroll
    for (int i = 0; i < Fr::N; i++) o.l[i] = wave_val[w][i];
    r = Fr::add(Fr::mul(r, XW), o);
  }
  const Fr nxt = fr_shfl_down(t, 1);                   // every lane takes part; lane 63 gets its own value back and drops it
  Fr s = Fr::mul(r, tab[1 + 63 - lane]);                 // S at the end of this lane's coefficients
  if (lane < 63u) s = Fr::add(s, nxt);
#pragma unroll
  for (int e = E - 1; e >= 0; e--) {
    if (base + e < len) q[base + e] = s;
    if (e) s = Fr::add(Fr::mul(s, X), a[e]);
  }
}

// out[j] = sum_k sc[k] polys[k len + j]; sc in Montgomery form.  out == polys is legal.
template <class Fr>
__global__ void __launch_bounds__(POLY_THREADS)
poly_lincomb_kernel(const Fr* polys, uint64_t len, uint32_t count, const Fr* __restrict__ sc, Fr* out) {
  const uint64_t j = (uint64_t)blockIdx.x * POLY_THREADS + threadIdx.x;
  if (j >= len) return;
  const Fr one = Fr::one();
  Fr acc = Fr::zero();
  for (uint32_t k = 0; k < count; k++) {
    const Fr c = sc[k];
    if (c.is_zero()) continue;
    Fr v = polys[(uint64_t)k * len + j];
    if (c != one) v = Fr::mul(v, c);
    acc = Fr::add(acc, v);
  }
  out[j] = acc;
}

// the tables of every level into ps.host: level l at l * POLY_TAB_STRIDE; x in Montgomery form
template <class Fr>
static void poly_tables(PolyScratch& ps, const PolyPlan& plan, const Fr& x) {
  ps.host.resize((size_t)plan.levels * POLY_TAB_STRIDE * sizeof(Fr));
  Fr* t = reinterpret_cast<Fr*>(ps.host.data());
  Fr X = x;
  for (uint32_t l = 0; l < plan.levels; l++, t += POLY_TAB_STRIDE) {
    const Fr XE = fr_pow_u64(X, plan.E);
    t[0] = X;
    t[1] = Fr::one();
    for (uint32_t i = 1; i <= 64; i++) t[1 + i] = Fr::mul(t[i], XE);
    X = fr_pow_u64(t[1 + 64], POLY_THREADS / 64);          // (X^(64 E))^4 = X^K: the next level's point
  }
}

// every buffer of one eval / div_linear at its size for this call: the one place that may allocate, before the first launch
template <class Fr>
static void poly_reserve(PolyScratch& ps, const PolyPlan& plan, uint64_t count, bool own_rem) {
  ps.levels.ensure((size_t)plan.scratch_elems * sizeof(Fr));
  ps.tab.ensure((size_t)POLY_MAX_LEVELS * POLY_TAB_STRIDE * sizeof(Fr));
  if (own_rem) ps.rem.ensure((size_t)count * sizeof(Fr));
}

// d_out[k] = p_k(x) for k < count on `st` (queued, not waited for); ps was reserved by poly_reserve with the same plan
template <class Curve>
static void poly_eval_run(const void* d_coeffs, uint64_t count, const PolyPlan& plan, const typename Curve::Fr& x, void* d_out,
                          PolyScratch& ps, hipStream_t st) {
  using Fr = typename Curve::Fr;
  if (!count) return;
  if (!plan.levels) {                                    // len = 0: the zero polynomial
    ARK_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)count * sizeof(Fr), st));
    return;
  }
  poly_tables<Fr>(ps, plan, x);
  ARK_CHECK_HIP(hipMemcpyAsync(ps.tab.p, ps.host.data(), ps.host.size(), hipMemcpyHostToDevice, st));
  const Fr* tab = ps.tab.as<Fr>();
  for (uint32_t l = 0; l < plan.levels; l++) {
    const Fr* in = l ? ps.levels.as<Fr>() + plan.off[l] : (const Fr*)d_coeffs;
    Fr* out = l + 1 < plan.levels ? ps.levels.as<Fr>() + plan.off[l + 1] : (Fr*)d_out;
    const dim3 grid((uint32_t)plan.len[l + 1], (uint32_t)count);
    ARK_BY_E(plan.E, ARK_LAUNCH((poly_chunk_kernel<Fr, PE>), grid, dim3(POLY_THREADS), 0, st, in, plan.len[l],
                                tab + (size_t)l * POLY_TAB_STRIDE, out));
    ARK_CHECK_LAUNCH();
  }
}

// d_q (count x len) and d_rem (count; nullptr: the scratch's) on `st` (queued); d_q == d_coeffs is legal
template <class Curve>
static void poly_div_run(const void* d_coeffs, uint64_t count, const PolyPlan& plan, const typename Curve::Fr& x, void* d_q,
                         void* d_rem, PolyScratch& ps, hipStream_t st) {
  using Fr = typename Curve::Fr;
  if (!count) return;
  if (!d_rem) d_rem = ps.rem.p;
  poly_eval_run<Curve>(d_coeffs, count, plan, x, d_rem, ps, st);
  const Fr* tab = ps.tab.as<Fr>();
  for (uint32_t l = plan.levels; l-- > 0;) {
    const Fr* in = l ? ps.levels.as<Fr>() + plan.off[l] : (const Fr*)d_coeffs;
    Fr* out = l ? ps.levels.as<Fr>() + plan.off[l] : (Fr*)d_q;
    const Fr* carry = l + 1 < plan.levels ? ps.levels.as<Fr>() + plan.off[l + 1] : nullptr;
    const dim3 grid((uint32_t)plan.len[l + 1], (uint32_t)count);
    ARK_BY_E(plan.E, ARK_LAUNCH((poly_apply_kernel<Fr, PE>), grid, dim3(POLY_THREADS), 0, st, in, plan.len[l], carry,
                                tab + (size_t)l * POLY_TAB_STRIDE, out));
    ARK_CHECK_LAUNCH();
  }
}

// d_out (len) = sum_k scalars[k] d_polys[k] on `st` (queued); scalars: count Montgomery images on the host.  ps.tab holds
// at least count Fr.
template <class Curve>
static void poly_lincomb_run(const void* d_polys, uint64_t len, uint64_t count, const typename Curve::Fr* scalars, void* d_out,
                             PolyScratch& ps, hipStream_t st) {
  using Fr = typename Curve::Fr;
  if (!len) return;
  if (!count) {
    ARK_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)len * sizeof(Fr), st));
    return;
  }
  ps.host.assign(reinterpret_cast<const unsigned char*>(scalars), reinterpret_cast<const unsigned char*>(scalars + count));
  ARK_CHECK_HIP(hipMemcpyAsync(ps.tab.p, ps.host.data(), ps.host.size(), hipMemcpyHostToDevice, st));
  const uint32_t grid = (uint32_t)((len + POLY_THREADS - 1) / POLY_THREADS);
  ARK_LAUNCH((poly_lincomb_kernel<Fr>), dim3(grid), dim3(POLY_THREADS), 0, st, (const Fr*)d_polys, len, (uint32_t)count,
             (const Fr*)ps.tab.as<Fr>(), (Fr*)d_out);
  ARK_CHECK_LAUNCH();
}

}  // namespace ark355
