// Sum-check of a GR1CS predicate over resident tables: the prover's side of ark-linear-sumcheck's IPForMLSumcheck::prove_round for
//     S = sum_i W[i] P(T_0[i], .., T_{t-1}[i]),   i < N = 2^v,
// P the resident polynomial program of a predicate (arity t, degree d as written: gr1cs_impl.cuh), T the t tables of
// ark355_gr1cs_mat_vec_dev (or any data), W an optional weight (typically eq(tau, .) of mle_impl.cuh).  D = d + (W ? 1 : 0); the
// message of a round is g(X) at X = 0 .. D, `points` = D + 1 values.  After j challenges the state is the tables folded j times by
// the rule of mle_fold_kernel; the message of round j + 1 is
//     g[X] = sum_{i < 2^(v-j-1)} Wx P(A_0, .., A_{t-1}),   A_k = T_k[2i] + X (T_k[2i+1] - T_k[2i]).
//
// Decomposition (gfx950, wave64).
//   sumcheck_round_kernel<FOLD, WEIGHT>   ONE kernel a round: fold and sum in one pass.  For the output pair (2i, 2i+1) a lane reads
//       entries 4i .. 4i+3 of each of the t + 1 tables of the previous state (128 contiguous bytes a table), folds them with the
//       challenge, stores the two folded values, then walks X = 0 .. D adding the difference each step -- no multiplication -- and
//       evaluates the polynomial program at each X.  FOLD = false is round 1: no challenge, the caller's tables, no store.
//       The loops over terms, factors and exponent bits are wave-uniform as in gr1cs_pred_kernel.  What a lane indexes at run time --
//       the t current values, their t differences, the D + 1 accumulators -- lies in LDS, limb-major [slot][limb][lane]: consecutive
//       lanes hit consecutive banks, a lane touches its own words only (no barrier), and nothing is left for scratch memory.  The
//       weight's value and difference have fixed names and stay in registers.  The workgroup is sized by 2 t + D + 1 slots of 32
//       bytes a lane to stay inside the default 64 KiB (sumcheck_lanes): 256 lanes up to 7 slots, 128 up to 15 (R1CS with a weight:
//       10), 64 up to 31, and for the shapes beyond (arity 16; 32 points) a 64-lane workgroup of which only the first 32 or 16 lanes
//       own pairs.  A lane owns SUMCHECK_LANE_PAIRS consecutive output pairs (policy, per call; it moves borders and never a byte).
//       A workgroup reduces its lanes' accumulators point by point: six shuffle steps, the wave values through LDS, one partial a
//       point: part[X G + g].  With one workgroup (G = 1) that partial IS the message: fold, sum and reduction are one launch.
//   evals_sum_kernel (evals_impl.cuh)     sums the G partials of every point, 2048 a workgroup, over as many levels as needed.
// No atomics.  The message is copied to the host and the call waits: the verifier's challenge depends on it.
//
// Ownership.  The handle borrows the caller's tables until round 2 has folded them into its own ping-pong buffers: (t + 1) N / 2
// elements for the odd states and (t + 1) N / 4 for the even ones, allocated in `begin` together with the partials of the largest
// round at one pair a lane; no later call allocates, and nothing lives in the context's scratch.  The polynomial program and the
// coefficient pool stay the gr1cs handle's: it must outlive the sumcheck handle.
#pragma once
#include <string>
#include "common.h"
#include "fr_wave.cuh"
#include "gr1cs_impl.cuh"
#include "evals_impl.cuh"
#include "mle_impl.cuh"

namespace ark355 {

constexpr uint32_t SUMCHECK_MAX_POINTS = 32;              // ARK355_SUMCHECK_MAX_POINTS
constexpr uint32_t SUMCHECK_LANE_PAIRS_DEFAULT = 1, SUMCHECK_LANE_PAIRS_MAX = 8;
constexpr uint32_t SUMCHECK_LDS_BYTES = (64u << 10) - 512;   // dynamic part; the wave values of the reduction are static
constexpr uint32_t SUMCHECK_MAX_GRID = 1u << 24;
constexpr uint64_t SUMCHECK_MAX_ELEMS = 1ull << 40;

// policy SUMCHECK_LANE_PAIRS -> the output pairs (outputs, for mle_fold_kernel) a lane owns: <= 0 selects the default, anything
// else is clamped to 1 .. 8
static inline uint32_t sumcheck_lane_pairs(int32_t policy) {
  if (policy <= 0) return SUMCHECK_LANE_PAIRS_DEFAULT;
  return (uint32_t)policy > SUMCHECK_LANE_PAIRS_MAX ? SUMCHECK_LANE_PAIRS_MAX : (uint32_t)policy;
}

static inline uint32_t sumcheck_slots(uint32_t arity, uint32_t points) { return 2 * arity + points; }
// lanes of a workgroup that own pairs: the largest power of two <= 256 whose slots fit SUMCHECK_LDS_BYTES (at least 16: 63 slots)
static inline uint32_t sumcheck_lanes(uint32_t arity, uint32_t points, uint32_t fr_bytes) {
  uint32_t lanes = 256;
  while (lanes > 16 && lanes * sumcheck_slots(arity, points) * fr_bytes > SUMCHECK_LDS_BYTES) lanes >>= 1;
  return lanes;
}
static inline uint32_t sumcheck_block(uint32_t lanes) { return lanes < 64 ? 64 : lanes; }

// the launches of one round over `pairs` output pairs: G workgroups, then evals_sum_kernel over len[1], .. down to 1
struct SumcheckPlan {
  uint32_t run = 1, levels = 0;
  uint64_t len[EVALS_MAX_LEVELS + 2] = {0, 0, 0, 0, 0, 0};
  uint64_t off[EVALS_MAX_LEVELS + 2] = {0, 0, 0, 0, 0, 0};
  uint64_t elems = 0;                // partials of all levels, per point
};
static inline SumcheckPlan sumcheck_plan(uint64_t pairs, uint32_t lanes, uint32_t run) {
  SumcheckPlan p;
  while ((pairs + (uint64_t)lanes * run - 1) / ((uint64_t)lanes * run) > SUMCHECK_MAX_GRID) run *= 2;
  p.run = run;
  p.len[0] = (pairs + (uint64_t)lanes * run - 1) / ((uint64_t)lanes * run);
  if (p.len[0] < 1) p.len[0] = 1;
  while (p.len[p.levels] > 1) {
    p.len[p.levels + 1] = (p.len[p.levels] + EVALS_SUM_CHUNK - 1) / EVALS_SUM_CHUNK;
    p.levels++;
  }
  for (uint32_t l = 0; l < p.levels; l++) {
    p.off[l] = p.elems;
    p.elems += p.len[l];
  }
  return p;
}

struct SumcheckDev {
  int curve = 0, device = -1;
  uint32_t arity = 0, num_vars = 0, points = 0, rounds_done = 0, lanes = 0;
  bool weight = false, finished = false;
  const uint32_t* prog = nullptr;    // borrowed from the gr1cs handle
  const void* pool = nullptr;
  const void* d_tables = nullptr;    // borrowed until round 2 returns (until finish when num_vars <= 1)
  const void* d_weight = nullptr;
  DevBuf odd, even;                  // states 1, 3, .. ((t + 1) N / 2) and 2, 4, .. ((t + 1) N / 4)
  DevBuf part;                       // partials of one round: points x plan.elems
  DevBuf res;                        // the message, then the finals: max(points, t + 1)
};

// P at the lane's current values: vals = [slot][limb][lanes], slot k < arity
template <class Fr>
ARK_D Fr sumcheck_eval_program(const uint32_t* __restrict__ prog, const Fr* __restrict__ pool, const uint32_t* vals, uint32_t lanes,
                               uint32_t lane) {
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
      Fr x;
#pragma unroll
      for (int l = 0; l < Fr::N; l++) x.l[l] = vals[(var * Fr::N + l) * lanes + lane];
      const Fr pw = gr1cs_pow<Fr>(x, e);
      prod = have ? Fr::mul(prod, pw) : pw;
      have = true;
    }
    Fr term = pool[ci];                    // a term without factors is the constant term
    if (have) term = ci ? Fr::mul(prod, term) : prod;
    acc = Fr::add(acc, term);
  }
  return acc;
}

// the two values of output pair i of one table: entries 2i, 2i+1 of the state (FOLD: folded from 4i .. 4i+3 of the previous one with r
// and stored)
template <class Fr, bool FOLD>
ARK_D void sumcheck_pair(const Fr* __restrict__ src, Fr* __restrict__ dst, uint64_t i, const Fr& r, Fr& lo, Fr& hi) {
  if (FOLD) {
    const Fr a = evals_load(src + 4 * i), b = evals_load(src + 4 * i + 1), c = evals_load(src + 4 * i + 2), d = evals_load(src + 4 * i + 3);
    lo = Fr::add(a, Fr::mul(r, Fr::sub(b, a)));
    hi = Fr::add(c, Fr::mul(r, Fr::sub(d, c)));
    evals_store(dst + 2 * i, lo);
    evals_store(dst + 2 * i + 1, hi);
  } else {
    lo = evals_load(src + 2 * i);
    hi = evals_load(src + 2 * i + 1);
  }
}

// blockDim.x = max(lanes, 64); dynamic LDS: (2 arity + D + 1) * 32 * lanes bytes.  part[X gridDim.x + blockIdx.x]
template <class Fr, bool FOLD, bool WEIGHT>
__global__ void __launch_bounds__(256)
sumcheck_round_kernel(const Fr* __restrict__ src, uint64_t src_stride, const Fr* __restrict__ wsrc, Fr* __restrict__ dst, uint64_t dst_stride,
                      Fr* __restrict__ wdst, uint64_t pairs, uint32_t arity, uint32_t D, const uint32_t* __restrict__ prog,
                      const Fr* __restrict__ pool, Fr r, uint32_t lanes, uint32_t run, Fr* __restrict__ part) {
  ARK_DYN_SMEM(uint32_t, lds);             // [2 arity + D + 1][Fr::N][lanes]: current values, differences, accumulators
  __shared__ uint32_t wave_val[2][4][Fr::N];
  const uint32_t tid = threadIdx.x;
  const bool active = tid < lanes;
  const uint32_t acc0 = 2 * arity;
  if (active) {                            // no barrier inside: a lane touches its own words only
    for (uint32_t X = 0; X <= D; X++) {
#pragma unroll
      for (int l = 0; l < Fr::N; l++) lds[((acc0 + X) * Fr::N + l) * lanes + tid] = 0;
    }
    const uint64_t first = ((uint64_t)blockIdx.x * lanes + tid) * run;
    for (uint32_t e = 0; e < run && first + e < pairs; e++) {
      const uint64_t i = first + e;
      for (uint32_t k = 0; k < arity; k++) {
        Fr lo, hi;
        sumcheck_pair<Fr, FOLD>(src + (uint64_t)k * src_stride, dst + (uint64_t)k * dst_stride, i, r, lo, hi);
        hi = Fr::sub(hi, lo);
#pragma unroll
        for (int l = 0; l < Fr::N; l++) {
          lds[(k * Fr::N + l) * lanes + tid] = lo.l[l];
          lds[((arity + k) * Fr::N + l) * lanes + tid] = hi.l[l];
        }
      }
      Fr w = Fr::zero(), wd = Fr::zero();
      if (WEIGHT) {
        sumcheck_pair<Fr, FOLD>(wsrc, wdst, i, r, w, wd);
        wd = Fr::sub(wd, w);
      }
      for (uint32_t X = 0; X <= D; X++) {
        Fr val = sumcheck_eval_program<Fr>(prog, pool, lds, lanes, tid);
        if (WEIGHT) val = Fr::mul(val, w);
        Fr a;
#pragma unroll
        for (int l = 0; l < Fr::N; l++) a.l[l] = lds[((acc0 + X) * Fr::N + l) * lanes + tid];
        a = Fr::add(a, val);
#pragma unroll
        for (int l = 0; l < Fr::N; l++) lds[((acc0 + X) * Fr::N + l) * lanes + tid] = a.l[l];
        if (X == D) break;
        for (uint32_t k = 0; k < arity; k++) {             // the next point: one addition a table
          Fr c, d;
#pragma unroll
          for (int l = 0; l < Fr::N; l++) {
            c.l[l] = lds[(k * Fr::N + l) * lanes + tid];
            d.l[l] = lds[((arity + k) * Fr::N + l) * lanes + tid];
          }
          c = Fr::add(c, d);
#pragma unroll
          for (int l = 0; l < Fr::N; l++) lds[(k * Fr::N + l) * lanes + tid] = c.l[l];
        }
        if (WEIGHT) w = Fr::add(w, wd);
      }
    }
  }
  // the workgroup's sum of every point: waves through shuffles, the wave values through LDS (two buffers, one barrier a point)
  const uint32_t waves = blockDim.x >> 6;
  for (uint32_t X = 0; X <= D; X++) {
    Fr v = Fr::zero();
    if (active) {
#pragma unroll
      for (int l = 0; l < Fr::N; l++) v.l[l] = lds[((acc0 + X) * Fr::N + l) * lanes + tid];
    }
    fr_group_sum<Fr>(v, wave_val[X & 1u], waves, part + (uint64_t)X * gridDim.x + blockIdx.x);
  }
}

// one round's launches on `st` (queued): the message ends in sc.res (points Fr).  FOLD rounds read `src` and write `dst`.
template <class Fr>
static void sumcheck_round_launch(SumcheckDev& sc, bool fold, const Fr* src, uint64_t src_stride, const Fr* wsrc, Fr* dst, uint64_t dst_stride,
                                  Fr* wdst, uint64_t pairs, const Fr& r, uint32_t run, hipStream_t st) {
  const SumcheckPlan plan = sumcheck_plan(pairs, sc.lanes, run);
  const uint32_t D = sc.points - 1;
  const dim3 grid((uint32_t)plan.len[0]), block(sumcheck_block(sc.lanes));
  const size_t smem = (size_t)sumcheck_slots(sc.arity, sc.points) * sizeof(Fr) * sc.lanes;
  Fr* out0 = plan.levels ? sc.part.as<Fr>() : sc.res.as<Fr>();
  const Fr* pool = (const Fr*)sc.pool;
#define ARK_SC_LAUNCH(F, W)                                                                                                       \
  ARK_LAUNCH((sumcheck_round_kernel<Fr, F, W>), grid, block, smem, st, src, src_stride, wsrc, dst, dst_stride, wdst, pairs, sc.arity, D, \
             sc.prog, pool, r, sc.lanes, plan.run, out0)
  if (fold) {
    if (sc.weight) ARK_SC_LAUNCH(true, true);
    else ARK_SC_LAUNCH(true, false);
  } else {
    if (sc.weight) ARK_SC_LAUNCH(false, true);
    else ARK_SC_LAUNCH(false, false);
  }
#undef ARK_SC_LAUNCH
  ARK_CHECK_LAUNCH();
  for (uint32_t l = 0; l < plan.levels; l++) {             // level l: points x len[l] -> points x len[l + 1]
    const bool last = l + 1 == plan.levels;
    const Fr* in = sc.part.as<Fr>() + (uint64_t)sc.points * plan.off[l];
    Fr* out = last ? sc.res.as<Fr>() : sc.part.as<Fr>() + (uint64_t)sc.points * plan.off[l + 1];
    ARK_LAUNCH((evals_sum_kernel<Fr>), dim3((uint32_t)plan.len[l + 1], sc.points), dim3(EVALS_THREADS), 0, st, in, plan.len[l], Fr::zero(), 0u,
               (const unsigned long long*)nullptr, (uint64_t)0, out);
    ARK_CHECK_LAUNCH();
  }
}

// the handle of one run: every refusal and every allocation of the run happens here
template <class Curve>
static SumcheckDev* sumcheck_begin(int device, const Gr1csDev& g, uint32_t p, const void* d_tables, const void* d_weight, uint32_t num_vars) {
  using Fr = typename Curve::Fr;
  const Gr1csPred& P = g.preds[p];
  const uint64_t D = P.degree + (d_weight ? 1 : 0);
  ARK_REQUIRE(P.degree < SUMCHECK_MAX_POINTS && D + 1 <= SUMCHECK_MAX_POINTS, ARK355_EINVAL,
              "ark355_gr1cs_sumcheck_begin_dev: the predicate's degree as written is " + std::to_string(P.degree) + ": a round would take " +
                  (P.degree < (1ull << 32) ? std::to_string(D + 1) : std::string("too many")) +
                  " points, more than ARK355_SUMCHECK_MAX_POINTS");
  std::unique_ptr<SumcheckDev> sc(new SumcheckDev());
  sc->curve = Curve::ID;
  sc->device = device;
  sc->arity = P.arity;
  sc->num_vars = num_vars;
  sc->points = (uint32_t)D + 1;
  sc->weight = d_weight != nullptr;
  sc->prog = P.prog.as<uint32_t>();
  sc->pool = g.pool.p;
  sc->d_tables = d_tables;
  sc->d_weight = d_weight;
  sc->lanes = sumcheck_lanes(P.arity, sc->points, sizeof(Fr));
  const uint64_t N = 1ull << num_vars, t1 = (uint64_t)P.arity + 1;
  if (num_vars >= 2) sc->odd.alloc((size_t)(t1 * (N / 2)) * sizeof(Fr));
  if (num_vars >= 3) sc->even.alloc((size_t)(t1 * (N / 4)) * sizeof(Fr));
  const SumcheckPlan widest = sumcheck_plan(N / 2, sc->lanes, 1);
  sc->part.alloc((size_t)(sc->points * (widest.elems + 1)) * sizeof(Fr));
  sc->res.alloc((size_t)(sc->points > t1 ? sc->points : t1) * sizeof(Fr));
  return sc.release();
}

// state j (after j folds) of the handle: where it lies and the distance between two tables
template <class Fr>
static const Fr* sumcheck_state(const SumcheckDev& sc, uint32_t j, uint64_t* stride, const Fr** weight) {
  *stride = 1ull << (sc.num_vars - j);
  if (j == 0) {
    *weight = (const Fr*)sc.d_weight;
    return (const Fr*)sc.d_tables;
  }
  const Fr* base = (j & 1u) ? sc.odd.as<Fr>() : sc.even.as<Fr>();
  *weight = base + (uint64_t)sc.arity * *stride;
  return base;
}

// round rounds_done + 1: folds with r when it is not the first, leaves the message at out (host, points Fr) and waits
template <class Curve>
static void sumcheck_round(SumcheckDev& sc, const typename Curve::Fr& r, uint32_t run, void* out, hipStream_t st) {
  using Fr = typename Curve::Fr;
  const uint32_t j = sc.rounds_done;                       // the state this round sums
  const uint64_t pairs = 1ull << (sc.num_vars - j - 1);
  uint64_t src_stride = 0, dst_stride = 0;
  const Fr *wsrc = nullptr, *wdst = nullptr;
  if (j == 0) {
    const Fr* src = sumcheck_state<Fr>(sc, 0, &src_stride, &wsrc);
    sumcheck_round_launch<Fr>(sc, false, src, src_stride, wsrc, (Fr*)nullptr, 0, (Fr*)nullptr, pairs, r, run, st);
  } else {
    const Fr* src = sumcheck_state<Fr>(sc, j - 1, &src_stride, &wsrc);
    const Fr* dst = sumcheck_state<Fr>(sc, j, &dst_stride, &wdst);
    sumcheck_round_launch<Fr>(sc, true, src, src_stride, wsrc, const_cast<Fr*>(dst), dst_stride, const_cast<Fr*>(wdst), pairs, r, run, st);
  }
  ARK_CHECK_HIP(hipMemcpyAsync(out, sc.res.p, (size_t)sc.points * sizeof(Fr), hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  sc.rounds_done = j + 1;
  if (j >= 1) sc.d_tables = sc.d_weight = nullptr;         // the borrow ends: the state is the handle's own from here on
}

// folds the last state with r (num_vars >= 1) and leaves T_0, .., T_{t-1}, W at out (host, t + 1 Fr)
template <class Curve>
static void sumcheck_finish(SumcheckDev& sc, const typename Curve::Fr& r, void* out, hipStream_t st) {
  using Fr = typename Curve::Fr;
  Fr* res = sc.res.as<Fr>();
  uint64_t stride = 0;
  const Fr* w = nullptr;
  if (sc.num_vars == 0) {
    const Fr* src = sumcheck_state<Fr>(sc, 0, &stride, &w);
    ARK_CHECK_HIP(hipMemcpyAsync(res, src, (size_t)sc.arity * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    if (sc.weight) ARK_CHECK_HIP(hipMemcpyAsync(res + sc.arity, w, sizeof(Fr), hipMemcpyDeviceToDevice, st));
  } else {
    const Fr* src = sumcheck_state<Fr>(sc, sc.num_vars - 1, &stride, &w);
    mle_fold_launch<Fr>(src, stride, 1, r, res, 1, sc.arity, 1, st);
    if (sc.weight) mle_fold_launch<Fr>(w, stride, 1, r, res + sc.arity, 1, 1, 1, st);
  }
  ARK_CHECK_HIP(hipMemcpyAsync(out, res, (size_t)(sc.arity + (sc.weight ? 1 : 0)) * sizeof(Fr), hipMemcpyDeviceToHost, st));
  ARK_CHECK_HIP(hipStreamSynchronize(st));
  if (!sc.weight) {
    const Fr one = Fr::one();
    memcpy((uint8_t*)out + (size_t)sc.arity * sizeof(Fr), one.l, sizeof(Fr));
  }
  sc.finished = true;
  sc.d_tables = sc.d_weight = nullptr;
}

}  // namespace ark355
