// Unit test of snark_amd/csrc/prove_plan.h (host-only logic): every schedule decision of a proof, over the WHOLE input space --
// 4 schedules x alone / in flight x plain / partials / communicator x both exchange modes x the on/off policies x key layouts.
// The checks are the rules that the comments of prove_run state, not a table copied from prove_plan().  The CPU tier cannot see
// them fail: its emulator runs every stream as one and never has a second proof in flight.
// g++ -std=c++17 -I snark_amd/csrc tests/cpp/test_prove_plan.cpp
#include <cstdio>
#include <initializer_list>
#include "prove_plan.h"

using namespace ark355;

static int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      if (failures < 20) fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                                    \
    }                                                                \
  } while (0)
#define IMPLIES(a, b) CHECK(!(a) || (b))

static bool all_main(const ProvePlan& p) {
  for (StreamRole r : {p.wm, p.sort_z, p.sort_h, p.acc, p.reduce, p.g2_tails, p.g1_side_tails, p.h_tails})
    if (r != ROLE_MAIN) return false;
  return true;
}

static bool same(const ProvePlan& a, const ProvePlan& b) {
  return a.one_stream == b.one_stream && a.spin == b.spin && a.plain == b.plain && a.check_sat == b.check_sat && a.dist_wm == b.dist_wm &&
         a.ring == b.ring && a.side_wm == b.side_wm && a.batch_tails == b.batch_tails && a.side_g2 == b.side_g2 && a.side_g1 == b.side_g1 &&
         a.side_h_tails == b.side_h_tails && a.acc_threads == b.acc_threads && a.epilogue == b.epilogue &&
         a.needs_feeders == b.needs_feeders && a.wm == b.wm && a.sort_z == b.sort_z && a.sort_h == b.sort_h && a.acc == b.acc &&
         a.reduce == b.reduce && a.g2_tails == b.g2_tails && a.g1_side_tails == b.g1_side_tails && a.h_tails == b.h_tails;
}
// everything but the accumulation workgroup size
static bool same_but_acc_threads(ProvePlan a, ProvePlan b) {
  a.acc_threads = b.acc_threads = 0;
  return same(a, b);
}

// the on/off policies a plan reads, as bits of `knobs`
enum { K_SIDE_WM, K_SIDE_G2, K_SIDE_G1, K_BATCH, K_SIDE_H, K_SPIN, K_CHECK_SAT, K_LOOPBACK, K_COUNT };
static TunePolicy policy_of(unsigned knobs) {
  TunePolicy pol;
  pol.side_wm = (knobs >> K_SIDE_WM) & 1;
  pol.side_g2_tails = (knobs >> K_SIDE_G2) & 1;
  pol.side_g1_tails = (knobs >> K_SIDE_G1) & 1;
  pol.batch_tails = (knobs >> K_BATCH) & 1;
  pol.side_h_tails = (knobs >> K_SIDE_H) & 1;
  pol.wait_spin = (knobs >> K_SPIN) & 1;
  pol.check_satisfied = (knobs >> K_CHECK_SAT) & 1;
  pol.dwm_loopback = (knobs >> K_LOOPBACK) & 1;
  return pol;
}

static void check_rules(const TunePolicy& pol, const ProveCase& k) {
  const ProvePlan p = prove_plan(pol, k);
  const bool one = k.sched == SCHED_ONE_STREAM || k.sched == SCHED_ONE_STREAM_SPIN;
  CHECK(p.one_stream == one);
  CHECK(p.acc == ROLE_MAIN);                                  // the accumulations never leave the proof's own stream
  CHECK(p.plain == (!k.comm && !k.partials));
  // a one-stream proof with others in flight: everything on the one stream, no feeder stream
  IMPLIES(one && k.concurrent, all_main(p) && !p.needs_feeders);
  CHECK(p.needs_feeders == !all_main(p));
  // the side streams of a one-stream proof: G1 aside => G2 aside => batched tails => one stream, no communicator; aside => alone
  IMPLIES(p.side_g1, p.side_g2);
  IMPLIES(p.side_g2, p.batch_tails && !k.concurrent);
  IMPLIES(p.batch_tails, one && !k.comm);
  IMPLIES(p.side_wm, one && !k.concurrent && !k.comm && !k.partials);
  IMPLIES(one, p.side_wm == (p.wm == ROLE_W) && p.side_wm == (p.sort_h == ROLE_W));
  IMPLIES(one, p.side_g2 == (p.g2_tails == ROLE_R) && p.side_g1 == (p.g1_side_tails == ROLE_R));
  IMPLIES(one, p.sort_z == ROLE_MAIN && p.reduce == ROLE_MAIN && p.h_tails == ROLE_MAIN && p.epilogue == EPILOGUE_NONE);
  // the five-stream pipeline: fixed roles, only the tails of H may move (to the sort stream)
  IMPLIES(!one, p.wm == ROLE_W && p.sort_z == ROLE_S && p.sort_h == ROLE_S && p.reduce == ROLE_R && p.g2_tails == ROLE_R &&
                    p.g1_side_tails == ROLE_R && (p.h_tails == ROLE_R || p.h_tails == ROLE_S));
  IMPLIES(!one, p.side_h_tails == (p.h_tails == ROLE_S));
  IMPLIES(!one, !p.side_wm && !p.batch_tails && p.epilogue == (k.sched == SCHED_PIPELINE_SYNC ? EPILOGUE_SYNC : EPILOGUE_CHECK_EVENTS));
  // the ring never moves the tails of H aside and never batches tails: its grouped sends are queued in one order on every rank
  CHECK(p.ring == (k.comm && k.ring));
  IMPLIES(p.ring, !p.side_h_tails && !p.batch_tails && p.h_tails == p.reduce);
  // the ring keeps the replicated witness map; the distributed one needs the key shard in its layout
  IMPLIES(p.dist_wm, k.h_dist && !p.ring);
  IMPLIES(p.dist_wm && !k.comm, pol.dwm_loopback != 0);
  IMPLIES(k.comm && k.h_dist && !k.ring, p.dist_wm);
  // CHECK_SATISFIED: plain proofs of a whole key only
  IMPLIES(p.check_sat, p.plain && k.shard_count <= 1 && pol.check_satisfied != 0);
  IMPLIES(pol.check_satisfied != 0 && p.plain && k.shard_count <= 1 && !p.dist_wm, p.check_sat);
  // ... and only with the replicated witness map, whose by-product the verdict is: a whole key in the layout of the distributed
  // map under DWM_LOOPBACK never runs it, and prove_run would copy a verdict nobody allocated
  IMPLIES(p.check_sat, !p.dist_wm);
  // one wave per workgroup only for a proof alone on one stream
  CHECK(p.acc_threads == ((one && !k.concurrent) ? 64 : 256));
  CHECK(p.spin == (pol.wait_spin != 0 || k.sched == SCHED_ONE_STREAM_SPIN));
  // A sharded proof is a collective: every rank queues the same operations whatever else runs on ITS device, and whatever the
  // policies of a lone one-stream proof say.
  if (k.comm) {
    ProveCase other = k;
    other.concurrent = !k.concurrent;
    CHECK(same_but_acc_threads(p, prove_plan(pol, other)));
    for (int bit : {K_SIDE_WM, K_SIDE_G2, K_SIDE_G1, K_BATCH}) {
      TunePolicy flipped = pol;
      int32_t* f = bit == K_SIDE_WM ? &flipped.side_wm : bit == K_SIDE_G2 ? &flipped.side_g2_tails : bit == K_SIDE_G1 ? &flipped.side_g1_tails : &flipped.batch_tails;
      *f = !*f;
      const ProvePlan q = prove_plan(flipped, k);
      CHECK(same(p, q));
    }
  }
}

// two curves = two instantiations of the prover: they must meet in ONE counter per device
template <int CurveId>
static int proofs_in_flight_seen_by_a_new_proof(int device) {
  InFlight me(device);
  return me.mine;
}

int main() {
  unsigned cases = 0;
  for (int sched = 0; sched < SCHED_COUNT; sched++)
    for (int concurrent = 0; concurrent < 2; concurrent++)
      for (int kind = 0; kind < 4; kind++)                  // plain, partials, communicator + all-gather, communicator + ring
        for (int h_dist = 0; h_dist < 2; h_dist++)
          for (uint32_t shard_count : {1u, 4u})
            for (unsigned knobs = 0; knobs < (1u << K_COUNT); knobs++) {
              ProveCase k;
              k.sched = sched;
              k.concurrent = concurrent != 0;
              k.partials = kind == 1;
              k.comm = kind >= 2;
              k.ring = kind == 3;
              k.h_dist = h_dist != 0;
              k.shard_count = shard_count;
              check_rules(policy_of(knobs), k);
              // without a communicator the exchange mode is never read
              if (!k.comm) {
                ProveCase r = k;
                r.ring = true;
                const ProvePlan a = prove_plan(policy_of(knobs), k), b = prove_plan(policy_of(knobs), r);
                CHECK(same(a, b));
              }
              cases++;
            }
  // the default policy gives today's plans
  {
    const TunePolicy def;
    ProveCase k;
    k.sched = SCHED_ONE_STREAM;
    const ProvePlan alone = prove_plan(def, k);
    CHECK(alone.side_wm && alone.batch_tails && alone.side_g2 && !alone.side_g1 && alone.acc_threads == 64 && !alone.check_sat && !alone.spin);
    CHECK(alone.wm == ROLE_W && alone.sort_h == ROLE_W && alone.g2_tails == ROLE_R && alone.g1_side_tails == ROLE_MAIN && alone.needs_feeders);
    k.concurrent = true;
    const ProvePlan shared = prove_plan(def, k);
    CHECK(shared.batch_tails && !shared.side_wm && !shared.side_g2 && shared.acc_threads == 256 && all_main(shared));
    k.sched = SCHED_PIPELINE;
    k.concurrent = false;
    k.comm = true;
    k.h_dist = true;
    k.shard_count = 8;
    const ProvePlan rank = prove_plan(def, k);
    CHECK(rank.h_tails == ROLE_S && rank.acc_threads == 256 && rank.dist_wm && rank.epilogue == EPILOGUE_CHECK_EVENTS && !rank.batch_tails);
    k.ring = true;
    const ProvePlan ring_rank = prove_plan(def, k);
    CHECK(ring_rank.h_tails == ROLE_R && !ring_rank.dist_wm);
  }
  // the in-flight counter: per device, shared by the curves
  {
    InFlight bls(5);
    CHECK(bls.mine == 1);
    CHECK(proofs_in_flight_seen_by_a_new_proof<1>(5) == 2 && proofs_in_flight_seen_by_a_new_proof<2>(5) == 2);
    CHECK(proofs_in_flight_seen_by_a_new_proof<2>(6) == 1);
    {
      InFlight bn(5);
      CHECK(bn.mine == 2 && bls.c.load() == 2);
    }
    CHECK(bls.c.load() == 1);
  }
  CHECK(InFlight::counter(5).load() == 0);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("prove plan: all checks passed (%u cases)\n", cases);
  return 0;
}
