// Every schedule decision of one proof (prove_run, groth16_impl.cuh), computed once from the policy, the resolved schedule and
// what kind of proof it is.  Plain host C++ (no HIP): the rules have their own unit test, tests/cpp/test_prove_plan.cpp, which
// walks the whole input space -- the CPU tier runs every stream as one and never has a second proof in flight, so nothing else
// sees a wrong stream role or the `concurrent` side of a decision before a GPU does.
#pragma once
#include <stdint.h>
#include <atomic>
#include "policy.h"

namespace ark355 {

// Proofs inside prove_run on one device, of EITHER curve: a BLS12-381 and a BN254 proof share the device like two of a kind.
struct InFlight {
  std::atomic<int>& c;
  int mine;          // the count including this proof, at its start
  explicit InFlight(int device) : c(counter(device)), mine(++c) {}
  ~InFlight() { --c; }
  InFlight(const InFlight&) = delete;
  InFlight& operator=(const InFlight&) = delete;
  static std::atomic<int>& counter(int device) {
    static std::atomic<int> per_device[64];
    return per_device[(unsigned)device & 63u];
  }
};

// The stream a piece of work is queued on.  MAIN is the proof's own stream (the lane of a one-stream proof, else the context's
// stream); W, S, R are the context's feeder streams: witness map, sorts, reductions.  prove_run maps roles to streams once.
enum StreamRole : int { ROLE_MAIN = 0, ROLE_W = 1, ROLE_S = 2, ROLE_R = 3, ROLE_COUNT = 4 };

// How the proof's thread leaves: nothing to do (one stream), query the last event of every feeder stream (complete by
// construction), or synchronise the sort and witness-map streams.  Measurements: prove_run's epilogue.
enum ProveEpilogue : int { EPILOGUE_NONE = 0, EPILOGUE_CHECK_EVENTS = 1, EPILOGUE_SYNC = 2 };

struct ProveCase {
  int sched = SCHED_ONE_STREAM;      // resolved: one of SCHED_ONE_STREAM .. SCHED_ONE_STREAM_SPIN
  bool concurrent = false;           // other proofs are in flight on the device
  bool comm = false;                 // a rank of ark355_prove_sharded (a collective: every rank must queue the same operations)
  bool ring = false;                 // ... combining by the bucket-level ring instead of the all-gather of window sums
  bool partials = false;             // ark355_prove_shard: hands back partial sums
  bool h_dist = false;               // PkDev::h_dist: the h query shard is in the layout of the distributed witness map
  uint32_t shard_count = 1;          // PkDev::shard_count
};

struct ProvePlan {
  bool one_stream = false;
  bool spin = false;                 // waits inside the HIP runtime
  bool plain = false;                // ark355_prove / _dev / _batch: a whole proof of a whole key
  // policy CHECK_SATISFIED: whole proofs of a whole key only (a rank of a sharded proof sees 1/G of the rows, and the ranks of a
  // collective must not disagree on its outcome)
  bool check_sat = false;
  bool dist_wm = false;              // the witness map sharded like the MSMs (witness_dist_impl.cuh)
  bool ring = false;
  // A one-stream proof that is ALONE on the device (policy SIDE_WM): the witness map and the sort of h beside the sort of z and the
  // accumulations of B2, A, B1 and L' instead of in front of them.
  bool side_wm = false;
  // One-stream proofs: the G1 tails of the four MSMs as one launch per step, behind the five accumulations.
  bool batch_tails = false;
  bool side_g2 = false;              // ... and, the proof being alone, its G2 tails underneath the four G1 accumulations
  bool side_g1 = false;              // ... and the tails of A, B1, L' as a batch of three behind them, under the H accumulation
  bool side_h_tails = false;         // multi-stream schedules: the tails of H on the sort stream, idle since the sort of h
  int acc_threads = 256;             // workgroup size of the LDS-free accumulation kernels: one wave for a proof alone on one stream
  ProveEpilogue epilogue = EPILOGUE_NONE;
  bool needs_feeders = false;        // some role is not MAIN: the context's three feeder streams must exist
  StreamRole wm = ROLE_MAIN;         // witness map (and, for a key shard, the part of the assignment only it needs)
  StreamRole sort_z = ROLE_MAIN;     // the one clearing dispatch and the sort of zx
  StreamRole sort_h = ROLE_MAIN;
  StreamRole acc = ROLE_MAIN;        // the five accumulations: always the proof's own stream
  StreamRole reduce = ROLE_MAIN;     // tails that are not moved aside, the last copy, the all-gather
  StreamRole g2_tails = ROLE_MAIN;
  StreamRole g1_side_tails = ROLE_MAIN;   // the batch of A, B1, L' (differs from `reduce` only with side_g1)
  StreamRole h_tails = ROLE_MAIN;
};

static inline ProvePlan prove_plan(const TunePolicy& pol, const ProveCase& k) {
  ProvePlan p;
  p.one_stream = k.sched == SCHED_ONE_STREAM || k.sched == SCHED_ONE_STREAM_SPIN;
  p.spin = pol.wait_spin != 0 || k.sched == SCHED_ONE_STREAM_SPIN;
  p.plain = !k.comm && !k.partials;
  // (the bucket ring interleaves its own send / receive steps with the MSMs and therefore keeps the replicated map; without a
  // communicator only the timing diagnostic DWM_LOOPBACK runs the distributed map)
  p.ring = k.comm && k.ring;
  p.dist_wm = k.h_dist && (k.comm ? !k.ring : pol.dwm_loopback != 0);
  // (the check is a by-product of the replicated witness map: the distributed one neither allocates nor clears its verdict)
  p.check_sat = pol.check_satisfied != 0 && p.plain && k.shard_count <= 1 && !p.dist_wm;
  p.side_wm = p.one_stream && !k.concurrent && p.plain && pol.side_wm != 0;
  p.batch_tails = p.one_stream && !k.comm && pol.batch_tails != 0;
  // with other proofs in flight everything stays on the one stream (a second stream per proof is exactly what the one-stream
  // schedule exists to avoid)
  p.side_g2 = p.batch_tails && !k.concurrent && pol.side_g2_tails != 0;
  p.side_g1 = p.side_g2 && pol.side_g1_tails != 0;
  // (not with the bucket ring: its grouped sends must be queued in one order on every rank)
  p.side_h_tails = !p.one_stream && !p.ring && pol.side_h_tails != 0;
  p.acc_threads = (p.one_stream && !k.concurrent) ? 64 : 256;
  p.epilogue = k.sched == SCHED_PIPELINE_SYNC ? EPILOGUE_SYNC : (p.one_stream ? EPILOGUE_NONE : EPILOGUE_CHECK_EVENTS);
  p.wm = (p.one_stream && !p.side_wm) ? ROLE_MAIN : ROLE_W;
  p.sort_z = p.one_stream ? ROLE_MAIN : ROLE_S;
  p.sort_h = p.side_wm ? ROLE_W : p.sort_z;
  p.acc = ROLE_MAIN;
  p.reduce = p.one_stream ? ROLE_MAIN : ROLE_R;
  p.g2_tails = p.side_g2 ? ROLE_R : p.reduce;
  p.g1_side_tails = p.side_g1 ? ROLE_R : p.reduce;
  p.h_tails = p.side_h_tails ? p.sort_z : p.reduce;
  p.needs_feeders = !p.one_stream || p.side_wm || p.side_g2;
  return p;
}

}  // namespace ark355
