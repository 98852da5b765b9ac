// extern "C" surface of libark355.so (include/ark355.h).  No C++ exception crosses this boundary:
// every entry point catches and maps to an error code (the reference builds with panic='abort' for
// exactly that reason, /root/reference/Cargo.toml:33,45).
#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <thread>
#include "api_impl.cuh"
#include "diag_field_impl.cuh"     // ark355_diag_field_ops: its kernels are compiled in this translation unit only

namespace ark355 {
extern template struct Api<BlsCurve>;
extern template struct Api<BnCurve>;
}  // namespace ark355

using namespace ark355;

struct ark355_pk {
  PkDev* d;
};
struct ark355_r1cs {
  R1csDev* d;
};
struct ark355_gr1cs {
  Gr1csDev* d;
};
struct ark355_sr1cs {
  Sr1csDev* d;
  ark355_gr1cs view;     // borrows d->sys: handed out by ark355_sr1cs_system, never freed on its own
};
struct ark355_bases {
  BasesDev* d;
};
struct ark355_comm {
  CommDev* d;
};
struct ark355_pvk {
  PvkDev* d;
};
struct ark355_sumcheck {
  SumcheckDev* d;
};

namespace {
struct CtxExtra {
  ProverScratch prover;
  GenericScratch generic;
  QuotientScratch quotient;
  ColumnsScratch columns;
  PolyScratch poly;
  EvalsScratch evals;
  MleScratch mle;
  MsmBatchScratch msm_batch;
  std::vector<ark355_ctx*> lanes;     // child contexts of ark355_prove_batch (same device, private streams/scratch)
  ~CtxExtra();
};
std::mutex g_extra_mu;
std::map<ark355_ctx*, CtxExtra*> g_extra;

CtxExtra& extra(ark355_ctx* ctx) {
  std::lock_guard<std::mutex> lk(g_extra_mu);
  auto it = g_extra.find(ctx);
  if (it == g_extra.end()) it = g_extra.emplace(ctx, new CtxExtra()).first;
  return *it->second;
}

CtxExtra::~CtxExtra() {
  for (ark355_ctx* c : lanes) ark355_ctx_destroy(c);
}

// locked: the caller already holds ctx->mu (ark355_diag_streams takes every context's mutex in one sorted try-lock pass)
template <class Fn>
int32_t guarded(ark355_ctx* ctx, Fn&& fn, bool locked = false) {
  try {
    if (ctx && !locked) {
      std::lock_guard<std::mutex> lk(ctx->mu);
      (void)hipSetDevice(ctx->device);
      fn();
    } else {
      if (ctx) (void)hipSetDevice(ctx->device);
      fn();
    }
    return ARK355_OK;
  } catch (const HipError& e) {
    if (ctx) ctx->last_error = e.what;
    return e.code;
  } catch (const std::bad_alloc&) {
    if (ctx) ctx->last_error = "host allocation failed";
    return ARK355_ENOMEM;
  } catch (const std::exception& e) {
    if (ctx) ctx->last_error = e.what();
    return ARK355_EINVAL;
  } catch (...) {
    if (ctx) ctx->last_error = "unknown error";
    return ARK355_EINVAL;
  }
}

#define CURVE_DISPATCH(curve, CALL)                                           \
  do {                                                                        \
    if ((curve) == ARK355_BLS12_381) {                                        \
      using A = Api<BlsCurve>;                                                \
      CALL;                                                                   \
    } else if ((curve) == ARK355_BN254) {                                     \
      using A = Api<BnCurve>;                                                 \
      CALL;                                                                   \
    } else {                                                                  \
      throw HipError{ARK355_EINVAL, "unknown curve id"};                      \
    }                                                                         \
  } while (0)
}  // namespace

extern "C" {

uint32_t ark355_version(void) { return (0u << 16) | 4u; }

int32_t ark355_sizes(int32_t curve, uint32_t what[4]) {
  return guarded(nullptr, [&] { CURVE_DISPATCH(curve, A::sizes(what)); });
}

int32_t ark355_ctx_create(int32_t device_id, ark355_ctx** out) {
  if (!out) return ARK355_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return ARK355_ENODEV;
  if (device_id < 0 || device_id >= count) return ARK355_EINVAL;
  ark355_ctx* ctx = new (std::nothrow) ark355_ctx();
  if (!ctx) return ARK355_ENOMEM;
  ctx->device = device_id;
  bool poison_in_env = false;
  ctx->policy = TunePolicy::from_env(&poison_in_env);       // the ONLY place the policy's environment is read (policy.h)
  // POISON_ALLOC is process-wide: the environment sets the one copy at the FIRST context that finds the variable (later contexts must
  // not undo an ark355_ctx_set_policy made in between); every context reports the copy's value
  static std::atomic<bool> poison_env_applied{false};
  if (poison_in_env && !poison_env_applied.exchange(true))
    poison_alloc_byte().store(poison_alloc_clamp(ctx->policy.poison_alloc), std::memory_order_relaxed);
  ctx->policy.poison_alloc = poison_alloc_byte().load(std::memory_order_relaxed);
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&ctx->stream) != hipSuccess) {
    delete ctx;
    return ARK355_EHIP;
  }
  // streams for one-stream proofs, probed (once per device, now: the device is idle) to sit on different hardware queues
  try {
    uint32_t want = 4;
    if (const char* e = getenv("GPU_MAX_HW_QUEUES")) {
      const int v = atoi(e);
      if (v >= 1 && v <= 16) want = (uint32_t)v;
    }
    LanePool::of(device_id).build(want);
  } catch (...) {
  }
  *out = ctx;
  return ARK355_OK;
}

void ark355_ctx_destroy(ark355_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  CtxExtra* ex = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_extra_mu);
    auto it = g_extra.find(ctx);
    if (it != g_extra.end()) {
      ex = it->second;
      g_extra.erase(it);
    }
  }
  delete ex;       // outside the lock: it destroys the batch worker contexts, which come back through here
  ctx->ntt_tables.clear();          // shared tables live on while another context of the device holds them
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int32_t ark355_host_alloc(uint64_t bytes, void** out) {
  if (!out) return ARK355_EINVAL;
  *out = nullptr;
  void* p = pinned_alloc(bytes);
  if (!p) return ARK355_ENOMEM;
  *out = p;
  return ARK355_OK;
}
void ark355_host_free(void* p) {
  pinned_free(p);
}

const char* ark355_last_error(const ark355_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int32_t ark355_ctx_set_policy(ark355_ctx* ctx, const char* name, int64_t value) {
  if (!ctx || !name) return ARK355_EINVAL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (ctx->policy.set(name, value) != 0) {
    ctx->last_error = std::string("unknown policy name: ") + name;
    return ARK355_EINVAL;
  }
  if (strcmp(name, "POISON_ALLOC") == 0) {
    ctx->policy.poison_alloc = poison_alloc_clamp(value);
    poison_alloc_byte().store(ctx->policy.poison_alloc, std::memory_order_relaxed);
  }
  return ARK355_OK;
}
int32_t ark355_ctx_get_policy(ark355_ctx* ctx, const char* name, int64_t* value) {
  if (!ctx || !name || !value) return ARK355_EINVAL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (strcmp(name, "POISON_ALLOC") == 0) ctx->policy.poison_alloc = poison_alloc_byte().load(std::memory_order_relaxed);   // process-wide
  return ctx->policy.get(name, value) == 0 ? ARK355_OK : ARK355_EINVAL;
}
int32_t ark355_sched_info(const ark355_ctx* ctx, const ark355_pk* pk, int32_t in_flight, ark355_sched_report* out) {
  if (!ctx || !pk || !pk->d || !out) return ARK355_EINVAL;
  memset(out, 0, sizeof(*out));
  out->latched = -1;
  out->last = ctx->last_sched;
  double mean[SCHED_COUNT];
  uint32_t n[SCHED_COUNT];
  int latched = -1;
  const uint64_t key = SchedTuner::key(prove_shape(pk->d->curve, pk->d->N, pk->d->m), in_flight != 0);
  if (SchedTuner::of(ctx->device).info(key, &latched, mean, n)) {
    out->latched = latched;
    static_assert(SCHED_COUNT == 4, "ark355_sched_report holds four schedules");
    for (int v = 0; v < SCHED_COUNT; v++) {
      out->mean_ms[v] = mean[v];
      out->samples[v] = n[v];
    }
  }
  return ARK355_OK;
}
int32_t ark355_diag_streams(ark355_ctx** ctxs, uint32_t count, int8_t* serialised) {
  if (!ctxs || !serialised || count == 0 || count > 16) return ARK355_EINVAL;
  for (uint32_t i = 0; i < count; i++)
    if (!ctxs[i]) return ARK355_EINVAL;
  // The probe synchronises and launches on EVERY passed context's stream, so every one of them is locked for its duration --
  // ctxs[0] included, all in ONE pass of try-locks in address order: no caller ever blocks while it holds a mutex, so two callers
  // with overlapping sets cannot deadlock (ctxs[0] used to be locked blockingly after the others), and a context
  // that is proving right now makes the call fail instead of racing with it.  The bookkeeping allocates: it
  // sits inside the same exception mapping as everything else.
  std::vector<std::unique_lock<std::mutex>> held;
  try {
    std::vector<ark355_ctx*> all(ctxs, ctxs + count);
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    for (ark355_ctx* c : all) {
      std::unique_lock<std::mutex> lk(c->mu, std::try_to_lock);
      if (!lk.owns_lock()) return ARK355_EINVAL;          // busy: the diagnostic wants an idle device
      held.push_back(std::move(lk));
    }
  } catch (const std::bad_alloc&) {
    return ARK355_ENOMEM;
  } catch (...) {
    return ARK355_EINVAL;
  }
  // streams probed: every context's own stream, then the three feeder streams of ctxs[0] (created if need be)
  return guarded(ctxs[0], [&] {
    CtxExtra& ex = extra(ctxs[0]);
    ex.prover.ensure_streams(ctxs[0]->policy.stream_prio != 0);
    std::vector<hipStream_t> st;
    for (uint32_t i = 0; i < count; i++) st.push_back(ctxs[i]->stream);
    st.push_back(ex.prover.sW);
    st.push_back(ex.prover.sS);
    st.push_back(ex.prover.sR);
    const size_t n = st.size();
    for (size_t i = 0; i < n; i++)
      for (size_t j = 0; j < n; j++)
        serialised[i * n + j] = (int8_t)(i == j ? 1 : diag_streams_serialised(st[i], st[j]));
  }, /*locked=*/true);
}
int32_t ark355_diag_dispatch(ark355_ctx* ctx, uint32_t launches, uint32_t spin_us, float* gap_us, uint32_t* lanes) {
  if (!ctx || !gap_us || launches == 0 || launches > 100000 || spin_us > 100000) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    *gap_us = diag_dispatch_gap_us(ctx->stream, launches, spin_us);
    if (lanes) *lanes = (uint32_t)LanePool::of(ctx->device).size();
  });
}
int32_t ark355_diag_mad_rate(ark355_ctx* ctx, float target_ms, float* tmad_per_s, float* elapsed_ms) {
  if (!ctx || !tmad_per_s || !(target_ms >= 0.1f) || target_ms > 1000.f) return ARK355_EINVAL;
  return guarded(ctx, [&] { *tmad_per_s = diag_mad_rate_t(ctx->stream, ctx->device, target_ms, elapsed_ms); });
}
int32_t ark355_diag_clocks(ark355_ctx* ctx, uint64_t* pairs, uint32_t capacity, uint32_t* count) {
  if (!ctx || !pairs || !count || capacity < DIAG_CLOCK_SLOTS) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    diag_clocks(ctx->stream, pairs);
    *count = DIAG_CLOCK_SLOTS;
  });
}
int32_t ark355_diag_msm_sort(ark355_ctx* ctx, int32_t curve, const ark355_bases* bases, const uint8_t* scalars, uint64_t n,
                             int32_t scalars_mont, uint32_t plan[ARK355_SORT_PLAN_WORDS], uint32_t* counts, uint32_t* offsets,
                             uint64_t bucket_capacity, uint32_t* sorted_keys, uint32_t* sorted_vals, uint64_t entry_capacity,
                             uint32_t* total) {
  if (!ctx || !plan || !total || (n && !scalars) || (bases && !bases->d)) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::diag_msm_sort(ctx, ex.generic, bases ? bases->d : nullptr, scalars, n, scalars_mont, plan, counts, offsets,
                                           bucket_capacity, sorted_keys, sorted_vals, entry_capacity, total));
  });
}
int32_t ark355_diag_field_ops(ark355_ctx* ctx, int32_t field, int32_t op, const uint32_t* const* operands, uint32_t operand_count,
                              uint64_t n, uint32_t* result, uint64_t result_capacity, uint32_t* flavour) {
  // every refusal below happens before any HIP call
  if (!ctx || !operands || !result || !flavour) return ARK355_EINVAL;
  FieldOpShape shape{};
  if (!diag_field_op_shape(field, op, shape)) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->last_error = "field diagnostic: unknown field / operation, or a combination the library does not instantiate";
    return ARK355_EINVAL;
  }
  if (operand_count != (uint32_t)shape.arity || n > ARK355_FIELD_OPS_MAX_N || result_capacity < n * (uint64_t)shape.out_words) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->last_error = "field diagnostic: operand count, element count or result capacity does not fit the operation";
    return ARK355_EINVAL;
  }
  for (int j = 0; j < shape.arity; j++)
    if (!operands[j]) return ARK355_EINVAL;
  return guarded(ctx, [&] { diag_field_ops_run(ctx->stream, field, op, shape, operands, n, result, flavour); });
}
int32_t ark355_sched_reset(const ark355_ctx* ctx) {
  if (!ctx) return ARK355_EINVAL;
  SchedTuner::of(ctx->device).reset();
  return ARK355_OK;
}

int32_t ark355_pk_load(ark355_ctx* ctx, int32_t curve, const ark355_pk_desc* desc, ark355_pk** out) {
  if (!ctx || !desc || !out) return ARK355_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    PkDev* d = nullptr;
    CURVE_DISPATCH(curve, d = A::pk_load(ctx->policy, desc, ctx->stream));
    *out = new ark355_pk{d};
  });
}
int32_t ark355_pk_load_shard(ark355_ctx* ctx, int32_t curve, const ark355_pk_desc* desc, uint32_t shard_index,
                             uint32_t shard_count, ark355_pk** out) {
  if (!ctx || !desc || !out) return ARK355_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    PkDev* d = nullptr;
    CURVE_DISPATCH(curve, d = A::pk_load(ctx->policy, desc, ctx->stream, shard_index, shard_count));
    *out = new ark355_pk{d};
  });
}
void ark355_pk_free(ark355_pk* pk) {
  if (!pk) return;
  delete pk->d;
  delete pk;
}

int32_t ark355_r1cs_load(ark355_ctx* ctx, int32_t curve, uint64_t n, uint64_t ell, uint64_t w,
                         const uint64_t* const row_ptr[3], const uint32_t* const col[3],
                         const uint8_t* const coeff[3], ark355_r1cs** out) {
  if (!ctx || !row_ptr || !col || !coeff || !out) return ARK355_EINVAL;
  *out = nullptr;
  for (int i = 0; i < 3; i++)
    if (!row_ptr[i]) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    R1csDev* d = nullptr;
    CURVE_DISPATCH(curve, d = A::r1cs_load(n, ell, w, row_ptr, col, coeff));
    d->device = ctx->device;
    *out = new ark355_r1cs{d};
  });
}
void ark355_r1cs_free(ark355_r1cs* r) {
  if (!r) return;
  delete r->d;
  delete r;
}
uint64_t ark355_r1cs_domain_size(const ark355_r1cs* r) { return r ? r->d->N : 0; }

// locked: the caller already holds ctx->mu (the parent lane of ark355_prove_batch)
static int32_t prove_common(ark355_ctx* ctx, const ark355_pk* pk, const ark355_r1cs* r1, const void* z, uint64_t z_len,
                            bool on_dev, const uint8_t* r, const uint8_t* s, ark355_proof_raw* out, bool locked = false) {
  if (!ctx || !pk || !r1 || !r || !s || !out) return ARK355_EINVAL;
  if (!z) {
    ctx->last_error = "null assignment pointer";
    return ARK355_EINVAL;
  }
  if (z_len < r1->d->m) {
    ctx->last_error = "assignment shorter than num_instance + num_witness";
    return ARK355_E_ASSIGNMENT_MISSING;
  }
  if (pk->d->shard_count != 1) {
    ctx->last_error = "this key handle is an MSM shard: use ark355_prove_shard + ark355_prove_combine";
    return ARK355_EINVAL;
  }
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(pk->d->curve, A::prove(ctx, ex.prover, *pk->d, *r1->d, z, on_dev, r, s, out));
  }, locked);
}

int32_t ark355_prove(ark355_ctx* ctx, const ark355_pk* pk, const ark355_r1cs* r1, const uint8_t* z, uint64_t z_len,
                     const uint8_t r[32], const uint8_t s[32], ark355_proof_raw* out) {
  return prove_common(ctx, pk, r1, z, z_len, false, r, s, out);
}
int32_t ark355_prove_dev(ark355_ctx* ctx, const ark355_pk* pk, const ark355_r1cs* r1, const void* d_z, uint64_t z_len,
                         const uint8_t r[32], const uint8_t s[32], ark355_proof_raw* out) {
  return prove_common(ctx, pk, r1, d_z, z_len, true, r, s, out);
}

int32_t ark355_prove_batch(ark355_ctx* ctx, const ark355_pk* pk, const ark355_r1cs* r1, const uint8_t* const* z,
                           uint64_t z_len, const uint8_t* r, const uint8_t* s, uint64_t count, uint32_t inflight,
                           ark355_proof_raw* out) {
  if (!ctx || !pk || !r1 || (count && (!z || !r || !s || !out))) return ARK355_EINVAL;
  if (inflight < 1 || inflight > 16) return ARK355_EINVAL;
  if (count == 0) return ARK355_OK;
#if defined(ARK_EMUL)
  inflight = 1;                        // the test-only emulator is single-threaded
#endif
  if (inflight > count) inflight = (uint32_t)count;
  int32_t first_err = ARK355_OK;
  std::string first_msg;
  const int32_t rc = guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    while (ex.lanes.size() + 1 < inflight) {
      ark355_ctx* c = nullptr;
      const int32_t e = ark355_ctx_create(ctx->device, &c);
      if (e != ARK355_OK) throw HipError{e, "ark355_prove_batch: cannot create a worker context"};
      ex.lanes.push_back(c);
    }
    for (ark355_ctx* c : ex.lanes) c->policy = ctx->policy;       // the workers prove under the caller's policy
    std::atomic<uint64_t> next{0};
    std::mutex err_mu;
    auto work = [&](ark355_ctx* lane) {
      for (;;) {
        const uint64_t i = next.fetch_add(1);
        if (i >= count) return;
        // (the parent's mutex is already held by this call: its share runs on the calling thread)
        const int32_t e = prove_common(lane, pk, r1, z[i], z_len, false, r + 32 * i, s + 32 * i, out + i, /*locked=*/lane == ctx);
        if (e != ARK355_OK) {
          std::lock_guard<std::mutex> lk(err_mu);
          if (first_err == ARK355_OK) {
            first_err = e;
            first_msg = "proof " + std::to_string(i) + ": " + lane->last_error;
          }
        }
      }
    };
    std::vector<std::thread> th;
    for (uint32_t k = 1; k < inflight; k++) th.emplace_back(work, ex.lanes[k - 1]);
    work(ctx);
    for (auto& t : th) t.join();
  });
  if (rc != ARK355_OK) return rc;
  if (first_err != ARK355_OK) ctx->last_error = first_msg;
  return first_err;
}

uint64_t ark355_partial_size(int32_t curve) {
  size_t n = 0;
  try {
    CURVE_DISPATCH(curve, n = A::partial_size());
  } catch (...) {
    return 0;
  }
  return n;
}

int32_t ark355_prove_shard(ark355_ctx* ctx, const ark355_pk* pk, const ark355_r1cs* r1, const uint8_t* z, uint64_t z_len,
                           const uint8_t r[32], const uint8_t s[32], uint8_t* out_partials) {
  if (!ctx || !pk || !r1 || !z || !r || !s || !out_partials) return ARK355_EINVAL;
  if (z_len < r1->d->m) return ARK355_E_ASSIGNMENT_MISSING;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(pk->d->curve, A::prove(ctx, ex.prover, *pk->d, *r1->d, z, false, r, s, nullptr, out_partials));
  });
}

int32_t ark355_prove_combine(ark355_ctx* ctx, int32_t curve, const uint8_t* partials, uint64_t count,
                             const uint8_t r[32], const uint8_t s[32], ark355_proof_raw* out) {
  if (!ctx || !partials || !count || !r || !s || !out) return ARK355_EINVAL;
  return guarded(ctx, [&] { CURVE_DISPATCH(curve, A::combine(partials, count, r, s, out)); });
}

int32_t ark355_comm_unique_id(uint8_t id[ARK355_COMM_ID_BYTES]) {
  if (!id) return ARK355_EINVAL;
  static_assert(sizeof(ncclUniqueId) <= ARK355_COMM_ID_BYTES, "communicator id does not fit");
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return ARK355_ERCCL;
  memset(id, 0, ARK355_COMM_ID_BYTES);
  memcpy(id, &u, sizeof(u));
  return ARK355_OK;
}

int32_t ark355_comm_init(ark355_ctx* ctx, const uint8_t id[ARK355_COMM_ID_BYTES], int32_t rank, int32_t world,
                         ark355_comm** out) {
  if (!ctx || !id || !out || world < 1 || rank < 0 || rank >= world) return ARK355_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    auto* d = new CommDev();
    d->rank = rank;
    d->world = world;
    d->device = ctx->device;
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    const ncclResult_t r = ncclCommInitRank(&d->comm, world, u, rank);
    if (r != ncclSuccess) {
      d->comm = nullptr;
      delete d;
      throw HipError{ARK355_ERCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)};
    }
    *out = new ark355_comm{d};
  });
}

void ark355_comm_destroy(ark355_comm* comm) {
  if (!comm) return;
  if (comm->d) (void)hipSetDevice(comm->d->device);
  delete comm->d;
  delete comm;
}

static int32_t prove_sharded_common(ark355_ctx* ctx, ark355_comm* comm, const ark355_pk* pk, const ark355_r1cs* r1,
                                    const void* z, bool on_dev, uint64_t z_len, const uint8_t* r, const uint8_t* s,
                                    int32_t mode, ark355_proof_raw* out) {
  if (!ctx || !comm || !pk || !r1 || !z || !r || !s || !out) return ARK355_EINVAL;
  if (mode != ARK355_SHARD_WINDOW && mode != ARK355_SHARD_BUCKET_RING) return ARK355_EINVAL;
  if (z_len < r1->d->m) {
    ctx->last_error = "assignment shorter than num_instance + num_witness";
    return ARK355_E_ASSIGNMENT_MISSING;
  }
  if ((int)pk->d->shard_count != comm->d->world || (int)pk->d->shard_index != comm->d->rank) {
    ctx->last_error = "key shard (index, count) does not match the communicator's (rank, world)";
    return ARK355_EINVAL;
  }
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(pk->d->curve, A::prove(ctx, ex.prover, *pk->d, *r1->d, z, on_dev, r, s, out, nullptr, comm->d, mode));
  });
}
int32_t ark355_prove_sharded(ark355_ctx* ctx, ark355_comm* comm, const ark355_pk* pk, const ark355_r1cs* r1,
                             const uint8_t* z, uint64_t z_len, const uint8_t r[32], const uint8_t s[32], int32_t mode,
                             ark355_proof_raw* out) {
  return prove_sharded_common(ctx, comm, pk, r1, z, false, z_len, r, s, mode, out);
}
int32_t ark355_prove_sharded_dev(ark355_ctx* ctx, ark355_comm* comm, const ark355_pk* pk, const ark355_r1cs* r1,
                                 const void* d_z, uint64_t z_len, const uint8_t r[32], const uint8_t s[32], int32_t mode,
                                 ark355_proof_raw* out) {
  return prove_sharded_common(ctx, comm, pk, r1, d_z, true, z_len, r, s, mode, out);
}

int32_t ark355_witness_map(ark355_ctx* ctx, const ark355_r1cs* r1, const uint8_t* z, uint64_t z_len, uint8_t* h_out) {
  if (!ctx || !r1 || !z || !h_out) return ARK355_EINVAL;
  if (z_len < r1->d->m) return ARK355_E_ASSIGNMENT_MISSING;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(r1->d->curve, A::witness_map(ctx, ex.prover, *r1->d, z, h_out));
  });
}

int32_t ark355_witness_map_dist_sim(ark355_ctx* ctx, const ark355_r1cs* r1, const uint8_t* z, uint64_t z_len, uint32_t world,
                                    uint8_t* h_out) {
  if (!ctx || !r1 || !z || !h_out) return ARK355_EINVAL;
  if (z_len < r1->d->m) return ARK355_E_ASSIGNMENT_MISSING;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(r1->d->curve, A::witness_map_dist_sim(ctx, ex.prover, *r1->d, z, world, h_out));
  });
}

int32_t ark355_is_satisfied(ark355_ctx* ctx, const ark355_r1cs* r1, const uint8_t* z, uint64_t z_len,
                            int64_t* first_bad) {
  if (!ctx || !r1 || !z || !first_bad) return ARK355_EINVAL;
  if (z_len < r1->d->m) return ARK355_E_ASSIGNMENT_MISSING;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(r1->d->curve, A::mat_vec(ctx, ex.prover, *r1->d, z, nullptr, nullptr, nullptr, first_bad));
  });
}

int32_t ark355_r1cs_mat_vec(ark355_ctx* ctx, const ark355_r1cs* r1, const uint8_t* z, uint64_t z_len, uint8_t* az,
                            uint8_t* bz, uint8_t* cz) {
  if (!ctx || !r1 || !z) return ARK355_EINVAL;
  if (z_len < r1->d->m) return ARK355_E_ASSIGNMENT_MISSING;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(r1->d->curve, A::mat_vec(ctx, ex.prover, *r1->d, z, az, bz, cz, nullptr));
  });
}

int32_t ark355_gr1cs_load(ark355_ctx* ctx, int32_t curve, uint64_t ell, uint64_t w, const ark355_predicate_desc* preds,
                          uint32_t n_preds, ark355_gr1cs** out) {
  if (!ctx || !out) return ARK355_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    Gr1csDev* d = nullptr;
    CURVE_DISPATCH(curve, d = A::gr1cs_load(ell, w, preds, n_preds));
    d->device = ctx->device;
    *out = new ark355_gr1cs{d};
  });
}
void ark355_gr1cs_free(ark355_gr1cs* g) {
  if (!g) return;
  delete g->d;
  delete g;
}
uint64_t ark355_gr1cs_num_constraints(const ark355_gr1cs* g) { return g ? g->d->total : 0; }

int32_t ark355_gr1cs_which_is_unsatisfied(ark355_ctx* ctx, const ark355_gr1cs* g, const uint8_t* z, uint64_t z_len,
                                          int64_t* predicate, int64_t* constraint) {
  if (!ctx || !g || !z || !predicate || !constraint) return ARK355_EINVAL;
  if (z_len < g->d->m) {
    ctx->last_error = "assignment shorter than num_instance + num_witness";
    return ARK355_E_ASSIGNMENT_MISSING;
  }
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(g->d->curve, A::gr1cs_check(ctx, ex.prover, *g->d, z, predicate, constraint));
  });
}

static int32_t gr1cs_vec_common(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* z, uint64_t z_len,
                                uint8_t* out, bool eval) {
  if (!ctx || !g || !z) return ARK355_EINVAL;
  if (predicate >= g->d->preds.size()) {
    ctx->last_error = "predicate index out of range";
    return ARK355_EINVAL;
  }
  if (!out && g->d->preds[predicate].n) return ARK355_EINVAL;
  if (z_len < g->d->m) {
    ctx->last_error = "assignment shorter than num_instance + num_witness";
    return ARK355_E_ASSIGNMENT_MISSING;
  }
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(g->d->curve, A::gr1cs_mat_vec(ctx, ex.prover, ex.generic, *g->d, predicate, z, out, eval));
  });
}
int32_t ark355_gr1cs_mat_vec(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* z, uint64_t z_len,
                             uint8_t* out) {
  return gr1cs_vec_common(ctx, g, predicate, z, z_len, out, false);
}
int32_t ark355_gr1cs_eval(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* z, uint64_t z_len,
                          uint8_t* out) {
  return gr1cs_vec_common(ctx, g, predicate, z, z_len, out, true);
}

int32_t ark355_gr1cs_r1cs(ark355_ctx* ctx, const ark355_gr1cs* g, ark355_r1cs** out) {
  if (!ctx || !g || !out) return ARK355_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    R1csDev* d = nullptr;
    CURVE_DISPATCH(g->d->curve, d = A::gr1cs_r1cs(ctx, *g->d));
    d->device = ctx->device;
    *out = new ark355_r1cs{d};
  });
}

static int32_t refuse(ark355_ctx* ctx, const char* msg, int32_t code = ARK355_EINVAL) {
  if (ctx) ctx->last_error = msg;
  return code;
}

int32_t ark355_gr1cs_dims(const ark355_gr1cs* g, uint64_t* num_instance, uint64_t* num_witness, uint32_t* n_preds) {
  if (!g || !g->d) return ARK355_EINVAL;
  if (num_instance) *num_instance = g->d->ell;
  if (num_witness) *num_witness = g->d->w;
  if (n_preds) *n_preds = (uint32_t)g->d->preds.size();
  return ARK355_OK;
}
int32_t ark355_gr1cs_pred_dims(const ark355_gr1cs* g, uint32_t predicate, uint32_t* arity, uint64_t* n_constraints, uint64_t* nnz) {
  if (!g || !g->d || predicate >= g->d->preds.size()) return ARK355_EINVAL;
  const Gr1csPred& P = g->d->preds[predicate];
  if (arity) *arity = P.arity;
  if (n_constraints) *n_constraints = P.n;
  if (nnz)
    for (uint32_t k = 0; k < P.arity; k++) nnz[k] = P.nnz[k];
  return ARK355_OK;
}
int32_t ark355_gr1cs_matrix(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, uint32_t which, uint64_t* row_ptr,
                            uint32_t* col, uint8_t* coeff, uint64_t entry_capacity) {
  if (!ctx) return ARK355_EINVAL;
  if (!g || !g->d) return refuse(ctx, "ark355_gr1cs_matrix: the gr1cs handle is NULL");
  if (predicate >= g->d->preds.size()) return refuse(ctx, "ark355_gr1cs_matrix: predicate index out of range");
  const Gr1csPred& P = g->d->preds[predicate];
  if (which >= P.arity) return refuse(ctx, "ark355_gr1cs_matrix: which must be below the predicate's arity");
  if (!row_ptr || !col || !coeff) return refuse(ctx, "ark355_gr1cs_matrix: row_ptr / col / coeff is NULL");
  if (entry_capacity < P.nnz[which])
    return refuse(ctx, "ark355_gr1cs_matrix: entry_capacity below the matrix's non-zeros (ark355_gr1cs_pred_dims)");
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(g->d->curve, A::gr1cs_matrix(ctx, ex.generic, *g->d, predicate, which, row_ptr, col, coeff));
  });
}

// ---- finalize() on the device (lcmap_impl.cuh) ------------------------------------------------------------------------------
int32_t ark355_gr1cs_from_lcs(ark355_ctx* ctx, int32_t curve, const ark355_lc_system_desc* system,
                              const ark355_predicate_lcs_desc* preds, uint32_t n_preds, ark355_gr1cs** out) {
  if (!ctx) return ARK355_EINVAL;
  if (!out) return refuse(ctx, "ark355_gr1cs_from_lcs: out is NULL");
  *out = nullptr;
  if (!system) return refuse(ctx, "ark355_gr1cs_from_lcs: system is NULL");
  return guarded(ctx, [&] {
    Gr1csDev* d = nullptr;
    CURVE_DISPATCH(curve, d = A::gr1cs_from_lcs(ctx, *system, preds, n_preds));
    d->device = ctx->device;
    *out = new ark355_gr1cs{d};
  });
}

// ---- Square R1CS (sr1cs_impl.cuh) ----------------------------------------------------------------------------------------

int32_t ark355_sr1cs_from_r1cs(ark355_ctx* ctx, const ark355_r1cs* r1cs, ark355_sr1cs** out) {
  if (!ctx) return ARK355_EINVAL;
  if (!out) return refuse(ctx, "ark355_sr1cs_from_r1cs: out is NULL");
  *out = nullptr;
  if (!r1cs || !r1cs->d) return refuse(ctx, "ark355_sr1cs_from_r1cs: r1cs is NULL");
  if (r1cs->d->device >= 0 && r1cs->d->device != ctx->device)
    return refuse(ctx, "ark355_sr1cs_from_r1cs: the r1cs handle lives on another device than the context");
  return guarded(ctx, [&] {
    Sr1csDev* d = nullptr;
    CURVE_DISPATCH(r1cs->d->curve, d = A::sr1cs_from_r1cs(ctx, *r1cs->d));
    *out = new ark355_sr1cs{d, ark355_gr1cs{&d->sys}};
  });
}
void ark355_sr1cs_free(ark355_sr1cs* s) {
  if (!s) return;
  delete s->d;
  delete s;
}
const ark355_gr1cs* ark355_sr1cs_system(const ark355_sr1cs* s) { return s ? &s->view : nullptr; }

int32_t ark355_sr1cs_dims(const ark355_sr1cs* s, uint64_t* num_instance, uint64_t* num_witness, uint64_t* num_constraints,
                          uint64_t nnz[2]) {
  if (!s) return ARK355_EINVAL;
  const Gr1csDev& g = s->d->sys;
  if (num_instance) *num_instance = g.ell;
  if (num_witness) *num_witness = g.w;
  if (num_constraints) *num_constraints = g.total;
  if (nnz) {
    nnz[0] = g.preds[0].nnz[0];
    nnz[1] = g.preds[0].nnz[1];
  }
  return ARK355_OK;
}

// the handle was built through a context of the same device
static int32_t sr1cs_handle_check(ark355_ctx* ctx, const ark355_sr1cs* s, const char* null_msg) {
  if (!s) return refuse(ctx, null_msg);
  if (s->d->device != ctx->device) return refuse(ctx, "the sr1cs handle lives on another device than the context");
  return ARK355_OK;
}

int32_t ark355_sr1cs_var_map(ark355_ctx* ctx, const ark355_sr1cs* s, int64_t* witness_col, int64_t* instance_col) {
  if (!ctx) return ARK355_EINVAL;
  if (int32_t rc = sr1cs_handle_check(ctx, s, "ark355_sr1cs_var_map: the sr1cs handle is NULL")) return rc;
  return guarded(ctx, [&] { sr1cs_var_map(*s->d, witness_col, instance_col, ctx->stream); });
}

int32_t ark355_sr1cs_matrix(ark355_ctx* ctx, const ark355_sr1cs* s, int32_t which, uint64_t* row_ptr, uint32_t* col, uint8_t* coeff,
                            uint64_t entry_capacity) {
  if (!ctx) return ARK355_EINVAL;
  if (int32_t rc = sr1cs_handle_check(ctx, s, "ark355_sr1cs_matrix: the sr1cs handle is NULL")) return rc;
  if (which < 0 || which > 1) return refuse(ctx, "ark355_sr1cs_matrix: which must be 0 or 1");
  if (!row_ptr || !col || !coeff) return refuse(ctx, "ark355_sr1cs_matrix: row_ptr / col / coeff is NULL");
  if (entry_capacity < s->d->sys.preds[0].nnz[which])
    return refuse(ctx, "ark355_sr1cs_matrix: entry_capacity below the matrix's non-zeros (ark355_sr1cs_dims)");
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(s->d->curve, A::sr1cs_matrix(ctx, ex.generic, *s->d, which, row_ptr, col, coeff));
  });
}

static int32_t sr1cs_assignment_common(ark355_ctx* ctx, const ark355_sr1cs* s, const void* z, uint64_t z_len, void* z_out, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  if (int32_t rc = sr1cs_handle_check(ctx, s, "ark355_sr1cs_assignment: the sr1cs handle is NULL")) return rc;
  if (!z || !z_out) return refuse(ctx, "ark355_sr1cs_assignment: z / z_out is NULL");
  if (z_len < s->d->m) return refuse(ctx, "assignment shorter than num_instance + num_witness", ARK355_E_ASSIGNMENT_MISSING);
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(s->d->curve, A::sr1cs_assignment(ctx, ex.prover, ex.generic, *s->d, z, z_out, on_dev));
  });
}
int32_t ark355_sr1cs_assignment(ark355_ctx* ctx, const ark355_sr1cs* s, const uint8_t* z, uint64_t z_len, uint8_t* z_out) {
  return sr1cs_assignment_common(ctx, s, z, z_len, z_out, false);
}
int32_t ark355_sr1cs_assignment_dev(ark355_ctx* ctx, const ark355_sr1cs* s, const void* d_z, uint64_t z_len, void* d_z_out) {
  return sr1cs_assignment_common(ctx, s, d_z, z_len, d_z_out, true);
}

// ---- quotient of a predicate (quotient_impl.cuh) -------------------------------------------------------------------------

// the dimensions of one call, or the code that refuses them; *why is set with every refusal
static int32_t quotient_dims_common(const ark355_gr1cs* g, uint32_t predicate, uint32_t log_n, QuotientDims* q, std::string* why) {
  if (!g || !g->d) {
    *why = "the gr1cs handle is NULL";
    return ARK355_EINVAL;
  }
  if (predicate >= g->d->preds.size()) {
    *why = "predicate index out of range";
    return ARK355_EINVAL;
  }
  int32_t rc = ARK355_EINVAL;
  const int32_t caught = guarded(nullptr, [&] {
    CURVE_DISPATCH(g->d->curve, rc = A::gr1cs_quotient_dims(g->d->preds[predicate], log_n, q, why));
  });
  return caught != ARK355_OK ? caught : rc;
}

int32_t ark355_gr1cs_quotient_dims(const ark355_gr1cs* g, uint32_t predicate, uint32_t log_n, uint64_t* degree,
                                   uint32_t* log_domain, uint32_t* log_ext, uint64_t* h_len) {
  QuotientDims q;
  std::string why;
  const int32_t rc = quotient_dims_common(g, predicate, log_n, &q, &why);
  if (degree) *degree = q.degree;
  if (log_domain) *log_domain = q.log_domain;
  if (log_ext) *log_ext = q.log_ext;
  if (h_len) *h_len = q.h_len;
  return rc;
}

static int32_t quotient_common(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* z, uint64_t z_len,
                               uint32_t log_n, void* h_out, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  QuotientDims q;
  std::string why;
  if (const int32_t rc = quotient_dims_common(g, predicate, log_n, &q, &why)) return refuse(ctx, ("ark355_gr1cs_quotient: " + why).c_str(), rc);
  if (!z || !h_out) return refuse(ctx, "ark355_gr1cs_quotient: z / h_out is NULL");
  if (g->d->device >= 0 && g->d->device != ctx->device)
    return refuse(ctx, "ark355_gr1cs_quotient: the gr1cs handle lives on another device than the context");
  if (z_len < g->d->m) return refuse(ctx, "assignment shorter than num_instance + num_witness", ARK355_E_ASSIGNMENT_MISSING);
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(g->d->curve, A::gr1cs_quotient(ctx, ex.prover, ex.quotient, *g->d, predicate, q, z, on_dev, h_out));
  });
}
int32_t ark355_gr1cs_quotient(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* z, uint64_t z_len,
                              uint32_t log_n, uint8_t* h_out) {
  return quotient_common(ctx, g, predicate, z, z_len, log_n, h_out, false);
}
int32_t ark355_gr1cs_quotient_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* d_z, uint64_t z_len,
                                  uint32_t log_n, void* d_h_out) {
  return quotient_common(ctx, g, predicate, d_z, z_len, log_n, d_h_out, true);
}

// ---- column polynomials of a predicate at a point (columns_impl.cuh) -------------------------------------------------------

// tau (canonical, below r) as the Montgomery image of curve `curve`; *why is set with every refusal.  No HIP call.
static int32_t tau_common(int32_t curve, const uint8_t* tau, BlsCurve::Fr* bls, BnCurve::Fr* bn, std::string* why) {
  bool ok = false;
  const int32_t caught = guarded(nullptr, [&] {
    if (curve == ARK355_BLS12_381) ok = Api<BlsCurve>::fr_from_canonical(tau, bls);
    else if (curve == ARK355_BN254) ok = Api<BnCurve>::fr_from_canonical(tau, bn);
    else throw HipError{ARK355_EINVAL, "unknown curve id"};
  });
  if (caught != ARK355_OK) {
    *why = "unknown curve id";
    return caught;
  }
  if (!ok) {
    *why = "tau is not below r";
    return ARK355_EINVAL;
  }
  return ARK355_OK;
}

static int32_t lagrange_common(ark355_ctx* ctx, int32_t curve, uint32_t log_n, const uint8_t* tau, void* out, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  if (!tau || !out) return refuse(ctx, "ark355_lagrange_fr: tau / out is NULL");
  BlsCurve::Fr t_bls;
  BnCurve::Fr t_bn;
  std::string why;
  if (const int32_t rc = tau_common(curve, tau, &t_bls, &t_bn, &why)) return refuse(ctx, ("ark355_lagrange_fr: " + why).c_str(), rc);
  const uint32_t two_adicity = curve == ARK355_BLS12_381 ? Api<BlsCurve>::two_adicity() : Api<BnCurve>::two_adicity();
  if (log_n > two_adicity)
    return refuse(ctx, "ark355_lagrange_fr: the evaluation domain exceeds the largest radix-2 domain of Fr", ARK355_E_POLY_DEGREE_TOO_LARGE);
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::lagrange(ctx, ex.columns, log_n, t_bls, out, on_dev);
    else Api<BnCurve>::lagrange(ctx, ex.columns, log_n, t_bn, out, on_dev);
  });
}
int32_t ark355_lagrange_fr(ark355_ctx* ctx, int32_t curve, uint32_t log_n, const uint8_t tau[32], uint8_t* out) {
  return lagrange_common(ctx, curve, log_n, tau, out, false);
}
int32_t ark355_lagrange_fr_dev(ark355_ctx* ctx, int32_t curve, uint32_t log_n, const uint8_t tau[32], void* d_out) {
  return lagrange_common(ctx, curve, log_n, tau, d_out, true);
}

// y != nullptr: the transposed products with the caller's y; tau != nullptr: with the Lagrange vector at tau
static int32_t columns_common(ark355_ctx* ctx, const char* who, const ark355_gr1cs* g, uint32_t predicate, const void* y, uint64_t y_len,
                              const uint8_t* tau, uint32_t log_n, void* out, bool on_dev, bool at) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = std::string(who) + ": ";
  if (!g || !g->d) return refuse(ctx, (pre + "the gr1cs handle is NULL").c_str());
  if (!out || (at ? !tau : !y)) return refuse(ctx, (pre + (at ? "tau / out is NULL" : "y / out is NULL")).c_str());
  if (predicate >= g->d->preds.size()) return refuse(ctx, (pre + "predicate index out of range").c_str());
  if (g->d->device >= 0 && g->d->device != ctx->device)
    return refuse(ctx, (pre + "the gr1cs handle lives on another device than the context").c_str());
  const Gr1csPred& P = g->d->preds[predicate];
  std::string why;
  BlsCurve::Fr t_bls;
  BnCurve::Fr t_bn;
  if (at) {
    if (const int32_t rc = tau_common(g->d->curve, tau, &t_bls, &t_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  } else if (y_len < P.n) {
    return refuse(ctx, (pre + "y is shorter than the predicate's row count").c_str());
  }
  ColumnsDims d;
  int32_t rc = ARK355_EINVAL;
  const int32_t caught = guarded(nullptr, [&] {
    CURVE_DISPATCH(g->d->curve, rc = A::gr1cs_columns_dims(*g->d, P, at, log_n, &d, &why));
  });
  if (caught != ARK355_OK) return refuse(ctx, (pre + "unknown curve id").c_str(), caught);
  if (rc != ARK355_OK) return refuse(ctx, (pre + why).c_str(), rc);
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (g->d->curve == ARK355_BLS12_381) Api<BlsCurve>::gr1cs_columns(ctx, ex.columns, *g->d, predicate, d, y, at ? &t_bls : nullptr, on_dev, out);
    else Api<BnCurve>::gr1cs_columns(ctx, ex.columns, *g->d, predicate, d, y, at ? &t_bn : nullptr, on_dev, out);
  });
}
int32_t ark355_gr1cs_mat_vec_t(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* y, uint64_t y_len, uint8_t* out) {
  return columns_common(ctx, "ark355_gr1cs_mat_vec_t", g, predicate, y, y_len, nullptr, 0, out, false, false);
}
int32_t ark355_gr1cs_mat_vec_t_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* d_y, uint64_t y_len, void* d_out) {
  return columns_common(ctx, "ark355_gr1cs_mat_vec_t", g, predicate, d_y, y_len, nullptr, 0, d_out, true, false);
}
int32_t ark355_gr1cs_columns_at(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t tau[32], uint32_t log_n, uint8_t* out) {
  return columns_common(ctx, "ark355_gr1cs_columns_at", g, predicate, nullptr, 0, tau, log_n, out, false, true);
}
int32_t ark355_gr1cs_columns_at_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t tau[32], uint32_t log_n, void* d_out) {
  return columns_common(ctx, "ark355_gr1cs_columns_at", g, predicate, nullptr, 0, tau, log_n, d_out, true, true);
}

// ---- polynomial openings (poly_impl.cuh) ---------------------------------------------------------------------------------------

// a canonical scalar named `name` as the Montgomery image of curve `curve`; *why is set with every refusal.  No HIP call.
static int32_t poly_scalar(int32_t curve, const uint8_t* v, const char* name, BlsCurve::Fr* bls, BnCurve::Fr* bn, std::string* why) {
  const int32_t rc = tau_common(curve, v, bls, bn, why);
  if (rc != ARK355_OK && *why == "tau is not below r") *why = std::string(name) + " is not below r";
  return rc;
}

// whether [a, a + an) and [b, b + bn) share a byte
static bool poly_overlap(const void* a, uint64_t an, const void* b, uint64_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return an && bn && x < y + bn && y < x + an;
}

// what eval, div_linear and lincomb refuse about (curve, len, count) alone
static int32_t poly_shape(int32_t curve, uint64_t len, uint64_t count, std::string* why) {
  if (curve != ARK355_BLS12_381 && curve != ARK355_BN254) {
    *why = "unknown curve id";
    return ARK355_EINVAL;
  }
  if (count > POLY_MAX_COUNT) {
    *why = "count exceeds ARK355_POLY_MAX_COUNT";
    return ARK355_EINVAL;
  }
  if (len >= (1ull << 32)) {
    *why = "len must stay below 2^32";
    return ARK355_EINVAL;
  }
  if (count * len >= POLY_MAX_ELEMS) {
    *why = "count * len must stay below 2^40";
    return ARK355_EINVAL;
  }
  return ARK355_OK;
}

static int32_t poly_eval_common(ark355_ctx* ctx, int32_t curve, const void* coeffs, uint64_t len, uint64_t count, const uint8_t* x,
                                void* out, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = "ark355_poly_eval_fr: ";
  std::string why;
  if (const int32_t rc = poly_shape(curve, len, count, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (!x || (count && !out) || (count * len && !coeffs)) return refuse(ctx, (pre + "coeffs / x / out is NULL").c_str());
  BlsCurve::Fr x_bls;
  BnCurve::Fr x_bn;
  if (const int32_t rc = poly_scalar(curve, x, "x", &x_bls, &x_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (poly_overlap(coeffs, count * len * 32, out, count * 32)) return refuse(ctx, (pre + "out overlaps coeffs").c_str());
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::poly_eval(ctx, ex.poly, coeffs, len, count, x_bls, out, on_dev);
    else Api<BnCurve>::poly_eval(ctx, ex.poly, coeffs, len, count, x_bn, out, on_dev);
  });
}
int32_t ark355_poly_eval_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* coeffs, uint64_t len, uint64_t count, const uint8_t x[32],
                            uint8_t* out) {
  return poly_eval_common(ctx, curve, coeffs, len, count, x, out, false);
}
int32_t ark355_poly_eval_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_coeffs, uint64_t len, uint64_t count, const uint8_t x[32],
                                void* d_out) {
  return poly_eval_common(ctx, curve, d_coeffs, len, count, x, d_out, true);
}

static int32_t poly_div_common(ark355_ctx* ctx, int32_t curve, const void* coeffs, uint64_t len, uint64_t count, const uint8_t* x,
                               void* q, void* rem, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = "ark355_poly_div_linear_fr: ";
  std::string why;
  if (const int32_t rc = poly_shape(curve, len, count, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  const uint64_t bytes = count * len * 32;
  if (!x || (bytes && (!coeffs || !q))) return refuse(ctx, (pre + "coeffs / x / q_out is NULL").c_str());
  BlsCurve::Fr x_bls;
  BnCurve::Fr x_bn;
  if (const int32_t rc = poly_scalar(curve, x, "x", &x_bls, &x_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (q != coeffs && poly_overlap(coeffs, bytes, q, bytes))
    return refuse(ctx, (pre + "q_out overlaps coeffs without being equal to it").c_str());
  if (rem && (poly_overlap(coeffs, bytes, rem, count * 32) || poly_overlap(q, bytes, rem, count * 32)))
    return refuse(ctx, (pre + "rem_out overlaps coeffs or q_out").c_str());
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::poly_div_linear(ctx, ex.poly, coeffs, len, count, x_bls, q, rem, on_dev);
    else Api<BnCurve>::poly_div_linear(ctx, ex.poly, coeffs, len, count, x_bn, q, rem, on_dev);
  });
}
int32_t ark355_poly_div_linear_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* coeffs, uint64_t len, uint64_t count,
                                  const uint8_t x[32], uint8_t* q_out, uint8_t* rem_out) {
  return poly_div_common(ctx, curve, coeffs, len, count, x, q_out, rem_out, false);
}
int32_t ark355_poly_div_linear_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_coeffs, uint64_t len, uint64_t count,
                                      const uint8_t x[32], void* d_q_out, void* d_rem_out) {
  return poly_div_common(ctx, curve, d_coeffs, len, count, x, d_q_out, d_rem_out, true);
}

static int32_t poly_lincomb_common(ark355_ctx* ctx, int32_t curve, const void* polys, uint64_t len, uint64_t count,
                                   const uint8_t* scalars, void* out, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = "ark355_poly_lincomb_fr: ";
  std::string why;
  if (const int32_t rc = poly_shape(curve, len, count, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if ((len && !out) || (count && !scalars) || (count * len && !polys)) return refuse(ctx, (pre + "polys / scalars / out is NULL").c_str());
  std::vector<BlsCurve::Fr> s_bls;
  std::vector<BnCurve::Fr> s_bn;
  const int32_t caught = guarded(nullptr, [&] {
    if (curve == ARK355_BLS12_381) s_bls.resize(count);
    else s_bn.resize(count);
  });
  if (caught != ARK355_OK) return refuse(ctx, (pre + "host allocation failed").c_str(), caught);
  for (uint64_t k = 0; k < count; k++) {
    BlsCurve::Fr a;
    BnCurve::Fr b;
    if (const int32_t rc = poly_scalar(curve, scalars + 32 * k, "a scalar", &a, &b, &why)) return refuse(ctx, (pre + why).c_str(), rc);
    if (curve == ARK355_BLS12_381) s_bls[k] = a;
    else s_bn[k] = b;
  }
  if (out != polys && poly_overlap(polys, count * len * 32, out, len * 32))
    return refuse(ctx, (pre + "out overlaps polys without being equal to it").c_str());
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::poly_lincomb(ctx, ex.poly, polys, len, count, s_bls.data(), out, on_dev);
    else Api<BnCurve>::poly_lincomb(ctx, ex.poly, polys, len, count, s_bn.data(), out, on_dev);
  });
}
int32_t ark355_poly_lincomb_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* polys, uint64_t len, uint64_t count, const uint8_t* scalars,
                               uint8_t* out) {
  return poly_lincomb_common(ctx, curve, polys, len, count, scalars, out, false);
}
int32_t ark355_poly_lincomb_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_polys, uint64_t len, uint64_t count,
                                   const uint8_t* scalars, void* d_out) {
  return poly_lincomb_common(ctx, curve, d_polys, len, count, scalars, d_out, true);
}

// ---- openings in the evaluation basis (evals_impl.cuh) -----------------------------------------------------------------------

// what eval and div_linear refuse about (curve, log_n, count) alone
static int32_t evals_shape(int32_t curve, uint32_t log_n, uint64_t count, std::string* why) {
  if (curve != ARK355_BLS12_381 && curve != ARK355_BN254) {
    *why = "unknown curve id";
    return ARK355_EINVAL;
  }
  if (count > POLY_MAX_COUNT) {
    *why = "count exceeds ARK355_POLY_MAX_COUNT";
    return ARK355_EINVAL;
  }
  const uint32_t two_adicity = curve == ARK355_BLS12_381 ? Api<BlsCurve>::two_adicity() : Api<BnCurve>::two_adicity();
  if (log_n > two_adicity) {
    *why = "the evaluation domain exceeds the largest radix-2 domain of Fr";
    return ARK355_E_POLY_DEGREE_TOO_LARGE;
  }
  if ((count << log_n) >= POLY_MAX_ELEMS) {              // count <= 2^10, log_n <= 32: no overflow
    *why = "count * 2^log_n must stay below 2^40";
    return ARK355_EINVAL;
  }
  return ARK355_OK;
}

static int32_t evals_eval_common(ark355_ctx* ctx, int32_t curve, const void* evals, uint32_t log_n, uint64_t count, int32_t coset,
                                 const uint8_t* x, void* out, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = "ark355_evals_eval_fr: ";
  std::string why;
  if (const int32_t rc = evals_shape(curve, log_n, count, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (!x || (count && (!out || !evals))) return refuse(ctx, (pre + "evals / x / out is NULL").c_str());
  BlsCurve::Fr x_bls;
  BnCurve::Fr x_bn;
  if (const int32_t rc = poly_scalar(curve, x, "x", &x_bls, &x_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (poly_overlap(evals, (count << log_n) * 32, out, count * 32)) return refuse(ctx, (pre + "out overlaps evals").c_str());
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::evals_eval(ctx, ex.evals, evals, log_n, count, coset != 0, x_bls, out, on_dev);
    else Api<BnCurve>::evals_eval(ctx, ex.evals, evals, log_n, count, coset != 0, x_bn, out, on_dev);
  });
}
int32_t ark355_evals_eval_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t log_n, uint64_t count, int32_t coset,
                             const uint8_t x[32], uint8_t* out) {
  return evals_eval_common(ctx, curve, evals, log_n, count, coset, x, out, false);
}
int32_t ark355_evals_eval_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t log_n, uint64_t count, int32_t coset,
                                 const uint8_t x[32], void* d_out) {
  return evals_eval_common(ctx, curve, d_evals, log_n, count, coset, x, d_out, true);
}

static int32_t evals_div_common(ark355_ctx* ctx, int32_t curve, const void* evals, uint32_t log_n, uint64_t count, int32_t coset,
                                const uint8_t* x, void* q, void* rem, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = "ark355_evals_div_linear_fr: ";
  std::string why;
  if (const int32_t rc = evals_shape(curve, log_n, count, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  const uint64_t bytes = (count << log_n) * 32;
  if (!x || (count && (!evals || !q))) return refuse(ctx, (pre + "evals / x / q_out is NULL").c_str());
  BlsCurve::Fr x_bls;
  BnCurve::Fr x_bn;
  if (const int32_t rc = poly_scalar(curve, x, "x", &x_bls, &x_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (q != evals && poly_overlap(evals, bytes, q, bytes))
    return refuse(ctx, (pre + "q_out overlaps evals without being equal to it").c_str());
  if (rem && (poly_overlap(evals, bytes, rem, count * 32) || poly_overlap(q, bytes, rem, count * 32)))
    return refuse(ctx, (pre + "rem_out overlaps evals or q_out").c_str());
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::evals_div_linear(ctx, ex.evals, evals, log_n, count, coset != 0, x_bls, q, rem, on_dev);
    else Api<BnCurve>::evals_div_linear(ctx, ex.evals, evals, log_n, count, coset != 0, x_bn, q, rem, on_dev);
  });
}
int32_t ark355_evals_div_linear_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t log_n, uint64_t count, int32_t coset,
                                   const uint8_t x[32], uint8_t* q_out, uint8_t* rem_out) {
  return evals_div_common(ctx, curve, evals, log_n, count, coset, x, q_out, rem_out, false);
}
int32_t ark355_evals_div_linear_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t log_n, uint64_t count,
                                       int32_t coset, const uint8_t x[32], void* d_q_out, void* d_rem_out) {
  return evals_div_common(ctx, curve, d_evals, log_n, count, coset, x, d_q_out, d_rem_out, true);
}

// the values of m_0 .. m_{t-1} over H_N in device memory: the refusals of ark355_gr1cs_quotient_dev about the same arguments, except
// that the predicate's degree does not matter here
int32_t ark355_gr1cs_mat_vec_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* d_z, uint64_t z_len,
                                 uint32_t log_n, void* d_out) {
  if (!ctx) return ARK355_EINVAL;
  QuotientDims q;
  std::string why;
  int32_t rc = quotient_dims_common(g, predicate, log_n, &q, &why);
  if (rc == ARK355_E_POLY_DEGREE_TOO_LARGE && q.log_domain <= (g->d->curve == ARK355_BLS12_381 ? Api<BlsCurve>::two_adicity()
                                                                                                : Api<BnCurve>::two_adicity()))
    rc = ARK355_OK;                                        // only the extended domain was too large: none is used here
  if (rc) return refuse(ctx, ("ark355_gr1cs_mat_vec_dev: " + why).c_str(), rc);
  if (!d_z || !d_out) return refuse(ctx, "ark355_gr1cs_mat_vec_dev: d_z / d_out is NULL");
  if (g->d->device >= 0 && g->d->device != ctx->device)
    return refuse(ctx, "ark355_gr1cs_mat_vec_dev: the gr1cs handle lives on another device than the context");
  if (z_len < g->d->m) return refuse(ctx, "assignment shorter than num_instance + num_witness", ARK355_E_ASSIGNMENT_MISSING);
  return guarded(ctx, [&] { CURVE_DISPATCH(g->d->curve, A::gr1cs_mat_vec_dev(ctx, *g->d, predicate, q, d_z, d_out)); });
}

// ---- multilinear extensions (mle_impl.cuh) ---------------------------------------------------------------------------------------

// what eq, fix and eval refuse about (curve, num_vars, count) alone
static int32_t mle_shape(int32_t curve, uint32_t num_vars, uint64_t count, std::string* why) {
  if (curve != ARK355_BLS12_381 && curve != ARK355_BN254) {
    *why = "unknown curve id";
    return ARK355_EINVAL;
  }
  if (count > POLY_MAX_COUNT) {
    *why = "count exceeds ARK355_POLY_MAX_COUNT";
    return ARK355_EINVAL;
  }
  if (num_vars > MLE_MAX_VARS) {
    *why = "num_vars must not exceed 40";
    return ARK355_EINVAL;
  }
  if ((count << num_vars) >= POLY_MAX_ELEMS) {             // count <= 2^10, num_vars <= 40: no overflow
    *why = "count * 2^num_vars must stay below 2^40";
    return ARK355_EINVAL;
  }
  return ARK355_OK;
}

// `n` canonical scalars as Montgomery images of curve `curve` (one of the two vectors is filled); *why is set with every refusal
static int32_t mle_point(int32_t curve, const uint8_t* point, uint32_t n, std::vector<BlsCurve::Fr>* bls, std::vector<BnCurve::Fr>* bn,
                         std::string* why) {
  bls->assign(curve == ARK355_BLS12_381 ? n : 0, BlsCurve::Fr::zero());
  bn->assign(curve == ARK355_BN254 ? n : 0, BnCurve::Fr::zero());
  for (uint32_t j = 0; j < n; j++) {
    BlsCurve::Fr a;
    BnCurve::Fr b;
    const std::string name = "point[" + std::to_string(j) + "]";
    if (const int32_t rc = poly_scalar(curve, point + 32 * (size_t)j, name.c_str(), &a, &b, why)) return rc;
    if (curve == ARK355_BLS12_381) (*bls)[j] = a;
    else (*bn)[j] = b;
  }
  return ARK355_OK;
}

static int32_t mle_eq_common(ark355_ctx* ctx, int32_t curve, uint32_t num_vars, const uint8_t* point, void* out, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = "ark355_mle_eq_fr: ";
  std::string why;
  if (const int32_t rc = mle_shape(curve, num_vars, 1, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (!out || (num_vars && !point)) return refuse(ctx, (pre + "point / out is NULL").c_str());
  std::vector<BlsCurve::Fr> p_bls;
  std::vector<BnCurve::Fr> p_bn;
  if (const int32_t rc = mle_point(curve, point, num_vars, &p_bls, &p_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::mle_eq(ctx, ex.mle, num_vars, p_bls.data(), out, on_dev);
    else Api<BnCurve>::mle_eq(ctx, ex.mle, num_vars, p_bn.data(), out, on_dev);
  });
}
int32_t ark355_mle_eq_fr(ark355_ctx* ctx, int32_t curve, uint32_t num_vars, const uint8_t* point, uint8_t* out) {
  return mle_eq_common(ctx, curve, num_vars, point, out, false);
}
int32_t ark355_mle_eq_fr_dev(ark355_ctx* ctx, int32_t curve, uint32_t num_vars, const uint8_t* point, void* d_out) {
  return mle_eq_common(ctx, curve, num_vars, point, d_out, true);
}

// fix (k < 0: eval, every variable) on host or device pointers
static int32_t mle_fix_common(ark355_ctx* ctx, const char* who, int32_t curve, const void* evals, uint32_t num_vars, uint64_t count,
                              const uint8_t* point, int64_t k_or_all, void* out, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = std::string(who) + ": ";
  std::string why;
  if (const int32_t rc = mle_shape(curve, num_vars, count, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (k_or_all > (int64_t)num_vars) return refuse(ctx, (pre + "k exceeds num_vars").c_str());
  const uint32_t k = k_or_all < 0 ? num_vars : (uint32_t)k_or_all;
  if ((k && !point) || (count && (!evals || !out))) return refuse(ctx, (pre + "evals / point / out is NULL").c_str());
  std::vector<BlsCurve::Fr> p_bls;
  std::vector<BnCurve::Fr> p_bn;
  if (const int32_t rc = mle_point(curve, point, k, &p_bls, &p_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (poly_overlap(evals, (count << num_vars) * 32, out, (count << (num_vars - k)) * 32)) return refuse(ctx, (pre + "out overlaps evals").c_str());
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::mle_fix(ctx, ex.mle, evals, num_vars, count, p_bls.data(), k, out, on_dev);
    else Api<BnCurve>::mle_fix(ctx, ex.mle, evals, num_vars, count, p_bn.data(), k, out, on_dev);
  });
}
int32_t ark355_mle_fix_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t num_vars, uint64_t count, const uint8_t* point,
                          uint32_t k, uint8_t* out) {
  return mle_fix_common(ctx, "ark355_mle_fix_fr", curve, evals, num_vars, count, point, k, out, false);
}
int32_t ark355_mle_fix_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t num_vars, uint64_t count, const uint8_t* point,
                              uint32_t k, void* d_out) {
  return mle_fix_common(ctx, "ark355_mle_fix_fr", curve, d_evals, num_vars, count, point, k, d_out, true);
}
int32_t ark355_mle_eval_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t num_vars, uint64_t count, const uint8_t* point,
                           uint8_t* out) {
  return mle_fix_common(ctx, "ark355_mle_eval_fr", curve, evals, num_vars, count, point, -1, out, false);
}
int32_t ark355_mle_eval_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t num_vars, uint64_t count, const uint8_t* point,
                               void* d_out) {
  return mle_fix_common(ctx, "ark355_mle_eval_fr", curve, d_evals, num_vars, count, point, -1, d_out, true);
}

// ---- multilinear openings (mle_open_impl.cuh) -------------------------------------------------------------------------------------

static int32_t mle_quotients_common(ark355_ctx* ctx, int32_t curve, const void* evals, uint32_t num_vars, uint64_t count,
                                    const uint8_t* point, void* q, void* rem, bool on_dev) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = "ark355_mle_quotients_fr: ";
  std::string why;
  if (const int32_t rc = mle_shape(curve, num_vars, count, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if ((num_vars && !point) || (count && (!evals || !q))) return refuse(ctx, (pre + "evals / point / q_out is NULL").c_str());
  std::vector<BlsCurve::Fr> p_bls;
  std::vector<BnCurve::Fr> p_bn;
  if (const int32_t rc = mle_point(curve, point, num_vars, &p_bls, &p_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  const uint64_t bytes = (count << num_vars) * 32;
  if (poly_overlap(evals, bytes, q, bytes)) return refuse(ctx, (pre + "q_out overlaps evals").c_str());
  if (rem && (poly_overlap(evals, bytes, rem, count * 32) || poly_overlap(q, bytes, rem, count * 32)))
    return refuse(ctx, (pre + "rem_out overlaps evals or q_out").c_str());
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381) Api<BlsCurve>::mle_quotients(ctx, ex.mle, evals, num_vars, count, p_bls.data(), q, rem, on_dev);
    else Api<BnCurve>::mle_quotients(ctx, ex.mle, evals, num_vars, count, p_bn.data(), q, rem, on_dev);
  });
}
int32_t ark355_mle_quotients_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t num_vars, uint64_t count,
                                const uint8_t* point, uint8_t* q_out, uint8_t* rem_out) {
  return mle_quotients_common(ctx, curve, evals, num_vars, count, point, q_out, rem_out, false);
}
int32_t ark355_mle_quotients_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t num_vars, uint64_t count,
                                    const uint8_t* point, void* d_q_out, void* d_rem_out) {
  return mle_quotients_common(ctx, curve, d_evals, num_vars, count, point, d_q_out, d_rem_out, true);
}

int32_t ark355_mle_open_dev(ark355_ctx* ctx, int32_t curve, const ark355_bases* const* level_bases, const void* d_evals,
                            uint32_t num_vars, const uint8_t* point, uint8_t* proofs_out, uint8_t* value_out) {
  if (!ctx) return ARK355_EINVAL;
  const std::string pre = "ark355_mle_open_dev: ";
  std::string why;
  if (const int32_t rc = mle_shape(curve, num_vars, 1, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  if (!d_evals || !value_out || (num_vars && (!point || !proofs_out)))
    return refuse(ctx, (pre + "d_evals / point / proofs_out / value_out is NULL").c_str());
  if (num_vars && !level_bases) return refuse(ctx, (pre + "level_bases is NULL").c_str());
  std::vector<const BasesDev*> bases(num_vars);
  for (uint32_t j = 0; j < num_vars; j++) {
    const std::string lvl = "the handle of level " + std::to_string(j);
    if (!level_bases[j] || !level_bases[j]->d) return refuse(ctx, (pre + lvl + " is NULL").c_str());
    const BasesDev* b = level_bases[j]->d;
    if (b->curve != curve) return refuse(ctx, (pre + lvl + " belongs to another curve").c_str());
    if (b->group != level_bases[0]->d->group) return refuse(ctx, (pre + lvl + " is of another group than level 0: the handles mix G1 and G2").c_str());
    if (b->n < (1ull << (num_vars - 1 - j)))
      return refuse(ctx, (pre + lvl + " holds " + std::to_string(b->n) + " bases, fewer than the 2^" + std::to_string(num_vars - 1 - j) + " of its quotient").c_str());
    bases[j] = b;
  }
  std::vector<BlsCurve::Fr> p_bls;
  std::vector<BnCurve::Fr> p_bn;
  if (const int32_t rc = mle_point(curve, point, num_vars, &p_bls, &p_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    if (curve == ARK355_BLS12_381)
      Api<BlsCurve>::mle_open_dev(ctx, ex.mle, ex.msm_batch, ex.generic, bases.data(), d_evals, num_vars, p_bls.data(), proofs_out, value_out);
    else Api<BnCurve>::mle_open_dev(ctx, ex.mle, ex.msm_batch, ex.generic, bases.data(), d_evals, num_vars, p_bn.data(), proofs_out, value_out);
  });
}

// ---- sum-check of a predicate (sumcheck_impl.cuh) -------------------------------------------------------------------------------

int32_t ark355_gr1cs_sumcheck_begin_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* d_tables,
                                        const void* d_weight, uint32_t num_vars, ark355_sumcheck** out) {
  if (!ctx) return ARK355_EINVAL;
  const char* pre = "ark355_gr1cs_sumcheck_begin_dev: ";
  if (!out) return refuse(ctx, (std::string(pre) + "out is NULL").c_str());
  *out = nullptr;
  if (!g || !g->d) return refuse(ctx, (std::string(pre) + "the gr1cs handle is NULL").c_str());
  if (!d_tables) return refuse(ctx, (std::string(pre) + "d_tables is NULL").c_str());
  if (predicate >= g->d->preds.size()) return refuse(ctx, (std::string(pre) + "predicate index out of range").c_str());
  if (g->d->device >= 0 && g->d->device != ctx->device)
    return refuse(ctx, (std::string(pre) + "the gr1cs handle lives on another device than the context").c_str());
  if (num_vars > MLE_MAX_VARS) return refuse(ctx, (std::string(pre) + "num_vars must not exceed 40").c_str());
  if ((((uint64_t)g->d->preds[predicate].arity + 1) << num_vars) >= SUMCHECK_MAX_ELEMS)
    return refuse(ctx, (std::string(pre) + "(arity + 1) * 2^num_vars must stay below 2^40").c_str());
  return guarded(ctx, [&] {
    SumcheckDev* d = nullptr;
    CURVE_DISPATCH(g->d->curve, d = A::sumcheck_begin(ctx, *g->d, predicate, d_tables, d_weight, num_vars));
    *out = new ark355_sumcheck{d};
  });
}

int32_t ark355_sumcheck_info(const ark355_sumcheck* sc, uint32_t* num_vars, uint32_t* arity, uint32_t* points, uint32_t* rounds_done) {
  if (!sc || !sc->d) return ARK355_EINVAL;
  if (num_vars) *num_vars = sc->d->num_vars;
  if (arity) *arity = sc->d->arity;
  if (points) *points = sc->d->points;
  if (rounds_done) *rounds_done = sc->d->rounds_done;
  return ARK355_OK;
}

// what round and finish share: the handle, the device, the challenge (present exactly when `want`) as a Montgomery image
static int32_t sumcheck_step_common(ark355_ctx* ctx, const char* pre, ark355_sumcheck* sc, const uint8_t* challenge, bool want, void* out,
                                    BlsCurve::Fr* r_bls, BnCurve::Fr* r_bn) {
  if (!sc || !sc->d) return refuse(ctx, (std::string(pre) + "the sumcheck handle is NULL").c_str());
  if (!out) return refuse(ctx, (std::string(pre) + "the output is NULL").c_str());
  if (sc->d->device != ctx->device) return refuse(ctx, (std::string(pre) + "the sumcheck handle lives on another device than the context").c_str());
  if (sc->d->finished) return refuse(ctx, (std::string(pre) + "the run is finished: only ark355_sumcheck_info and ark355_sumcheck_free are legal").c_str());
  if (want && !challenge) return refuse(ctx, (std::string(pre) + "call out of order: this call needs a challenge").c_str());
  if (!want && challenge) return refuse(ctx, (std::string(pre) + "call out of order: this call takes no challenge (NULL)").c_str());
  *r_bls = BlsCurve::Fr::zero();
  *r_bn = BnCurve::Fr::zero();
  if (want) {
    std::string why;
    if (const int32_t rc = poly_scalar(sc->d->curve, challenge, "challenge", r_bls, r_bn, &why)) return refuse(ctx, (pre + why).c_str(), rc);
  }
  return ARK355_OK;
}

int32_t ark355_sumcheck_round(ark355_ctx* ctx, ark355_sumcheck* sc, const uint8_t* challenge, uint8_t* evals_out) {
  if (!ctx) return ARK355_EINVAL;
  const char* pre = "ark355_sumcheck_round: ";
  if (sc && sc->d && !sc->d->finished && sc->d->rounds_done >= sc->d->num_vars)
    return refuse(ctx, (std::string(pre) + "call out of order: every round has run").c_str());
  BlsCurve::Fr r_bls;
  BnCurve::Fr r_bn;
  if (const int32_t rc = sumcheck_step_common(ctx, pre, sc, challenge, sc && sc->d && sc->d->rounds_done > 0, evals_out, &r_bls, &r_bn)) return rc;
  return guarded(ctx, [&] {
    if (sc->d->curve == ARK355_BLS12_381) Api<BlsCurve>::sumcheck_round(ctx, *sc->d, r_bls, evals_out);
    else Api<BnCurve>::sumcheck_round(ctx, *sc->d, r_bn, evals_out);
  });
}

int32_t ark355_sumcheck_finish(ark355_ctx* ctx, ark355_sumcheck* sc, const uint8_t* challenge, uint8_t* finals_out) {
  if (!ctx) return ARK355_EINVAL;
  const char* pre = "ark355_sumcheck_finish: ";
  if (sc && sc->d && !sc->d->finished && sc->d->rounds_done < sc->d->num_vars)
    return refuse(ctx, (std::string(pre) + "call out of order: rounds are still to run").c_str());
  BlsCurve::Fr r_bls;
  BnCurve::Fr r_bn;
  if (const int32_t rc = sumcheck_step_common(ctx, pre, sc, challenge, sc && sc->d && sc->d->num_vars > 0, finals_out, &r_bls, &r_bn)) return rc;
  return guarded(ctx, [&] {
    if (sc->d->curve == ARK355_BLS12_381) Api<BlsCurve>::sumcheck_finish(ctx, *sc->d, r_bls, finals_out);
    else Api<BnCurve>::sumcheck_finish(ctx, *sc->d, r_bn, finals_out);
  });
}

void ark355_sumcheck_free(ark355_sumcheck* sc) {
  if (!sc) return;
  delete sc->d;
  delete sc;
}

int32_t ark355_ntt_fr(ark355_ctx* ctx, int32_t curve, uint8_t* data, uint32_t log_n, int32_t inverse, int32_t coset) {
  if (!ctx || !data) return ARK355_EINVAL;
  if (log_n > 40) return ARK355_E_POLY_DEGREE_TOO_LARGE;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::ntt_host(ctx, ex.generic, data, log_n, inverse != 0, coset != 0));
  });
}

int32_t ark355_ntt_fr_dev(ark355_ctx* ctx, int32_t curve, void* d_data, void* d_scratch, uint32_t log_n,
                          int32_t inverse, int32_t coset, void* stream) {
  if (!ctx || !d_data || !d_scratch) return ARK355_EINVAL;
  if (log_n > 40) return ARK355_E_POLY_DEGREE_TOO_LARGE;
  return guarded(ctx, [&] {
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    CURVE_DISPATCH(curve, A::ntt_dev(ctx, d_data, d_scratch, log_n, inverse != 0, coset != 0, st));
  });
}

static int32_t msm_host_common(ark355_ctx* ctx, int32_t curve, int group, const uint8_t* bases, const uint8_t* scalars,
                               uint64_t n, uint8_t* out) {
  if (!ctx || !out || (n && (!bases || !scalars))) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::msm_host(ctx, ex.generic, group, bases, scalars, n, out));
  });
}
int32_t ark355_msm_g1(ark355_ctx* ctx, int32_t curve, const uint8_t* bases, const uint8_t* scalars, uint64_t n,
                      uint8_t* out) {
  return msm_host_common(ctx, curve, 1, bases, scalars, n, out);
}
int32_t ark355_msm_g2(ark355_ctx* ctx, int32_t curve, const uint8_t* bases, const uint8_t* scalars, uint64_t n,
                      uint8_t* out) {
  return msm_host_common(ctx, curve, 2, bases, scalars, n, out);
}

int32_t ark355_bases_load(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* bases, uint64_t n,
                          ark355_bases** out) {
  if (!ctx || !out || (n && !bases) || (group != 1 && group != 2)) return ARK355_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    BasesDev* d = nullptr;
    CURVE_DISPATCH(curve, d = A::bases_load(ctx->policy, group, bases, n, ctx->stream));
    d->device = ctx->device;
    *out = new ark355_bases{d};
  });
}
void ark355_bases_free(ark355_bases* b) {
  if (!b) return;
  delete b->d;
  delete b;
}

int32_t ark355_msm_dev(ark355_ctx* ctx, const ark355_bases* bases, const void* d_scalars, uint64_t n,
                       int32_t scalars_mont, uint8_t* out_affine) {
  if (!ctx || !bases || !out_affine || (n && !d_scalars)) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(bases->d->curve, A::msm_dev(ctx, ex.generic, *bases->d, d_scalars, n, scalars_mont, out_affine, true));
  });
}
int32_t ark355_msm_dev_partial(ark355_ctx* ctx, const ark355_bases* bases, const void* d_scalars, uint64_t n,
                               int32_t scalars_mont, uint8_t* out_xyzz) {
  if (!ctx || !bases || !out_xyzz || (n && !d_scalars)) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(bases->d->curve, A::msm_dev(ctx, ex.generic, *bases->d, d_scalars, n, scalars_mont, out_xyzz, false));
  });
}

// ---- batched short MSMs (msm_batch_impl.cuh): every refusal precedes the first allocation, copy or launch
int32_t ark355_msm_batch_dev(ark355_ctx* ctx, const ark355_bases* const* bases, const void* const* d_scalars, const uint64_t* n,
                             uint64_t count, int32_t scalars_mont, uint8_t* out_affine) {
  if (!ctx) return ARK355_EINVAL;
  if (count == 0) return ARK355_OK;
  const std::string pre = "ark355_msm_batch_dev: ";
  if (!bases || !d_scalars || !n || !out_affine) return refuse(ctx, (pre + "bases / d_scalars / n / out_affine is NULL").c_str());
  if (count > ARK355_MSM_BATCH_MAX)
    return refuse(ctx, (pre + std::to_string(count) + " segments, more than ARK355_MSM_BATCH_MAX = " + std::to_string(ARK355_MSM_BATCH_MAX)).c_str());
  std::vector<const BasesDev*> hs(count);
  for (uint64_t s = 0; s < count; s++) {
    const std::string seg = "segment " + std::to_string(s) + ": ";
    if (!bases[s] || !bases[s]->d) return refuse(ctx, (pre + seg + "the handle is NULL").c_str());
    const BasesDev* b = bases[s]->d;
    if (b->device != ctx->device) return refuse(ctx, (pre + seg + "the handle lives on another device than the context").c_str());
    if (b->curve != bases[0]->d->curve) return refuse(ctx, (pre + seg + "the handle belongs to another curve than segment 0's").c_str());
    if (b->group != bases[0]->d->group)
      return refuse(ctx, (pre + seg + "the handle is of another group than segment 0's: the handles mix G1 and G2").c_str());
    if (n[s] > b->n)
      return refuse(ctx, (pre + seg + std::to_string(n[s]) + " scalars, more than the handle's " + std::to_string(b->n) + " bases").c_str());
    if (n[s] && !d_scalars[s]) return refuse(ctx, (pre + seg + "d_scalars is NULL").c_str());
    hs[s] = b;
  }
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(hs[0]->curve, A::msm_batch_dev(ctx, ex.msm_batch, ex.generic, hs.data(), d_scalars, n, count, scalars_mont, out_affine));
  });
}

int32_t ark355_xyzz_sum(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* partials, uint64_t count,
                        uint8_t* out_affine) {
  if (!ctx || !out_affine || (count && !partials) || (group != 1 && group != 2) || count >= (1ull << 31))
    return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::xyzz_sum(ctx, ex.generic, group, partials, count, out_affine));
  });
}

int32_t ark355_fixed_base_mul(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* base,
                              const uint8_t* scalars, uint64_t n, uint8_t* out_affine) {
  if (!ctx || !base || (n && (!scalars || !out_affine)) || (group != 1 && group != 2)) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::fixed_base(ctx, ex.generic, group, base, scalars, n, out_affine));
  });
}
int32_t ark355_fixed_base_mul_dev(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* base, const void* d_scalars,
                                  uint64_t n, int32_t scalars_mont, uint8_t* out_affine) {
  if (!ctx) return ARK355_EINVAL;
  if (!base || (n && (!d_scalars || !out_affine))) return refuse(ctx, "ark355_fixed_base_mul_dev: base / d_scalars / out_affine is NULL");
  if (group != 1 && group != 2) return refuse(ctx, "ark355_fixed_base_mul_dev: group must be 1 or 2");
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::fixed_base_dev(ctx, ex.generic, group, base, d_scalars, n, scalars_mont != 0, out_affine));
  });
}

uint64_t ark355_point_size(int32_t curve, int32_t group, int32_t compressed) {
  if (group != 1 && group != 2) return 0;
  size_t n = 0;
  try {
    CURVE_DISPATCH(curve, n = A::point_size(group, compressed != 0));
  } catch (...) {
    return 0;
  }
  return n;
}

int32_t ark355_pk_load_bytes(ark355_ctx* ctx, int32_t curve, const uint8_t* bytes, uint64_t len, int32_t compressed,
                             int32_t validate, ark355_pk** out) {
  if (!ctx || !bytes || !out || validate < 0 || validate > 2) return ARK355_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    PkDev* d = nullptr;
    CURVE_DISPATCH(curve, d = A::pk_load_bytes(ctx, bytes, len, compressed != 0, validate));
    *out = new ark355_pk{d};
  });
}

int32_t ark355_pk_dims(const ark355_pk* pk, uint64_t* num_instance, uint64_t* num_witness, uint64_t* domain_size) {
  if (!pk || !pk->d) return ARK355_EINVAL;
  if (num_instance) *num_instance = pk->d->ell;
  if (num_witness) *num_witness = pk->d->w;
  if (domain_size) *domain_size = pk->d->N;
  return ARK355_OK;
}

int32_t ark355_pk_table_info(const ark355_pk* pk, uint32_t* window_bits, uint32_t* windows, uint32_t* table_stride,
                             uint64_t* table_bytes) {
  if (!pk || !pk->d) return ARK355_EINVAL;
  const MsmPlan& p = pk->d->a_ext.plan;
  if (window_bits) *window_bits = p.c;
  if (windows) *windows = p.windows;
  if (table_stride) *table_stride = pk->d->wstride;
  if (table_bytes) *table_bytes = pk->d->table_bytes();
  return ARK355_OK;
}

int32_t ark355_pk_h_eval(const ark355_pk* pk, int32_t* state, uint32_t* binds, float* bind_seconds) {
  if (!pk || !pk->d) return ARK355_EINVAL;
  if (state) *state = pk->d->h_state.load();
  if (binds) *binds = pk->d->binds;
  if (bind_seconds) *bind_seconds = (float)pk->d->bind_seconds;
  return ARK355_OK;
}

int32_t ark355_hbasis_transform(ark355_ctx* ctx, int32_t curve, const uint8_t* h_query, uint32_t log_n, uint8_t* out_e,
                                uint8_t* out_u) {
  if (!ctx || !h_query || (!out_e && !out_u)) return ARK355_EINVAL;
  return guarded(ctx, [&] { CURVE_DISPATCH(curve, A::hbasis_transform(ctx, h_query, log_n, out_e, out_u)); });
}

int32_t ark355_hbasis_gather(ark355_ctx* ctx, const ark355_r1cs* r1, const uint8_t* u, uint8_t* out_d) {
  if (!ctx || !r1 || !r1->d || !u || !out_d) return ARK355_EINVAL;
  return guarded(ctx, [&] { CURVE_DISPATCH(r1->d->curve, A::hbasis_gather_host(ctx, *r1->d, u, out_d)); });
}

int32_t ark355_points_decode(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* in, uint64_t n,
                             int32_t compressed, int32_t validate, uint8_t* out_raw) {
  if (!ctx || (group != 1 && group != 2) || (n && (!in || !out_raw)) || validate < 0 || validate > 2) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::points_decode(ctx, ex.generic, group, in, n, compressed != 0, validate, out_raw));
  });
}

int32_t ark355_points_encode(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* in_raw, uint64_t n,
                             int32_t compressed, uint8_t* out) {
  if (!ctx || (group != 1 && group != 2) || (n && (!in_raw || !out))) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::points_encode(ctx, ex.generic, group, in_raw, n, compressed != 0, out));
  });
}

int32_t ark355_proof_to_bytes(int32_t curve, const ark355_proof_raw* proof, int32_t compressed, uint8_t* out) {
  if (!proof || !out) return ARK355_EINVAL;
  return guarded(nullptr, [&] { CURVE_DISPATCH(curve, A::proof_to_bytes(proof, compressed != 0, out)); });
}

int32_t ark355_proof_from_bytes(int32_t curve, const uint8_t* in, uint64_t len, int32_t compressed, int32_t validate,
                                ark355_proof_raw* out) {
  if (!in || !out || validate < 0 || validate > 2) return ARK355_EINVAL;
  return guarded(nullptr, [&] { CURVE_DISPATCH(curve, A::proof_from_bytes(in, len, compressed != 0, validate, out)); });
}

int32_t ark355_verify_batch(ark355_ctx* ctx, int32_t curve, const ark355_vk_desc* vk, const ark355_proof_raw* proofs,
                            const uint8_t* public_inputs, const uint8_t* rho, uint64_t count, int32_t* ok) {
  if (!ctx || !vk || !proofs || !ok || !vk->alpha_g1 || !vk->beta_g2 || !vk->gamma_g2 || !vk->delta_g2 || !vk->gamma_abc_g1 ||
      (vk->num_instance > 1 && !public_inputs))
    return ARK355_EINVAL;
  *ok = 0;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    bool good = false;
    CURVE_DISPATCH(curve, good = A::verify_batch(ctx, ex.generic, vk, proofs, public_inputs, rho, count));
    *ok = good ? 1 : 0;
  });
}

int32_t ark355_multi_pairing(ark355_ctx* ctx, int32_t curve, const uint8_t* g1, const uint8_t* g2, uint64_t n, uint8_t* out_gt,
                             int32_t* is_one) {
  if (!ctx || (n && (!g1 || !g2))) return ARK355_EINVAL;
  if (is_one) *is_one = 0;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::multi_pairing(ctx, ex.generic, g1, g2, n, out_gt, is_one));
  });
}

int32_t ark355_pairing_groups(ark355_ctx* ctx, int32_t curve, const uint8_t* g1, const uint8_t* g2, uint64_t groups,
                              uint32_t group_len, uint8_t* out_gt, uint8_t* is_one) {
  if (!ctx) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::pairing_groups(ctx, ex.generic, g1, g2, groups, group_len, out_gt, is_one));
  });
}

int32_t ark355_verify_each(ark355_ctx* ctx, int32_t curve, const ark355_vk_desc* vk, const ark355_proof_raw* proofs,
                           const uint8_t* public_inputs, uint64_t count, uint8_t* ok) {
  if (!ctx || !vk || (count && (!proofs || !ok)) || !vk->alpha_g1 || !vk->beta_g2 || !vk->gamma_g2 || !vk->delta_g2 ||
      !vk->gamma_abc_g1)
    return ARK355_EINVAL;
  if (ok) memset(ok, 0, count);
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::verify_each(ctx, ex.generic, vk, proofs, public_inputs, count, ok));
  });
}

int32_t ark355_vk_process(ark355_ctx* ctx, int32_t curve, const ark355_vk_desc* vk, ark355_pvk** out) {
  if (out) *out = nullptr;
  if (!ctx || !vk || !out || !vk->alpha_g1 || !vk->beta_g2 || !vk->gamma_g2 || !vk->delta_g2 || !vk->gamma_abc_g1)
    return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    PvkDev* d = nullptr;
    CURVE_DISPATCH(curve, d = A::vk_process(ctx, ex.generic, vk));
    *out = new ark355_pvk{d};
  });
}

void ark355_pvk_free(ark355_pvk* pvk) {
  if (!pvk) return;
  if (pvk->d) (void)hipSetDevice(pvk->d->device);
  delete pvk->d;
  delete pvk;
}

int32_t ark355_pvk_info(const ark355_pvk* pvk, int32_t* curve, uint64_t* num_instance, uint64_t* resident_bytes) {
  if (!pvk || !pvk->d) return ARK355_EINVAL;
  if (curve) *curve = pvk->d->curve;
  if (num_instance) *num_instance = pvk->d->ell;
  if (resident_bytes) *resident_bytes = pvk->d->resident_bytes();
  return ARK355_OK;
}

int32_t ark355_pvk_alpha_beta(const ark355_pvk* pvk, uint8_t* out_gt) {
  if (!pvk || !pvk->d || !out_gt) return ARK355_EINVAL;
  memcpy(out_gt, pvk->d->alpha_beta.data(), pvk->d->alpha_beta.size());
  return ARK355_OK;
}

int32_t ark355_pvk_pairings(ark355_ctx* ctx, const ark355_pvk* pvk, int32_t which, const uint8_t* g1, uint64_t n, uint8_t* out_gt,
                            uint8_t* is_one) {
  if (!ctx || !pvk || !pvk->d) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(pvk->d->curve, A::pvk_pairings(ctx, ex.generic, *pvk->d, which, g1, n, out_gt, is_one));
  });
}

int32_t ark355_verify_each_pvk(ark355_ctx* ctx, const ark355_pvk* pvk, const ark355_proof_raw* proofs, const uint8_t* public_inputs,
                               uint64_t count, uint8_t* ok) {
  if (!ctx || !pvk || !pvk->d || (count && (!proofs || !ok))) return ARK355_EINVAL;
  if (ok) memset(ok, 0, count);
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(pvk->d->curve, A::verify_each_pvk(ctx, ex.generic, *pvk->d, proofs, public_inputs, count, ok));
  });
}

int32_t ark355_verify_each_bytes(ark355_ctx* ctx, const ark355_pvk* pvk, const uint8_t* proofs, uint64_t count, int32_t compressed,
                                 int32_t validate, const uint8_t* public_inputs, uint8_t* ok, uint8_t* status) {
  if (!ctx) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    ARK_REQUIRE(pvk && pvk->d, ARK355_EINVAL, "ark355_verify_each_bytes: pvk is NULL");
    ARK_REQUIRE(count == 0 || proofs, ARK355_EINVAL, "ark355_verify_each_bytes: proofs is NULL");
    ARK_REQUIRE(count == 0 || ok, ARK355_EINVAL, "ark355_verify_each_bytes: ok is NULL");
    ARK_REQUIRE(validate >= 0 && validate <= 2, ARK355_EINVAL, "ark355_verify_each_bytes: unknown validate");
    ARK_REQUIRE(count <= 0xFFFFFFFFull / 3, ARK355_EINVAL, "ark355_verify_each_bytes: count: 3 * count must stay below 2^32");
    if (count) memset(ok, 0, count);
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(pvk->d->curve,
                   A::verify_each_bytes(ctx, ex.generic, *pvk->d, proofs, count, compressed != 0, validate, public_inputs, ok, status));
  });
}

int32_t ark355_proofs_from_bytes(ark355_ctx* ctx, int32_t curve, const uint8_t* in, uint64_t count, int32_t compressed,
                                 int32_t validate, ark355_proof_raw* out, uint8_t* status) {
  if (!ctx) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    ARK_REQUIRE(count == 0 || in, ARK355_EINVAL, "ark355_proofs_from_bytes: in is NULL");
    ARK_REQUIRE(count == 0 || out, ARK355_EINVAL, "ark355_proofs_from_bytes: out is NULL");
    ARK_REQUIRE(count == 0 || status, ARK355_EINVAL, "ark355_proofs_from_bytes: status is NULL");
    ARK_REQUIRE(validate >= 0 && validate <= 2, ARK355_EINVAL, "ark355_proofs_from_bytes: unknown validate");
    ARK_REQUIRE(count <= 0xFFFFFFFFull / 3, ARK355_EINVAL, "ark355_proofs_from_bytes: count: 3 * count must stay below 2^32");
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::proofs_from_bytes(ctx, ex.generic, in, count, compressed != 0, validate, out, status));
  });
}

int32_t ark355_points_check(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* raw, uint64_t n, int32_t method,
                            uint8_t* status) {
  if (!ctx) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    ARK_REQUIRE(group == 1 || group == 2, ARK355_EINVAL, "ark355_points_check: group must be 1 or 2");
    ARK_REQUIRE(method == 0 || method == 1, ARK355_EINVAL, "ark355_points_check: unknown method");
    ARK_REQUIRE(n == 0 || raw, ARK355_EINVAL, "ark355_points_check: raw is NULL");
    ARK_REQUIRE(n == 0 || status, ARK355_EINVAL, "ark355_points_check: status is NULL");
    ARK_REQUIRE(n <= 0xFFFFFFFFull, ARK355_EINVAL, "ark355_points_check: n must stay below 2^32");
    CtxExtra& ex = extra(ctx);
    CURVE_DISPATCH(curve, A::points_check(ctx, ex.generic, group, raw, n, method, status));
  });
}

int32_t ark355_verify_batch_pvk(ark355_ctx* ctx, const ark355_pvk* pvk, const ark355_proof_raw* proofs, const uint8_t* public_inputs,
                                const uint8_t* rho, uint64_t count, int32_t* ok) {
  if (!ctx || !pvk || !pvk->d || !proofs || !ok || (pvk->d->ell > 1 && !public_inputs)) return ARK355_EINVAL;
  *ok = 0;
  return guarded(ctx, [&] {
    CtxExtra& ex = extra(ctx);
    bool good = false;
    CURVE_DISPATCH(pvk->d->curve, good = A::verify_batch_pvk(ctx, ex.generic, *pvk->d, proofs, public_inputs, rho, count));
    *ok = good ? 1 : 0;
  });
}

int32_t ark355_setup_scalars(int32_t curve, uint64_t n, uint64_t ell, uint64_t w, const uint64_t* const row_ptr[3],
                             const uint32_t* const col[3], const uint8_t* const coeff[3], const uint8_t* trapdoor,
                             uint8_t* out_u, uint8_t* out_v, uint8_t* out_w, uint8_t* out_l, uint8_t* out_gamma_abc,
                             uint8_t* out_h) {
  // zero-length outputs may be NULL (l when num_witness == 0, h when the domain has one point)
  if (!row_ptr || !col || !coeff || !trapdoor || !out_u || !out_v || !out_w || (w && !out_l) || !out_gamma_abc ||
      (n + ell > 1 && !out_h))
    return ARK355_EINVAL;
  for (int i = 0; i < 3; i++)
    if (!row_ptr[i] || (row_ptr[i][n] && (!col[i] || !coeff[i]))) return ARK355_EINVAL;
  return guarded(nullptr, [&] {
    CURVE_DISPATCH(curve, A::setup_scalars(n, ell, w, row_ptr, col, coeff, trapdoor, out_u, out_v, out_w, out_l, out_gamma_abc, out_h));
  });
}

int32_t ark355_setup(ark355_ctx* ctx, const ark355_r1cs* r1cs, const uint8_t* g1_base, const uint8_t* g2_base,
                     const uint8_t* trapdoor, const ark355_setup_out* out, ark355_pk** out_pk) {
  if (out_pk) *out_pk = nullptr;
  if (!ctx) return ARK355_EINVAL;
  return guarded(ctx, [&] {
    ARK_REQUIRE(r1cs && r1cs->d, ARK355_EINVAL, "ark355_setup: r1cs is NULL");
    ARK_REQUIRE(g1_base && g2_base, ARK355_EINVAL, "ark355_setup: a base is NULL");
    ARK_REQUIRE(trapdoor, ARK355_EINVAL, "ark355_setup: trapdoor is NULL");
    ARK_REQUIRE(out || out_pk, ARK355_EINVAL, "ark355_setup: neither out nor out_pk is given");
    PkDev* d = nullptr;
    CURVE_DISPATCH(r1cs->d->curve, d = A::setup(ctx, *r1cs->d, g1_base, g2_base, trapdoor, out, out_pk != nullptr));
    if (out_pk) *out_pk = new ark355_pk{d};
  });
}

int32_t ark355_get_timings(const ark355_ctx* ctx, ark355_timings* out) {
  if (!ctx || !out) return ARK355_EINVAL;
  *out = ctx->timings;
  return ARK355_OK;
}

int32_t ark355_get_kernel_stats(const ark355_ctx* ctx, float* accumulate_ms, uint64_t* launches, uint64_t* points) {
  if (!ctx) return ARK355_EINVAL;
  if (accumulate_ms) *accumulate_ms = ctx->acc_ms;
  if (launches) *launches = ctx->acc_launches;
  if (points) *points = ctx->acc_points;
  return ARK355_OK;
}

}  // extern "C"
