/* ark355.h -- C ABI of libark355.so, the MI355X (gfx950) Groth16 prover backend.
 *
 * This is the drop-in boundary for the hot path of `ark_snark::SNARK::prove`
 * (/root/reference/snark/src/lib.rs:50-54): the Rust host keeps `ark-relations`' ConstraintSystem
 * (/root/reference/relations/src/gr1cs/constraint_system.rs) untouched, extracts
 *   - the R1CS matrices once per circuit   (to_matrices, constraint_system.rs:768-774;
 *                                           Matrix<F> = Vec<Vec<(F, usize)>>, utils/matrix.rs:4)
 *   - the full assignment z per proof      (instance_assignment || witness_assignment,
 *                                           constraint_system.rs:193-206, assignment.rs:11-21)
 * and calls the entry points below; see INTEGRATION.md for the Rust `extern "C"` block.
 *
 * Conventions:
 *  - every function returns int32: 0 = OK, negative = error (no exception crosses the boundary);
 *  - field elements are ark-ff memory images: little-endian u64 limbs, MONTGOMERY form
 *    (Fr: 32 B; Fq: 48 B BLS12-381 / 32 B BN254).  MSM scalars and r, s are CANONICAL
 *    (`into_bigint`) 32-byte little-endian integers;
 *  - G1 affine = x || y ; G2 affine = x.c0 || x.c1 || y.c0 || y.c1 ; the point at infinity is the
 *    all-zero encoding (the shim maps `Affine::infinity == true` to zeros and back);
 *  - the caller owns all host buffers; the library copies during the call and never retains host
 *    pointers.  Handles are opaque and freed by the matching *_free / *_destroy;
 *  - `*_dev` variants take DEVICE pointers (HIP allocations of the calling process).  The library reads them on
 *    its own streams: the CALLER must have completed (stream- or device-synchronised) whatever produced those
 *    buffers before the call.  Only ark355_ntt_fr_dev takes the producer's stream (void*, NULL = the context's own)
 *    and orders itself on it.
 */
#ifndef ARK355_H
#define ARK355_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ark355_ctx ark355_ctx;
typedef struct ark355_pk ark355_pk;
typedef struct ark355_r1cs ark355_r1cs;
typedef struct ark355_gr1cs ark355_gr1cs;
typedef struct ark355_sr1cs ark355_sr1cs;     /* a resident R1CS rewritten as Square R1CS: ark355_sr1cs_from_r1cs */
typedef struct ark355_bases ark355_bases;     /* resident MSM bases: ark355_bases_load */

enum { ARK355_BLS12_381 = 0, ARK355_BN254 = 1 };

/* error codes; the -16.. block mirrors ark_relations SynthesisError (utils/error.rs:5-21) */
enum {
  ARK355_OK = 0,
  ARK355_EINVAL = -1,
  ARK355_ENOMEM = -2,
  ARK355_EHIP = -3,
  ARK355_ERCCL = -4,
  ARK355_ENODEV = -5,
  ARK355_E_ASSIGNMENT_MISSING = -16,      /* SynthesisError::AssignmentMissing        (error.rs:9)  */
  ARK355_E_UNSATISFIABLE = -17,           /* SynthesisError::Unsatisfiable            (error.rs:14) */
  ARK355_E_POLY_DEGREE_TOO_LARGE = -18    /* SynthesisError::PolynomialDegreeTooLarge (error.rs:16) */
};

/* ---- context ------------------------------------------------------------------------------ */
int32_t ark355_ctx_create(int32_t device_id, ark355_ctx** out);
void ark355_ctx_destroy(ark355_ctx* ctx);
const char* ark355_last_error(const ark355_ctx* ctx);
/* library/ABI version: (major << 16) | minor */
uint32_t ark355_version(void);
/* sizes in bytes for `curve`: what[0]=Fr, [1]=Fq, [2]=G1 affine, [3]=G2 affine */
int32_t ark355_sizes(int32_t curve, uint32_t what[4]);

/* ---- runtime policy ------------------------------------------------------------------------------------------------
 * Every runtime switch of the library lives in ONE per-context struct (snark_amd/csrc/policy.h).  The environment
 * variables ARK355_<NAME> are read exactly once, by ark355_ctx_create; afterwards a context's policy changes only through
 * ark355_ctx_set_policy -- nothing on the proving path reads the environment, and two contexts of a process may differ
 * (A/B measurements inside one process).  Names (value = integer):
 *   per proof     SCHED (-1 measured choice [default], 0 one stream, 1 five-stream pipeline, 2 pipeline + epilogue stream
 *                 synchronises, 3 one stream + wait inside the HIP runtime), SCHED_EXPLORE (samples per schedule before the
 *                 measured choice latches; 0 = static defaults), WAIT_SPIN, WAIT_ADAPT, STREAM_PRIO, BATCH_TAILS,
 *                 SIDE_G2_TAILS, SIDE_WM, SIDE_G1_TAILS (a proof alone on the device: G2 tails / witness map / the tails of A, B1, L' on
 *                 side streams), SIDE_H_TAILS (pipeline: the last MSM's tails on the sort stream),
 *                 TRACE_HOST; legacy spellings SERIAL (1 -> SCHED 0, 0 -> SCHED 1) and EPILOGUE_SYNC (on a pipeline: 1 -> 2);
 *   per key load  MSM_C, MSM_C_H (window size of all tables / of the h_query table; 0 = planner), PACK_ROWS
 *                 (table rows bit-packed 1 / one word per limb 0 / per curve -1), TABLE_STRIDE, HBM_BUDGET_MB, SHARD_DIST_WM, RCCL_SELF (diagnostic: a rank at world size 1 exchanges with
 *                 itself) -- read when a key or base set is loaded THROUGH this context;
 *   per call      MSM_SEG, ACC_THREADS (workgroup size of the LDS-free accumulation kernels: 64 / 128 / 256; 0 [default]: 64 for a
 *                 proof alone on one stream, else 256), NTT_RMAX, NTT_DIRECT_MAX, NTT_NOFUSE (A/B and test knobs).
 *                 CHECK_SATISFIED (default 0: a proof is computed for whatever z is handed in, as ark-groth16's release build does;
 *                 1: ark355_prove / _dev / _batch also compare a_i b_i with c_i on the rows the witness map computes anyway -- the
 *                 check ark-groth16 runs under debug_assert!(cs.is_satisfied()) -- and return ARK355_E_UNSATISFIABLE, with the index
 *                 of the first unsatisfied constraint in ark355_last_error, instead of a proof that cannot verify).
 *                 H_EVAL (read at the FIRST proof of a whole key, which decides for the life of that key: 1 its h query moves to
 *                 the evaluation basis of the coset -- a proof then runs four transforms instead of six, same proof bytes --, 0 it
 *                 stays in the coefficient basis, -1 [default] evaluation basis from domain size 2^16 on; key shards always keep the
 *                 coefficient basis; see ark355_pk_h_eval),
 *                 PAIRING_DEVICE (0 host threads, 1 device, -1 [default] device from PAIRING_DEVICE_MIN pairs on) and
 *                 PAIRING_DEVICE_MIN: where the Miller loops of ark355_multi_pairing and ark355_verify_batch run;
 *                 PAIRING_EACH_MIN: the "from ... on" of ark355_pairing_groups and ark355_verify_each, in groups / proofs.
 *                 LCS_ROW_LDS_MAX (ark355_gr1cs_from_lcs: the longest expanded LC whose sort-and-merge runs in LDS, 1 .. 1024
 *                 [default 1024, what the workgroup's 8 KiB of keys hold]; longer ones take the path that works at any length).
 *                 COLS_LANE_MAX (ark355_gr1cs_mat_vec_t / ark355_gr1cs_columns_at: the longest column a single lane sums
 *                 [default 64; <= 0 selects it]; longer ones are cut into chunks of 2048 entries, one workgroup each).
 *                 POLY_LANE_COEFFS (ark355_poly_eval_fr / ark355_poly_div_linear_fr: the consecutive coefficients a lane owns
 *                 [default 8; <= 0 selects it; clamped to 1 .. 8]; a test knob, the outputs do not depend on it).
 *                 EVALS_LANE_POINTS (ark355_evals_eval_fr / ark355_evals_div_linear_fr: the consecutive domain points a lane owns
 *                 [default 8; <= 0 selects it; clamped to 1 .. 8]; a test knob, the outputs do not depend on it).
 *                 SUMCHECK_LANE_PAIRS (ark355_sumcheck_round: the consecutive output pairs a lane owns; ark355_mle_fix_fr /
 *                 ark355_mle_eval_fr: the consecutive outputs a lane owns [default 1; <= 0 selects it; clamped to 1 .. 8]; the
 *                 outputs do not depend on it).
 *                 MLE_OPEN_LANE_ENTRIES (ark355_mle_quotients_fr / ark355_mle_open_dev: the consecutive table entries a lane owns
 *                 [default 8; <= 0 selects it; clamped to 1 .. 8 and rounded down to a power of two]; the outputs do not depend
 *                 on it).
 *                 MSM_BATCH_SMALL_MAX (ark355_msm_batch_dev / ark355_mle_open_dev: the longest segment that takes the short route
 *                 [default: see that block; negative selects it; 0 switches the route off; clamped to 2^14]; the outputs do not
 *                 depend on it).
 * ARK355_EINVAL for an unknown name.  ark355_prove_batch runs its worker contexts under the caller's policy.
 * (No counterpart in the reference: ark-groth16 has no runtime knobs; rayon's thread count is its only one.) */
int32_t ark355_ctx_set_policy(ark355_ctx* ctx, const char* name, int64_t value);
int32_t ark355_ctx_get_policy(ark355_ctx* ctx, const char* name, int64_t* value);

/* What the measured schedule choice (SCHED = -1) has seen for proofs shaped like `pk` on this context's device, for the
 * class "alone on the device" (in_flight = 0) or "other proofs in flight" (in_flight != 0): the schedule it latched
 * (-1 while still exploring / never run), per schedule the samples taken and their mean wall time in ms, and the
 * schedule the LAST proof of this context ran as.  ark355_sched_reset forgets the device's measurements. */
typedef struct {
  int32_t latched;
  int32_t last;
  uint32_t samples[4];
  double mean_ms[4];
} ark355_sched_report;
int32_t ark355_sched_info(const ark355_ctx* ctx, const ark355_pk* pk, int32_t in_flight, ark355_sched_report* out);
int32_t ark355_sched_reset(const ark355_ctx* ctx);
/* Diagnostic: which of the library's HIP streams share an in-order hardware queue of the runtime (streams on one queue
 * serialise whatever their events say).  Probes, on an IDLE device, the own streams of `count` (<= 16) contexts followed
 * by the three feeder streams of ctxs[0]'s pipeline: serialised is an (count + 3) x (count + 3) row-major matrix,
 * [i][j] = 1 when a kernel on stream j waited for a spinning kernel on stream i, 0 when it overtook it, -1 when the build
 * cannot measure it.  bench.py prints it; nothing on the proving path depends on it. */
int32_t ark355_diag_streams(ark355_ctx** ctxs, uint32_t count, int8_t* serialised);
/* Diagnostic: GPU-side cost of one dispatch in an in-order stream on this box: `launches` kernels that each spin for
 * `spin_us`, back to back; *gap_us = elapsed / launches - spin_us (a few us on most boxes, 50-90 us on some: see
 * DESIGN.md section 10).  *lanes (may be NULL) = the number of streams on pairwise different hardware queues the library
 * found for one-stream proofs on this device (probed once, at the first ark355_ctx_create). */
int32_t ark355_diag_dispatch(ark355_ctx* ctx, uint32_t launches, uint32_t spin_us, float* gap_us, uint32_t* lanes);
/* Diagnostic: the rate at which THIS box issues v_mad_u64_u32 right now -- the instruction the bucket-accumulation kernels are
 * made of, at their occupancy (two waves per SIMD), for about target_ms (0.1 .. 1000) milliseconds on the context's stream.
 * *tmad_per_s = 10^12 multiply-adds per second over the whole chip (negative: the build cannot measure it), *elapsed_ms (may be
 * NULL) = the duration of the measuring launch.  The sustained gfx clock under the power cap differs from box to box by a few
 * per cent; bench.py prices its integer roofline against this reading and reports box-normalised times with it. */
int32_t ark355_diag_mad_rate(ark355_ctx* ctx, float target_ms, float* tmad_per_s, float* elapsed_ms);
/* Diagnostic: the GPU's free-running counters, read by one wave per compute unit at (nearly) the same moment on the context's
 * stream (the call synchronises that stream): pairs[2 i] = shader-clock cycles (s_memtime: follows the gfx clock the power
 * management grants), pairs[2 i + 1] = ticks of the constant 100 MHz reference (s_memrealtime), for compute unit slot i < *count
 * (1024 slots; zeros where no wave landed; capacity = pairs the buffer holds, at least 1024).  The cycle counters of different
 * compute units differ by arbitrary offsets: two calls bracket a region, and per slot present in both
 * (cycles delta) / (ticks delta) x 100 MHz is the region's mean gfx clock; bench.py reports the median over the slots and
 * `gfx_cycles_per_constraint` with it. */
int32_t ark355_diag_clocks(ark355_ctx* ctx, uint64_t* pairs, uint32_t capacity, uint32_t* count);
/* Diagnostic: the SORT stage of an MSM on its own -- signed window digits, bucket histogram, exclusive scan, placement --
 * exactly as every MSM and proof runs it (the library's own msm_sort_plan / msm_sort_run on the context's stream and scratch),
 * with everything it leaves on the device copied back.  bases == NULL: the plan of a one-shot MSM of n terms (no window tables,
 * every window its own bucket set); a handle: the plan of that handle's window tables (n <= its rows, same curve).  scalars: n
 * host scalars of 32 bytes, canonical, or Montgomery images with scalars_mont != 0.
 *   plan[0] window bits c, [1] windows per scalar, [2] window stride, [3] bucket sets, [4] buckets in all (sets x 2^(c-1)),
 *   [5] 1 when scalars above (r - 1) / 2 are replaced by r - k with flipped signs, [6] table rows per window block (the handle's
 *   rows; 0 without tables), [7] 1 when the one-pass counting sort ran (more first-level bins than the two-level sort keeps in LDS);
 *   *total = number of non-zero digits;
 *   counts / offsets: per bucket its entries and their exclusive prefix sum (bucket_capacity >= plan[4] words each);
 *   sorted_keys / sorted_vals: *total entries grouped by bucket (entry_capacity >= *total words each): key = set * 2^(c-1) +
 *   digit - 1 with window w in set w % stride, value = (w / stride) * plan[6] + scalar index, bit 31 = subtract.  The order
 *   inside a bucket is unspecified.
 * Each of the two array pairs may be NULL (both of a pair): a call with all four NULL returns the plan and *total, so that the
 * caller can size its buffers.  ARK355_EINVAL: a NULL context, plan or total (before any HIP call), a capacity below what is
 * needed (plan and *total are written all the same), a handle of another curve, more scalars than the handle has rows. */
#define ARK355_SORT_PLAN_WORDS 8
int32_t ark355_diag_msm_sort(ark355_ctx* ctx, int32_t curve, const ark355_bases* bases, const uint8_t* scalars, uint64_t n,
                             int32_t scalars_mont, uint32_t plan[ARK355_SORT_PLAN_WORDS], uint32_t* counts, uint32_t* offsets,
                             uint64_t bucket_capacity, uint32_t* sorted_keys, uint32_t* sorted_vals, uint64_t entry_capacity,
                             uint32_t* total);
/* Diagnostic (a TEST entry): one field primitive of the library's arithmetic layers on operands the caller designed, one lane per
 * element on the context's stream (workgroups of 256 lanes, any n up to ARK355_FIELD_OPS_MAX_N).  The kernels call the very functions
 * the production kernels call, instantiated on the production parameter classes; nothing is converted, reduced or checked on the way
 * in, so an operand must satisfy the documented precondition of the operation it is sent to (csrc/field.cuh, csrc/field28.cuh).
 *   field   ARK355_FLD_*: the 32-bit-limb Montgomery fields Fq / Fr of both curves, their quadratic extensions Fq2, and the
 *           radix-2^28 form of Fq the bucket kernels compute in (Fq28).
 *   op      ARK355_FOP_*.  Fq / Fr: ADD SUB NEG DBL MUL (inlined multiplier) MUL_NI (out of line) SQR MUL2SUM (x0 x1 + x2 x3) MUL_SUB
 *           (x0 x1 - x2 x3) INV TO_MONT FROM_MONT.  Fq2: ADD SUB NEG MUL MUL_NI SQR SQR_NI INV MUL_SUB.  Fq28: FROM_FP TO_FP
 *           TO_FP_LT8 NORM CANON IS_ZERO (is_zero_mod_p) IS_ZERO_INL HINT (multiple_hint) ADD MUL SQR MUL2SUM MUL4SUM
 *           (x0 x1 + x2 x3 + x4 x5 + x6 x7), COND_SUB + log2 K for K = 1, 2, 4, 8, 16, and the biased FOP28_SUB + 16 K + BETA
 *           (x0 - x1 + K p) / FOP28_NEG + 16 K + BETA (K p - x0) for the (K, BETA) classes the bucket and tail kernels instantiate:
 *           sub (3,1) (5,1) (6,1) (8,1) (11,1); neg (2,1) (3,1) (3,3) (4,2) (4,3) (5,1) (5,4) (6,1) (8,1).  (The Fq28 codes are
 *           the ARK355_FOP28_* values.)
 *   operands  operand_count host arrays of n elements each, raw little-endian 32-bit limb words: 12 (BLS12-381 Fq) or 8 words per
 *           Fq / Fr element, twice that per Fq2 element (c0 then c1), 14 (BLS12-381) or 10 (BN254) words per Fq28 element --
 *           FROM_FP takes Fq words.  operand_count must be the operation's arity (1, 2, 4 or 8).
 *   result  n elements of the same layout (TO_FP / TO_FP_LT8: Fq words; IS_ZERO / IS_ZERO_INL / HINT: one word per element);
 *           result_capacity = the words the buffer holds.
 *   *flavour  written by the kernel itself: 1 when it was compiled with the inline-assembly multiplier of field.cuh (the device
 *           build), 0 otherwise (the portable multiplier).
 * ARK355_EINVAL, before any HIP call: a NULL context, operands, operand array, result or flavour; an unknown field or operation; a
 * combination the library cannot instantiate (MUL2SUM / MUL_SUB on BLS12-381 Fr, whose modulus leaves one spare top bit where the
 * dual-product chain needs two; an operation of another field type; a bias class no kernel uses); a wrong operand_count; n above the
 * limit; a result_capacity below n elements. */
#define ARK355_FIELD_OPS_MAX_N (1u << 24)
enum {
  ARK355_FLD_BLS_FQ = 0, ARK355_FLD_BLS_FR = 1, ARK355_FLD_BN_FQ = 2, ARK355_FLD_BN_FR = 3, ARK355_FLD_BLS_FQ2 = 4,
  ARK355_FLD_BN_FQ2 = 5, ARK355_FLD_BLS_FQ28 = 6, ARK355_FLD_BN_FQ28 = 7
};
enum {
  ARK355_FOP_ADD = 0, ARK355_FOP_SUB = 1, ARK355_FOP_NEG = 2, ARK355_FOP_DBL = 3, ARK355_FOP_MUL = 4, ARK355_FOP_MUL_NI = 5,
  ARK355_FOP_SQR = 6, ARK355_FOP_MUL2SUM = 7, ARK355_FOP_MUL_SUB = 8, ARK355_FOP_INV = 9, ARK355_FOP_TO_MONT = 10,
  ARK355_FOP_FROM_MONT = 11, ARK355_FOP_SQR_NI = 12,
  ARK355_FOP28_FROM_FP = 32, ARK355_FOP28_TO_FP = 33, ARK355_FOP28_TO_FP_LT8 = 34, ARK355_FOP28_NORM = 35, ARK355_FOP28_CANON = 36,
  ARK355_FOP28_IS_ZERO = 37, ARK355_FOP28_IS_ZERO_INL = 38, ARK355_FOP28_HINT = 39, ARK355_FOP28_ADD = 40, ARK355_FOP28_MUL = 41,
  ARK355_FOP28_SQR = 42, ARK355_FOP28_MUL2SUM = 43, ARK355_FOP28_MUL4SUM = 44, ARK355_FOP28_COND_SUB = 48,
  ARK355_FOP28_SUB = 256, ARK355_FOP28_NEG = 512
};
int32_t ark355_diag_field_ops(ark355_ctx* ctx, int32_t field, int32_t op, const uint32_t* const* operands, uint32_t operand_count,
                              uint64_t n, uint32_t* result, uint64_t result_capacity, uint32_t* flavour);

/* Page-locked host memory for assignments / key vectors handed to the entry points below: H2D copies from pinned
 * memory run at PCIe rate (~55 GB/s) and truly asynchronously; pageable memory is staged by the runtime at a fraction
 * of that (a 32 MiB assignment at n = 2^20: ~0.6 ms pinned vs several ms pageable).  Optional: every entry point accepts
 * ordinary memory too. */
int32_t ark355_host_alloc(uint64_t bytes, void** out);
void ark355_host_free(void* p);

/* ---- proving key (replaces holding ark_groth16::ProvingKey<E> on the host; SNARK::ProvingKey,
 *      snark/src/lib.rs:25) ------------------------------------------------------------------- */
typedef struct {
  uint64_t num_instance;      /* ell, including the constant One (constraint_system.rs:218-220) */
  uint64_t num_witness;       /* w   (constraint_system.rs:223-225)                            */
  uint64_t domain_size;       /* N = next_pow2(n + ell); h_query holds N-1 points              */
  const uint8_t* a_query;     /* (ell+w) G1 */
  const uint8_t* b_g1_query;  /* (ell+w) G1 */
  const uint8_t* b_g2_query;  /* (ell+w) G2 */
  const uint8_t* h_query;     /* (N-1)   G1 */
  const uint8_t* l_query;     /* w       G1 */
  const uint8_t* alpha_g1;
  const uint8_t* beta_g1;
  const uint8_t* delta_g1;
  const uint8_t* beta_g2;
  const uint8_t* delta_g2;
} ark355_pk_desc;

int32_t ark355_pk_load(ark355_ctx* ctx, int32_t curve, const ark355_pk_desc* desc, ark355_pk** out);
void ark355_pk_free(ark355_pk* pk);

/* ---- R1CS matrices in CSR (replaces walking Matrix<F> rows on the host: mat_vec_mul,
 *      utils/matrix.rs:26-36; column convention Variable::get_variable_index,
 *      utils/variable.rs:105-113: 0 = One, 1..ell-1 = instance, ell.. = witness) --------------- */
int32_t ark355_r1cs_load(ark355_ctx* ctx, int32_t curve, uint64_t n_constraints, uint64_t num_instance,
                         uint64_t num_witness, const uint64_t* const row_ptr[3],
                         const uint32_t* const col[3], const uint8_t* const coeff[3],
                         ark355_r1cs** out);
void ark355_r1cs_free(ark355_r1cs* r1cs);
/* domain size N the library will use for this instance */
uint64_t ark355_r1cs_domain_size(const ark355_r1cs* r1cs);

/* ---- proof (SNARK::Proof, snark/src/lib.rs:32): affine A (G1), B (G2), C (G1), Montgomery raw.
 *      The arrays are sized for BLS12-381 (96 / 192 B); BN254 points (64 / 128 B) occupy the leading bytes of each
 *      array and the rest is zero -- ark355_sizes() gives the sizes in use. */
typedef struct {
  uint8_t a[96];
  uint8_t b[192];
  uint8_t c[96];
} ark355_proof_raw;

/* SNARK::prove hot path (snark/src/lib.rs:50-54; upstream create_proof_with_reduction_and_matrices):
 * z = full assignment (ell+w Fr, Montgomery), r/s canonical.  Returns ARK355_E_ASSIGNMENT_MISSING if
 * z_len < ell+w. */
int32_t ark355_prove(ark355_ctx* ctx, const ark355_pk* pk, const ark355_r1cs* r1cs, const uint8_t* z,
                     uint64_t z_len, const uint8_t r[32], const uint8_t s[32], ark355_proof_raw* out);
/* same, z already resident in HBM */
int32_t ark355_prove_dev(ark355_ctx* ctx, const ark355_pk* pk, const ark355_r1cs* r1cs, const void* d_z,
                         uint64_t z_len, const uint8_t r[32], const uint8_t s[32], ark355_proof_raw* out);

/* Many independent proofs of ONE circuit on one GPU (BASELINE.json configs[4]: 64 proofs at n = 2^18, eight per
 * GPU).  Replaces a pool of OS threads that each call SNARK::prove (snark/src/lib.rs:50-54) -- the reference's
 * ConstraintSystemRef is Rc<RefCell<..>> (constraint_system_ref.rs:33), so upstream parallelism is exactly "one
 * thread per proof" (Threading).  z[i]: host assignment of proof i (z_len Fr each, Montgomery);
 * r, s: count x 32 B canonical; out: count proofs.  Up to `inflight` (1..16) proofs are in flight on private
 * streams and scratch owned by `ctx`; the key and CSR handles are shared, read-only.  While one proof is in a
 * serial phase (digit sort, last bucket reduction, host finish) the others keep the CUs busy.  Returns the error
 * of the first failing proof (out[] of the others is still written). */
int32_t ark355_prove_batch(ark355_ctx* ctx, const ark355_pk* pk, const ark355_r1cs* r1cs, const uint8_t* const* z,
                           uint64_t z_len, const uint8_t* r, const uint8_t* s, uint64_t count, uint32_t inflight,
                           ark355_proof_raw* out);

/* ---- one proof, MSM term ranges sharded over several GPUs (BASELINE.json configs[2]) ----------
 * Every rank loads shard `shard_index` of `shard_count` of the SAME key descriptor (terms
 * [T*i/G, T*(i+1)/G) of each query vector), computes the witness map redundantly, and returns the five
 * partial sums (A, B1, L', H as G1 XYZZ, then B2 as G2 XYZZ; ark355_partial_size() bytes).  The ranks
 * exchange the partials (an all-gather of <1 KiB per rank: RCCL has no elliptic-curve reduction operator) and
 * each calls ark355_prove_combine, which adds them and finishes the proof -- byte-identical to ark355_prove. */
int32_t ark355_pk_load_shard(ark355_ctx* ctx, int32_t curve, const ark355_pk_desc* desc, uint32_t shard_index,
                             uint32_t shard_count, ark355_pk** out);
uint64_t ark355_partial_size(int32_t curve);
int32_t ark355_prove_shard(ark355_ctx* ctx, const ark355_pk* pk_shard, const ark355_r1cs* r1cs, const uint8_t* z,
                           uint64_t z_len, const uint8_t r[32], const uint8_t s[32], uint8_t* out_partials);
int32_t ark355_prove_combine(ark355_ctx* ctx, int32_t curve, const uint8_t* partials, uint64_t count,
                             const uint8_t r[32], const uint8_t s[32], ark355_proof_raw* out);

/* ---- the exchange behind the ABI: RCCL communicator + collective sharded prove -----------------------------------
 * The reference's parallel unit is one OS thread per proof (ConstraintSystemRef is Rc<RefCell<..>>,
 * relations/src/gr1cs/constraint_system_ref.rs:33) behind SNARK::prove (snark/src/lib.rs:50-54); a single LARGE proof
 * (BASELINE.json configs[2]) is instead split here by MSM term ranges over the GPUs of a node, one host process per GPU.
 * Rank 0 obtains a communicator id (ark355_comm_unique_id) and hands it to the other ranks over whatever channel the
 * host already has (the Rust shim: its own IPC; the Python mirror: torch.distributed's store); every rank then calls
 * ark355_comm_init -- a collective, like ncclCommInitRank underneath.
 * ark355_prove_sharded is collective too: every rank passes its key shard (ark355_pk_load_shard with the rank as shard
 * index and the world size as shard count), the SAME full assignment z and the SAME r, s; every rank receives the same
 * proof, byte-identical to ark355_prove with the whole key.  `mode`:
 *   ARK355_SHARD_WINDOW       one ncclAllGather of the five XYZZ partial sums from HBM (default; latency-bound);
 *   ARK355_SHARD_BUCKET_RING  ring reduce-scatter of the bucket arrays (ncclSend/ncclRecv + EC-add kernel) before the
 *                             bucket reduction -- the literal "all-reduce of partial bucket sums" -- then the all-gather.
 * RCCL failures return ARK355_ERCCL (ark355_last_error has RCCL's message). */
typedef struct ark355_comm ark355_comm;
#define ARK355_COMM_ID_BYTES 128
enum { ARK355_SHARD_WINDOW = 0, ARK355_SHARD_BUCKET_RING = 1 };
int32_t ark355_comm_unique_id(uint8_t id[ARK355_COMM_ID_BYTES]);
int32_t ark355_comm_init(ark355_ctx* ctx, const uint8_t id[ARK355_COMM_ID_BYTES], int32_t rank, int32_t world,
                         ark355_comm** out);
void ark355_comm_destroy(ark355_comm* comm);
int32_t ark355_prove_sharded(ark355_ctx* ctx, ark355_comm* comm, const ark355_pk* pk_shard, const ark355_r1cs* r1cs,
                             const uint8_t* z, uint64_t z_len, const uint8_t r[32], const uint8_t s[32], int32_t mode,
                             ark355_proof_raw* out);
/* same, z already resident in this rank's HBM */
int32_t ark355_prove_sharded_dev(ark355_ctx* ctx, ark355_comm* comm, const ark355_pk* pk_shard, const ark355_r1cs* r1cs,
                                 const void* d_z, uint64_t z_len, const uint8_t r[32], const uint8_t s[32], int32_t mode,
                                 ark355_proof_raw* out);

/* ---- ark-serialize wire formats (SNARK::{ProvingKey, VerifyingKey, Proof}: CanonicalSerialize +
 *      CanonicalDeserialize, snark/src/lib.rs:25-36) ------------------------------------------------------------------
 * Point encodings as upstream writes them: BLS12-381 zcash/IETF (big-endian, flags in the first byte), BN254 ark-ec
 * SWFlags (little-endian, flags in the last byte); compressed != 0 selects the compressed form.  `validate`:
 *   ARK355_VALIDATE_FULL (1)   everything ark-serialize's Validate::Yes checks: reduced coordinates, the curve equation
 *                              (uncompressed form; compressed points are on the curve by construction) AND membership in
 *                              the prime-order subgroup (BLS12-381 G1/G2, BN254 G2; the endomorphism tests described at
 *                              ark355_points_check, equivalent to [r]P = O) -- use it for anything that
 *                              comes from an untrusted party (proofs: a small-order component vanishes in the pairing, so
 *                              without the test one proof has many accepted encodings);
 *   ARK355_VALIDATE_CURVE (2)  the same without the subgroup test (a 64- to 128-bit scalar multiplication per point): the
 *                              explicit opt-out for key material from a trusted source;
 *   ARK355_VALIDATE_NONE (0)   Validate::No.
 * Flag combinations upstream rejects in every mode are rejected in every mode here: BLS12-381 sort bit without the
 * compressed bit or together with the infinity bit, a compressed bit that does not match the requested form
 * (ark-bls12-381 EncodingFlags::get_flags); BN254 both flag bits set (ark-ec SWFlags::from_u8).  Bytes under an infinity
 * flag, in every mode as upstream: BLS12-381 must be all zero (its point readers refuse anything else), BN254 must be
 * reduced field elements and are otherwise ignored (ark-ec's generic reader returns the identity). */
#define ARK355_VALIDATE_NONE 0
#define ARK355_VALIDATE_FULL 1
#define ARK355_VALIDATE_CURVE 2
/* bytes of one encoded point of `group` (1 | 2) */
uint64_t ark355_point_size(int32_t curve, int32_t group, int32_t compressed);
/* the byte stream of an ark_groth16::ProvingKey<E> (vk, beta_g1, delta_g1, a_query, b_g1_query, b_g2_query, h_query,
 * l_query) -> resident key, exactly as ark355_pk_load would build it from the decoded vectors.  The points are decoded
 * on the device (one lane per point; the compressed form costs a square root each).  ARK355_EINVAL for truncated /
 * inconsistent streams and bad points (ark355_last_error names the vector and index). */
int32_t ark355_pk_load_bytes(ark355_ctx* ctx, int32_t curve, const uint8_t* bytes, uint64_t len, int32_t compressed,
                             int32_t validate, ark355_pk** out);
/* dimensions of a resident key: num_instance (ell), num_witness (w), domain size N */
int32_t ark355_pk_dims(const ark355_pk* pk, uint64_t* num_instance, uint64_t* num_witness, uint64_t* domain_size);
/* How a resident key sits in HBM: Pippenger window size c, windows per scalar, window stride of its tables
 * (1 = a table per window: one bucket set, no doublings; s > 1 = every s-th window has a table and an MSM keeps s
 * bucket sets -- chosen at load time as the smallest stride whose tables fit the device next to the provers' scratch;
 * ARK355_ENOMEM from the load when none does) and the bytes its five window tables occupy.  Any pointer may be NULL.
 * (No counterpart in the reference: ark-groth16 keeps `ProvingKey<E>` as plain vectors in host memory.) */
int32_t ark355_pk_table_info(const ark355_pk* pk, uint32_t* window_bits, uint32_t* windows, uint32_t* table_stride,
                             uint64_t* table_bytes);
/* The h query of a resident key (policy H_EVAL of ark355_ctx_set_policy): *state = 0 while the key has not proven yet, 1 once it has settled on the
 * coefficient basis, 2 once its h query is in the evaluation basis of the coset (the key is then bound to the R1CS handle of its
 * first proof and answers every other handle with ARK355_EINVAL).  *binds: how many conversions the key went through (0 or 1:
 * contexts whose first proofs on one key start together wait for the one that converts it).  *bind_seconds: what the conversion
 * took.  Any pointer may be NULL. */
int32_t ark355_pk_h_eval(const ark355_pk* pk, int32_t* state, uint32_t* binds, float* bind_seconds);
/* The two transforms over G1 behind that conversion, on host vectors (tests, diagnostics).  h_query: 2^log_n - 1 raw affine
 * points H_k; index 2^log_n - 1 enters as infinity.  With N = 2^log_n, g the coset generator, w the N-th root of unity:
 *   out_e[j] = sum_k g^-k w^-jk H_k / (N (g^N - 1)),   out_u[j] = sum_k w^-jk H_k / (N (g^N - 1)),   N raw affine points each.
 * Either output may be NULL.  1 <= log_n <= 23. */
int32_t ark355_hbasis_transform(ark355_ctx* ctx, int32_t curve, const uint8_t* h_query, uint32_t log_n, uint8_t* out_e,
                                uint8_t* out_u);
/* out_d[i] = sum_j C[j][i] u[j] over the resident matrix C of `r1`: u is domain_size raw affine points, out_d gets
 * num_instance + num_witness (an empty column gives infinity). */
int32_t ark355_hbasis_gather(ark355_ctx* ctx, const ark355_r1cs* r1, const uint8_t* u, uint8_t* out_d);
/* n encoded points <-> n raw affine images (x || y Montgomery; the layout of every other entry point), on the device */
int32_t ark355_points_decode(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* in, uint64_t n,
                             int32_t compressed, int32_t validate, uint8_t* out_raw);
int32_t ark355_points_encode(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* in_raw, uint64_t n,
                             int32_t compressed, uint8_t* out);
/* Proof = a || b || c; out must hold 2 * point_size(G1) + point_size(G2) bytes */
int32_t ark355_proof_to_bytes(int32_t curve, const ark355_proof_raw* proof, int32_t compressed, uint8_t* out);
int32_t ark355_proof_from_bytes(int32_t curve, const uint8_t* in, uint64_t len, int32_t compressed, int32_t validate,
                                ark355_proof_raw* out);

/* ---- building blocks ---------------------------------------------------------------------- */
/* R1CS -> QAP witness map h[0..N) (Montgomery), SURVEY Appendix A steps 1-5 */
int32_t ark355_witness_map(ark355_ctx* ctx, const ark355_r1cs* r1cs, const uint8_t* z, uint64_t z_len,
                           uint8_t* h_out);
/* The same map computed the way the `world` GPUs of a sharded proof compute it (every rank owns 1/world of each vector,
 * three all-to-all exchanges; snark_amd/csrc/witness_dist_impl.cuh), with ALL ranks on this one device and
 * device-to-device copies as the exchange: the test / diagnostic entry of the distributed path on a single GPU
 * (ark355_prove_sharded runs it over RCCL).  world: a power of two >= 2 with 8 * world^2 <= N; ARK355_EINVAL otherwise. */
int32_t ark355_witness_map_dist_sim(ark355_ctx* ctx, const ark355_r1cs* r1cs, const uint8_t* z, uint64_t z_len,
                                    uint32_t world, uint8_t* h_out);
/* which_is_unsatisfied (constraint_system.rs:661-687) for the R1CS predicate: first_bad = -1 if
 * satisfied, else the first constraint index with <A_i,z>*<B_i,z> != <C_i,z> */
int32_t ark355_is_satisfied(ark355_ctx* ctx, const ark355_r1cs* r1cs, const uint8_t* z, uint64_t z_len,
                            int64_t* first_bad);
/* A z, B z, C z (n Fr each, Montgomery): mat_vec_mul, utils/matrix.rs:26-36 */
int32_t ark355_r1cs_mat_vec(ark355_ctx* ctx, const ark355_r1cs* r1cs, const uint8_t* z, uint64_t z_len,
                            uint8_t* az, uint8_t* bz, uint8_t* cz);

/* ---- GR1CS: every predicate of a constraint system, not only "R1CS" ------------------------------------------------
 * ark-relations keeps a BTreeMap<Label, PredicateConstraintSystem> (constraint_system.rs:44-97): every predicate is a sparse
 * multivariate polynomial of some arity t over t matrices (predicate/polynomial_constraint.rs), "R1CS" (x0 x1 - x2) merely the
 * one registered by default, and to_matrices returns one list of matrices PER LABEL.  A handle holds all of them on the device,
 * with one coefficient pool; the satisfaction check is one fused kernel per predicate (one lane per row: the t inner products,
 * the polynomial, a 64-bit atomic minimum) and one 8-byte copy back for the whole system (snark_amd/csrc/gr1cs_impl.cuh).
 * Limits, checked at load (ARK355_EINVAL beyond them; exponents may be any uint32_t): */
#define ARK355_GR1CS_MAX_ARITY 16
#define ARK355_GR1CS_MAX_TERMS 256
#define ARK355_GR1CS_MAX_FACTORS 1024
#define ARK355_GR1CS_MAX_PREDICATES 1024
#define ARK355_GR1CS_MAX_ROWS 4294967295
typedef struct {
  const char* label;              /* NUL-terminated UTF-8, unique within one load                                        */
  uint32_t arity;                 /* t in 1 .. ARK355_GR1CS_MAX_ARITY                                                    */
  uint64_t n_constraints;         /* rows of each of the t matrices (<= ARK355_GR1CS_MAX_ROWS, as is every matrix's number
                                     of entries); 0 is legal: the default "R1CS" predicate of a circuit without R1CS rows */
  uint32_t n_terms;               /* polynomial = sum_k term_coeff[k] * prod_{j in [term_ptr[k], term_ptr[k+1])} x_{term_var[j]} ^ term_exp[j];
                                     <= ARK355_GR1CS_MAX_TERMS terms, <= ARK355_GR1CS_MAX_FACTORS factors in all; a term without
                                     factors is the constant term, a repeated variable multiplies, exponent 0 contributes 1 */
  const uint8_t* term_coeff;      /* n_terms Fr, Montgomery                                                              */
  const uint32_t* term_ptr;       /* n_terms + 1, non-decreasing from 0                                                  */
  const uint32_t* term_var;       /* each < arity                                                                        */
  const uint32_t* term_exp;
  const uint64_t* const* row_ptr; /* arity CSR matrices (row_ptr: n_constraints + 1 each), the column convention and       */
  const uint32_t* const* col;     /* semantics of ark355_r1cs_load: repeated columns of a row are summed, an empty row is  */
  const uint8_t* const* coeff;    /* the zero linear combination                                                          */
} ark355_predicate_desc;
/* to_matrices for all labels plus get_predicate (constraint_system.rs:768-774, predicate/mod.rs): preds[0 .. n_preds) in any
 * order, n_preds <= ARK355_GR1CS_MAX_PREDICATES.  ARK355_EINVAL (with a message, never a fault) for arity 0, a variable >= arity,
 * a column >= num_instance + num_witness, a row_ptr that decreases, duplicate labels, a NULL where a count is nonzero and
 * anything beyond the limits above. */
int32_t ark355_gr1cs_load(ark355_ctx* ctx, int32_t curve, uint64_t num_instance, uint64_t num_witness,
                          const ark355_predicate_desc* preds, uint32_t n_preds, ark355_gr1cs** out);
void ark355_gr1cs_free(ark355_gr1cs* g);
/* sum of the predicates' rows (constraint_system.rs:210-215) */
uint64_t ark355_gr1cs_num_constraints(const ark355_gr1cs* g);
/* which_is_unsatisfied (constraint_system.rs:652-687): the labels are visited in byte-wise lexicographic order (the BTreeMap's),
 * rows ascending; *predicate = the CALLER's index (into preds of the load) of the first failing predicate in that order,
 * *constraint = its first failing row -- the reference's "<label> - <row>" -- and (-1, -1) when every row is satisfied.
 * ARK355_E_ASSIGNMENT_MISSING if z_len < num_instance + num_witness. */
int32_t ark355_gr1cs_which_is_unsatisfied(ark355_ctx* ctx, const ark355_gr1cs* g, const uint8_t* z, uint64_t z_len,
                                          int64_t* predicate, int64_t* constraint);
/* mat_vec_mul (utils/matrix.rs:26-36) for each of the t matrices of predicate `predicate` (caller's index): out = t x n Fr,
 * matrix-major, Montgomery */
int32_t ark355_gr1cs_mat_vec(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* z, uint64_t z_len,
                             uint8_t* out);
/* PolynomialPredicate::eval on every row (predicate/polynomial_constraint.rs:33-48): out[i] = P(M_0 z, .., M_{t-1} z)_i, n Fr,
 * Montgomery; zero exactly where row i is satisfied */
int32_t ark355_gr1cs_eval(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* z, uint64_t z_len,
                          uint8_t* out);
/* An ordinary ark355_r1cs handle, for ark355_prove* and freed with ark355_r1cs_free, from the predicate labelled "R1CS", built on the
 * device from the resident matrices.  Groth16 proves R1CS only: ARK355_EINVAL when any OTHER predicate carries a constraint
 * (ark355_last_error names its label) -- a proof that drops constraints is not obtainable through this path -- and when the
 * label "R1CS" is absent or not the polynomial x0 x1 - x2 of arity 3. */
int32_t ark355_gr1cs_r1cs(ark355_ctx* ctx, const ark355_gr1cs* g, ark355_r1cs** out);

/* to_matrices() of any resident system (constraint_system.rs:768-774), the read-back of what the entries below and
 * ark355_sr1cs_from_r1cs build on the device.  ark355_gr1cs_dims: any pointer may be NULL.  ark355_gr1cs_pred_dims: nnz takes
 * `arity` entries, any pointer may be NULL; ARK355_EINVAL for a predicate index out of range.  ark355_gr1cs_matrix: matrix `which`
 * (< arity) of predicate `predicate` in the CSR convention of ark355_r1cs_load: row_ptr n_constraints + 1 entries, col and coeff
 * (Montgomery Fr) at least entry_capacity >= nnz[which] entries. */
int32_t ark355_gr1cs_dims(const ark355_gr1cs* g, uint64_t* num_instance, uint64_t* num_witness, uint32_t* n_preds);
int32_t ark355_gr1cs_pred_dims(const ark355_gr1cs* g, uint32_t predicate, uint32_t* arity, uint64_t* n_constraints, uint64_t* nnz);
int32_t ark355_gr1cs_matrix(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, uint32_t which, uint64_t* row_ptr,
                            uint32_t* col, uint8_t* coeff, uint64_t entry_capacity);

/* ---- finalize() on the device: inline the LC map, outline instances (snark_amd/csrc/lcmap_impl.cuh) -------------------------
 * ConstraintSystem::finalize() + to_matrices() (constraint_system.rs:691-804, :826-863; instance_outliner.rs) from the memory
 * images ark-relations keeps before finalize: LcMap's three flat arrays (lc_map.rs:51-56), Variable as a packed u64
 * (utils/variable.rs:4-14: tag in the top 3 bits, payload in the low 61) and InternedField indices into the interner's pool
 * (field_interner.rs:24-69).  All host arrays are copied during the call.
 *
 * Column of a variable: One -> 0; Instance(i) -> i (i < num_instance; Instance(0) is legal and is column 0); Witness(j) ->
 * num_instance + j.  expand(Zero) = 0, expand(v) = 1 * col(v), expand(Lc(k)) = sum over the entries (c, v) of LC k of
 * pool[c] * expand(v); LC k may reference only LCs of a smaller index (constraint_system.rs:735).  Row i of matrix t of a
 * predicate is expand(args[t][i]); the argument may be a bare variable, Zero or an LC (get_lc, :777-788).
 * Every row is stored in CANONICAL FORM: columns strictly ascending, repeated columns merged, entries whose merged coefficient
 * is zero dropped; a row that cancels is empty; a coefficient equal to one carries pool index 0.  The reference compacts only
 * when some LC uses another (:722-725) and otherwise keeps stored order and repeats: it agrees with this entry as linear forms.
 *
 * outline = 1 (outline_r1cs, the label "R1CS", arity 3) or 2 (outline_sr1cs, "SR1CS", arity 2): when that label is absent from
 * preds nothing happens, as in finalize (:698-704).  A present label of another arity is ARK355_EINVAL -- the reference would
 * remap the map and then drop the ArityMismatch of the appended rows; this entry refuses instead.  Otherwise, with ell =
 * num_instance and w = num_witness: num_witness' = w + ell; INSIDE THE LC MAP ONLY One and Instance(0) become Witness(w) and
 * Instance(i) becomes Witness(w + i) -- a bare variable passed directly as a predicate argument is not remapped (the reference
 * rewrites lc_map only, and new_lc_add_helper hands a single-term coefficient-one LC back as the variable itself, :472-499;
 * the quirk is kept) -- and ell rows are appended to the target: R1CS row 0: A = B = col(ell + w), C = col 0; row i: A =
 * col(ell + w), B = col(ell + w + i), C = col i; SR1CS row i: M0 = col i - col(ell + w + i), M1 empty.  The matching assignment
 * is z || 1 || z[1 .. ell).
 *
 * ARK355_EINVAL, with a message that names the array and the first offending index and never a fault (every index is checked
 * by a device pass before a kernel follows it): a NULL where a count is non-zero; lc_offsets[0] != 0 or a decreasing offset; a
 * tag above 4; an instance index >= num_instance, a witness index >= num_witness, an LC index >= n_lcs; an LC entry that
 * references an LC of an index >= its own; a coefficient index >= n_pool; n_pool < 2, pool[0] != 1 or pool[1] != -1; duplicate
 * labels; what ark355_gr1cs_load refuses about a polynomial; a matrix above ARK355_GR1CS_MAX_ROWS non-zeros.  ARK355_ENOMEM when
 * an intermediate does not fit the device or 32-bit indices.  n_lcs = 0, predicates without rows and num_instance = 1 are legal.
 * Policy LCS_ROW_LDS_MAX (per call): the longest expanded LC that is sorted in LDS; longer ones take the any-length path.
 * The result is an ordinary handle: ark355_gr1cs_free, every ark355_gr1cs_* entry, ark355_gr1cs_r1cs -> ark355_sr1cs_from_r1cs. */
#define ARK355_VAR_ZERO 0
#define ARK355_VAR_ONE 1
#define ARK355_VAR_INSTANCE 2
#define ARK355_VAR_WITNESS 3
#define ARK355_VAR_LC 4
typedef struct {                  /* PredicateConstraintSystem before to_matrices (predicate/mod.rs:81-94)                */
  const char* label;
  uint32_t arity;
  uint64_t n_constraints;
  uint32_t n_terms;               /* the polynomial, as in ark355_predicate_desc                                          */
  const uint8_t* term_coeff;
  const uint32_t* term_ptr;
  const uint32_t* term_var;
  const uint32_t* term_exp;
  const uint64_t* const* args;    /* arity arrays of n_constraints Variables: argument_lcs, column-wise                    */
} ark355_predicate_lcs_desc;
typedef struct {
  uint64_t num_instance;
  uint64_t num_witness;
  uint64_t n_lcs;                 /* LcMap: lc_offsets has n_lcs + 1 entries, lc_offsets[0] == 0, non-decreasing          */
  const uint64_t* lc_offsets;
  const uint64_t* lc_vars;        /* lc_offsets[n_lcs] Variables                                                          */
  const uint32_t* lc_coeffs;      /* ... and their indices into pool                                                      */
  uint64_t n_pool;                /* FieldInterner::vec, Montgomery Fr: n_pool >= 2, pool[0] == 1, pool[1] == -1          */
  const uint8_t* pool;
  int32_t outline;                /* 0 none, 1 outline_r1cs, 2 outline_sr1cs                                              */
} ark355_lc_system_desc;
int32_t ark355_gr1cs_from_lcs(ark355_ctx* ctx, int32_t curve, const ark355_lc_system_desc* system,
                              const ark355_predicate_lcs_desc* preds, uint32_t n_preds, ark355_gr1cs** out);

/* ---- Square R1CS: Sr1csAdapter on the device (relations/src/sr1cs/mod.rs:124-265) -----------------------------------------
 * The adapter behind the GM17-style provers (Polymath, Garuda, Pari): n rows <A_i,z><B_i,z> = <C_i,z> become 2n + P rows of the
 * predicate "SR1CS" (x0^2 - x1, arity 2):
 *     row 2i       M0 = A_i + B_i,   M1 = 4 C_i + s_i          s_i: the square variable of row i, (<A_i,z> - <B_i,z>)^2
 *     row 2i + 1   M0 = A_i - B_i,   M1 = s_i
 *     row 2n+k-1   M0 = v_k - x_k,   M1 empty                  one per public variable p_k (ascending) that occurs in A, B or C
 * over renumbered variables: every old column that occurs, public or witness, becomes a witness allocated at its first
 * occurrence (rows ascending; A, then B, then C; entries in stored order; a zero coefficient counts), the square variable of a
 * row follows the row's new variables, and the publics that occur become the inputs 1 .. P.  A public that never occurs gets
 * no input (mod.rs:177-181, :253-262).  num_instance' = 1 + P, num_witness' = U + n with U the old columns that occur.
 * The system is built on the device from the resident CSR arrays (snark_amd/csrc/sr1cs_impl.cuh): no matrix visits the host.
 * Entry order within a row and the merging of repeated columns are unspecified, as for ark355_r1cs_load. */
/* r1cs_to_sr1cs / r1cs_to_sr1cs_with_assignment (mod.rs:124-183, :191-265: the same matrices).  The handle owns copies of what
 * it needs: `r1cs` may be freed afterwards.  ARK355_EINVAL (with a message) for a NULL argument, a handle of another curve or
 * device, 1 + P + U + n >= 2^31 variables, 2 (nnz A + nnz B) + 2 P or nnz C + 2 n above ARK355_GR1CS_MAX_ROWS, a row of 2^30
 * entries or more.  n = 0 is legal: no rows, num_instance' = 1. */
int32_t ark355_sr1cs_from_r1cs(ark355_ctx* ctx, const ark355_r1cs* r1cs, ark355_sr1cs** out);
void ark355_sr1cs_free(ark355_sr1cs* s);
/* the resident system, borrowed: valid until ark355_sr1cs_free, never passed to ark355_gr1cs_free.  One predicate, index 0,
 * label "SR1CS" (predicate/polynomial_constraint.rs): every ark355_gr1cs_* entry works on it, ark355_gr1cs_r1cs refuses it. */
const ark355_gr1cs* ark355_sr1cs_system(const ark355_sr1cs* s);
/* num_instance', num_witness', 2n + P, the non-zeros of M0 and M1; any pointer may be NULL */
int32_t ark355_sr1cs_dims(const ark355_sr1cs* s, uint64_t* num_instance, uint64_t* num_witness, uint64_t* num_constraints,
                          uint64_t nnz[2]);
/* the two BTreeMaps of the adapter (mod.rs:129-130), per old column: num_instance + num_witness entries each, either may be NULL.
 * witness_col[j]: the column of its witness copy (0 for column 0, -1 when j never occurs); instance_col[j]: its new input k
 * for j = p_k, -1 otherwise */
int32_t ark355_sr1cs_var_map(ark355_ctx* ctx, const ark355_sr1cs* s, int64_t* witness_col, int64_t* instance_col);
/* to_matrices()["SR1CS"][which] (which = 0 | 1) in the CSR convention of ark355_r1cs_load: row_ptr 2n + P + 1, col and coeff
 * (Montgomery Fr) nnz[which] entries; ARK355_EINVAL when entry_capacity (entries col and coeff can hold) is below that */
int32_t ark355_sr1cs_matrix(ark355_ctx* ctx, const ark355_sr1cs* s, int32_t which, uint64_t* row_ptr, uint32_t* col,
                            uint8_t* coeff, uint64_t entry_capacity);
/* the assignment of r1cs_to_sr1cs_with_assignment (mod.rs:199-262): z (num_instance + num_witness Fr, Montgomery) -> z_out
 * (num_instance' + num_witness' Fr), every element written.  Two launches: the squares (<A_i,z> - <B_i,z>)^2 of
 * evaluate_constraint (mod.rs:24-56, :238) and the scatter of the copies.  ARK355_E_ASSIGNMENT_MISSING if
 * z_len < num_instance + num_witness.  The _dev variant reads and writes device memory and returns when z_out is complete. */
int32_t ark355_sr1cs_assignment(ark355_ctx* ctx, const ark355_sr1cs* s, const uint8_t* z, uint64_t z_len, uint8_t* z_out);
int32_t ark355_sr1cs_assignment_dev(ark355_ctx* ctx, const ark355_sr1cs* s, const void* d_z, uint64_t z_len, void* d_z_out);

/* ---- Quotient polynomial of any predicate (snark_amd/csrc/quotient_impl.cuh) -------------------------------------------------
 * The step between the assignment of a resident system and the MSMs of a prover over it: for predicate `predicate` (the CALLER's
 * index, as in ark355_gr1cs_eval) with polynomial P of arity t over the matrices M_0 .. M_{t-1} of n rows
 * (predicate/polynomial_constraint.rs; for the system of ark355_sr1cs_system P = x0^2 - x1, sr1cs/mod.rs), on ANY handle -- from
 * ark355_gr1cs_load, from ark355_gr1cs_from_lcs, or the borrowed one of ark355_sr1cs_system:
 *     h(X) = P(m_0(X), .., m_{t-1}(X)) / (X^N - 1).
 * Domain: N = 2^log_domain.  log_n = 0 selects the smallest power of two >= max(n, 2); otherwise log_domain = log_n, and
 *   2^log_n < n is ARK355_EINVAL.  m_k interpolates M_k z over H_N = {w_N^i}; rows n .. N-1 are zero rows: every m_k is 0 there.
 *   A NON-ZERO CONSTANT TERM of P therefore makes the padded rows unsatisfied unless N = n.
 * degree: d, the total degree of P as written: the maximum over its terms of the sum of the term's exponents, summed in 64 bits
 *   (an exponent is any uint32_t).  A term whose coefficient is zero still counts; x^0 contributes 0; a term without factors has
 *   degree 0, as has a polynomial without terms.
 * Extension: D = 1 for d <= 2, otherwise the smallest power of two >= d - 1; log_ext = log2(D); h_len = D * N.
 * Output: h_out = h_len Fr, Montgomery, fully reduced: the coefficients (h_out[j] that of X^j) of the unique polynomial of
 *   degree < D N that agrees with P(m_0(X), .., m_{t-1}(X)) / (X^N - 1) on the coset g H_{DN} = {g w_{DN}^i}, g the generator of
 *   Fr's multiplicative group that every coset transform of this library uses (ark355_ntt_fr with coset = 1) and
 *   w_{DN} the 2^(log_domain + log_ext)-th root of unity of ark355_ntt_fr.
 *   For an assignment that satisfies all N rows (the padded ones included) this is the exact quotient: its degree is at most
 *   (d - 1) N - d and every coefficient above that is zero.  For any other assignment the output is still the value the sentence
 *   above defines -- the promise ark355_witness_map makes for a b - c -- and proves nothing.
 * n = 0 is legal: N = 2, every m_k = 0, h is the constant P(0, .., 0) divided by X^N - 1 on the coset and interpolated.
 * Errors (each leaves a message for ark355_last_error when a context was passed; all are detected before any allocation or
 * launch): ARK355_E_POLY_DEGREE_TOO_LARGE when log_domain or log_domain + log_ext exceeds the two-adicity of Fr (32 for
 * BLS12-381, 28 for BN254); ARK355_EINVAL for a NULL pointer, a predicate index out of range, 2^log_n < n, or a handle built
 * through a context of another device; ARK355_E_ASSIGNMENT_MISSING if z_len < num_instance + num_witness.  ARK355_ENOMEM when
 * the scratch does not fit the device: 2 t vectors of D N Fr (grow-only, owned by the context) plus the D constants
 * (g^N w_D^s - 1)^-1.
 * ark355_gr1cs_quotient_dims runs no HIP call and needs no context; any out pointer may be NULL.  degree, log_domain and
 * log_ext are written whenever the handle and the index are valid -- a refusal reports the 64-bit degree it refused -- and
 * h_len is 0 unless the return value is ARK355_OK.  Its refusals are the ones ark355_gr1cs_quotient makes about the same
 * (g, predicate, log_n), with the same codes.
 * ark355_gr1cs_quotient reads z (num_instance + num_witness Fr, Montgomery) and writes h_out in host memory.  The _dev variant
 * reads d_z and writes d_h_out (h_len Fr) in device memory; like ark355_sr1cs_assignment_dev it works on the context's stream
 * and returns when d_h_out is complete, so its output may feed ark355_msm_dev (scalars_mont = 1) directly. */
int32_t ark355_gr1cs_quotient_dims(const ark355_gr1cs* g, uint32_t predicate, uint32_t log_n, uint64_t* degree,
                                   uint32_t* log_domain, uint32_t* log_ext, uint64_t* h_len);
int32_t ark355_gr1cs_quotient(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* z, uint64_t z_len,
                              uint32_t log_n, uint8_t* h_out);
int32_t ark355_gr1cs_quotient_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* d_z, uint64_t z_len,
                                  uint32_t log_n, void* d_h_out);

/* ---- Column polynomials of any predicate at a point (snark_amd/csrc/columns_impl.cuh) ----------------------------------------
 * The generator's half of a resident system, for ANY handle (ark355_gr1cs_load, ark355_sr1cs_system, ark355_gr1cs_from_lcs) and
 * any predicate of it: the scalars of a key over the system are its column polynomials at the trapdoor point tau,
 *     cols[k][j] = sum_i M_k[i][j] L_i(tau)        (k < t, j < m = num_instance + num_witness),
 * what R1CSToQAP::instance_map_with_evaluation computes as a, b, c for R1CS (without its extra instance rows: a caller who wants
 * them appends the rows e_j to M_0).  Fr values are Montgomery images of 32 bytes, tau is a canonical
 * 32-byte little-endian integer (>= r: ARK355_EINVAL), `predicate` is the CALLER's index.  The _dev variants read and write
 * device memory of the calling process, work on the context's stream and return when the output is complete, so that
 * "matrices -> key scalars -> key points" (ark355_gr1cs_columns_at_dev -> ark355_fixed_base_mul_dev, scalars_mont = 1) stays on
 * the device.  No matrix, and not the Lagrange vector, visits the host.
 * Refusals, all made before any allocation or launch and all with a message in ark355_last_error; the context works after
 * every one of them: ARK355_EINVAL for a NULL pointer, a predicate index out of range, tau >= r, 2^log_n < n, y_len < n, a
 * handle built through a context of another device, t m + 1 >= 2^32 or the predicate's non-zeros summed over its t matrices
 * >= 2^32; ARK355_E_POLY_DEGREE_TOO_LARGE for a domain beyond the two-adicity of Fr; ARK355_ENOMEM when the scratch does not
 * fit (it is allocated before the first launch).  Policy COLS_LANE_MAX (per call) moves the threshold between the two gather
 * paths and never the result. */

/* evaluate_all_lagrange_coefficients: out[i] = L_i(tau) over H_N = {w_N^i}, N = 2^log_n, 0 <= log_n <= two-adicity of Fr
 * (ARK355_E_POLY_DEGREE_TOO_LARGE beyond it).  tau inside the domain gives the indicator vector; N = 1 gives {1}. */
int32_t ark355_lagrange_fr(ark355_ctx* ctx, int32_t curve, uint32_t log_n, const uint8_t tau[32], uint8_t* out);
int32_t ark355_lagrange_fr_dev(ark355_ctx* ctx, int32_t curve, uint32_t log_n, const uint8_t tau[32], void* d_out);

/* Transposed mat_vec_mul for the t matrices of one predicate: out = t x m Fr, matrix-major, m = num_instance + num_witness,
 * out[k][j] = sum over the STORED entries (i, j, c) of M_k of c * y[i]  (repeated columns of a row each contribute, a stored
 * zero contributes zero, a column without entries is zero).  y: n Fr (the predicate's rows); y_len < n is ARK355_EINVAL.
 * Every one of the t m outputs is written.  n = 0 is legal: all zero. */
int32_t ark355_gr1cs_mat_vec_t(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t* y, uint64_t y_len, uint8_t* out);
int32_t ark355_gr1cs_mat_vec_t_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* d_y, uint64_t y_len, void* d_out);

/* The column polynomials of predicate `predicate` at tau: out[k][j] = sum_i M_k[i][j] L_i(tau) = (M_k^T L(tau))_j, the
 * generalisation of R1CSToQAP::instance_map_with_evaluation's a, b, c to any predicate.  Domain exactly as for
 * ark355_gr1cs_quotient: log_n = 0 selects the smallest power of two >= max(n, 2), otherwise N = 2^log_n and 2^log_n < n is
 * ARK355_EINVAL; rows n .. N-1 are zero rows.  The Lagrange vector never visits the host. */
int32_t ark355_gr1cs_columns_at(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t tau[32], uint32_t log_n, uint8_t* out);
int32_t ark355_gr1cs_columns_at_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const uint8_t tau[32], uint32_t log_n, void* d_out);

/* ---- Polynomial openings: evaluate, divide by X - x, combine (snark_amd/csrc/poly_impl.cuh) -----------------------------------
 * What a KZG-style prover (Polymath, Pari, Garuda) does with a challenge x once it has committed: evaluate its polynomials at x
 * (ark-poly DensePolynomial::evaluate), form the witness polynomial (p(X) - p(x)) / (X - x) (ark-poly-commit
 * KZG10::compute_witness_polynomial) and fold several polynomials with powers of a second challenge (DensePolynomial's Add and
 * Mul<F>), so that "assignment -> quotient -> commitments -> openings" stays on the device.  The reference tree holds only the
 * traits and the relations and has no counterpart.
 * Conventions: Fr values are Montgomery images of 32 bytes; outputs are fully reduced; x and the scalars are canonical 32-byte
 * little-endian integers, a value >= r is ARK355_EINVAL.  `count` polynomials of `len` coefficients lie back to back:
 * polynomial k at element k * len, coeffs[k][j] the coefficient of X^j.  The _dev variants read and write device memory of the
 * calling process on the context's stream and return when the output is complete; x and the scalars stay host pointers.
 * eval: out[k] = sum_j coeffs[k][j] x^j, count Fr.  len = 0 gives 0; x = 0 gives coeffs[k][0].
 * div_linear: q_out has the layout of the input, count x len Fr, every element written:
 *     q_out[k][j] = sum_{i > j} coeffs[k][i] x^(i-j-1) for j < len - 1,  q_out[k][len-1] = 0,  rem_out[k] = p_k(x),
 *   the bytes ark355_poly_eval_fr returns, so that p_k(X) = q_k(X) (X - x) + rem_k holds coefficient by coefficient, for any p
 *   and any x, a root or not.  A row of q_out feeds ark355_msm_dev (scalars_mont = 1) with the bases that committed p.
 *   rem_out may be NULL: nothing beyond q_out is written then.  len = 0 writes only rem = 0; len = 1 gives q = {0}, rem = c_0.
 *   In place is legal: q_out == coeffs exactly (every lane loads its coefficients before it stores its quotients and reads
 *   no other lane's input).  Any other overlap of the two ranges, or of rem_out with either, is ARK355_EINVAL.
 * lincomb: out[j] = sum_k scalars[k] * polys[k][j], len Fr; scalars: count x 32 bytes in HOST memory for both variants.
 *   count = 0 writes zeros.  out == polys exactly (in place on polynomial 0) is legal; any other overlap is ARK355_EINVAL.
 * count = 0 returns ARK355_OK and writes nothing, except for lincomb, which writes its len zeros.
 * Refusals, all made before any allocation or launch, each with a message in ark355_last_error; the context works after every
 * one of them: ARK355_EINVAL for a NULL pointer where something is to be read or written (x always; the scalars when
 * count > 0; coefficients and outputs when they hold at least one element), an unknown curve, x or a scalar >= r,
 * len >= 2^32, count * len >= 2^40 (every index is 64-bit; the bound only keeps byte counts far from overflow),
 * count > ARK355_POLY_MAX_COUNT (all three entries), and the overlaps above.  ARK355_ENOMEM when the scratch does not fit: it
 * is grow-only, owned by the context and reserved before the first launch -- 32 * count * (ceil(len / 2048) + ..) bytes of
 * partial values for eval and div_linear, and for the host variants the staging of the polynomials.
 * Policy POLY_LANE_COEFFS (per call; default 8; <= 0 selects it; clamped to 1 .. 8): the consecutive coefficients one lane
 * owns, 256 times as many a workgroup.  It moves the borders of the decomposition and never a byte of any output. */
#define ARK355_POLY_MAX_COUNT 1024
int32_t ark355_poly_eval_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* coeffs, uint64_t len, uint64_t count, const uint8_t x[32],
                            uint8_t* out);
int32_t ark355_poly_eval_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_coeffs, uint64_t len, uint64_t count,
                                const uint8_t x[32], void* d_out);
int32_t ark355_poly_div_linear_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* coeffs, uint64_t len, uint64_t count,
                                  const uint8_t x[32], uint8_t* q_out, uint8_t* rem_out);
int32_t ark355_poly_div_linear_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_coeffs, uint64_t len, uint64_t count,
                                      const uint8_t x[32], void* d_q_out, void* d_rem_out);
int32_t ark355_poly_lincomb_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* polys, uint64_t len, uint64_t count,
                               const uint8_t* scalars, uint8_t* out);
int32_t ark355_poly_lincomb_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_polys, uint64_t len, uint64_t count,
                                   const uint8_t* scalars, void* d_out);

/* ---- Openings in the evaluation basis: evaluate and divide by X - x (snark_amd/csrc/evals_impl.cuh) ---------------------------
 * The same two steps for a polynomial held as its values over a domain, as a prover with a Lagrange-basis key holds it
 * (ark355_lagrange_fr_dev -> ark355_fixed_base_mul_dev build such a key; ark-poly Evaluations::interpolate + evaluate and
 * KZG10::compute_witness_polynomial are the two-transform route this replaces).  No transform runs.
 * N = 2^log_n, w the N-th root of unity of ark355_ntt_fr, s = 1 for coset = 0 and the coset generator of ark355_ntt_fr for
 * coset != 0, a_i = s w^i.  `count` vectors of N Montgomery Fr lie back to back: evals[k][i] = p_k(a_i) for the unique p_k of degree
 * < N.  x is a canonical 32-byte little-endian integer below r.  The _dev variants work on the context's stream and return when
 * the output is complete; x stays a host pointer.
 * eval: out[k] = p_k(x), count Fr: the bytes ark355_poly_eval_fr returns on the coefficients ark355_ntt_fr(inverse = 1, coset)
 *   gives.  For x = a_j that is evals[k][j].
 * div_linear: q_out[k][i] = q_k(a_i) for q_k(X) = (p_k(X) - p_k(x)) / (X - x), count x N Fr, every element written: byte for byte
 *   ark355_ntt_fr(forward, coset) of the q_out of ark355_poly_div_linear_fr on the interpolated coefficients (q_k has degree
 *   <= N - 2, so its N values are exact).  For a_i != x that is (evals[k][i] - y_k) / (a_i - x); at the one j with a_j = x, if any,
 *   - sum_{i != j} q[k][i] w^(i-j).  rem_out[k] = p_k(x), the bytes of eval; rem_out may be NULL.  N = 1 gives q = {0}.
 *   A row of q_out feeds ark355_msm_dev (scalars_mont = 1) with the Lagrange-basis bases that committed evals.
 *   In place is legal: q_out == evals exactly.  Any other overlap of the two ranges, or of rem_out with either, is ARK355_EINVAL.
 * count = 0 returns ARK355_OK and writes nothing.
 * Refusals, all made before any allocation or launch, each with a message in ark355_last_error; the context works after every
 * one of them: ARK355_EINVAL for a NULL pointer where something is to be read or written (x always; evals and the outputs when
 * count > 0), an unknown curve, x >= r, count > ARK355_POLY_MAX_COUNT, count * N >= 2^40 and the overlaps above;
 * ARK355_E_POLY_DEGREE_TOO_LARGE for log_n above the two-adicity of Fr (32 / 28).  ARK355_ENOMEM when the scratch does not fit:
 * it is grow-only, owned by the context and reserved before the first launch -- 32 * count * (ceil(N / 2048) + ..) bytes of
 * partial sums, 12 KiB of tables, and for the host variants the staging of the vectors.
 * Policy EVALS_LANE_POINTS (per call; default 8; <= 0 selects it; clamped to 1 .. 8): the consecutive points one lane owns, 256
 * times as many a workgroup; one field inversion serves a whole workgroup (2048 points at the default).  It never changes a byte
 * of any output. */
int32_t ark355_evals_eval_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t log_n, uint64_t count, int32_t coset,
                             const uint8_t x[32], uint8_t* out);
int32_t ark355_evals_eval_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t log_n, uint64_t count, int32_t coset,
                                 const uint8_t x[32], void* d_out);
int32_t ark355_evals_div_linear_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t log_n, uint64_t count, int32_t coset,
                                   const uint8_t x[32], uint8_t* q_out, uint8_t* rem_out);
int32_t ark355_evals_div_linear_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t log_n, uint64_t count,
                                       int32_t coset, const uint8_t x[32], void* d_q_out, void* d_rem_out);
/* The values of the argument polynomials m_0 .. m_{t-1} of predicate `predicate` over H_N in DEVICE memory: d_out[k][i] =
 * (M_k z)_i for i < n and zero for n <= i < N, t x N Montgomery Fr, matrix-major -- what ark355_gr1cs_mat_vec returns to the host,
 * padded to the domain, so that ark355_evals_eval_fr_dev / ark355_evals_div_linear_fr_dev open m_k without a transform.  The
 * domain rule is that of ark355_gr1cs_quotient (log_n = 0: the smallest power of two >= max(n, 2)), and so are the refusals and
 * their codes, except that ARK355_E_POLY_DEGREE_TOO_LARGE applies to the domain alone: the predicate's degree plays no part. */
int32_t ark355_gr1cs_mat_vec_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* d_z, uint64_t z_len,
                                 uint32_t log_n, void* d_out);

/* ---- Multilinear extensions: the eq table, fixing variables, evaluation (snark_amd/csrc/mle_impl.cuh) ---------------------------
 * The multilinear side of a prover (Spartan- or Garuda-style) over the same resident tables: ark-poly's
 * DenseMultilinearExtension::evaluate and ::fix_variables, little-endian variable order.  v = num_vars, N = 2^v.  A table f holds N
 * Montgomery Fr; index i = sum_j b_j 2^j; f~(x_0 .. x_{v-1}) = sum_i f[i] prod_j (b_j x_j + (1 - b_j)(1 - x_j)): variable 0 is the
 * lowest index bit.  The t x N output of ark355_gr1cs_mat_vec_dev is t such tables.  Fixing variable 0 to r gives
 * f'[i] = f[2i] + r (f[2i+1] - f[2i]), N / 2 entries; the old variable j + 1 becomes variable j.  A point is `num_vars` (fix: k)
 * canonical 32-byte little-endian integers below r, back to back, always in HOST memory.  The _dev variants work on the context's
 * stream and return when the output is complete.
 * eq:   out[i] = prod_j (b_j point_j + (1 - b_j)(1 - point_j)), N Fr; num_vars = 0 writes {1}.  For a point in {0,1}^v it is the
 *   indicator of that index.
 * fix:  variables 0 .. k-1 of `count` back-to-back tables fixed to point[0 .. k): count x 2^(v-k) Fr, back to back, every element
 *   written.  k = 0 copies.  In place is not offered (a lane's output index is another lane's input): any overlap of out with evals
 *   is ARK355_EINVAL.
 * eval: out[k] = f~_k(point), count Fr: the bytes fix gives with k = num_vars.
 * count = 0 returns ARK355_OK and writes nothing.  Every output is fully reduced: the bytes do not depend on the route.
 * Refusals, all made before any allocation or launch, each with a message in ark355_last_error; the context works after every one
 * of them: ARK355_EINVAL for a NULL pointer where something is to be read or written, an unknown curve, a point coordinate >= r,
 * count > ARK355_POLY_MAX_COUNT, num_vars > 40 (the two-adicity of Fr plays no part), count * N >= 2^40, k > num_vars and the
 * overlap above.  ARK355_ENOMEM when the scratch does not fit: it is grow-only, owned by the context and reserved before the first
 * launch -- 32 * count * (N / 2 + N / 4) bytes for the halvings of fix / eval, and for the host variants the staging of the tables.
 * Policy SUMCHECK_LANE_PAIRS (below) also sets the consecutive outputs a lane of fix / eval owns; it never changes a byte. */
int32_t ark355_mle_eq_fr(ark355_ctx* ctx, int32_t curve, uint32_t num_vars, const uint8_t* point, uint8_t* out);
int32_t ark355_mle_eq_fr_dev(ark355_ctx* ctx, int32_t curve, uint32_t num_vars, const uint8_t* point, void* d_out);
int32_t ark355_mle_fix_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t num_vars, uint64_t count, const uint8_t* point,
                          uint32_t k, uint8_t* out);
int32_t ark355_mle_fix_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t num_vars, uint64_t count,
                              const uint8_t* point, uint32_t k, void* d_out);
int32_t ark355_mle_eval_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t num_vars, uint64_t count, const uint8_t* point,
                           uint8_t* out);
int32_t ark355_mle_eval_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t num_vars, uint64_t count,
                               const uint8_t* point, void* d_out);

/* ---- Multilinear openings: quotient tables and PST proofs (snark_amd/csrc/mle_open_impl.cuh) ---------------------------------------
 * The multilinear counterpart of ark355_poly_div_linear_fr: what ark-poly-commit's MultilinearPC::open (PST13) computes for a
 * committed table f at the point p a sum-check ends at.  Conventions of the block above: Montgomery Fr, variable 0 the lowest index
 * bit, the point `num_vars` canonical 32-byte integers below r in HOST memory, `count` tables back to back, v = num_vars, N = 2^v.
 * With f^(0) = f and f^(j+1)[i] = f^(j)[2i] + p_j (f^(j)[2i+1] - f^(j)[2i]), the rule of ark355_mle_fix_fr, the quotient tables are
 *     q_j[i] = f^(j)[2i+1] - f^(j)[2i],   i < 2^(v-1-j),   j = 0 .. v-1
 * and satisfy f~(X) - f~(p) = sum_j (X_j - p_j) q_j~(X_{j+1}, .., X_{v-1}) for every X.
 * quotients: q_out holds count x N Fr, every element written.  Table c starts at element c N; inside it level j occupies the
 *   elements N - 2^(v-j) .. N - 2^(v-j) + 2^(v-1-j) - 1 -- the levels back to back, largest first -- and element N - 1 is f~_c(p),
 *   byte for byte what ark355_mle_eval_fr returns.  rem_out (count Fr) receives the same values and may be NULL.  v = 0 writes only
 *   the value.  Every output is fully reduced: the bytes do not depend on the decomposition.  A level's row feeds ark355_msm_dev
 *   (scalars_mont = 1) directly; its offset is a multiple of 32 bytes.  In place is not offered: any overlap of q_out with evals,
 *   or of rem_out with either, is ARK355_EINVAL.  count = 0 returns ARK355_OK and writes nothing.
 * open_dev: one table in DEVICE memory.  The quotients go to the context's own scratch; for level j the entry runs the MSM of q_j
 *   against level_bases[j], a resident handle of at least 2^(v-1-j) points (the route of ark355_msm_dev with Montgomery scalars).
 *   proofs_out (host): v affine points of the handles' group, G1 or G2, an all-zero quotient level giving the point at infinity
 *   (all-zero bytes); value_out (host): f~(p), one Fr.  v = 0 writes only the value and reads no handle.  With the key
 *   level_bases[j][i] = eq((t_{j+1} .. t_{v-1}), i) g the verifier checks e(C - [y] g, h) = prod_j e(pi_j, [t_j - p_j] h).
 * Refusals, all made before any allocation or launch, each with a message in ark355_last_error; the context works after every one
 * of them: ARK355_EINVAL for a NULL pointer where something is read or written, an unknown curve, a point coordinate >= r,
 * count > ARK355_POLY_MAX_COUNT, num_vars > 40, count * N >= 2^40 and the overlaps above; for open_dev also level_bases NULL with
 * v > 0, a NULL handle, a handle of another curve, handles of mixed groups and a handle with too few bases (the message names the
 * level).  ARK355_ENOMEM when the scratch does not fit: it is grow-only, owned by the context and reserved before the first launch
 * -- 32 * count * (N / 2048 + N / 2048^2) bytes of pass rows, for the host variant the staging of the tables and of the output, for
 * open_dev N Fr of quotients; none of it is shared with the scratch of the MSMs.
 * Policy MLE_OPEN_LANE_ENTRIES (per call; default 8; <= 0 selects it; clamped to 1 .. 8 and rounded down to a power of two): the
 * consecutive entries one lane owns, 256 times as many a workgroup, log2 of that many halvings a pass.  It moves every border of the
 * decomposition and never a byte of any output. */
int32_t ark355_mle_quotients_fr(ark355_ctx* ctx, int32_t curve, const uint8_t* evals, uint32_t num_vars, uint64_t count,
                                const uint8_t* point, uint8_t* q_out, uint8_t* rem_out);
int32_t ark355_mle_quotients_fr_dev(ark355_ctx* ctx, int32_t curve, const void* d_evals, uint32_t num_vars, uint64_t count,
                                    const uint8_t* point, void* d_q_out, void* d_rem_out);
int32_t ark355_mle_open_dev(ark355_ctx* ctx, int32_t curve, const ark355_bases* const* level_bases, const void* d_evals,
                            uint32_t num_vars, const uint8_t* point, uint8_t* proofs_out, uint8_t* value_out);

/* ---- Batched short MSMs: many independent inner products in one launch sequence (snark_amd/csrc/msm_batch_impl.cuh) ---------------
 * `count` independent MSMs, out[s] = sum_{i < n[s]} scalars_s[i] * bases[s][i]: ark-ec's VariableBaseMSM::msm_bigint once per
 * segment -- the levels of a multilinear opening (ark355_mle_open_dev hands all its levels to this driver), the commitments to many
 * small tables.
 * bases[s]: a resident handle (ark355_bases_load); the same handle may appear many times.  d_scalars[s]: n[s] Fr in DEVICE memory,
 *   canonical, or Montgomery images when scalars_mont != 0, as for ark355_msm_dev.  n[s] = 0 reads neither.
 * out_affine (host): count affine points of the handles' group back to back; infinity is all-zero bytes, and so is n[s] = 0.
 * Contract: for every segment the bytes are exactly what ark355_msm_dev(ctx, bases[s], d_scalars[s], n[s], scalars_mont, ..) writes
 *   -- the result is a canonical affine point, whichever route computes it.
 * Refusals, all made before any allocation, copy or launch, each with a message in ark355_last_error that names the segment where
 * there is one; the context works after every one of them: ARK355_EINVAL for a NULL ctx; with count > 0 for a NULL bases, d_scalars,
 * n or out_affine; for count > ARK355_MSM_BATCH_MAX; for a NULL handle (required even where n[s] = 0: the handles fix the group and
 * so the output stride); for a handle of another device than the context's, handles of mixed curves or of mixed groups; for n[s]
 * above the handle's point count; for a NULL d_scalars[s] with n[s] > 0.  ARK355_ENOMEM when the scratch does not fit.  count = 0
 * returns ARK355_OK and writes nothing.
 * Policy MSM_BATCH_SMALL_MAX (per call; int32; default 512, the measured crossover; negative selects it; 0 switches the short route off; clamped to 2^14):
 * a segment with 1 <= n[s] <= MSM_BATCH_SMALL_MAX takes the short route -- the signed window digits of the handle's own plan, then
 * plain sums of the handle's table rows (about 128 mixed additions a scalar at every window size, no sort, no bucket), all such
 * segments of a call in ONE launch sequence with one host wait, the last 2 c group operations a bucket set and one batched inversion
 * on the host.  Every other non-empty segment runs through the pipeline of ark355_msm_dev, one after another.  The policy moves
 * segments between the routes and never a byte of any output.
 * Scratch: grow-only, owned by the context, reserved before the first launch, shared with neither the MSM pipeline's scratch nor the
 * openings' -- one descriptor a short segment, 4 bytes per (scalar, window) and c XYZZ sums per bucket set of every short segment. */
#define ARK355_MSM_BATCH_MAX 4096
int32_t ark355_msm_batch_dev(ark355_ctx* ctx, const ark355_bases* const* bases, const void* const* d_scalars, const uint64_t* n,
                             uint64_t count, int32_t scalars_mont, uint8_t* out_affine);

/* ---- Sum-check of a GR1CS predicate over resident tables (snark_amd/csrc/sumcheck_impl.cuh) ------------------------------------
 * The prover's side of ark-linear-sumcheck's IPForMLSumcheck::prove_round for the claim
 *     S = sum_{i < N} W[i] * P(T_0[i], .., T_{t-1}[i]),   N = 2^num_vars,
 * P the polynomial of predicate `predicate` (the caller's index) of any resident handle, t its arity.
 * d_tables: t x N Montgomery Fr in device memory, matrix-major -- what ark355_gr1cs_mat_vec_dev writes with 2^log_n = N, but any
 *   data is legal.  d_weight: N Fr, or NULL for weight 1 everywhere; typically the output of ark355_mle_eq_fr_dev.
 * d = the predicate's degree as written (the 64-bit quantity ark355_gr1cs_quotient_dims reports), D = d + (d_weight ? 1 : 0),
 * points = D + 1 <= ARK355_SUMCHECK_MAX_POINTS.  A degree as written above the true degree only yields extra, still correct, points.
 * After j challenges the state is the tables folded j times by the rule of ark355_mle_fix_fr: T^(j), W^(j) of 2^(v-j) entries.
 * round: the message of round j + 1 (j = 0 .. v-1) is, for X = 0 .. D,
 *     g[X] = sum_{i < 2^(v-j-1)} Wx * P(A_0, .., A_{t-1}),   A_k = T_k^(j)[2i] + X (T_k^(j)[2i+1] - T_k^(j)[2i]),
 *   Wx formed likewise from W^(j), or 1: `points` Montgomery Fr at evals_out (host).  So g_1(0) + g_1(1) = S and
 *   g_{j+1}(0) + g_{j+1}(1) = g_j(r_j).  Round 1 takes challenge = NULL; round j + 1 > 1 takes r_j (canonical, below r, host), folds
 *   with it and then sums.  A call out of order -- NULL later, non-NULL first, a round after the v-th -- is ARK355_EINVAL and leaves
 *   the state untouched, and so does a challenge >= r.
 * finish: folds with r_v and returns T_0^(v)[0], .., T_{t-1}^(v)[0], W^(v)[0] (1 without a weight): t + 1 Fr at finals_out (host).
 *   The verifier's last check is g_v(r_v) = W * P(T_0, .., T_{t-1}).  finals_out[k] is ark355_mle_eval_fr of table k at (r_1 .. r_v).
 *   num_vars = 0: no round is legal and finish(NULL) returns the inputs' single entries.  finish before the v-th round is
 *   ARK355_EINVAL; after finish only info and free are legal.
 * Ownership: the handle borrows d_tables and d_weight read-only and never writes them; the borrow lasts until the call of round 2
 *   returns (until finish when num_vars <= 1): after that the caller may free or overwrite them.  From round 2 on the handle works
 *   in its own buffers of (t + 1)(N / 2 + N / 4) Fr; they and the partial-sum buffers are allocated in begin (ARK355_ENOMEM there),
 *   no later call allocates, and the state lives in the handle, not in the context's scratch: any other entry may run on the same
 *   context between two rounds.  The gr1cs handle must outlive the sumcheck handle (the polynomial stays resident there).  Every
 *   round returns after one host wait: the next challenge depends on its message.
 * Refusals at begin, each with a message, the context works after every one: ARK355_EINVAL for a NULL g, d_tables or out, a
 *   predicate index out of range, a handle of another device, num_vars > 40, (t + 1) N >= 2^40, and points >
 *   ARK355_SUMCHECK_MAX_POINTS (the message names the degree).  *out is NULL after a refusal.
 * Policy SUMCHECK_LANE_PAIRS (per call; default 1; <= 0 selects it; clamped to 1 .. 8): the consecutive output pairs one lane of the
 *   round kernel owns.  It moves borders and never changes a byte of any output. */
#define ARK355_SUMCHECK_MAX_POINTS 32
typedef struct ark355_sumcheck ark355_sumcheck;
int32_t ark355_gr1cs_sumcheck_begin_dev(ark355_ctx* ctx, const ark355_gr1cs* g, uint32_t predicate, const void* d_tables,
                                        const void* d_weight, uint32_t num_vars, ark355_sumcheck** out);
int32_t ark355_sumcheck_info(const ark355_sumcheck* sc, uint32_t* num_vars, uint32_t* arity, uint32_t* points, uint32_t* rounds_done);
int32_t ark355_sumcheck_round(ark355_ctx* ctx, ark355_sumcheck* sc, const uint8_t* challenge, uint8_t* evals_out);
int32_t ark355_sumcheck_finish(ark355_ctx* ctx, ark355_sumcheck* sc, const uint8_t* challenge, uint8_t* finals_out);
void ark355_sumcheck_free(ark355_sumcheck* sc);

/* in-place radix-2 NTT over Fr, natural order in and out (ark-poly Radix2EvaluationDomain
 * fft / ifft / coset_fft / coset_ifft).  Errors with ARK355_E_POLY_DEGREE_TOO_LARGE past the
 * field's two-adicity. */
int32_t ark355_ntt_fr(ark355_ctx* ctx, int32_t curve, uint8_t* data, uint32_t log_n, int32_t inverse,
                      int32_t coset);
int32_t ark355_ntt_fr_dev(ark355_ctx* ctx, int32_t curve, void* d_data, void* d_scratch, uint32_t log_n,
                          int32_t inverse, int32_t coset, void* stream);

/* sum_i scalars[i] * bases[i] -> affine (ark-ec VariableBaseMSM::msm_bigint semantics: canonical
 * scalars; zero scalars and infinity bases contribute nothing) */
int32_t ark355_msm_g1(ark355_ctx* ctx, int32_t curve, const uint8_t* bases, const uint8_t* scalars,
                      uint64_t n, uint8_t* out_affine);
int32_t ark355_msm_g2(ark355_ctx* ctx, int32_t curve, const uint8_t* bases, const uint8_t* scalars,
                      uint64_t n, uint8_t* out_affine);

/* device-resident MSM: bases are uploaded once into a handle, scalars live in HBM */
int32_t ark355_bases_load(ark355_ctx* ctx, int32_t curve, int32_t group /*1|2*/, const uint8_t* bases,
                          uint64_t n, ark355_bases** out);
void ark355_bases_free(ark355_bases* b);
/* scalars_mont != 0: the scalars are Montgomery Fr images and are converted on device */
int32_t ark355_msm_dev(ark355_ctx* ctx, const ark355_bases* bases, const void* d_scalars, uint64_t n,
                       int32_t scalars_mont, uint8_t* out_affine);
/* partial result as raw XYZZ (4 coordinates, Montgomery) for cross-GPU combination */
int32_t ark355_msm_dev_partial(ark355_ctx* ctx, const ark355_bases* bases, const void* d_scalars,
                               uint64_t n, int32_t scalars_mont, uint8_t* out_xyzz);
/* sum of `count` raw XYZZ partials -> affine (the local EC-add after the RCCL all-gather) */
int32_t ark355_xyzz_sum(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* partials,
                        uint64_t count, uint8_t* out_affine);

/* out[i] = scalars[i] * base (fixed base, canonical scalars) -> affine; used by
 * circuit_specific_setup (snark/src/lib.rs:43-46) to build the query vectors.
 * A scalar is read as a 256-bit little-endian integer k and need not be below r.  Fewer than 512 scalars are multiplied out by
 * double-and-add over all 256 bits, 512 or more through a table of d 2^(8 w) base (w < 32, d < 256); both compute k * base in the
 * group, which for a base in the subgroup of prime order r is (k mod r) * base: k = r and k = 2 r give the point at infinity
 * (all zero), k = 2^256 - 1 gives ((2^256 - 1) mod r) * base.  On the table route such a k can bring the running sum to plus or
 * minus the row of the last window (k = r, 2 r: minus; k = 2 d 2^248 - r with d = ceil(r / 2^248): plus); the mixed addition
 * doubles or cancels there (tests/grouplaw_cases.py).  For a base outside that subgroup (G2 takes any point of the twist, BLS12-381
 * G1 any point of the curve) the result is still k * base, which then depends on k itself and not only on k mod r.  A base at
 * infinity gives infinity for every k. */
int32_t ark355_fixed_base_mul(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* base,
                              const uint8_t* scalars, uint64_t n, uint8_t* out_affine);
/* ark355_fixed_base_mul with the scalars in device memory; scalars_mont != 0: Montgomery images, converted on the device
 * (the convention of ark355_msm_dev).  Same output bytes as ark355_fixed_base_mul on the same values. */
int32_t ark355_fixed_base_mul_dev(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* base, const void* d_scalars,
                                  uint64_t n, int32_t scalars_mont, uint8_t* out_affine);

/* ---- batch verification (SNARK::verify / verify_with_processed_vk, snark/src/lib.rs:59-80) ------
 * Checks `count` proofs of ONE verifying key at once with the random-linear-combination test
 *   prod_j e(rho_j A_j, B_j) = e((sum rho_j) alpha, beta) e(sum_i (sum_j rho_j x_ji) gamma_abc_i, gamma) e(sum rho_j C_j, delta):
 * count + 3 Miller loops and ONE final exponentiation instead of 4 count pairings.  The two multi-scalar sums run on
 * the device; the final exponentiation on the host; the curve checks, rho_j A_j and the Miller loops on host threads or on
 * the device (policy PAIRING_DEVICE, below).  public_inputs: count x (num_instance - 1)
 * Fr (Montgomery; the leading One is implicit, as in SNARK::verify); rho: count x 32 B canonical, non-zero, drawn by
 * the caller from its rng (soundness error ~ 1/|rho|); NULL is allowed for count == 1 (plain verification).
 * *ok = 1 iff every proof verifies (with overwhelming probability over rho). */
typedef struct {
  uint64_t num_instance;        /* ell = gamma_abc_g1 length */
  const uint8_t* alpha_g1;
  const uint8_t* beta_g2;
  const uint8_t* gamma_g2;
  const uint8_t* delta_g2;
  const uint8_t* gamma_abc_g1;  /* ell G1 */
} ark355_vk_desc;
int32_t ark355_verify_batch(ark355_ctx* ctx, int32_t curve, const ark355_vk_desc* vk, const ark355_proof_raw* proofs,
                            const uint8_t* public_inputs, const uint8_t* rho, uint64_t count, int32_t* ok);

/* ark-ec Pairing::multi_pairing: GT = final_exponentiation(prod_i miller_loop(P_i, Q_i)).
 * g1: n raw affine G1 images, g2: n raw affine G2 images (Montgomery, as everywhere in this header); a pair with either
 * point at infinity contributes one, n == 0 gives one.  out_gt: 12 Fq, Montgomery, in ark-ff's Fp12 memory order
 *   c0.c0.c0, c0.c0.c1, c0.c1.c0, c0.c1.c1, c0.c2.c0, c0.c2.c1, c1.c0.c0, ..., c1.c2.c1
 * over the tower Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), xi = 1 + u (BLS12-381) or
 * 9 + u (BN254).  *is_one = 1 iff GT is the identity (the pairing-product check).
 * Every point is checked against its curve equation first: one that fails gives ARK355_EINVAL and ark355_last_error
 * names the argument and the index.  Subgroup membership is NOT checked (that is ark355_points_decode's
 * ARK355_VALIDATE_FULL, as for ark355_verify_batch); a point on its curve but outside the r-torsion returns cleanly with
 * an unspecified value.
 * Policy PAIRING_DEVICE (this call and ark355_verify_batch): 0 Miller loops on host threads, 1 on the device, -1 (default)
 * on the device when the call has at least PAIRING_DEVICE_MIN pairs (count + 3 for ark355_verify_batch).  The final
 * exponentiation runs on the host, once per call. */
int32_t ark355_multi_pairing(ark355_ctx* ctx, int32_t curve, const uint8_t* g1, const uint8_t* g2, uint64_t n,
                             uint8_t* out_gt /* may be NULL */, int32_t* is_one /* may be NULL */);

/* ark-ec Pairing::pairing, elementwise or per group: groups x group_len consecutive pairs,
 *   GT_k = final_exponentiation(prod_{i in group k} miller_loop(P_i, Q_i)),
 * every GT_k byte for byte what ark355_multi_pairing returns for that group's pairs alone (group_len = 1: one pairing per
 * pair).  g1 / g2: groups * group_len raw affine images, below 2^32 in all; a pair with either point at infinity
 * contributes one.  out_gt: groups x 12 Fq in the layout of ark355_multi_pairing; is_one: groups bytes, 1 where GT_k is the
 * identity.  groups == 0 returns ARK355_OK and writes nothing.  ARK355_EINVAL: group_len == 0 or above
 * ARK355_PAIRING_GROUP_MAX (one long product is ark355_multi_pairing's), a NULL point array with pairs to read, a point
 * off its curve (ark355_last_error names g1[i] / g2[i], i the index into the flat list).  Subgroup membership is NOT checked.
 * Policy PAIRING_DEVICE as for ark355_multi_pairing, but "by size" (-1) reads PAIRING_EACH_MIN, counted in groups: on the
 * device route the final exponentiations run there too, one lane per group (the exact power (q^12 - 1) / r); the host
 * route pays one of them per group on at most 16 threads and is the slow second checker. */
#define ARK355_PAIRING_GROUP_MAX 64
int32_t ark355_pairing_groups(ark355_ctx* ctx, int32_t curve, const uint8_t* g1, const uint8_t* g2, uint64_t groups,
                              uint32_t group_len, uint8_t* out_gt /* may be NULL */, uint8_t* is_one /* may be NULL */);

/* SNARK::verify (snark/src/lib.rs:59-80) for every proof of ONE key on its own: ok[j] = 1 iff
 *   e(A_j, B_j) = e(alpha, beta) e(sum_i x_ji gamma_abc_i, gamma) e(C_j, delta),
 * the verdict of ark355_verify_batch on proof j alone with rho = NULL -- no random combination, no soundness error.
 * proofs, public_inputs as for ark355_verify_batch (num_instance == 1: no public inputs, public_inputs may be NULL); ok:
 * count bytes.  A proof with a point off its curve gets ok[j] = 0, the call still returns ARK355_OK and the other verdicts
 * are unaffected.  The key's own points are checked once: one off its curve gives ARK355_EINVAL naming the field.
 * Policy PAIRING_DEVICE / PAIRING_EACH_MIN (counted in proofs) as for ark355_pairing_groups: on the device route the curve
 * checks, the prepared inputs, the 3 count Miller loops and the count final exponentiations are kernels and only ok returns. */
int32_t ark355_verify_each(ark355_ctx* ctx, int32_t curve, const ark355_vk_desc* vk, const ark355_proof_raw* proofs,
                           const uint8_t* public_inputs, uint64_t count, uint8_t* ok);

/* ---- processed verifying key (type ProcessedVerifyingKey, SNARK::process_vk, SNARK::verify_with_processed_vk;
 * snark/src/lib.rs:36,69-80; upstream ark-groth16 PreparedVerifyingKey) -------------------------------------------------
 * A verifier holds a handful of keys and sees proofs forever: ark355_vk_process does the per-key work of ark355_verify_each
 * once and keeps the result resident, and the *_pvk entries verify against the handle.
 *   - the curve checks of the key's 4 + num_instance points (ARK355_EINVAL naming the field, as ark355_verify_each refuses them);
 *   - e(alpha, beta), the alpha_g1_beta_g2 of PreparedVerifyingKey;
 *   - gamma_abc_g1 in HBM;
 *   - the P-independent line coefficients of beta, gamma and delta (ark-ec G2Prepared), which the Miller loops against
 *     these points read instead of walking the point again for every proof.
 * A key point at infinity is legal, as it is for ark355_verify_each: its pairs contribute one.  num_instance == 0 and NULL
 * pointers are ARK355_EINVAL.  The handle belongs to the DEVICE of the creating context, not to the context: it is immutable
 * and may be used from any context of that device, from several at once, and after the creating context is destroyed; a
 * context of another device gets ARK355_EINVAL.  Free it with ark355_pvk_free once no call uses it.
 * Upstream's ProcessedVerifyingKey is serializable; the handle is NOT.  The serializable object remains the VerifyingKey it
 * was made from (process it again after loading), exactly as ark355_pk relates to ProvingKey. */
typedef struct ark355_pvk ark355_pvk;
/* SNARK::process_vk (snark/src/lib.rs:69-73) */
int32_t ark355_vk_process(ark355_ctx* ctx, int32_t curve, const ark355_vk_desc* vk, ark355_pvk** out);
void ark355_pvk_free(ark355_pvk* pvk);
/* curve id, gamma_abc_g1 length, bytes of HBM the handle holds; any pointer may be NULL */
int32_t ark355_pvk_info(const ark355_pvk* pvk, int32_t* curve, uint64_t* num_instance, uint64_t* resident_bytes);
/* PreparedVerifyingKey::alpha_g1_beta_g2: 12 Fq in the layout of ark355_multi_pairing, byte for byte what that entry
 * returns for the one pair (alpha_g1, beta_g2) */
int32_t ark355_pvk_alpha_beta(const ark355_pvk* pvk, uint8_t* out_gt);
/* ark-ec Pairing::pairing against one G2Prepared, elementwise: GT_i = e(P_i, Q) with Q the key's beta (which = 0), gamma (1)
 * or delta (2).  Each value is byte for byte what ark355_pairing_groups returns for the n pairs (P_i, Q) with group_len 1.
 * g1: n raw affine G1 images; P_i off its curve is ARK355_EINVAL naming g1[i]; P_i or Q at infinity gives one.  n == 0
 * returns ARK355_OK and writes nothing; a NULL g1 with n > 0 and which outside 0 .. 2 are ARK355_EINVAL.  Route policy as
 * for ark355_pairing_groups (PAIRING_DEVICE / PAIRING_EACH_MIN, counted in pairs); the host route walks Q again per pair. */
int32_t ark355_pvk_pairings(ark355_ctx* ctx, const ark355_pvk* pvk, int32_t which /* 0 beta, 1 gamma, 2 delta */,
                            const uint8_t* g1, uint64_t n, uint8_t* out_gt /* may be NULL */, uint8_t* is_one /* may be NULL */);
/* SNARK::verify_with_processed_vk (snark/src/lib.rs:76-80), per proof: ok[j] is ark355_verify_each's on the same key, proofs
 * and inputs, on both routes and under the same rules (a proof off its curve gets ok[j] = 0 and the call returns ARK355_OK;
 * count == 0 writes nothing; num_instance == 1 allows public_inputs == NULL).  count == 1 is verify_with_processed_vk itself.
 * Policy PAIRING_DEVICE / PAIRING_EACH_MIN as for ark355_verify_each.  On the device route only the count pairs (A_j, B_j)
 * walk a G2 point; the 2 count pairs against gamma and delta read the handle's lines. */
int32_t ark355_verify_each_pvk(ark355_ctx* ctx, const ark355_pvk* pvk, const ark355_proof_raw* proofs,
                               const uint8_t* public_inputs, uint64_t count, uint8_t* ok);
/* ark355_verify_batch with the key taken from the handle (its points were checked at process time): the same verdict. */
int32_t ark355_verify_batch_pvk(ark355_ctx* ctx, const ark355_pvk* pvk, const ark355_proof_raw* proofs,
                                const uint8_t* public_inputs, const uint8_t* rho, uint64_t count, int32_t* ok);

/* ---- proofs as wire bytes (Proof: CanonicalDeserialize, snark/src/lib.rs:32) -----------------------------------------------
 * A verifier receives proofs as ark-serialize bytes.  These entries decode them on the device, one lane per point, and a bad
 * or malleated encoding costs exactly its own proof: it is reported per proof, never as an error of the call.  The subgroup
 * test of ARK355_VALIDATE_FULL is the endomorphism test ark-bls12-381 / ark-bn254 use upstream (phi(P) = -[x^2]P on
 * BLS12-381 G1, psi(P) = [x]P on its G2, psi(P) = [6x^2]P on BN254 G2), equivalent to [r]P = O for points on the curve.
 * ARK355_EINVAL is for arguments only: a NULL pointer with a non-zero count, an unknown validate or method,
 * 3 * count >= 2^32, a handle of another device (ark355_last_error names the argument). */
/* ark-ec is_on_curve + is_in_correct_subgroup_assuming_on_curve for n raw affine images, one lane per point:
 * status[i] = 0, WIRE_NOT_ON_CURVE (2) or WIRE_NOT_IN_SUBGROUP (4); infinity is 0.  method 0: [r]P, 1: the endomorphism tests. */
int32_t ark355_points_check(ark355_ctx* ctx, int32_t curve, int32_t group, const uint8_t* raw, uint64_t n, int32_t method,
                            uint8_t* status);
/* count proofs (a || b || c each, the layout of ark355_proof_from_bytes) decoded on the device.  status[j] = 0, or
 * (k << 4) | wire status of the FIRST failing point in the order a (k=1), b (2), c (3), the wire status being 1 coordinate not
 * reduced, 2 not on the curve, 3 bad flag bits, 4 not in the subgroup; out[j] is all zero where status[j] != 0. */
int32_t ark355_proofs_from_bytes(ark355_ctx* ctx, int32_t curve, const uint8_t* in, uint64_t count, int32_t compressed,
                                 int32_t validate, ark355_proof_raw* out, uint8_t* status);
/* Proof::deserialize_with_mode + SNARK::verify_with_processed_vk per proof, without the proofs visiting the host as points:
 * ok[j] = 1 iff proof j decodes under `validate` AND verifies; status (may be NULL) as above.  public_inputs, count == 0,
 * num_instance == 1 and the route policy exactly as for ark355_verify_each_pvk (the host route decodes on host threads and
 * gives the same ok and status). */
int32_t ark355_verify_each_bytes(ark355_ctx* ctx, const ark355_pvk* pvk, const uint8_t* proofs, uint64_t count,
                                 int32_t compressed, int32_t validate, const uint8_t* public_inputs, uint8_t* ok,
                                 uint8_t* status);

/* The scalars of the Groth16 generator (circuit_specific_setup, snark/src/lib.rs:43-46; upstream
 * generate_parameters_with_qap) from the R1CS matrices in CSR and the five trapdoor elements tau, alpha, beta, gamma,
 * delta (5 x 32 B canonical): u_j(tau), v_j(tau), w_j(tau) (num_instance + num_witness each), l_j (num_witness),
 * gamma_abc_j (num_instance), h_i (N - 1) -- canonical 32-byte values ready for ark355_fixed_base_mul.  Host threads
 * only (the library's own field code); ARK355_E_POLY_DEGREE_TOO_LARGE past the field's two-adicity. */
int32_t ark355_setup_scalars(int32_t curve, uint64_t n_constraints, uint64_t num_instance, uint64_t num_witness,
                             const uint64_t* const row_ptr[3], const uint32_t* const col[3],
                             const uint8_t* const coeff[3], const uint8_t* trapdoor, uint8_t* out_u, uint8_t* out_v,
                             uint8_t* out_w, uint8_t* out_l, uint8_t* out_gamma_abc, uint8_t* out_h);

/* The Groth16 generator on the device: from the resident matrices and the trapdoor to a resident proving key, without the
 * key visiting the host unless the caller asks for it.  g1_base / g2_base: raw affine generators (must lie on their curves);
 * trapdoor as for ark355_setup_scalars, every element below r, gamma and delta non-zero.  The outputs are, byte for byte,
 * what ark355_setup_scalars + ark355_fixed_base_mul + ark355_pk_load produce from the same inputs (a zero scalar gives the
 * all-zero point).  `out` (may be NULL): host memory, caller-owned, every pointer optional (NULL = not wanted); *out_pk (may be
 * NULL) is an ordinary handle under the context's load-time policy, freed with ark355_pk_free.  At least one of the two must
 * be given.  Work nobody asked for is skipped: without out_pk a query vector whose pointer is NULL is never multiplied out,
 * and a call that wants only u, v, w runs no curve arithmetic.  ARK355_EINVAL (with a message) for NULL arguments, a trapdoor
 * element >= r, gamma or delta zero, a base off its curve; ARK355_ENOMEM from the table planner as for ark355_pk_load.
 * Sharded keys: take the host vectors and call ark355_pk_load_shard.  (Kernels: snark_amd/csrc/setup_impl.cuh.) */
typedef struct {
  uint8_t* alpha_g1;      /* 1 G1 each, raw affine */
  uint8_t* beta_g1;
  uint8_t* delta_g1;
  uint8_t* beta_g2;       /* 1 G2 each */
  uint8_t* gamma_g2;
  uint8_t* delta_g2;
  uint8_t* gamma_abc_g1;  /* ell G1 */
  uint8_t* a_query;       /* (ell+w) G1 */
  uint8_t* b_g1_query;    /* (ell+w) G1 */
  uint8_t* b_g2_query;    /* (ell+w) G2 */
  uint8_t* h_query;       /* (N-1)   G1 */
  uint8_t* l_query;       /* w       G1 */
  uint8_t* u;             /* (ell+w) canonical 32-byte scalars each: u_j(tau), v_j(tau), w_j(tau) */
  uint8_t* v;
  uint8_t* w;
} ark355_setup_out;
int32_t ark355_setup(ark355_ctx* ctx, const ark355_r1cs* r1cs, const uint8_t* g1_base, const uint8_t* g2_base,
                     const uint8_t* trapdoor, const ark355_setup_out* out, ark355_pk** out_pk);

/* ---- timings of the last prove on this context (ms, measured with HIP events) --------------- */
typedef struct {
  float total_ms;
  float h2d_ms;
  float witness_map_ms;
  float msm_h_ms;
  float msm_l_ms;
  float msm_ab_g1_ms;
  float msm_b_g2_ms;
  float finalize_ms;
} ark355_timings;
int32_t ark355_get_timings(const ark355_ctx* ctx, ark355_timings* out);

/* per-kernel HIP-event timing of the dominant kernel (bucket accumulation) of the last MSM/prove
 * on this context: sum of launch durations (ms), number of launches, points accumulated */
int32_t ark355_get_kernel_stats(const ark355_ctx* ctx, float* accumulate_ms, uint64_t* launches,
                                uint64_t* points);

#ifdef __cplusplus
}
#endif
#endif /* ARK355_H */
