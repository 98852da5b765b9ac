//! `extern "C"` image of `include/ark355.h` -- one declaration per entry point, same order, same argument lists.
//! tests/test_rust_shim.py parses both files and fails when they drift apart.
#![allow(non_camel_case_types, dead_code)]

use core::ffi::{c_char, c_void};

#[repr(C)]
pub struct ark355_ctx {
    _p: [u8; 0],
}
#[repr(C)]
pub struct ark355_pk {
    _p: [u8; 0],
}
#[repr(C)]
pub struct ark355_r1cs {
    _p: [u8; 0],
}
#[repr(C)]
pub struct ark355_gr1cs {
    _p: [u8; 0],
}
#[repr(C)]
pub struct ark355_sr1cs {
    _p: [u8; 0],
}
#[repr(C)]
pub struct ark355_comm {
    _p: [u8; 0],
}
#[repr(C)]
pub struct ark355_bases {
    _p: [u8; 0],
}
#[repr(C)]
pub struct ark355_pvk {
    _p: [u8; 0],
}
/// one sum-check run over resident tables: `ark355_gr1cs_sumcheck_begin_dev`
#[repr(C)]
pub struct ark355_sumcheck {
    _p: [u8; 0],
}

pub const ARK355_BLS12_381: i32 = 0;
pub const ARK355_BN254: i32 = 1;

pub const ARK355_OK: i32 = 0;
pub const ARK355_EINVAL: i32 = -1;
pub const ARK355_ENOMEM: i32 = -2;
pub const ARK355_EHIP: i32 = -3;
pub const ARK355_ERCCL: i32 = -4;
pub const ARK355_ENODEV: i32 = -5;
pub const ARK355_E_ASSIGNMENT_MISSING: i32 = -16;
pub const ARK355_E_UNSATISFIABLE: i32 = -17;
pub const ARK355_E_POLY_DEGREE_TOO_LARGE: i32 = -18;

pub const ARK355_COMM_ID_BYTES: usize = 128;
pub const ARK355_SHARD_WINDOW: i32 = 0;
pub const ARK355_SHARD_BUCKET_RING: i32 = 1;
/// `validate` of the wire-format entry points: Validate::No / Validate::Yes (curve + prime-order subgroup) / curve only
pub const ARK355_VALIDATE_NONE: i32 = 0;
pub const ARK355_VALIDATE_FULL: i32 = 1;
pub const ARK355_VALIDATE_CURVE: i32 = 2;
/// limits of `ark355_gr1cs_load` (ARK355_EINVAL beyond them)
pub const ARK355_GR1CS_MAX_ARITY: u32 = 16;
pub const ARK355_GR1CS_MAX_TERMS: u32 = 256;
pub const ARK355_GR1CS_MAX_FACTORS: u32 = 1024;
pub const ARK355_GR1CS_MAX_PREDICATES: u32 = 1024;
pub const ARK355_GR1CS_MAX_ROWS: u64 = 4294967295;
/// tags of a packed `Variable` (top 3 bits; payload in the low 61): `ark355_gr1cs_from_lcs`
pub const ARK355_VAR_ZERO: u64 = 0;
pub const ARK355_VAR_ONE: u64 = 1;
pub const ARK355_VAR_INSTANCE: u64 = 2;
pub const ARK355_VAR_WITNESS: u64 = 3;
pub const ARK355_VAR_LC: u64 = 4;
pub const ARK355_PAIRING_GROUP_MAX: u32 = 64;
/// most polynomials one call of the `ark355_poly_*` entries takes
pub const ARK355_POLY_MAX_COUNT: u32 = 1024;
/// most segments one call of `ark355_msm_batch_dev` takes
pub const ARK355_MSM_BATCH_MAX: u64 = 4096;
/// most evaluation points of one sum-check round: the predicate's degree as written, plus one with a weight, plus one
pub const ARK355_SUMCHECK_MAX_POINTS: u32 = 32;
/// words of the `plan` array of `ark355_diag_msm_sort`
pub const ARK355_SORT_PLAN_WORDS: usize = 8;
/// most elements one call of `ark355_diag_field_ops` takes
pub const ARK355_FIELD_OPS_MAX_N: u64 = 1 << 24;
/// fields of `ark355_diag_field_ops`
pub const ARK355_FLD_BLS_FQ: i32 = 0;
pub const ARK355_FLD_BLS_FR: i32 = 1;
pub const ARK355_FLD_BN_FQ: i32 = 2;
pub const ARK355_FLD_BN_FR: i32 = 3;
pub const ARK355_FLD_BLS_FQ2: i32 = 4;
pub const ARK355_FLD_BN_FQ2: i32 = 5;
pub const ARK355_FLD_BLS_FQ28: i32 = 6;
pub const ARK355_FLD_BN_FQ28: i32 = 7;
/// operations of `ark355_diag_field_ops`: Fq / Fr / Fq2 ...
pub const ARK355_FOP_ADD: i32 = 0;
pub const ARK355_FOP_SUB: i32 = 1;
pub const ARK355_FOP_NEG: i32 = 2;
pub const ARK355_FOP_DBL: i32 = 3;
pub const ARK355_FOP_MUL: i32 = 4;
pub const ARK355_FOP_MUL_NI: i32 = 5;
pub const ARK355_FOP_SQR: i32 = 6;
pub const ARK355_FOP_MUL2SUM: i32 = 7;
pub const ARK355_FOP_MUL_SUB: i32 = 8;
pub const ARK355_FOP_INV: i32 = 9;
pub const ARK355_FOP_TO_MONT: i32 = 10;
pub const ARK355_FOP_FROM_MONT: i32 = 11;
pub const ARK355_FOP_SQR_NI: i32 = 12;
/// ... and the radix-2^28 form of Fq (COND_SUB + log2 K; SUB / NEG + 16 K + BETA)
pub const ARK355_FOP28_FROM_FP: i32 = 32;
pub const ARK355_FOP28_TO_FP: i32 = 33;
pub const ARK355_FOP28_TO_FP_LT8: i32 = 34;
pub const ARK355_FOP28_NORM: i32 = 35;
pub const ARK355_FOP28_CANON: i32 = 36;
pub const ARK355_FOP28_IS_ZERO: i32 = 37;
pub const ARK355_FOP28_IS_ZERO_INL: i32 = 38;
pub const ARK355_FOP28_HINT: i32 = 39;
pub const ARK355_FOP28_ADD: i32 = 40;
pub const ARK355_FOP28_MUL: i32 = 41;
pub const ARK355_FOP28_SQR: i32 = 42;
pub const ARK355_FOP28_MUL2SUM: i32 = 43;
pub const ARK355_FOP28_MUL4SUM: i32 = 44;
pub const ARK355_FOP28_COND_SUB: i32 = 48;
pub const ARK355_FOP28_SUB: i32 = 256;
pub const ARK355_FOP28_NEG: i32 = 512;

#[repr(C)]
pub struct ark355_pk_desc {
    pub num_instance: u64,
    pub num_witness: u64,
    pub domain_size: u64,
    pub a_query: *const u8,
    pub b_g1_query: *const u8,
    pub b_g2_query: *const u8,
    pub h_query: *const u8,
    pub l_query: *const u8,
    pub alpha_g1: *const u8,
    pub beta_g1: *const u8,
    pub delta_g1: *const u8,
    pub beta_g2: *const u8,
    pub delta_g2: *const u8,
}

/// One predicate of `ark355_gr1cs_load`: the polynomial (sum_k term_coeff[k] * prod_{j in [term_ptr[k], term_ptr[k+1])}
/// x_{term_var[j]} ^ term_exp[j]) and its `arity` matrices in CSR.
#[repr(C)]
pub struct ark355_predicate_desc {
    pub label: *const c_char,
    pub arity: u32,
    pub n_constraints: u64,
    pub n_terms: u32,
    pub term_coeff: *const u8,
    pub term_ptr: *const u32,
    pub term_var: *const u32,
    pub term_exp: *const u32,
    pub row_ptr: *const *const u64,
    pub col: *const *const u32,
    pub coeff: *const *const u8,
}

/// One predicate of `ark355_gr1cs_from_lcs`: the polynomial as in `ark355_predicate_desc` and `argument_lcs`, column-wise
/// (`arity` arrays of `n_constraints` packed Variables).
#[repr(C)]
pub struct ark355_predicate_lcs_desc {
    pub label: *const c_char,
    pub arity: u32,
    pub n_constraints: u64,
    pub n_terms: u32,
    pub term_coeff: *const u8,
    pub term_ptr: *const u32,
    pub term_var: *const u32,
    pub term_exp: *const u32,
    pub args: *const *const u64,
}

/// A constraint system before `finalize()`: the three flat arrays of `LcMap` and the interner's pool (Montgomery Fr;
/// entries 0 and 1 are 1 and -1).  `outline`: 0 none, 1 `outline_r1cs`, 2 `outline_sr1cs`.
#[repr(C)]
pub struct ark355_lc_system_desc {
    pub num_instance: u64,
    pub num_witness: u64,
    pub n_lcs: u64,
    pub lc_offsets: *const u64,
    pub lc_vars: *const u64,
    pub lc_coeffs: *const u32,
    pub n_pool: u64,
    pub pool: *const u8,
    pub outline: i32,
}

#[repr(C)]
pub struct ark355_vk_desc {
    pub num_instance: u64,
    pub alpha_g1: *const u8,
    pub beta_g2: *const u8,
    pub gamma_g2: *const u8,
    pub delta_g2: *const u8,
    pub gamma_abc_g1: *const u8,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct ark355_proof_raw {
    pub a: [u8; 96],
    pub b: [u8; 192],
    pub c: [u8; 96],
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct ark355_timings {
    pub total_ms: f32,
    pub h2d_ms: f32,
    pub witness_map_ms: f32,
    pub msm_h_ms: f32,
    pub msm_l_ms: f32,
    pub msm_ab_g1_ms: f32,
    pub msm_b_g2_ms: f32,
    pub finalize_ms: f32,
}

/// What the measured schedule choice has seen for one (proof shape, alone | in flight) class: `ark355_sched_info`.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct ark355_sched_report {
    pub latched: i32,
    pub last: i32,
    pub samples: [u32; 4],
    pub mean_ms: [f64; 4],
}

/// Where `ark355_setup` writes what the caller wants of the key: host memory, every pointer optional (null = not wanted).
#[repr(C)]
pub struct ark355_setup_out {
    pub alpha_g1: *mut u8,
    pub beta_g1: *mut u8,
    pub delta_g1: *mut u8,
    pub beta_g2: *mut u8,
    pub gamma_g2: *mut u8,
    pub delta_g2: *mut u8,
    pub gamma_abc_g1: *mut u8,
    pub a_query: *mut u8,
    pub b_g1_query: *mut u8,
    pub b_g2_query: *mut u8,
    pub h_query: *mut u8,
    pub l_query: *mut u8,
    pub u: *mut u8,
    pub v: *mut u8,
    pub w: *mut u8,
}

extern "C" {
    pub fn ark355_ctx_create(device_id: i32, out: *mut *mut ark355_ctx) -> i32;
    pub fn ark355_ctx_destroy(ctx: *mut ark355_ctx);
    pub fn ark355_last_error(ctx: *const ark355_ctx) -> *const c_char;
    pub fn ark355_version() -> u32;
    pub fn ark355_sizes(curve: i32, what: *mut u32) -> i32;

    pub fn ark355_ctx_set_policy(ctx: *mut ark355_ctx, name: *const c_char, value: i64) -> i32;
    pub fn ark355_ctx_get_policy(ctx: *mut ark355_ctx, name: *const c_char, value: *mut i64) -> i32;
    pub fn ark355_sched_info(ctx: *const ark355_ctx, pk: *const ark355_pk, in_flight: i32, out: *mut ark355_sched_report) -> i32;
    pub fn ark355_sched_reset(ctx: *const ark355_ctx) -> i32;
    pub fn ark355_diag_streams(ctxs: *mut *mut ark355_ctx, count: u32, serialised: *mut i8) -> i32;
    pub fn ark355_diag_dispatch(ctx: *mut ark355_ctx, launches: u32, spin_us: u32, gap_us: *mut f32, lanes: *mut u32) -> i32;
    pub fn ark355_diag_mad_rate(ctx: *mut ark355_ctx, target_ms: f32, tmad_per_s: *mut f32, elapsed_ms: *mut f32) -> i32;
    pub fn ark355_diag_clocks(ctx: *mut ark355_ctx, pairs: *mut u64, capacity: u32, count: *mut u32) -> i32;
    /// Diagnostic: the sort stage of an MSM on its own (digits, histogram, scan, placement), copied back to the host.
    pub fn ark355_diag_msm_sort(
        ctx: *mut ark355_ctx,
        curve: i32,
        bases: *const ark355_bases,
        scalars: *const u8,
        n: u64,
        scalars_mont: i32,
        plan: *mut u32,
        counts: *mut u32,
        offsets: *mut u32,
        bucket_capacity: u64,
        sorted_keys: *mut u32,
        sorted_vals: *mut u32,
        entry_capacity: u64,
        total: *mut u32,
    ) -> i32;
    /// Diagnostic (test entry): one field primitive (`ARK355_FOP_*`) of field `ARK355_FLD_*` on `n` elements per operand
    /// array of raw limb words, one lane per element; `*flavour` = 1 when the kernel ran the inline-assembly multiplier.
    pub fn ark355_diag_field_ops(
        ctx: *mut ark355_ctx,
        field: i32,
        op: i32,
        operands: *const *const u32,
        operand_count: u32,
        n: u64,
        result: *mut u32,
        result_capacity: u64,
        flavour: *mut u32,
    ) -> i32;

    pub fn ark355_host_alloc(bytes: u64, out: *mut *mut c_void) -> i32;
    pub fn ark355_host_free(p: *mut c_void);

    pub fn ark355_pk_load(ctx: *mut ark355_ctx, curve: i32, desc: *const ark355_pk_desc, out: *mut *mut ark355_pk) -> i32;
    pub fn ark355_pk_free(pk: *mut ark355_pk);

    pub fn ark355_r1cs_load(
        ctx: *mut ark355_ctx,
        curve: i32,
        n_constraints: u64,
        num_instance: u64,
        num_witness: u64,
        row_ptr: *const *const u64,
        col: *const *const u32,
        coeff: *const *const u8,
        out: *mut *mut ark355_r1cs,
    ) -> i32;
    pub fn ark355_r1cs_free(r1cs: *mut ark355_r1cs);
    pub fn ark355_r1cs_domain_size(r1cs: *const ark355_r1cs) -> u64;

    pub fn ark355_prove(
        ctx: *mut ark355_ctx,
        pk: *const ark355_pk,
        r1cs: *const ark355_r1cs,
        z: *const u8,
        z_len: u64,
        r: *const u8,
        s: *const u8,
        out: *mut ark355_proof_raw,
    ) -> i32;
    pub fn ark355_prove_dev(
        ctx: *mut ark355_ctx,
        pk: *const ark355_pk,
        r1cs: *const ark355_r1cs,
        d_z: *const c_void,
        z_len: u64,
        r: *const u8,
        s: *const u8,
        out: *mut ark355_proof_raw,
    ) -> i32;
    pub fn ark355_prove_batch(
        ctx: *mut ark355_ctx,
        pk: *const ark355_pk,
        r1cs: *const ark355_r1cs,
        z: *const *const u8,
        z_len: u64,
        r: *const u8,
        s: *const u8,
        count: u64,
        inflight: u32,
        out: *mut ark355_proof_raw,
    ) -> i32;

    pub fn ark355_pk_load_shard(
        ctx: *mut ark355_ctx,
        curve: i32,
        desc: *const ark355_pk_desc,
        shard_index: u32,
        shard_count: u32,
        out: *mut *mut ark355_pk,
    ) -> i32;
    pub fn ark355_partial_size(curve: i32) -> u64;
    pub fn ark355_prove_shard(
        ctx: *mut ark355_ctx,
        pk_shard: *const ark355_pk,
        r1cs: *const ark355_r1cs,
        z: *const u8,
        z_len: u64,
        r: *const u8,
        s: *const u8,
        out_partials: *mut u8,
    ) -> i32;
    pub fn ark355_prove_combine(
        ctx: *mut ark355_ctx,
        curve: i32,
        partials: *const u8,
        count: u64,
        r: *const u8,
        s: *const u8,
        out: *mut ark355_proof_raw,
    ) -> i32;

    pub fn ark355_comm_unique_id(id: *mut u8) -> i32;
    pub fn ark355_comm_init(ctx: *mut ark355_ctx, id: *const u8, rank: i32, world: i32, out: *mut *mut ark355_comm) -> i32;
    pub fn ark355_comm_destroy(comm: *mut ark355_comm);
    pub fn ark355_prove_sharded(
        ctx: *mut ark355_ctx,
        comm: *mut ark355_comm,
        pk_shard: *const ark355_pk,
        r1cs: *const ark355_r1cs,
        z: *const u8,
        z_len: u64,
        r: *const u8,
        s: *const u8,
        mode: i32,
        out: *mut ark355_proof_raw,
    ) -> i32;
    pub fn ark355_prove_sharded_dev(
        ctx: *mut ark355_ctx,
        comm: *mut ark355_comm,
        pk_shard: *const ark355_pk,
        r1cs: *const ark355_r1cs,
        d_z: *const c_void,
        z_len: u64,
        r: *const u8,
        s: *const u8,
        mode: i32,
        out: *mut ark355_proof_raw,
    ) -> i32;

    pub fn ark355_point_size(curve: i32, group: i32, compressed: i32) -> u64;
    pub fn ark355_pk_load_bytes(
        ctx: *mut ark355_ctx,
        curve: i32,
        bytes: *const u8,
        len: u64,
        compressed: i32,
        validate: i32,
        out: *mut *mut ark355_pk,
    ) -> i32;
    pub fn ark355_pk_dims(pk: *const ark355_pk, num_instance: *mut u64, num_witness: *mut u64, domain_size: *mut u64) -> i32;
    pub fn ark355_pk_table_info(pk: *const ark355_pk, window_bits: *mut u32, windows: *mut u32, table_stride: *mut u32, table_bytes: *mut u64) -> i32;
    pub fn ark355_pk_h_eval(pk: *const ark355_pk, state: *mut i32, binds: *mut u32, bind_seconds: *mut f32) -> i32;
    pub fn ark355_hbasis_transform(ctx: *mut ark355_ctx, curve: i32, h_query: *const u8, log_n: u32, out_e: *mut u8, out_u: *mut u8) -> i32;
    pub fn ark355_hbasis_gather(ctx: *mut ark355_ctx, r1: *const ark355_r1cs, u: *const u8, out_d: *mut u8) -> i32;
    pub fn ark355_points_decode(
        ctx: *mut ark355_ctx,
        curve: i32,
        group: i32,
        input: *const u8,
        n: u64,
        compressed: i32,
        validate: i32,
        out_raw: *mut u8,
    ) -> i32;
    pub fn ark355_points_encode(
        ctx: *mut ark355_ctx,
        curve: i32,
        group: i32,
        in_raw: *const u8,
        n: u64,
        compressed: i32,
        out: *mut u8,
    ) -> i32;
    pub fn ark355_proof_to_bytes(curve: i32, proof: *const ark355_proof_raw, compressed: i32, out: *mut u8) -> i32;
    pub fn ark355_proof_from_bytes(
        curve: i32,
        input: *const u8,
        len: u64,
        compressed: i32,
        validate: i32,
        out: *mut ark355_proof_raw,
    ) -> i32;

    pub fn ark355_witness_map(ctx: *mut ark355_ctx, r1cs: *const ark355_r1cs, z: *const u8, z_len: u64, h_out: *mut u8) -> i32;
    pub fn ark355_witness_map_dist_sim(ctx: *mut ark355_ctx, r1cs: *const ark355_r1cs, z: *const u8, z_len: u64, world: u32, h_out: *mut u8) -> i32;
    pub fn ark355_is_satisfied(ctx: *mut ark355_ctx, r1cs: *const ark355_r1cs, z: *const u8, z_len: u64, first_bad: *mut i64) -> i32;
    pub fn ark355_r1cs_mat_vec(
        ctx: *mut ark355_ctx,
        r1cs: *const ark355_r1cs,
        z: *const u8,
        z_len: u64,
        az: *mut u8,
        bz: *mut u8,
        cz: *mut u8,
    ) -> i32;

    pub fn ark355_gr1cs_load(
        ctx: *mut ark355_ctx,
        curve: i32,
        num_instance: u64,
        num_witness: u64,
        preds: *const ark355_predicate_desc,
        n_preds: u32,
        out: *mut *mut ark355_gr1cs,
    ) -> i32;
    pub fn ark355_gr1cs_free(g: *mut ark355_gr1cs);
    pub fn ark355_gr1cs_num_constraints(g: *const ark355_gr1cs) -> u64;
    pub fn ark355_gr1cs_which_is_unsatisfied(
        ctx: *mut ark355_ctx,
        g: *const ark355_gr1cs,
        z: *const u8,
        z_len: u64,
        predicate: *mut i64,
        constraint: *mut i64,
    ) -> i32;
    pub fn ark355_gr1cs_mat_vec(ctx: *mut ark355_ctx, g: *const ark355_gr1cs, predicate: u32, z: *const u8, z_len: u64, out: *mut u8) -> i32;
    pub fn ark355_gr1cs_eval(ctx: *mut ark355_ctx, g: *const ark355_gr1cs, predicate: u32, z: *const u8, z_len: u64, out: *mut u8) -> i32;
    pub fn ark355_gr1cs_r1cs(ctx: *mut ark355_ctx, g: *const ark355_gr1cs, out: *mut *mut ark355_r1cs) -> i32;
    pub fn ark355_gr1cs_dims(g: *const ark355_gr1cs, num_instance: *mut u64, num_witness: *mut u64, n_preds: *mut u32) -> i32;
    pub fn ark355_gr1cs_pred_dims(g: *const ark355_gr1cs, predicate: u32, arity: *mut u32, n_constraints: *mut u64, nnz: *mut u64) -> i32;
    pub fn ark355_gr1cs_matrix(
        ctx: *mut ark355_ctx,
        g: *const ark355_gr1cs,
        predicate: u32,
        which: u32,
        row_ptr: *mut u64,
        col: *mut u32,
        coeff: *mut u8,
        entry_capacity: u64,
    ) -> i32;
    pub fn ark355_gr1cs_from_lcs(
        ctx: *mut ark355_ctx,
        curve: i32,
        system: *const ark355_lc_system_desc,
        preds: *const ark355_predicate_lcs_desc,
        n_preds: u32,
        out: *mut *mut ark355_gr1cs,
    ) -> i32;

    pub fn ark355_sr1cs_from_r1cs(ctx: *mut ark355_ctx, r1cs: *const ark355_r1cs, out: *mut *mut ark355_sr1cs) -> i32;
    pub fn ark355_sr1cs_free(s: *mut ark355_sr1cs);
    pub fn ark355_sr1cs_system(s: *const ark355_sr1cs) -> *const ark355_gr1cs;
    pub fn ark355_sr1cs_dims(
        s: *const ark355_sr1cs,
        num_instance: *mut u64,
        num_witness: *mut u64,
        num_constraints: *mut u64,
        nnz: *mut u64,
    ) -> i32;
    pub fn ark355_sr1cs_var_map(ctx: *mut ark355_ctx, s: *const ark355_sr1cs, witness_col: *mut i64, instance_col: *mut i64) -> i32;
    pub fn ark355_sr1cs_matrix(
        ctx: *mut ark355_ctx,
        s: *const ark355_sr1cs,
        which: i32,
        row_ptr: *mut u64,
        col: *mut u32,
        coeff: *mut u8,
        entry_capacity: u64,
    ) -> i32;
    pub fn ark355_sr1cs_assignment(ctx: *mut ark355_ctx, s: *const ark355_sr1cs, z: *const u8, z_len: u64, z_out: *mut u8) -> i32;
    pub fn ark355_sr1cs_assignment_dev(ctx: *mut ark355_ctx, s: *const ark355_sr1cs, d_z: *const c_void, z_len: u64, d_z_out: *mut c_void) -> i32;
    /// quotient of predicate `predicate` over N = 2^log_domain (`log_n` = 0: the smallest power of two >= max(n, 2)); see
    /// include/ark355.h for the definition of degree, D = 2^log_ext and h_len = D * N.  No HIP call; any out pointer may be null.
    pub fn ark355_gr1cs_quotient_dims(
        g: *const ark355_gr1cs,
        predicate: u32,
        log_n: u32,
        degree: *mut u64,
        log_domain: *mut u32,
        log_ext: *mut u32,
        h_len: *mut u64,
    ) -> i32;
    pub fn ark355_gr1cs_quotient(ctx: *mut ark355_ctx, g: *const ark355_gr1cs, predicate: u32, z: *const u8, z_len: u64, log_n: u32, h_out: *mut u8) -> i32;
    pub fn ark355_gr1cs_quotient_dev(
        ctx: *mut ark355_ctx,
        g: *const ark355_gr1cs,
        predicate: u32,
        d_z: *const c_void,
        z_len: u64,
        log_n: u32,
        d_h_out: *mut c_void,
    ) -> i32;

    /// column polynomials of any predicate at a point (include/ark355.h): L_i(tau) over 2^log_n points, the transposed
    /// products M_k^T y of one predicate, and the two composed; `_dev` variants read and write device memory.
    pub fn ark355_lagrange_fr(ctx: *mut ark355_ctx, curve: i32, log_n: u32, tau: *const u8, out: *mut u8) -> i32;
    pub fn ark355_lagrange_fr_dev(ctx: *mut ark355_ctx, curve: i32, log_n: u32, tau: *const u8, d_out: *mut c_void) -> i32;
    pub fn ark355_gr1cs_mat_vec_t(ctx: *mut ark355_ctx, g: *const ark355_gr1cs, predicate: u32, y: *const u8, y_len: u64, out: *mut u8) -> i32;
    pub fn ark355_gr1cs_mat_vec_t_dev(
        ctx: *mut ark355_ctx,
        g: *const ark355_gr1cs,
        predicate: u32,
        d_y: *const c_void,
        y_len: u64,
        d_out: *mut c_void,
    ) -> i32;
    pub fn ark355_gr1cs_columns_at(ctx: *mut ark355_ctx, g: *const ark355_gr1cs, predicate: u32, tau: *const u8, log_n: u32, out: *mut u8) -> i32;
    pub fn ark355_gr1cs_columns_at_dev(
        ctx: *mut ark355_ctx,
        g: *const ark355_gr1cs,
        predicate: u32,
        tau: *const u8,
        log_n: u32,
        d_out: *mut c_void,
    ) -> i32;

    // polynomial openings (snark_amd/csrc/poly_impl.cuh): evaluate, divide by X - x, combine; `count` polynomials of `len`
    // Montgomery coefficients back to back, x and the scalars canonical 32-byte little-endian integers in host memory
    pub fn ark355_poly_eval_fr(ctx: *mut ark355_ctx, curve: i32, coeffs: *const u8, len: u64, count: u64, x: *const u8, out: *mut u8) -> i32;
    pub fn ark355_poly_eval_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_coeffs: *const c_void,
        len: u64,
        count: u64,
        x: *const u8,
        d_out: *mut c_void,
    ) -> i32;
    pub fn ark355_poly_div_linear_fr(
        ctx: *mut ark355_ctx,
        curve: i32,
        coeffs: *const u8,
        len: u64,
        count: u64,
        x: *const u8,
        q_out: *mut u8,
        rem_out: *mut u8,
    ) -> i32;
    pub fn ark355_poly_div_linear_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_coeffs: *const c_void,
        len: u64,
        count: u64,
        x: *const u8,
        d_q_out: *mut c_void,
        d_rem_out: *mut c_void,
    ) -> i32;
    pub fn ark355_poly_lincomb_fr(
        ctx: *mut ark355_ctx,
        curve: i32,
        polys: *const u8,
        len: u64,
        count: u64,
        scalars: *const u8,
        out: *mut u8,
    ) -> i32;
    pub fn ark355_poly_lincomb_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_polys: *const c_void,
        len: u64,
        count: u64,
        scalars: *const u8,
        d_out: *mut c_void,
    ) -> i32;

    pub fn ark355_evals_eval_fr(
        ctx: *mut ark355_ctx,
        curve: i32,
        evals: *const u8,
        log_n: u32,
        count: u64,
        coset: i32,
        x: *const u8,
        out: *mut u8,
    ) -> i32;
    pub fn ark355_evals_eval_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_evals: *const c_void,
        log_n: u32,
        count: u64,
        coset: i32,
        x: *const u8,
        d_out: *mut c_void,
    ) -> i32;
    pub fn ark355_evals_div_linear_fr(
        ctx: *mut ark355_ctx,
        curve: i32,
        evals: *const u8,
        log_n: u32,
        count: u64,
        coset: i32,
        x: *const u8,
        q_out: *mut u8,
        rem_out: *mut u8,
    ) -> i32;
    pub fn ark355_evals_div_linear_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_evals: *const c_void,
        log_n: u32,
        count: u64,
        coset: i32,
        x: *const u8,
        d_q_out: *mut c_void,
        d_rem_out: *mut c_void,
    ) -> i32;
    pub fn ark355_gr1cs_mat_vec_dev(
        ctx: *mut ark355_ctx,
        g: *const ark355_gr1cs,
        predicate: u32,
        d_z: *const c_void,
        z_len: u64,
        log_n: u32,
        d_out: *mut c_void,
    ) -> i32;

    pub fn ark355_mle_eq_fr(ctx: *mut ark355_ctx, curve: i32, num_vars: u32, point: *const u8, out: *mut u8) -> i32;
    pub fn ark355_mle_eq_fr_dev(ctx: *mut ark355_ctx, curve: i32, num_vars: u32, point: *const u8, d_out: *mut c_void) -> i32;
    pub fn ark355_mle_fix_fr(
        ctx: *mut ark355_ctx,
        curve: i32,
        evals: *const u8,
        num_vars: u32,
        count: u64,
        point: *const u8,
        k: u32,
        out: *mut u8,
    ) -> i32;
    pub fn ark355_mle_fix_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_evals: *const c_void,
        num_vars: u32,
        count: u64,
        point: *const u8,
        k: u32,
        d_out: *mut c_void,
    ) -> i32;
    pub fn ark355_mle_eval_fr(
        ctx: *mut ark355_ctx,
        curve: i32,
        evals: *const u8,
        num_vars: u32,
        count: u64,
        point: *const u8,
        out: *mut u8,
    ) -> i32;
    pub fn ark355_mle_eval_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_evals: *const c_void,
        num_vars: u32,
        count: u64,
        point: *const u8,
        d_out: *mut c_void,
    ) -> i32;

    pub fn ark355_mle_quotients_fr(
        ctx: *mut ark355_ctx,
        curve: i32,
        evals: *const u8,
        num_vars: u32,
        count: u64,
        point: *const u8,
        q_out: *mut u8,
        rem_out: *mut u8,
    ) -> i32;
    pub fn ark355_mle_quotients_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_evals: *const c_void,
        num_vars: u32,
        count: u64,
        point: *const u8,
        d_q_out: *mut c_void,
        d_rem_out: *mut c_void,
    ) -> i32;
    pub fn ark355_mle_open_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        level_bases: *const *const ark355_bases,
        d_evals: *const c_void,
        num_vars: u32,
        point: *const u8,
        proofs_out: *mut u8,
        value_out: *mut u8,
    ) -> i32;

    pub fn ark355_msm_batch_dev(
        ctx: *mut ark355_ctx,
        bases: *const *const ark355_bases,
        d_scalars: *const *const c_void,
        n: *const u64,
        count: u64,
        scalars_mont: i32,
        out_affine: *mut u8,
    ) -> i32;

    pub fn ark355_gr1cs_sumcheck_begin_dev(
        ctx: *mut ark355_ctx,
        g: *const ark355_gr1cs,
        predicate: u32,
        d_tables: *const c_void,
        d_weight: *const c_void,
        num_vars: u32,
        out: *mut *mut ark355_sumcheck,
    ) -> i32;
    pub fn ark355_sumcheck_info(
        sc: *const ark355_sumcheck,
        num_vars: *mut u32,
        arity: *mut u32,
        points: *mut u32,
        rounds_done: *mut u32,
    ) -> i32;
    pub fn ark355_sumcheck_round(ctx: *mut ark355_ctx, sc: *mut ark355_sumcheck, challenge: *const u8, evals_out: *mut u8) -> i32;
    pub fn ark355_sumcheck_finish(ctx: *mut ark355_ctx, sc: *mut ark355_sumcheck, challenge: *const u8, finals_out: *mut u8) -> i32;
    pub fn ark355_sumcheck_free(sc: *mut ark355_sumcheck);

    pub fn ark355_ntt_fr(ctx: *mut ark355_ctx, curve: i32, data: *mut u8, log_n: u32, inverse: i32, coset: i32) -> i32;
    pub fn ark355_ntt_fr_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        d_data: *mut c_void,
        d_scratch: *mut c_void,
        log_n: u32,
        inverse: i32,
        coset: i32,
        stream: *mut c_void,
    ) -> i32;

    pub fn ark355_msm_g1(ctx: *mut ark355_ctx, curve: i32, bases: *const u8, scalars: *const u8, n: u64, out_affine: *mut u8) -> i32;
    pub fn ark355_msm_g2(ctx: *mut ark355_ctx, curve: i32, bases: *const u8, scalars: *const u8, n: u64, out_affine: *mut u8) -> i32;

    pub fn ark355_bases_load(ctx: *mut ark355_ctx, curve: i32, group: i32, bases: *const u8, n: u64, out: *mut *mut ark355_bases) -> i32;
    pub fn ark355_bases_free(b: *mut ark355_bases);
    pub fn ark355_msm_dev(
        ctx: *mut ark355_ctx,
        bases: *const ark355_bases,
        d_scalars: *const c_void,
        n: u64,
        scalars_mont: i32,
        out_affine: *mut u8,
    ) -> i32;
    pub fn ark355_msm_dev_partial(
        ctx: *mut ark355_ctx,
        bases: *const ark355_bases,
        d_scalars: *const c_void,
        n: u64,
        scalars_mont: i32,
        out_xyzz: *mut u8,
    ) -> i32;
    pub fn ark355_xyzz_sum(ctx: *mut ark355_ctx, curve: i32, group: i32, partials: *const u8, count: u64, out_affine: *mut u8) -> i32;

    pub fn ark355_fixed_base_mul(
        ctx: *mut ark355_ctx,
        curve: i32,
        group: i32,
        base: *const u8,
        scalars: *const u8,
        n: u64,
        out_affine: *mut u8,
    ) -> i32;
    pub fn ark355_fixed_base_mul_dev(
        ctx: *mut ark355_ctx,
        curve: i32,
        group: i32,
        base: *const u8,
        d_scalars: *const c_void,
        n: u64,
        scalars_mont: i32,
        out_affine: *mut u8,
    ) -> i32;

    pub fn ark355_verify_batch(
        ctx: *mut ark355_ctx,
        curve: i32,
        vk: *const ark355_vk_desc,
        proofs: *const ark355_proof_raw,
        public_inputs: *const u8,
        rho: *const u8,
        count: u64,
        ok: *mut i32,
    ) -> i32;

    /// `Pairing::multi_pairing` over raw affine images; `out_gt` (12 Fq, ark-ff `Fp12` memory order) and `is_one` may be null.
    pub fn ark355_multi_pairing(
        ctx: *mut ark355_ctx,
        curve: i32,
        g1: *const u8,
        g2: *const u8,
        n: u64,
        out_gt: *mut u8,
        is_one: *mut i32,
    ) -> i32;

    /// `Pairing::pairing` per group of `group_len` consecutive pairs; `out_gt` (groups x 12 Fq) and `is_one` (groups bytes) may be null.
    pub fn ark355_pairing_groups(
        ctx: *mut ark355_ctx,
        curve: i32,
        g1: *const u8,
        g2: *const u8,
        groups: u64,
        group_len: u32,
        out_gt: *mut u8,
        is_one: *mut u8,
    ) -> i32;

    /// `SNARK::verify` for every proof of one key on its own: `ok` receives `count` bytes.
    pub fn ark355_verify_each(
        ctx: *mut ark355_ctx,
        curve: i32,
        vk: *const ark355_vk_desc,
        proofs: *const ark355_proof_raw,
        public_inputs: *const u8,
        count: u64,
        ok: *mut u8,
    ) -> i32;

    /// `SNARK::process_vk`: the per-key work of verification, once; the handle is resident and immutable.
    pub fn ark355_vk_process(ctx: *mut ark355_ctx, curve: i32, vk: *const ark355_vk_desc, out: *mut *mut ark355_pvk) -> i32;
    pub fn ark355_pvk_free(pvk: *mut ark355_pvk);
    pub fn ark355_pvk_info(pvk: *const ark355_pvk, curve: *mut i32, num_instance: *mut u64, resident_bytes: *mut u64) -> i32;
    /// `PreparedVerifyingKey::alpha_g1_beta_g2` (12 Fq, ark-ff `Fp12` memory order)
    pub fn ark355_pvk_alpha_beta(pvk: *const ark355_pvk, out_gt: *mut u8) -> i32;
    /// `Pairing::pairing` of n G1 points against one prepared point of the key (0 beta, 1 gamma, 2 delta)
    pub fn ark355_pvk_pairings(
        ctx: *mut ark355_ctx,
        pvk: *const ark355_pvk,
        which: i32,
        g1: *const u8,
        n: u64,
        out_gt: *mut u8,
        is_one: *mut u8,
    ) -> i32;
    /// `SNARK::verify_with_processed_vk` for every proof on its own: `ok` receives `count` bytes.
    pub fn ark355_verify_each_pvk(
        ctx: *mut ark355_ctx,
        pvk: *const ark355_pvk,
        proofs: *const ark355_proof_raw,
        public_inputs: *const u8,
        count: u64,
        ok: *mut u8,
    ) -> i32;
    pub fn ark355_verify_batch_pvk(
        ctx: *mut ark355_ctx,
        pvk: *const ark355_pvk,
        proofs: *const ark355_proof_raw,
        public_inputs: *const u8,
        rho: *const u8,
        count: u64,
        ok: *mut i32,
    ) -> i32;

    /// curve + subgroup status of n raw affine images (method 0: `[r]P`, 1: the endomorphism tests)
    pub fn ark355_points_check(
        ctx: *mut ark355_ctx,
        curve: i32,
        group: i32,
        raw: *const u8,
        n: u64,
        method: i32,
        status: *mut u8,
    ) -> i32;
    /// `count` proofs decoded on the device; one status byte per proof, a bad proof is not an error of the call
    pub fn ark355_proofs_from_bytes(
        ctx: *mut ark355_ctx,
        curve: i32,
        input: *const u8,
        count: u64,
        compressed: i32,
        validate: i32,
        out: *mut ark355_proof_raw,
        status: *mut u8,
    ) -> i32;
    /// `Proof::deserialize_with_mode` + `SNARK::verify_with_processed_vk` per proof from wire bytes
    pub fn ark355_verify_each_bytes(
        ctx: *mut ark355_ctx,
        pvk: *const ark355_pvk,
        proofs: *const u8,
        count: u64,
        compressed: i32,
        validate: i32,
        public_inputs: *const u8,
        ok: *mut u8,
        status: *mut u8,
    ) -> i32;

    pub fn ark355_setup_scalars(
        curve: i32,
        n_constraints: u64,
        num_instance: u64,
        num_witness: u64,
        row_ptr: *const *const u64,
        col: *const *const u32,
        coeff: *const *const u8,
        trapdoor: *const u8,
        out_u: *mut u8,
        out_v: *mut u8,
        out_w: *mut u8,
        out_l: *mut u8,
        out_gamma_abc: *mut u8,
        out_h: *mut u8,
    ) -> i32;
    pub fn ark355_setup(
        ctx: *mut ark355_ctx,
        r1cs: *const ark355_r1cs,
        g1_base: *const u8,
        g2_base: *const u8,
        trapdoor: *const u8,
        out: *const ark355_setup_out,
        out_pk: *mut *mut ark355_pk,
    ) -> i32;

    pub fn ark355_get_timings(ctx: *const ark355_ctx, out: *mut ark355_timings) -> i32;
    pub fn ark355_get_kernel_stats(ctx: *const ark355_ctx, accumulate_ms: *mut f32, launches: *mut u64, points: *mut u64) -> i32;
}
