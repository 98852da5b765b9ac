"""ctypes binding of the C ABI declared in ``include/ark355.h``.

This is the Python-side image of the ``extern "C"`` block a Rust maintainer would write (see
INTEGRATION.md).  It is deliberately free of torch: plain pointers and sizes only.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

BLS12_381 = 0
BN254 = 1

OK = 0
EINVAL = -1
ENOMEM = -2
EHIP = -3
ERCCL = -4
ENODEV = -5
E_ASSIGNMENT_MISSING = -16
E_UNSATISFIABLE = -17
E_POLY_DEGREE_TOO_LARGE = -18
COMM_ID_BYTES = 128
SHARD_WINDOW = 0
SHARD_BUCKET_RING = 1
GR1CS_MAX_ARITY = 16
GR1CS_MAX_TERMS = 256
GR1CS_MAX_FACTORS = 1024
GR1CS_MAX_PREDICATES = 1024
GR1CS_MAX_ROWS = 4294967295
SORT_PLAN_WORDS = 8
# ark355_diag_field_ops: fields and operation codes (ARK355_FLD_* / ARK355_FOP_* / ARK355_FOP28_* of include/ark355.h)
FIELD_OPS_MAX_N = 1 << 24
FLD = {"BlsFq": 0, "BlsFr": 1, "BnFq": 2, "BnFr": 3, "BlsFq2": 4, "BnFq2": 5, "BlsFq28": 6, "BnFq28": 7}
FOP = {"add": 0, "sub": 1, "neg": 2, "dbl": 3, "mul": 4, "mul_ni": 5, "sqr": 6, "mul2sum": 7, "mul_sub": 8, "inv": 9,
       "to_mont": 10, "from_mont": 11, "sqr_ni": 12}
FOP28 = {"from_fp": 32, "to_fp": 33, "to_fp_lt8": 34, "norm": 35, "canon": 36, "is_zero_mod_p": 37, "is_zero_mod_p_inl": 38,
         "multiple_hint": 39, "add": 40, "mul": 41, "sqr": 42, "mul2sum": 43, "mul4sum": 44, "cond_sub": 48, "sub": 0x100,
         "neg": 0x200}

_ERR_NAMES = {
    EINVAL: "EINVAL", ENOMEM: "ENOMEM", EHIP: "EHIP", ERCCL: "ERCCL", ENODEV: "ENODEV",
    E_ASSIGNMENT_MISSING: "AssignmentMissing", E_UNSATISFIABLE: "Unsatisfiable",
    E_POLY_DEGREE_TOO_LARGE: "PolynomialDegreeTooLarge",
}

# every symbol include/ark355.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "ark355_ctx_create", "ark355_ctx_destroy", "ark355_last_error", "ark355_version", "ark355_sizes",
    "ark355_host_alloc", "ark355_host_free",
    "ark355_pk_load", "ark355_pk_free", "ark355_r1cs_load", "ark355_r1cs_free",
    "ark355_r1cs_domain_size", "ark355_prove", "ark355_prove_dev", "ark355_witness_map", "ark355_witness_map_dist_sim",
    "ark355_is_satisfied", "ark355_r1cs_mat_vec",
    "ark355_gr1cs_load", "ark355_gr1cs_free", "ark355_gr1cs_num_constraints", "ark355_gr1cs_which_is_unsatisfied",
    "ark355_gr1cs_mat_vec", "ark355_gr1cs_eval", "ark355_gr1cs_r1cs",
    "ark355_gr1cs_dims", "ark355_gr1cs_pred_dims", "ark355_gr1cs_matrix", "ark355_gr1cs_from_lcs",
    "ark355_sr1cs_from_r1cs", "ark355_sr1cs_free", "ark355_sr1cs_system", "ark355_sr1cs_dims", "ark355_sr1cs_var_map",
    "ark355_sr1cs_matrix", "ark355_sr1cs_assignment", "ark355_sr1cs_assignment_dev",
    "ark355_gr1cs_quotient_dims", "ark355_gr1cs_quotient", "ark355_gr1cs_quotient_dev",
    "ark355_lagrange_fr", "ark355_lagrange_fr_dev", "ark355_gr1cs_mat_vec_t", "ark355_gr1cs_mat_vec_t_dev",
    "ark355_gr1cs_columns_at", "ark355_gr1cs_columns_at_dev",
    "ark355_poly_eval_fr", "ark355_poly_eval_fr_dev", "ark355_poly_div_linear_fr", "ark355_poly_div_linear_fr_dev",
    "ark355_poly_lincomb_fr", "ark355_poly_lincomb_fr_dev",
    "ark355_evals_eval_fr", "ark355_evals_eval_fr_dev", "ark355_evals_div_linear_fr", "ark355_evals_div_linear_fr_dev",
    "ark355_gr1cs_mat_vec_dev",
    "ark355_mle_eq_fr", "ark355_mle_eq_fr_dev", "ark355_mle_fix_fr", "ark355_mle_fix_fr_dev", "ark355_mle_eval_fr", "ark355_mle_eval_fr_dev",
    "ark355_mle_quotients_fr", "ark355_mle_quotients_fr_dev", "ark355_mle_open_dev",
    "ark355_gr1cs_sumcheck_begin_dev", "ark355_sumcheck_info", "ark355_sumcheck_round", "ark355_sumcheck_finish", "ark355_sumcheck_free",
    "ark355_ntt_fr", "ark355_ntt_fr_dev",
    "ark355_msm_g1", "ark355_msm_g2", "ark355_bases_load", "ark355_bases_free", "ark355_msm_dev", "ark355_msm_batch_dev",
    "ark355_msm_dev_partial", "ark355_xyzz_sum", "ark355_fixed_base_mul", "ark355_fixed_base_mul_dev", "ark355_get_timings",
    "ark355_get_kernel_stats", "ark355_pk_load_shard", "ark355_partial_size", "ark355_prove_shard",
    "ark355_prove_combine", "ark355_prove_batch", "ark355_comm_unique_id", "ark355_comm_init", "ark355_comm_destroy",
    "ark355_prove_sharded", "ark355_prove_sharded_dev", "ark355_point_size", "ark355_pk_load_bytes", "ark355_pk_dims",
    "ark355_pk_table_info", "ark355_pk_h_eval", "ark355_hbasis_transform", "ark355_hbasis_gather",
    "ark355_points_decode", "ark355_points_encode", "ark355_proof_to_bytes", "ark355_proof_from_bytes",
    "ark355_setup_scalars", "ark355_setup", "ark355_verify_batch", "ark355_multi_pairing", "ark355_pairing_groups", "ark355_verify_each",
    "ark355_vk_process", "ark355_pvk_free", "ark355_pvk_info", "ark355_pvk_alpha_beta", "ark355_pvk_pairings",
    "ark355_verify_each_pvk", "ark355_verify_batch_pvk",
    "ark355_points_check", "ark355_proofs_from_bytes", "ark355_verify_each_bytes",
    "ark355_ctx_set_policy", "ark355_ctx_get_policy", "ark355_sched_info", "ark355_sched_reset", "ark355_diag_streams", "ark355_diag_dispatch",
    "ark355_diag_mad_rate", "ark355_diag_clocks", "ark355_diag_msm_sort", "ark355_diag_field_ops",
]

SCHED_NAMES = {-1: "auto", 0: "one_stream", 1: "pipeline", 2: "pipeline_sync", 3: "one_stream_spin"}


class Ark355Error(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__("%s (%d)%s" % (_ERR_NAMES.get(code, "error"), code, (": " + msg) if msg else ""))


class PkDesc(C.Structure):
    _fields_ = [
        ("num_instance", C.c_uint64), ("num_witness", C.c_uint64), ("domain_size", C.c_uint64),
        ("a_query", C.c_void_p), ("b_g1_query", C.c_void_p), ("b_g2_query", C.c_void_p),
        ("h_query", C.c_void_p), ("l_query", C.c_void_p),
        ("alpha_g1", C.c_void_p), ("beta_g1", C.c_void_p), ("delta_g1", C.c_void_p),
        ("beta_g2", C.c_void_p), ("delta_g2", C.c_void_p),
    ]


class VkDesc(C.Structure):
    _fields_ = [("num_instance", C.c_uint64), ("alpha_g1", C.c_void_p), ("beta_g2", C.c_void_p), ("gamma_g2", C.c_void_p),
                ("delta_g2", C.c_void_p), ("gamma_abc_g1", C.c_void_p)]


class PredicateDesc(C.Structure):
    _fields_ = [("label", C.c_char_p), ("arity", C.c_uint32), ("n_constraints", C.c_uint64), ("n_terms", C.c_uint32),
                ("term_coeff", C.c_void_p), ("term_ptr", C.c_void_p), ("term_var", C.c_void_p), ("term_exp", C.c_void_p),
                ("row_ptr", C.c_void_p), ("col", C.c_void_p), ("coeff", C.c_void_p)]


class PredicateLcsDesc(C.Structure):
    _fields_ = [("label", C.c_char_p), ("arity", C.c_uint32), ("n_constraints", C.c_uint64), ("n_terms", C.c_uint32),
                ("term_coeff", C.c_void_p), ("term_ptr", C.c_void_p), ("term_var", C.c_void_p), ("term_exp", C.c_void_p),
                ("args", C.c_void_p)]


class LcSystemDesc(C.Structure):
    _fields_ = [("num_instance", C.c_uint64), ("num_witness", C.c_uint64), ("n_lcs", C.c_uint64), ("lc_offsets", C.c_void_p),
                ("lc_vars", C.c_void_p), ("lc_coeffs", C.c_void_p), ("n_pool", C.c_uint64), ("pool", C.c_void_p),
                ("outline", C.c_int32)]


# tags of a packed Variable (utils/variable.rs:4-14): tag << 61 | payload
VAR_ZERO, VAR_ONE, VAR_INSTANCE, VAR_WITNESS, VAR_LC = 0, 1, 2, 3, 4
VAR_TAG_SHIFT = 61

SETUP_OUT_FIELDS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "a_query",
                    "b_g1_query", "b_g2_query", "h_query", "l_query", "u", "v", "w")


class SetupOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SETUP_OUT_FIELDS]


class ProofRaw(C.Structure):
    _fields_ = [("a", C.c_uint8 * 96), ("b", C.c_uint8 * 192), ("c", C.c_uint8 * 96)]


class SchedReport(C.Structure):
    _fields_ = [("latched", C.c_int32), ("last", C.c_int32), ("samples", C.c_uint32 * 4), ("mean_ms", C.c_double * 4)]


class Timings(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "total_ms", "h2d_ms", "witness_map_ms", "msm_h_ms", "msm_l_ms", "msm_ab_g1_ms", "msm_b_g2_ms",
        "finalize_ms")]


def _buf(b):
    """bytes / bytearray / numpy array -> (ctypes pointer, keepalive)."""
    if b is None:
        return None, None
    if isinstance(b, np.ndarray):
        a = np.ascontiguousarray(b)
        return a.ctypes.data_as(C.c_void_p), a
    if isinstance(b, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, bytearray) else np.frombuffer(b, dtype=np.uint8)
        return a.ctypes.data_as(C.c_void_p), a
    raise TypeError(type(b))


class Lib:
    """Loaded libark355 with typed signatures and thin call helpers."""

    def __init__(self, path: str):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path = path
        self.dll = C.CDLL(path)          # RTLD_LOCAL: the emulator test build exports the same symbol names
        d = self.dll
        vp, u64, u32, i32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64
        P = C.POINTER
        d.ark355_ctx_create.argtypes = [i32, P(vp)]
        d.ark355_ctx_destroy.argtypes = [vp]
        d.ark355_ctx_destroy.restype = None
        d.ark355_last_error.argtypes = [vp]
        d.ark355_last_error.restype = C.c_char_p
        d.ark355_version.restype = u32
        d.ark355_sizes.argtypes = [i32, P(u32 * 4)]
        d.ark355_host_alloc.argtypes = [u64, P(vp)]
        d.ark355_host_free.argtypes = [vp]
        d.ark355_host_free.restype = None
        d.ark355_pk_load.argtypes = [vp, i32, P(PkDesc), P(vp)]
        d.ark355_pk_free.argtypes = [vp]
        d.ark355_pk_free.restype = None
        d.ark355_r1cs_load.argtypes = [vp, i32, u64, u64, u64, P(vp * 3), P(vp * 3), P(vp * 3), P(vp)]
        d.ark355_r1cs_free.argtypes = [vp]
        d.ark355_r1cs_free.restype = None
        d.ark355_r1cs_domain_size.argtypes = [vp]
        d.ark355_r1cs_domain_size.restype = u64
        d.ark355_prove.argtypes = [vp, vp, vp, vp, u64, vp, vp, P(ProofRaw)]
        d.ark355_prove_dev.argtypes = [vp, vp, vp, vp, u64, vp, vp, P(ProofRaw)]
        d.ark355_witness_map.argtypes = [vp, vp, vp, u64, vp]
        d.ark355_witness_map_dist_sim.argtypes = [vp, vp, vp, u64, C.c_uint32, vp]
        d.ark355_is_satisfied.argtypes = [vp, vp, vp, u64, P(i64)]
        d.ark355_r1cs_mat_vec.argtypes = [vp, vp, vp, u64, vp, vp, vp]
        d.ark355_gr1cs_load.argtypes = [vp, i32, u64, u64, P(PredicateDesc), u32, P(vp)]
        d.ark355_gr1cs_free.argtypes = [vp]
        d.ark355_gr1cs_free.restype = None
        d.ark355_gr1cs_num_constraints.argtypes = [vp]
        d.ark355_gr1cs_num_constraints.restype = u64
        d.ark355_gr1cs_which_is_unsatisfied.argtypes = [vp, vp, vp, u64, P(i64), P(i64)]
        d.ark355_gr1cs_mat_vec.argtypes = [vp, vp, u32, vp, u64, vp]
        d.ark355_gr1cs_eval.argtypes = [vp, vp, u32, vp, u64, vp]
        d.ark355_gr1cs_r1cs.argtypes = [vp, vp, P(vp)]
        d.ark355_gr1cs_dims.argtypes = [vp, P(u64), P(u64), P(u32)]
        d.ark355_gr1cs_pred_dims.argtypes = [vp, u32, P(u32), P(u64), vp]
        d.ark355_gr1cs_matrix.argtypes = [vp, vp, u32, u32, vp, vp, vp, u64]
        d.ark355_gr1cs_from_lcs.argtypes = [vp, i32, P(LcSystemDesc), P(PredicateLcsDesc), u32, P(vp)]
        d.ark355_sr1cs_from_r1cs.argtypes = [vp, vp, P(vp)]
        d.ark355_sr1cs_free.argtypes = [vp]
        d.ark355_sr1cs_free.restype = None
        d.ark355_sr1cs_system.argtypes = [vp]
        d.ark355_sr1cs_system.restype = vp
        d.ark355_sr1cs_dims.argtypes = [vp, P(u64), P(u64), P(u64), P(u64 * 2)]
        d.ark355_sr1cs_var_map.argtypes = [vp, vp, vp, vp]
        d.ark355_sr1cs_matrix.argtypes = [vp, vp, i32, vp, vp, vp, u64]
        d.ark355_sr1cs_assignment.argtypes = [vp, vp, vp, u64, vp]
        d.ark355_sr1cs_assignment_dev.argtypes = [vp, vp, vp, u64, vp]
        d.ark355_gr1cs_quotient_dims.argtypes = [vp, u32, u32, P(u64), P(u32), P(u32), P(u64)]
        d.ark355_gr1cs_quotient.argtypes = [vp, vp, u32, vp, u64, u32, vp]
        d.ark355_gr1cs_quotient_dev.argtypes = [vp, vp, u32, vp, u64, u32, vp]
        d.ark355_lagrange_fr.argtypes = [vp, i32, u32, vp, vp]
        d.ark355_lagrange_fr_dev.argtypes = [vp, i32, u32, vp, vp]
        d.ark355_gr1cs_mat_vec_t.argtypes = [vp, vp, u32, vp, u64, vp]
        d.ark355_gr1cs_mat_vec_t_dev.argtypes = [vp, vp, u32, vp, u64, vp]
        d.ark355_gr1cs_columns_at.argtypes = [vp, vp, u32, vp, u32, vp]
        d.ark355_gr1cs_columns_at_dev.argtypes = [vp, vp, u32, vp, u32, vp]
        d.ark355_poly_eval_fr.argtypes = [vp, i32, vp, u64, u64, vp, vp]
        d.ark355_poly_eval_fr_dev.argtypes = [vp, i32, vp, u64, u64, vp, vp]
        d.ark355_poly_div_linear_fr.argtypes = [vp, i32, vp, u64, u64, vp, vp, vp]
        d.ark355_poly_div_linear_fr_dev.argtypes = [vp, i32, vp, u64, u64, vp, vp, vp]
        d.ark355_poly_lincomb_fr.argtypes = [vp, i32, vp, u64, u64, vp, vp]
        d.ark355_poly_lincomb_fr_dev.argtypes = [vp, i32, vp, u64, u64, vp, vp]
        d.ark355_evals_eval_fr.argtypes = [vp, i32, vp, u32, u64, i32, vp, vp]
        d.ark355_evals_eval_fr_dev.argtypes = [vp, i32, vp, u32, u64, i32, vp, vp]
        d.ark355_evals_div_linear_fr.argtypes = [vp, i32, vp, u32, u64, i32, vp, vp, vp]
        d.ark355_evals_div_linear_fr_dev.argtypes = [vp, i32, vp, u32, u64, i32, vp, vp, vp]
        d.ark355_gr1cs_mat_vec_dev.argtypes = [vp, vp, u32, vp, u64, u32, vp]
        d.ark355_mle_eq_fr.argtypes = [vp, i32, u32, vp, vp]
        d.ark355_mle_eq_fr_dev.argtypes = [vp, i32, u32, vp, vp]
        d.ark355_mle_fix_fr.argtypes = [vp, i32, vp, u32, u64, vp, u32, vp]
        d.ark355_mle_fix_fr_dev.argtypes = [vp, i32, vp, u32, u64, vp, u32, vp]
        d.ark355_mle_eval_fr.argtypes = [vp, i32, vp, u32, u64, vp, vp]
        d.ark355_mle_eval_fr_dev.argtypes = [vp, i32, vp, u32, u64, vp, vp]
        d.ark355_mle_quotients_fr.argtypes = [vp, i32, vp, u32, u64, vp, vp, vp]
        d.ark355_mle_quotients_fr_dev.argtypes = [vp, i32, vp, u32, u64, vp, vp, vp]
        d.ark355_mle_open_dev.argtypes = [vp, i32, vp, vp, u32, vp, vp, vp]
        d.ark355_gr1cs_sumcheck_begin_dev.argtypes = [vp, vp, u32, vp, vp, u32, P(vp)]
        d.ark355_sumcheck_info.argtypes = [vp, P(u32), P(u32), P(u32), P(u32)]
        d.ark355_sumcheck_round.argtypes = [vp, vp, vp, vp]
        d.ark355_sumcheck_finish.argtypes = [vp, vp, vp, vp]
        d.ark355_sumcheck_free.argtypes = [vp]
        d.ark355_sumcheck_free.restype = None
        d.ark355_ntt_fr.argtypes = [vp, i32, vp, u32, i32, i32]
        d.ark355_ntt_fr_dev.argtypes = [vp, i32, vp, vp, u32, i32, i32, vp]
        d.ark355_msm_g1.argtypes = [vp, i32, vp, vp, u64, vp]
        d.ark355_msm_g2.argtypes = [vp, i32, vp, vp, u64, vp]
        d.ark355_bases_load.argtypes = [vp, i32, i32, vp, u64, P(vp)]
        d.ark355_bases_free.argtypes = [vp]
        d.ark355_bases_free.restype = None
        d.ark355_msm_dev.argtypes = [vp, vp, vp, u64, i32, vp]
        d.ark355_msm_dev_partial.argtypes = [vp, vp, vp, u64, i32, vp]
        d.ark355_msm_batch_dev.argtypes = [vp, vp, vp, vp, u64, i32, vp]
        d.ark355_xyzz_sum.argtypes = [vp, i32, i32, vp, u64, vp]
        d.ark355_fixed_base_mul.argtypes = [vp, i32, i32, vp, vp, u64, vp]
        d.ark355_fixed_base_mul_dev.argtypes = [vp, i32, i32, vp, vp, u64, i32, vp]
        d.ark355_pk_load_shard.argtypes = [vp, i32, P(PkDesc), u32, u32, P(vp)]
        d.ark355_partial_size.argtypes = [i32]
        d.ark355_partial_size.restype = u64
        d.ark355_prove_shard.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp]
        d.ark355_prove_combine.argtypes = [vp, i32, vp, u64, vp, vp, P(ProofRaw)]
        d.ark355_prove_batch.argtypes = [vp, vp, vp, vp, u64, vp, vp, u64, u32, vp]
        d.ark355_comm_unique_id.argtypes = [vp]
        d.ark355_comm_init.argtypes = [vp, vp, i32, i32, P(vp)]
        d.ark355_comm_destroy.argtypes = [vp]
        d.ark355_comm_destroy.restype = None
        d.ark355_prove_sharded.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, i32, P(ProofRaw)]
        d.ark355_prove_sharded_dev.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, i32, P(ProofRaw)]
        d.ark355_point_size.argtypes = [i32, i32, i32]
        d.ark355_point_size.restype = u64
        d.ark355_pk_load_bytes.argtypes = [vp, i32, vp, u64, i32, i32, P(vp)]
        d.ark355_pk_dims.argtypes = [vp, P(u64), P(u64), P(u64)]
        d.ark355_pk_table_info.argtypes = [vp, P(C.c_uint32), P(C.c_uint32), P(C.c_uint32), P(u64)]
        d.ark355_pk_h_eval.argtypes = [vp, P(i32), P(C.c_uint32), P(C.c_float)]
        d.ark355_hbasis_transform.argtypes = [vp, i32, vp, C.c_uint32, vp, vp]
        d.ark355_hbasis_gather.argtypes = [vp, vp, vp, vp]
        d.ark355_points_decode.argtypes = [vp, i32, i32, vp, u64, i32, i32, vp]
        d.ark355_points_encode.argtypes = [vp, i32, i32, vp, u64, i32, vp]
        d.ark355_proof_to_bytes.argtypes = [i32, P(ProofRaw), i32, vp]
        d.ark355_proof_from_bytes.argtypes = [i32, vp, u64, i32, i32, P(ProofRaw)]
        d.ark355_setup_scalars.argtypes = [i32, u64, u64, u64, P(vp * 3), P(vp * 3), P(vp * 3), vp, vp, vp, vp, vp, vp, vp]
        d.ark355_setup.argtypes = [vp, vp, vp, vp, vp, P(SetupOut), P(vp)]
        d.ark355_verify_batch.argtypes = [vp, i32, P(VkDesc), vp, vp, vp, u64, P(i32)]
        d.ark355_multi_pairing.argtypes = [vp, i32, vp, vp, u64, vp, P(i32)]
        d.ark355_pairing_groups.argtypes = [vp, i32, vp, vp, u64, C.c_uint32, vp, vp]
        d.ark355_verify_each.argtypes = [vp, i32, P(VkDesc), vp, vp, u64, vp]
        d.ark355_vk_process.argtypes = [vp, i32, P(VkDesc), P(vp)]
        d.ark355_pvk_free.argtypes = [vp]
        d.ark355_pvk_free.restype = None
        d.ark355_pvk_info.argtypes = [vp, P(i32), P(u64), P(u64)]
        d.ark355_pvk_alpha_beta.argtypes = [vp, vp]
        d.ark355_pvk_pairings.argtypes = [vp, vp, i32, vp, u64, vp, vp]
        d.ark355_verify_each_pvk.argtypes = [vp, vp, vp, vp, u64, vp]
        d.ark355_points_check.argtypes = [vp, i32, i32, vp, u64, i32, vp]
        d.ark355_proofs_from_bytes.argtypes = [vp, i32, vp, u64, i32, i32, vp, vp]
        d.ark355_verify_each_bytes.argtypes = [vp, vp, vp, u64, i32, i32, vp, vp, vp]
        d.ark355_verify_batch_pvk.argtypes = [vp, vp, vp, vp, vp, u64, P(i32)]
        d.ark355_ctx_set_policy.argtypes = [vp, C.c_char_p, i64]
        d.ark355_ctx_get_policy.argtypes = [vp, C.c_char_p, P(i64)]
        d.ark355_sched_info.argtypes = [vp, vp, i32, P(SchedReport)]
        d.ark355_sched_reset.argtypes = [vp]
        d.ark355_diag_streams.argtypes = [vp, u32, vp]
        d.ark355_diag_dispatch.argtypes = [vp, u32, u32, P(C.c_float), P(u32)]
        d.ark355_diag_mad_rate.argtypes = [vp, C.c_float, P(C.c_float), P(C.c_float)]
        d.ark355_diag_clocks.argtypes = [vp, P(u64), u32, P(u32)]
        d.ark355_diag_msm_sort.argtypes = [vp, i32, vp, vp, u64, i32, P(u32 * SORT_PLAN_WORDS), vp, vp, u64, vp, vp, u64, P(u32)]
        d.ark355_diag_field_ops.argtypes = [vp, i32, i32, P(vp), u32, u64, vp, u64, P(u32)]
        d.ark355_get_timings.argtypes = [vp, P(Timings)]
        d.ark355_get_kernel_stats.argtypes = [vp, P(C.c_float), P(u64), P(u64)]
        for name in SYMBOLS:
            fn = getattr(d, name)
            if fn.restype is C.c_int:      # default: make every status-returning call int32
                fn.restype = i32

    # ---- runtime policy (include/ark355.h "runtime policy") ------------------------------------------
    def ctx_set_policy(self, ctx, name, value):
        self.check(ctx, self.dll.ark355_ctx_set_policy(ctx, name.encode(), int(value)))

    def ctx_get_policy(self, ctx, name):
        v = C.c_int64()
        self.check(ctx, self.dll.ark355_ctx_get_policy(ctx, name.encode(), C.byref(v)))
        return int(v.value)

    def policy(self, ctx, **kw):
        """context manager: set policy values on `ctx`, restore the previous ones on exit"""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = {k: self.ctx_get_policy(ctx, k) for k in kw}
            try:
                for k, v in kw.items():
                    self.ctx_set_policy(ctx, k, v)
                yield
            finally:
                for k, v in old.items():
                    self.ctx_set_policy(ctx, k, v)
        return cm()

    def sched_info(self, ctx, pk, in_flight):
        r = SchedReport()
        self.check(ctx, self.dll.ark355_sched_info(ctx, pk, 1 if in_flight else 0, C.byref(r)))
        return {"latched": SCHED_NAMES.get(r.latched, str(r.latched)), "last": SCHED_NAMES.get(r.last, str(r.last)),
                "samples": {SCHED_NAMES[i]: int(r.samples[i]) for i in range(4) if r.samples[i]},
                "mean_ms": {SCHED_NAMES[i]: round(float(r.mean_ms[i]), 3) for i in range(4) if r.samples[i]}}

    def diag_streams(self, ctxs):
        """ark355_diag_streams: rows of the serialisation matrix over [ctx streams..., sW, sS, sR of ctxs[0]]"""
        n = len(ctxs) + 3
        arr = (C.c_void_p * len(ctxs))(*ctxs)
        out = (C.c_int8 * (n * n))()
        self.check(ctxs[0], self.dll.ark355_diag_streams(arr, len(ctxs), out))
        return [[int(out[i * n + j]) for j in range(n)] for i in range(n)]

    def diag_dispatch(self, ctx, launches=200, spin_us=20):
        gap, lanes = C.c_float(0), C.c_uint32(0)
        self.check(ctx, self.dll.ark355_diag_dispatch(ctx, launches, spin_us, C.byref(gap), C.byref(lanes)))
        return {"gap_us": round(float(gap.value), 2), "launches": launches, "spin_us": spin_us, "lanes": int(lanes.value)}

    def diag_mad_rate(self, ctx, target_ms=20.0):
        """T (10^12) v_mad_u64_u32 per second this box issues right now at the accumulation kernels' occupancy (< 0: emulator)."""
        rate, ms = C.c_float(0), C.c_float(0)
        self.check(ctx, self.dll.ark355_diag_mad_rate(ctx, float(target_ms), C.byref(rate), C.byref(ms)))
        return {"tmad_per_s": float(rate.value), "elapsed_ms": float(ms.value)}

    def diag_clocks(self, ctx):
        """{slot: (shader-clock cycles, ticks of the constant 100 MHz reference)} read on the GPU, one pair per compute unit."""
        cap = 1024
        buf = (C.c_uint64 * (2 * cap))()
        cnt = C.c_uint32(0)
        self.check(ctx, self.dll.ark355_diag_clocks(ctx, buf, cap, C.byref(cnt)))
        return {i: (int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(int(cnt.value)) if buf[2 * i + 1]}

    def diag_msm_sort(self, ctx, curve, scalars, n, mont=0, bases=None, arrays=True):
        """ark355_diag_msm_sort: the sort stage of an MSM over `n` host scalars (32 bytes each; Montgomery images with mont=1),
        planned without tables (bases=None) or for the window tables of a bases_load handle.  Returns the plan, `total` and --
        unless arrays=False -- counts / offsets (one word per bucket) and sorted_keys / sorted_vals (total words) as numpy
        arrays.  Two calls: the first, without arrays, sizes the buffers of the second."""
        sp, keep = _buf(scalars)
        plan = (C.c_uint32 * SORT_PLAN_WORDS)()
        total = C.c_uint32(0)
        self.check(ctx, self.dll.ark355_diag_msm_sort(ctx, curve, bases, sp, n, int(mont), C.byref(plan), None, None, 0, None, None, 0,
                                                      C.byref(total)))
        names = ("c", "windows", "wstride", "key_windows", "total_buckets", "negate_high", "row_stride", "one_pass")
        out = dict(zip(names, (int(v) for v in plan)))
        out["total"] = int(total.value)
        if not arrays:
            return out
        nb, ne = out["total_buckets"], out["total"]
        counts, offsets = np.empty(nb, dtype=np.uint32), np.empty(nb, dtype=np.uint32)
        keys, vals = np.empty(max(ne, 1), dtype=np.uint32), np.empty(max(ne, 1), dtype=np.uint32)
        plan2 = (C.c_uint32 * SORT_PLAN_WORDS)()
        self.check(ctx, self.dll.ark355_diag_msm_sort(ctx, curve, bases, sp, n, int(mont), C.byref(plan2), counts.ctypes.data, offsets.ctypes.data,
                                                      nb, keys.ctypes.data, vals.ctypes.data, ne, C.byref(total)))
        assert list(plan2) == list(plan) and int(total.value) == ne
        out.update(counts=counts, offsets=offsets, sorted_keys=keys[:ne], sorted_vals=vals[:ne])
        return out

    def diag_field_ops(self, ctx, field, op, operands, n, out_words):
        """ark355_diag_field_ops: one field primitive (FOP_* / FOP28_*) of field FLD_* on `n` elements per operand, one lane per
        element.  operands: numpy uint32 arrays of n x words raw limb words each; out_words: words per result element.  Returns
        (result as an (n, out_words) uint32 array, flavour word: 1 when the kernel ran the inline-assembly multiplier)."""
        ops = [np.ascontiguousarray(o, dtype=np.uint32) for o in operands]
        ptrs = (C.c_void_p * max(len(ops), 1))(*[o.ctypes.data for o in ops])
        res = np.zeros((max(n, 1), out_words), dtype=np.uint32)
        flavour = C.c_uint32(0xFFFFFFFF)
        self.check(ctx, self.dll.ark355_diag_field_ops(ctx, int(field), int(op), ptrs, len(ops), n, res.ctypes.data, n * out_words,
                                                       C.byref(flavour)))
        return res[:n], int(flavour.value)

    @staticmethod
    def diag_clocks_delta(c0, c1):
        """Two diag_clocks readings -> (median gfx clock in MHz over the compute units present in both, elapsed ms, units used)."""
        ratios, ticks = [], []
        for k, (a0, r0) in c0.items():
            if k in c1:
                a1, r1 = c1[k]
                if a1 > a0 and r1 > r0:
                    ratios.append((a1 - a0) / (r1 - r0) * 100.0)
                    ticks.append(r1 - r0)
        if not ratios:
            return None, None, 0
        ratios.sort()
        ticks.sort()
        return ratios[len(ratios) // 2], ticks[len(ticks) // 2] / 1e5, len(ratios)

    def sched_reset(self, ctx):
        self.check(ctx, self.dll.ark355_sched_reset(ctx))

    # ---- helpers ---------------------------------------------------------------------------------
    def check(self, ctx, rc):
        if rc != OK:
            msg = ""
            if ctx:
                m = self.dll.ark355_last_error(ctx)
                msg = m.decode() if m else ""
            raise Ark355Error(rc, msg)

    def sizes(self, curve):
        out = (C.c_uint32 * 4)()
        self.check(None, self.dll.ark355_sizes(curve, C.byref(out)))
        return {"fr": out[0], "fq": out[1], "g1": out[2], "g2": out[3]}

    def ctx_create(self, device=0):
        h = C.c_void_p()
        rc = self.dll.ark355_ctx_create(device, C.byref(h))
        if rc != OK:
            raise Ark355Error(rc, "ark355_ctx_create")
        return h

    def ctx_destroy(self, ctx):
        self.dll.ark355_ctx_destroy(ctx)

    def pk_load(self, ctx, curve, ell, w, N, a_query, b_g1_query, b_g2_query, h_query, l_query,
                alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, shard=None):
        keep = []
        d = PkDesc()
        d.num_instance, d.num_witness, d.domain_size = ell, w, N
        for name, val in (("a_query", a_query), ("b_g1_query", b_g1_query), ("b_g2_query", b_g2_query),
                          ("h_query", h_query), ("l_query", l_query), ("alpha_g1", alpha_g1),
                          ("beta_g1", beta_g1), ("delta_g1", delta_g1), ("beta_g2", beta_g2),
                          ("delta_g2", delta_g2)):
            p, k = _buf(val if (val is None or len(val)) else None)
            keep.append(k)
            setattr(d, name, p.value if p is not None else None)
        h = C.c_void_p()
        if shard is None:
            self.check(ctx, self.dll.ark355_pk_load(ctx, curve, C.byref(d), C.byref(h)))
        else:
            self.check(ctx, self.dll.ark355_pk_load_shard(ctx, curve, C.byref(d), shard[0], shard[1], C.byref(h)))
        return h

    def r1cs_load(self, ctx, curve, n, ell, w, mats):
        """mats: three (row_ptr u64[n+1], col u32[nnz], coeff bytes nnz*fr) tuples."""
        keep = []
        rp = (C.c_void_p * 3)()
        cl = (C.c_void_p * 3)()
        cf = (C.c_void_p * 3)()
        for i, (row_ptr, col, coeff) in enumerate(mats):
            a = np.ascontiguousarray(row_ptr, dtype=np.uint64)
            b = np.ascontiguousarray(col, dtype=np.uint32)
            c, kc = _buf(coeff if len(coeff) else b"\0")
            if b.size == 0:
                b = np.zeros(1, np.uint32)          # a valid pointer for an empty matrix (never read: nnz == 0)
            keep += [a, b, kc]
            rp[i] = a.ctypes.data
            cl[i] = b.ctypes.data
            cf[i] = c.value
        h = C.c_void_p()
        self.check(ctx, self.dll.ark355_r1cs_load(ctx, curve, n, ell, w, C.byref(rp), C.byref(cl), C.byref(cf),
                                                  C.byref(h)))
        return h

    def prove(self, ctx, pk, r1cs, z, z_len, r: bytes, s: bytes, sizes, z_is_device_ptr=False):
        out = ProofRaw()
        rb, k1 = _buf(r)
        sb, k2 = _buf(s)
        if z_is_device_ptr:
            rc = self.dll.ark355_prove_dev(ctx, pk, r1cs, C.c_void_p(z), z_len, rb, sb, C.byref(out))
        else:
            zb, k3 = _buf(z)
            rc = self.dll.ark355_prove(ctx, pk, r1cs, zb, z_len, rb, sb, C.byref(out))
        self.check(ctx, rc)
        return bytes(out.a)[:sizes["g1"]], bytes(out.b)[:sizes["g2"]], bytes(out.c)[:sizes["g1"]]

    def prove_batch(self, ctx, pk, r1cs, zs, z_len, rs, ss, sizes, inflight=3):
        """ark355_prove_batch: `zs` host assignments (bytes), `rs`/`ss` canonical 32-byte scalars, one per proof."""
        count = len(zs)
        out = (ProofRaw * max(1, count))()
        bufs = [_buf(z) for z in zs]
        ptrs = (C.c_void_p * max(1, count))(*[C.cast(b[0], C.c_void_p) for b in bufs])
        rb, k1 = _buf(b"".join(rs) if count else None)
        sb, k2 = _buf(b"".join(ss) if count else None)
        rc = self.dll.ark355_prove_batch(ctx, pk, r1cs, ptrs, z_len, rb, sb, count, int(inflight), out)
        self.check(ctx, rc)
        return [(bytes(o.a)[:sizes["g1"]], bytes(o.b)[:sizes["g2"]], bytes(o.c)[:sizes["g1"]]) for o in out[:count]]

    def prove_shard(self, ctx, curve, pk_shard, r1cs, z, z_len, r: bytes, s: bytes):
        out = np.zeros(self.dll.ark355_partial_size(curve), dtype=np.uint8)
        zb, k1 = _buf(z)
        rb, k2 = _buf(r)
        sb, k3 = _buf(s)
        self.check(ctx, self.dll.ark355_prove_shard(ctx, pk_shard, r1cs, zb, z_len, rb, sb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def prove_combine(self, ctx, curve, partials: bytes, count, r: bytes, s: bytes, sizes):
        out = ProofRaw()
        pb, k1 = _buf(partials)
        rb, k2 = _buf(r)
        sb, k3 = _buf(s)
        self.check(ctx, self.dll.ark355_prove_combine(ctx, curve, pb, count, rb, sb, C.byref(out)))
        return bytes(out.a)[:sizes["g1"]], bytes(out.b)[:sizes["g2"]], bytes(out.c)[:sizes["g1"]]

    # ---- ark-serialize wire formats behind the ABI ------------------------------------------------------------
    def point_size(self, curve, group, compressed):
        return int(self.dll.ark355_point_size(curve, group, int(bool(compressed))))

    def pk_load_bytes(self, ctx, curve, data: bytes, compressed=False, validate=True):
        h = C.c_void_p()
        db, k = _buf(data)
        self.check(ctx, self.dll.ark355_pk_load_bytes(ctx, curve, db, len(data), int(bool(compressed)), int(validate),
                                                      C.byref(h)))
        return h

    def pk_table_info(self, pk):
        c, w, st, by = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        self.check(None, self.dll.ark355_pk_table_info(pk, C.byref(c), C.byref(w), C.byref(st), C.byref(by)))
        return {"window_bits": c.value, "windows": w.value, "table_stride": st.value, "table_bytes": by.value}

    def pk_h_eval(self, pk):
        """State of a key's h query: 'undecided' before its first proof, then 'coeff' or 'eval' (policy H_EVAL)."""
        st, n, sec = C.c_int32(0), C.c_uint32(0), C.c_float(0.0)
        self.check(None, self.dll.ark355_pk_h_eval(pk, C.byref(st), C.byref(n), C.byref(sec)))
        return {"state": ("undecided", "coeff", "eval")[st.value], "binds": n.value, "bind_seconds": sec.value}

    def hbasis_transform(self, ctx, curve, h_query, log_n, want_e=True, want_u=True):
        """(E', U'): the h query (2^log_n - 1 raw affine G1 points) in the evaluation basis of the coset / of the domain."""
        g1 = self.sizes(curve)["g1"]
        n = 1 << log_n
        assert len(h_query) == (n - 1) * g1
        hb, k = _buf(h_query)
        oe = (C.c_uint8 * (n * g1))() if want_e else None
        ou = (C.c_uint8 * (n * g1))() if want_u else None
        self.check(ctx, self.dll.ark355_hbasis_transform(ctx, curve, hb, log_n, oe, ou))
        return (bytes(oe) if want_e else None), (bytes(ou) if want_u else None)

    def hbasis_gather(self, ctx, r1cs, curve, u, m):
        """D_i = sum_j C[j][i] u_j for the m columns of the resident C; u: domain_size raw affine G1 points."""
        g1 = self.sizes(curve)["g1"]
        ub, k = _buf(u)
        out = (C.c_uint8 * (m * g1))()
        self.check(ctx, self.dll.ark355_hbasis_gather(ctx, r1cs, ub, out))
        return bytes(out)

    def pk_dims(self, pk):
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self.check(None, self.dll.ark355_pk_dims(pk, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def points_decode(self, ctx, curve, group, data: bytes, n, compressed, validate, raw_size):
        out = np.zeros(max(1, n * raw_size), dtype=np.uint8)
        db, k = _buf(data if n else None)
        self.check(ctx, self.dll.ark355_points_decode(ctx, curve, group, db, n, int(bool(compressed)), int(validate),
                                                      out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:n * raw_size]

    def points_encode(self, ctx, curve, group, raw: bytes, n, compressed):
        sz = self.point_size(curve, group, compressed)
        out = np.zeros(max(1, n * sz), dtype=np.uint8)
        rb, k = _buf(raw if n else None)
        self.check(ctx, self.dll.ark355_points_encode(ctx, curve, group, rb, n, int(bool(compressed)),
                                                      out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:n * sz]

    def proof_to_bytes(self, curve, a: bytes, b: bytes, c: bytes, compressed=True) -> bytes:
        p = ProofRaw()
        C.memmove(p.a, a, len(a))
        C.memmove(p.b, b, len(b))
        C.memmove(p.c, c, len(c))
        n = 2 * self.point_size(curve, 1, compressed) + self.point_size(curve, 2, compressed)
        out = np.zeros(n, dtype=np.uint8)
        self.check(None, self.dll.ark355_proof_to_bytes(curve, C.byref(p), int(bool(compressed)), out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def proof_from_bytes(self, curve, data: bytes, sizes, compressed=True, validate=True):
        p = ProofRaw()
        db, k = _buf(data)
        rc = self.dll.ark355_proof_from_bytes(curve, db, len(data), int(bool(compressed)), int(validate), C.byref(p))
        if rc != OK:
            raise Ark355Error(rc, "ark355_proof_from_bytes")
        return bytes(p.a)[:sizes["g1"]], bytes(p.b)[:sizes["g2"]], bytes(p.c)[:sizes["g1"]]

    # ---- RCCL behind the ABI ----------------------------------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        out = np.zeros(COMM_ID_BYTES, dtype=np.uint8)
        self.check(None, self.dll.ark355_comm_unique_id(out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def comm_init(self, ctx, comm_id: bytes, rank: int, world: int):
        h = C.c_void_p()
        ib, k = _buf(comm_id)
        self.check(ctx, self.dll.ark355_comm_init(ctx, ib, rank, world, C.byref(h)))
        return h

    def comm_destroy(self, comm):
        self.dll.ark355_comm_destroy(comm)

    def prove_sharded(self, ctx, comm, pk_shard, r1cs, z, z_len, r: bytes, s: bytes, sizes, mode=SHARD_WINDOW,
                      z_is_device_ptr=False):
        out = ProofRaw()
        rb, k2 = _buf(r)
        sb, k3 = _buf(s)
        if z_is_device_ptr:
            rc = self.dll.ark355_prove_sharded_dev(ctx, comm, pk_shard, r1cs, C.c_void_p(z), z_len, rb, sb, int(mode),
                                                   C.byref(out))
        else:
            zb, k1 = _buf(z)
            rc = self.dll.ark355_prove_sharded(ctx, comm, pk_shard, r1cs, zb, z_len, rb, sb, int(mode), C.byref(out))
        self.check(ctx, rc)
        return bytes(out.a)[:sizes["g1"]], bytes(out.b)[:sizes["g2"]], bytes(out.c)[:sizes["g1"]]

    def witness_map(self, ctx, r1cs, z, z_len, fr_size):
        N = self.dll.ark355_r1cs_domain_size(r1cs)
        out = np.zeros(N * fr_size, dtype=np.uint8)
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_witness_map(ctx, r1cs, zb, z_len, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def witness_map_dist_sim(self, ctx, r1cs, z, z_len, fr_size, world):
        """h as the `world` ranks of a sharded proof compute it, all ranks on this device (test / diagnostic entry)"""
        N = self.dll.ark355_r1cs_domain_size(r1cs)
        out = np.zeros(N * fr_size, dtype=np.uint8)
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_witness_map_dist_sim(ctx, r1cs, zb, z_len, int(world), out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def is_satisfied(self, ctx, r1cs, z, z_len):
        fb = C.c_int64(0)
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_is_satisfied(ctx, r1cs, zb, z_len, C.byref(fb)))
        return fb.value

    def mat_vec(self, ctx, r1cs, z, z_len, n, fr_size):
        outs = [np.zeros(max(1, n * fr_size), dtype=np.uint8) for _ in range(3)]
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_r1cs_mat_vec(ctx, r1cs, zb, z_len, *[o.ctypes.data_as(C.c_void_p) for o in outs]))
        return [o.tobytes()[:n * fr_size] for o in outs]

    # ---- GR1CS: every predicate of a constraint system (include/ark355.h "GR1CS") ---------------------------------
    def gr1cs_load(self, ctx, curve, ell, w, preds):
        """preds: a list of (label str, arity, n_constraints, term_coeff bytes, term_ptr u32[n_terms + 1], term_var u32[],
        term_exp u32[], mats) with mats = arity (row_ptr u64[n + 1], col u32[nnz], coeff bytes) tuples; an entry of a
        tuple may be None to hand the library a NULL pointer."""
        keep = []

        def ptr(a, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.size == 0:
                a = np.zeros(1, dtype)               # a valid pointer for an empty array (never read)
            keep.append(a)
            return a.ctypes.data

        descs = (PredicateDesc * max(1, len(preds)))()
        for d, (label, arity, n, term_coeff, term_ptr, term_var, term_exp, mats) in zip(descs, preds):
            d.label = label.encode("utf-8") if label is not None else None
            d.arity, d.n_constraints = arity, n
            d.n_terms = (len(term_ptr) - 1) if term_ptr is not None else (len(term_coeff) // 32 if term_coeff is not None else 0)
            d.term_coeff = ptr(np.frombuffer(term_coeff, dtype=np.uint8), np.uint8) if term_coeff is not None else None
            d.term_ptr, d.term_var, d.term_exp = ptr(term_ptr, np.uint32), ptr(term_var, np.uint32), ptr(term_exp, np.uint32)
            if mats is not None:
                k = max(1, len(mats))
                rp, cl, cf = (C.c_void_p * k)(), (C.c_void_p * k)(), (C.c_void_p * k)()
                for i, (row_ptr, col, coeff) in enumerate(mats):
                    rp[i] = ptr(row_ptr, np.uint64)
                    cl[i] = ptr(col, np.uint32)
                    cf[i] = ptr(np.frombuffer(coeff, dtype=np.uint8), np.uint8) if coeff is not None else None
                keep += [rp, cl, cf]
                d.row_ptr, d.col, d.coeff = C.addressof(rp), C.addressof(cl), C.addressof(cf)
        h = C.c_void_p()
        self.check(ctx, self.dll.ark355_gr1cs_load(ctx, curve, ell, w, descs, len(preds), C.byref(h)))
        return h

    def gr1cs_free(self, g):
        self.dll.ark355_gr1cs_free(g)

    def gr1cs_num_constraints(self, g):
        return self.dll.ark355_gr1cs_num_constraints(g)

    def gr1cs_which_is_unsatisfied(self, ctx, g, z, z_len):
        """(caller's predicate index, row) of the first unsatisfied constraint in label order, or None"""
        pred, row = C.c_int64(0), C.c_int64(0)
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_gr1cs_which_is_unsatisfied(ctx, g, zb, z_len, C.byref(pred), C.byref(row)))
        return None if pred.value < 0 else (pred.value, row.value)

    def gr1cs_mat_vec(self, ctx, g, predicate, z, z_len, arity, n, fr_size):
        """the arity vectors M_k z of one predicate (n Fr each, Montgomery)"""
        out = np.zeros(max(1, arity * n * fr_size), dtype=np.uint8)
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_gr1cs_mat_vec(ctx, g, predicate, zb, z_len, out.ctypes.data_as(C.c_void_p)))
        b = out.tobytes()
        return [b[i * n * fr_size:(i + 1) * n * fr_size] for i in range(arity)]

    def gr1cs_eval(self, ctx, g, predicate, z, z_len, n, fr_size):
        """the residual of every row of one predicate (n Fr, Montgomery; zero where the row is satisfied)"""
        out = np.zeros(max(1, n * fr_size), dtype=np.uint8)
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_gr1cs_eval(ctx, g, predicate, zb, z_len, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:n * fr_size]

    def gr1cs_quotient_dims(self, g, predicate, log_n=0):
        """(degree, log_domain, log_ext, h_len) of the quotient of one predicate (no device work)"""
        deg, ld, le, hl = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        self.check(None, self.dll.ark355_gr1cs_quotient_dims(g, predicate, log_n, C.byref(deg), C.byref(ld), C.byref(le), C.byref(hl)))
        return deg.value, ld.value, le.value, hl.value

    def gr1cs_quotient(self, ctx, g, predicate, z, z_len, log_n, h_len, fr_size):
        """h = P(m_0, .., m_{t-1}) / (X^N - 1): h_len coefficients, Montgomery"""
        out = np.zeros(max(1, h_len * fr_size), dtype=np.uint8)
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_gr1cs_quotient(ctx, g, predicate, zb, z_len, log_n, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:h_len * fr_size]

    def gr1cs_quotient_dev(self, ctx, g, predicate, d_z, z_len, log_n, d_h_out):
        """the same on device pointers (ints): d_h_out takes h_len Fr; returns when it is complete"""
        self.check(ctx, self.dll.ark355_gr1cs_quotient_dev(ctx, g, predicate, C.c_void_p(d_z), z_len, log_n, C.c_void_p(d_h_out)))

    # ---- column polynomials of a predicate at a point (csrc/columns_impl.cuh) --------------------------------------
    def lagrange_fr(self, ctx, curve, log_n, tau: bytes, fr_size=32):
        """L_i(tau) for i < 2^log_n (tau: canonical 32 bytes, little-endian): 2^log_n Montgomery Fr"""
        out = np.zeros((1 << log_n) * fr_size, dtype=np.uint8)
        tb, k = _buf(tau)
        self.check(ctx, self.dll.ark355_lagrange_fr(ctx, curve, log_n, tb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def lagrange_fr_dev(self, ctx, curve, log_n, tau: bytes, d_out):
        tb, k = _buf(tau)
        self.check(ctx, self.dll.ark355_lagrange_fr_dev(ctx, curve, log_n, tb, C.c_void_p(d_out)))

    def gr1cs_mat_vec_t(self, ctx, g, predicate, y, y_len, out_len, fr_size=32):
        """M_k^T y of one predicate: out_len = arity * (num_instance + num_witness) Montgomery Fr, matrix-major"""
        out = np.zeros(max(1, out_len * fr_size), dtype=np.uint8)
        yb, k = _buf(y if len(y) else b"\0")
        self.check(ctx, self.dll.ark355_gr1cs_mat_vec_t(ctx, g, predicate, yb, y_len, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:out_len * fr_size]

    def gr1cs_mat_vec_t_dev(self, ctx, g, predicate, d_y, y_len, d_out):
        self.check(ctx, self.dll.ark355_gr1cs_mat_vec_t_dev(ctx, g, predicate, C.c_void_p(d_y), y_len, C.c_void_p(d_out)))

    def gr1cs_columns_at(self, ctx, g, predicate, tau: bytes, log_n, out_len, fr_size=32):
        """the column polynomials of one predicate at tau: out_len = arity * (num_instance + num_witness) Montgomery Fr"""
        out = np.zeros(max(1, out_len * fr_size), dtype=np.uint8)
        tb, k = _buf(tau)
        self.check(ctx, self.dll.ark355_gr1cs_columns_at(ctx, g, predicate, tb, log_n, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:out_len * fr_size]

    def gr1cs_columns_at_dev(self, ctx, g, predicate, tau: bytes, log_n, d_out):
        tb, k = _buf(tau)
        self.check(ctx, self.dll.ark355_gr1cs_columns_at_dev(ctx, g, predicate, tb, log_n, C.c_void_p(d_out)))

    # ---- polynomial openings (csrc/poly_impl.cuh) --------------------------------------------------------------------
    def poly_eval_fr(self, ctx, curve, coeffs, length, count, x: bytes, fr_size=32):
        """p_k(x) for `count` polynomials of `length` Montgomery coefficients lying back to back (x: canonical 32 bytes,
        little-endian): count Montgomery Fr"""
        out = np.zeros(max(1, count * fr_size), dtype=np.uint8)
        cb, k = _buf(coeffs if len(coeffs) else b"\0")
        xb, kx = _buf(x)
        self.check(ctx, self.dll.ark355_poly_eval_fr(ctx, curve, cb, length, count, xb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:count * fr_size]

    def poly_eval_fr_dev(self, ctx, curve, d_coeffs, length, count, x: bytes, d_out):
        xb, kx = _buf(x)
        self.check(ctx, self.dll.ark355_poly_eval_fr_dev(ctx, curve, C.c_void_p(d_coeffs), length, count, xb, C.c_void_p(d_out)))

    def poly_div_linear_fr(self, ctx, curve, coeffs, length, count, x: bytes, want_rem=True, fr_size=32):
        """(q, rem): q_k = (p_k - p_k(x)) / (X - x) in the layout of the input, rem_k = p_k(x) (None when want_rem is false)"""
        q = np.zeros(max(1, count * length * fr_size), dtype=np.uint8)
        rem = np.zeros(max(1, count * fr_size), dtype=np.uint8)
        cb, k = _buf(coeffs if len(coeffs) else b"\0")
        xb, kx = _buf(x)
        self.check(ctx, self.dll.ark355_poly_div_linear_fr(ctx, curve, cb, length, count, xb, q.ctypes.data_as(C.c_void_p),
                                                           rem.ctypes.data_as(C.c_void_p) if want_rem else None))
        return q.tobytes()[:count * length * fr_size], (rem.tobytes()[:count * fr_size] if want_rem else None)

    def poly_div_linear_fr_dev(self, ctx, curve, d_coeffs, length, count, x: bytes, d_q_out, d_rem_out=None):
        """the same on device pointers (ints); d_q_out == d_coeffs divides in place; d_rem_out may be None"""
        xb, kx = _buf(x)
        self.check(ctx, self.dll.ark355_poly_div_linear_fr_dev(ctx, curve, C.c_void_p(d_coeffs), length, count, xb, C.c_void_p(d_q_out),
                                                               C.c_void_p(d_rem_out) if d_rem_out else None))

    def poly_lincomb_fr(self, ctx, curve, polys, length, count, scalars: bytes, fr_size=32):
        """sum_k scalars[k] polys[k]: `length` Montgomery Fr (scalars: count canonical 32-byte integers)"""
        out = np.zeros(max(1, length * fr_size), dtype=np.uint8)
        pb, k = _buf(polys if len(polys) else b"\0")
        sb, ks = _buf(scalars if len(scalars) else b"\0")
        self.check(ctx, self.dll.ark355_poly_lincomb_fr(ctx, curve, pb, length, count, sb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:length * fr_size]

    def poly_lincomb_fr_dev(self, ctx, curve, d_polys, length, count, scalars: bytes, d_out):
        """the same on device pointers (ints); the scalars stay host bytes; d_out == d_polys combines in place on polynomial 0"""
        sb, ks = _buf(scalars if len(scalars) else b"\0")
        self.check(ctx, self.dll.ark355_poly_lincomb_fr_dev(ctx, curve, C.c_void_p(d_polys), length, count, sb, C.c_void_p(d_out)))

    # ---- openings in the evaluation basis (csrc/evals_impl.cuh) --------------------------------------------------------
    def evals_eval_fr(self, ctx, curve, evals, log_n, count, coset, x: bytes, fr_size=32):
        """p_k(x) for `count` polynomials held as their 2^log_n Montgomery values over the domain (coset != 0: over the coset of
        ark355_ntt_fr), lying back to back (x: canonical 32 bytes, little-endian): count Montgomery Fr"""
        out = np.zeros(max(1, count * fr_size), dtype=np.uint8)
        eb, k = _buf(evals if len(evals) else b"\0")
        xb, kx = _buf(x)
        self.check(ctx, self.dll.ark355_evals_eval_fr(ctx, curve, eb, log_n, count, coset, xb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:count * fr_size]

    def evals_eval_fr_dev(self, ctx, curve, d_evals, log_n, count, coset, x: bytes, d_out):
        xb, kx = _buf(x)
        self.check(ctx, self.dll.ark355_evals_eval_fr_dev(ctx, curve, C.c_void_p(d_evals), log_n, count, coset, xb, C.c_void_p(d_out)))

    def evals_div_linear_fr(self, ctx, curve, evals, log_n, count, coset, x: bytes, want_rem=True, fr_size=32):
        """(q, rem): the values of q_k = (p_k - p_k(x)) / (X - x) over the same domain, in the layout of the input, and
        rem_k = p_k(x) (None when want_rem is false)"""
        size = (count << log_n) * fr_size
        q = np.zeros(max(1, size), dtype=np.uint8)
        rem = np.zeros(max(1, count * fr_size), dtype=np.uint8)
        eb, k = _buf(evals if len(evals) else b"\0")
        xb, kx = _buf(x)
        self.check(ctx, self.dll.ark355_evals_div_linear_fr(ctx, curve, eb, log_n, count, coset, xb, q.ctypes.data_as(C.c_void_p),
                                                            rem.ctypes.data_as(C.c_void_p) if want_rem else None))
        return q.tobytes()[:size], (rem.tobytes()[:count * fr_size] if want_rem else None)

    def evals_div_linear_fr_dev(self, ctx, curve, d_evals, log_n, count, coset, x: bytes, d_q_out, d_rem_out=None):
        """the same on device pointers (ints); d_q_out == d_evals divides in place; d_rem_out may be None"""
        xb, kx = _buf(x)
        self.check(ctx, self.dll.ark355_evals_div_linear_fr_dev(ctx, curve, C.c_void_p(d_evals), log_n, count, coset, xb,
                                                                C.c_void_p(d_q_out), C.c_void_p(d_rem_out) if d_rem_out else None))

    def gr1cs_mat_vec_dev(self, ctx, g, predicate, d_z, z_len, log_n, d_out):
        """the values of m_0 .. m_{t-1} over H_N on device pointers (ints): t x N Montgomery Fr, rows n .. N-1 zero"""
        self.check(ctx, self.dll.ark355_gr1cs_mat_vec_dev(ctx, g, predicate, C.c_void_p(d_z), z_len, log_n, C.c_void_p(d_out)))

    # ---- multilinear extensions (csrc/mle_impl.cuh) -----------------------------------------------------------------------
    def mle_eq_fr(self, ctx, curve, num_vars, point: bytes, fr_size=32):
        """eq(point, i) for i < 2^num_vars (point: num_vars canonical 32-byte integers, little-endian): 2^num_vars Montgomery Fr"""
        out = np.zeros(fr_size << num_vars, dtype=np.uint8)
        pb, k = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_eq_fr(ctx, curve, num_vars, pb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def mle_eq_fr_dev(self, ctx, curve, num_vars, point: bytes, d_out):
        pb, k = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_eq_fr_dev(ctx, curve, num_vars, pb, C.c_void_p(d_out)))

    def mle_fix_fr(self, ctx, curve, evals, num_vars, count, point: bytes, k, fr_size=32):
        """variables 0 .. k-1 of `count` back-to-back tables of 2^num_vars Montgomery Fr fixed to point[0 .. k): count x 2^(num_vars-k)"""
        size = (count << max(num_vars - k, 0)) * fr_size
        out = np.zeros(max(1, size), dtype=np.uint8)
        eb, ke = _buf(evals if len(evals) else b"\0")
        pb, kp = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_fix_fr(ctx, curve, eb, num_vars, count, pb, k, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:size]

    def mle_fix_fr_dev(self, ctx, curve, d_evals, num_vars, count, point: bytes, k, d_out):
        pb, kp = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_fix_fr_dev(ctx, curve, C.c_void_p(d_evals), num_vars, count, pb, k, C.c_void_p(d_out)))

    def mle_eval_fr(self, ctx, curve, evals, num_vars, count, point: bytes, fr_size=32):
        """f~_k(point) for k < count: count Montgomery Fr"""
        out = np.zeros(max(1, count * fr_size), dtype=np.uint8)
        eb, ke = _buf(evals if len(evals) else b"\0")
        pb, kp = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_eval_fr(ctx, curve, eb, num_vars, count, pb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:count * fr_size]

    def mle_eval_fr_dev(self, ctx, curve, d_evals, num_vars, count, point: bytes, d_out):
        pb, kp = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_eval_fr_dev(ctx, curve, C.c_void_p(d_evals), num_vars, count, pb, C.c_void_p(d_out)))

    # ---- multilinear openings (csrc/mle_open_impl.cuh) ----------------------------------------------------------------------
    def mle_quotients_fr(self, ctx, curve, evals, num_vars, count, point: bytes, want_rem=True, fr_size=32):
        """(q, rem): the quotient tables of `count` tables of 2^num_vars Montgomery Fr at `point`, count x 2^num_vars Fr -- level j of
        table c at element (c << num_vars) + mle_level(num_vars, j)[0], the value f~_c(point) in the table's last element -- and the
        count values again (None when want_rem is false)"""
        size = (count << num_vars) * fr_size
        q = np.zeros(max(1, size), dtype=np.uint8)
        rem = np.zeros(max(1, count * fr_size), dtype=np.uint8)
        eb, ke = _buf(evals if len(evals) else b"\0")
        pb, kp = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_quotients_fr(ctx, curve, eb, num_vars, count, pb, q.ctypes.data_as(C.c_void_p),
                                                         rem.ctypes.data_as(C.c_void_p) if want_rem else None))
        return q.tobytes()[:size], (rem.tobytes()[:count * fr_size] if want_rem else None)

    def mle_quotients_fr_dev(self, ctx, curve, d_evals, num_vars, count, point: bytes, d_q_out, d_rem_out=None):
        """the same on device pointers (ints); d_rem_out may be None; no overlap of the three ranges is legal"""
        pb, kp = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_quotients_fr_dev(ctx, curve, C.c_void_p(d_evals), num_vars, count, pb, C.c_void_p(d_q_out),
                                                             C.c_void_p(d_rem_out) if d_rem_out else None))

    def mle_open_dev(self, ctx, curve, level_bases, d_evals, num_vars, point: bytes, point_size, fr_size=32):
        """(proofs, value): the PST opening of one table in device memory against num_vars resident base handles (level j: at least
        2^(num_vars-1-j) points): num_vars affine points of point_size bytes, and f~(point) as one Montgomery Fr"""
        proofs = np.zeros(max(1, num_vars * point_size), dtype=np.uint8)
        value = np.zeros(fr_size, dtype=np.uint8)
        arr = (C.c_void_p * max(1, num_vars))(*[h if isinstance(h, C.c_void_p) else C.c_void_p(h) for h in level_bases])
        pb, kp = _buf(point if len(point) else b"\0")
        self.check(ctx, self.dll.ark355_mle_open_dev(ctx, curve, arr, C.c_void_p(d_evals), num_vars, pb, proofs.ctypes.data_as(C.c_void_p),
                                                     value.ctypes.data_as(C.c_void_p)))
        return proofs.tobytes()[:num_vars * point_size], value.tobytes()

    # ---- sum-check of a predicate (csrc/sumcheck_impl.cuh) ------------------------------------------------------------------
    def gr1cs_sumcheck_begin_dev(self, ctx, g, predicate, d_tables, d_weight, num_vars):
        """a sumcheck handle over arity x 2^num_vars Fr at d_tables and 2^num_vars Fr at d_weight (None: weight 1), device pointers"""
        h = C.c_void_p()
        self.check(ctx, self.dll.ark355_gr1cs_sumcheck_begin_dev(ctx, g, predicate, C.c_void_p(d_tables) if d_tables else None,
                                                                 C.c_void_p(d_weight) if d_weight else None, num_vars, C.byref(h)))
        return h

    def sumcheck_info(self, sc):
        """(num_vars, arity, points, rounds_done)"""
        v = [C.c_uint32(0) for _ in range(4)]
        self.check(None, self.dll.ark355_sumcheck_info(sc, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def sumcheck_round(self, ctx, sc, challenge, points, fr_size=32):
        """the message of the next round: `points` Montgomery Fr (challenge: None exactly in round 1, else canonical 32 bytes)"""
        out = np.zeros(max(1, points * fr_size), dtype=np.uint8)
        cb, k = _buf(challenge)
        self.check(ctx, self.dll.ark355_sumcheck_round(ctx, sc, cb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:points * fr_size]

    def sumcheck_finish(self, ctx, sc, challenge, arity, fr_size=32):
        """T_0, .., T_{t-1}, W at the point of the challenges: arity + 1 Montgomery Fr"""
        out = np.zeros((arity + 1) * fr_size, dtype=np.uint8)
        cb, k = _buf(challenge)
        self.check(ctx, self.dll.ark355_sumcheck_finish(ctx, sc, cb, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def sumcheck_free(self, sc):
        self.dll.ark355_sumcheck_free(sc)

    def gr1cs_r1cs(self, ctx, g):
        """an ark355_r1cs handle from the predicate labelled "R1CS" (refused when another predicate has a row)"""
        h = C.c_void_p()
        self.check(ctx, self.dll.ark355_gr1cs_r1cs(ctx, g, C.byref(h)))
        return h

    def gr1cs_dims(self, g):
        """(num_instance, num_witness, n_preds) of a resident system"""
        ell, w, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self.check(None, self.dll.ark355_gr1cs_dims(g, C.byref(ell), C.byref(w), C.byref(n)))
        return ell.value, w.value, n.value

    def gr1cs_pred_dims(self, g, predicate):
        """(arity, n_constraints, (nnz of each matrix)) of one predicate (caller's index)"""
        arity, n = C.c_uint32(0), C.c_uint64(0)
        self.check(None, self.dll.ark355_gr1cs_pred_dims(g, predicate, C.byref(arity), C.byref(n), None))
        nnz = (C.c_uint64 * max(1, arity.value))()
        self.check(None, self.dll.ark355_gr1cs_pred_dims(g, predicate, None, None, C.addressof(nnz)))
        return arity.value, n.value, tuple(nnz[k] for k in range(arity.value))

    def gr1cs_matrix(self, ctx, g, predicate, which, rows, nnz, fr_size, entry_capacity=None):
        """(row_ptr u64[rows + 1], col u32[nnz], coeff bytes) of matrix `which` of one predicate: to_matrices() of a resident system"""
        rp = np.zeros(rows + 1, dtype=np.uint64)
        col = np.zeros(max(1, nnz), dtype=np.uint32)
        cf = np.zeros(max(1, nnz * fr_size), dtype=np.uint8)
        cap = nnz if entry_capacity is None else entry_capacity
        self.check(ctx, self.dll.ark355_gr1cs_matrix(ctx, g, predicate, which, rp.ctypes.data_as(C.c_void_p),
                                                     col.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), cap))
        return rp, col[:nnz], cf.tobytes()[:nnz * fr_size]

    # ---- finalize() on the device (include/ark355.h "finalize() on the device") -------------------------------------
    def gr1cs_from_lcs(self, ctx, curve, ell, w, lc_offsets, lc_vars, lc_coeffs, pool, preds, outline=0, n_lcs=None, n_pool=None, n_preds=None):
        """lc_offsets u64[n_lcs + 1], lc_vars u64[], lc_coeffs u32[], pool = Montgomery Fr bytes; preds: a list of (label,
        arity, n_constraints, term_coeff bytes, term_ptr u32[], term_var u32[], term_exp u32[], args) with args = arity u64
        arrays of packed Variables.  Any array may be None to hand the library a NULL pointer; n_lcs / n_pool / n_preds
        override the counts the arrays imply."""
        keep = []

        def ptr(a, dtype):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.size == 0:
                a = np.zeros(1, dtype)               # a valid pointer for an empty array (never read)
            keep.append(a)
            return a.ctypes.data

        sysd = LcSystemDesc()
        sysd.num_instance, sysd.num_witness, sysd.outline = ell, w, outline
        sysd.n_lcs = n_lcs if n_lcs is not None else (len(lc_offsets) - 1 if lc_offsets is not None else 0)
        sysd.lc_offsets, sysd.lc_vars, sysd.lc_coeffs = ptr(lc_offsets, np.uint64), ptr(lc_vars, np.uint64), ptr(lc_coeffs, np.uint32)
        sysd.n_pool = n_pool if n_pool is not None else (len(pool) // 32 if pool is not None else 0)
        sysd.pool = ptr(np.frombuffer(pool, dtype=np.uint8), np.uint8) if pool is not None else None
        descs = None
        if preds is not None:
            descs = (PredicateLcsDesc * max(1, len(preds)))()
            for d, (label, arity, n, term_coeff, term_ptr, term_var, term_exp, args) in zip(descs, preds):
                d.label = label.encode("utf-8") if label is not None else None
                d.arity, d.n_constraints = arity, n
                d.n_terms = (len(term_ptr) - 1) if term_ptr is not None else (len(term_coeff) // 32 if term_coeff is not None else 0)
                d.term_coeff = ptr(np.frombuffer(term_coeff, dtype=np.uint8), np.uint8) if term_coeff is not None else None
                d.term_ptr, d.term_var, d.term_exp = ptr(term_ptr, np.uint32), ptr(term_var, np.uint32), ptr(term_exp, np.uint32)
                if args is not None:
                    ap = (C.c_void_p * max(1, len(args)))()
                    for i, a in enumerate(args):
                        ap[i] = ptr(a, np.uint64)
                    keep.append(ap)
                    d.args = C.addressof(ap)
        h = C.c_void_p()
        if n_preds is None:
            n_preds = len(preds) if preds is not None else 0
        self.check(ctx, self.dll.ark355_gr1cs_from_lcs(ctx, curve, C.byref(sysd), descs, n_preds, C.byref(h)))
        return h

    # ---- Square R1CS: Sr1csAdapter on the device (include/ark355.h "Square R1CS") -----------------------------------
    def sr1cs_from_r1cs(self, ctx, r1cs):
        """an ark355_sr1cs handle from a resident R1CS (freed with sr1cs_free; the r1cs handle may be freed first)"""
        h = C.c_void_p()
        self.check(ctx, self.dll.ark355_sr1cs_from_r1cs(ctx, r1cs, C.byref(h)))
        return h

    def sr1cs_free(self, s):
        self.dll.ark355_sr1cs_free(s)

    def sr1cs_system(self, s):
        """the borrowed ark355_gr1cs handle of the resident system (never passed to gr1cs_free)"""
        return C.c_void_p(self.dll.ark355_sr1cs_system(s))

    def sr1cs_dims(self, s):
        """(num_instance', num_witness', rows, (nnz M0, nnz M1))"""
        ell, w, n, nnz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 2)()
        self.check(None, self.dll.ark355_sr1cs_dims(s, C.byref(ell), C.byref(w), C.byref(n), C.byref(nnz)))
        return ell.value, w.value, n.value, (nnz[0], nnz[1])

    def sr1cs_var_map(self, ctx, s, m):
        """(witness_col, instance_col): int64 arrays over the m old columns (-1: none)"""
        wit, inst = np.zeros(max(1, m), dtype=np.int64), np.zeros(max(1, m), dtype=np.int64)
        self.check(ctx, self.dll.ark355_sr1cs_var_map(ctx, s, wit.ctypes.data_as(C.c_void_p), inst.ctypes.data_as(C.c_void_p)))
        return wit[:m], inst[:m]

    def sr1cs_matrix(self, ctx, s, which, rows, nnz, fr_size, entry_capacity=None):
        """(row_ptr u64[rows + 1], col u32[nnz], coeff bytes) of matrix `which`"""
        rp = np.zeros(rows + 1, dtype=np.uint64)
        col = np.zeros(max(1, nnz), dtype=np.uint32)
        cf = np.zeros(max(1, nnz * fr_size), dtype=np.uint8)
        cap = nnz if entry_capacity is None else entry_capacity
        self.check(ctx, self.dll.ark355_sr1cs_matrix(ctx, s, which, rp.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                                     cf.ctypes.data_as(C.c_void_p), cap))
        return rp, col[:nnz], cf.tobytes()[:nnz * fr_size]

    def sr1cs_assignment(self, ctx, s, z, z_len, m_out, fr_size):
        """z (Montgomery bytes) -> z' (m_out Fr, Montgomery bytes)"""
        out = np.zeros(max(1, m_out * fr_size), dtype=np.uint8)
        zb, k = _buf(z)
        self.check(ctx, self.dll.ark355_sr1cs_assignment(ctx, s, zb, z_len, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:m_out * fr_size]

    def sr1cs_assignment_dev(self, ctx, s, d_z, z_len, d_z_out):
        """device pointers (ints): z -> z'; returns when z' is complete"""
        self.check(ctx, self.dll.ark355_sr1cs_assignment_dev(ctx, s, C.c_void_p(d_z), z_len, C.c_void_p(d_z_out)))

    def ntt(self, ctx, curve, data: bytes, log_n, inverse=False, coset=False):
        a = np.frombuffer(bytearray(data), dtype=np.uint8)
        self.check(ctx, self.dll.ark355_ntt_fr(ctx, curve, a.ctypes.data_as(C.c_void_p), log_n, int(inverse), int(coset)))
        return a.tobytes()

    def ntt_dev(self, ctx, curve, d_data, d_scratch, log_n, inverse=False, coset=False, stream=None):
        """in place on DEVICE pointers (2^log_n Fr each; the content of d_scratch afterwards is unspecified), queued on `stream`
        (a hipStream_t as an integer; None = the context's own) and NOT synchronised: the caller waits for that stream"""
        self.check(ctx, self.dll.ark355_ntt_fr_dev(ctx, curve, C.c_void_p(d_data), C.c_void_p(d_scratch), log_n, int(inverse),
                                                   int(coset), C.c_void_p(stream) if stream else None))

    def msm(self, ctx, curve, group, bases: bytes, scalars: bytes, n, out_size):
        out = np.zeros(out_size, dtype=np.uint8)
        bb, k1 = _buf(bases if n else None)
        sb, k2 = _buf(scalars if n else None)
        fn = self.dll.ark355_msm_g1 if group == 1 else self.dll.ark355_msm_g2
        self.check(ctx, fn(ctx, curve, bb, sb, n, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def bases_load(self, ctx, curve, group, bases, n):
        h = C.c_void_p()
        bb, k = _buf(bases if n else None)
        self.check(ctx, self.dll.ark355_bases_load(ctx, curve, group, bb, n, C.byref(h)))
        return h

    def msm_dev(self, ctx, bases_h, d_scalars_ptr, n, mont, out_size, partial=False):
        out = np.zeros(out_size, dtype=np.uint8)
        fn = self.dll.ark355_msm_dev_partial if partial else self.dll.ark355_msm_dev
        self.check(ctx, fn(ctx, bases_h, C.c_void_p(d_scalars_ptr), n, int(mont), out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def msm_batch_dev(self, ctx, handles, d_ptrs, ns, mont, out_size):
        """ark355_msm_batch_dev: len(ns) independent MSMs, segment s over ns[s] scalars at the device pointer d_ptrs[s] (None where
        ns[s] is 0) against the resident handle handles[s]; all handles of one curve and group.  Returns the affine points, out_size
        bytes each, back to back."""
        count = len(ns)
        assert len(handles) == count and len(d_ptrs) == count
        out = np.zeros(max(1, count * out_size), dtype=np.uint8)
        hs = (C.c_void_p * max(1, count))(*[h if isinstance(h, C.c_void_p) else C.c_void_p(h) for h in handles])
        ps = (C.c_void_p * max(1, count))(*[C.c_void_p(p) if p else None for p in d_ptrs])
        nn = (C.c_uint64 * max(1, count))(*[int(x) for x in ns])
        self.check(ctx, self.dll.ark355_msm_batch_dev(ctx, hs, ps, nn, count, int(mont), out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:count * out_size]

    def xyzz_sum(self, ctx, curve, group, partials: bytes, count, out_size):
        out = np.zeros(out_size, dtype=np.uint8)
        pb, k = _buf(partials if count else None)
        self.check(ctx, self.dll.ark355_xyzz_sum(ctx, curve, group, pb, count, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def fixed_base_mul_dev(self, ctx, curve, group, base: bytes, d_scalars, n, scalars_mont, point_size):
        """ark355_fixed_base_mul over n scalars in device memory (d_scalars: int); scalars_mont: they are Montgomery images"""
        out = np.zeros(max(1, n * point_size), dtype=np.uint8)
        bb, k1 = _buf(base)
        self.check(ctx, self.dll.ark355_fixed_base_mul_dev(ctx, curve, group, bb, C.c_void_p(d_scalars), n, 1 if scalars_mont else 0,
                                                           out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:n * point_size]

    def fixed_base_mul(self, ctx, curve, group, base: bytes, scalars, n, point_size):
        out = np.zeros(max(1, n * point_size), dtype=np.uint8)
        bb, k1 = _buf(base)
        sb, k2 = _buf(scalars if n else None)
        self.check(ctx, self.dll.ark355_fixed_base_mul(ctx, curve, group, bb, sb, n, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()[:n * point_size]

    def setup_scalars(self, curve, n, ell, w, mats, trapdoor: bytes):
        """ark355_setup_scalars: mats as for r1cs_load; trapdoor = tau|alpha|beta|gamma|delta (5 x 32 B canonical).
        Returns dict of canonical byte strings u, v, w (m each), l (w), gamma_abc (ell), h (N - 1)."""
        keep = []
        rp = (C.c_void_p * 3)()
        cl = (C.c_void_p * 3)()
        cf = (C.c_void_p * 3)()
        for i, (row_ptr, col, coeff) in enumerate(mats):
            a = np.ascontiguousarray(row_ptr, dtype=np.uint64)
            b = np.ascontiguousarray(col, dtype=np.uint32)
            if b.size == 0:
                b = np.zeros(1, dtype=np.uint32)
            c, kc = _buf(coeff if len(coeff) else bytes(32))
            keep += [a, b, kc]
            rp[i], cl[i], cf[i] = a.ctypes.data, b.ctypes.data, c.value
        N = 1
        while N < n + ell:
            N <<= 1
        m = ell + w
        outs = {k: np.zeros(max(1, cnt) * 32, dtype=np.uint8)
                for k, cnt in (("u", m), ("v", m), ("w", m), ("l", w), ("gamma_abc", ell), ("h", N - 1))}
        tb, kt = _buf(trapdoor)
        self.check(None, self.dll.ark355_setup_scalars(curve, n, ell, w, C.byref(rp), C.byref(cl), C.byref(cf), tb,
                                                       *[outs[k].ctypes.data_as(C.c_void_p) for k in ("u", "v", "w", "l", "gamma_abc", "h")]))
        cnts = {"u": m, "v": m, "w": m, "l": w, "gamma_abc": ell, "h": N - 1}
        return {k: outs[k][:cnts[k] * 32] for k in outs}

    def setup(self, ctx, r1cs, g1_base: bytes, g2_base: bytes, trapdoor: bytes, dims, sizes, want=SETUP_OUT_FIELDS, want_pk=True):
        """ark355_setup: the Groth16 generator on the device.  r1cs: an ark355_r1cs handle; dims = (ell, w, N) of it; sizes as
        from sizes(); trapdoor = tau|alpha|beta|gamma|delta (5 x 32 B canonical); want: the fields of ark355_setup_out to
        fetch (None or empty: out = NULL, the key never visits the host); want_pk: also return the resident key.
        Returns (dict of numpy byte arrays keyed by field name, ark355_pk handle or None)."""
        ell, w, N = dims
        m, g1, g2 = ell + w, sizes["g1"], sizes["g2"]
        nbytes = dict(alpha_g1=g1, beta_g1=g1, delta_g1=g1, beta_g2=g2, gamma_g2=g2, delta_g2=g2, gamma_abc_g1=ell * g1,
                      a_query=m * g1, b_g1_query=m * g1, b_g2_query=m * g2, h_query=(N - 1) * g1, l_query=w * g1,
                      u=m * 32, v=m * 32, w=m * 32)
        outs, so = {}, None
        if want:
            so = SetupOut()
            for k in want:
                outs[k] = np.zeros(max(1, nbytes[k]), dtype=np.uint8)
                setattr(so, k, outs[k].ctypes.data)
        b1, k1 = _buf(g1_base)
        b2, k2 = _buf(g2_base)
        tb, k3 = _buf(trapdoor)
        h = C.c_void_p()
        self.check(ctx, self.dll.ark355_setup(ctx, r1cs, b1, b2, tb, C.byref(so) if so is not None else None,
                                              C.byref(h) if want_pk else None))
        return {k: outs[k][:nbytes[k]] for k in outs}, (h if want_pk else None)

    def verify_batch(self, ctx, curve, vk_parts, proofs, public_inputs: bytes, rho=None) -> bool:
        """ark355_verify_batch.  vk_parts: (alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1) raw images; proofs: list of
        (a, b, c) raw images; public_inputs: count x (ell - 1) Montgomery Fr; rho: list of canonical 32-byte values or None."""
        alpha, beta2, gamma2, delta2, gabc = vk_parts
        keep = []
        d = VkDesc()
        for name, val in (("alpha_g1", alpha), ("beta_g2", beta2), ("gamma_g2", gamma2), ("delta_g2", delta2), ("gamma_abc_g1", gabc)):
            p, k = _buf(val)
            keep.append(k)
            setattr(d, name, p.value)
        g1 = len(alpha)
        d.num_instance = len(gabc) // g1
        arr = (ProofRaw * len(proofs))()
        for i, (a, b, c) in enumerate(proofs):
            C.memmove(arr[i].a, a, len(a))
            C.memmove(arr[i].b, b, len(b))
            C.memmove(arr[i].c, c, len(c))
        ib, k1 = _buf(public_inputs if len(public_inputs) else None)
        rb, k2 = _buf(b"".join(rho) if rho else None)
        ok = C.c_int32(0)
        self.check(ctx, self.dll.ark355_verify_batch(ctx, curve, C.byref(d), arr, ib, rb, len(proofs), C.byref(ok)))
        return bool(ok.value)

    def _vk_desc(self, vk_parts, keep):
        alpha, beta2, gamma2, delta2, gabc = vk_parts
        d = VkDesc()
        for name, val in (("alpha_g1", alpha), ("beta_g2", beta2), ("gamma_g2", gamma2), ("delta_g2", delta2), ("gamma_abc_g1", gabc)):
            p, k = _buf(val)
            keep.append(k)
            setattr(d, name, p.value)
        d.num_instance = len(gabc) // len(alpha)
        return d

    def verify_each(self, ctx, curve, vk_parts, proofs, public_inputs: bytes):
        """ark355_verify_each: one verdict per proof.  Arguments as for verify_batch (no rho).  Returns a list of bool."""
        keep = []
        d = self._vk_desc(vk_parts, keep)
        arr = (ProofRaw * max(1, len(proofs)))()
        for i, (a, b, c) in enumerate(proofs):
            C.memmove(arr[i].a, a, len(a))
            C.memmove(arr[i].b, b, len(b))
            C.memmove(arr[i].c, c, len(c))
        ib, k1 = _buf(public_inputs if len(public_inputs) else None)
        ok = np.zeros(max(1, len(proofs)), dtype=np.uint8)
        self.check(ctx, self.dll.ark355_verify_each(ctx, curve, C.byref(d), arr, ib, len(proofs), ok.ctypes.data_as(C.c_void_p)))
        return [bool(v) for v in ok[:len(proofs)]]

    # ---- the processed verifying key (include/ark355.h "processed verifying key") -----------------------------------------
    @staticmethod
    def _proof_array(proofs):
        arr = (ProofRaw * max(1, len(proofs)))()
        for i, (a, b, c) in enumerate(proofs):
            C.memmove(arr[i].a, a, len(a))
            C.memmove(arr[i].b, b, len(b))
            C.memmove(arr[i].c, c, len(c))
        return arr

    def vk_process(self, ctx, curve, vk_parts):
        """ark355_vk_process: vk_parts as for verify_batch -> the handle (free it with pvk_free)."""
        keep = []
        d = self._vk_desc(vk_parts, keep)
        h = C.c_void_p()
        self.check(ctx, self.dll.ark355_vk_process(ctx, curve, C.byref(d), C.byref(h)))
        return h

    def pvk_free(self, pvk):
        self.dll.ark355_pvk_free(pvk)

    def pvk_info(self, pvk):
        curve, ell, nbytes = C.c_int32(-1), C.c_uint64(0), C.c_uint64(0)
        self.check(None, self.dll.ark355_pvk_info(pvk, C.byref(curve), C.byref(ell), C.byref(nbytes)))
        return {"curve": int(curve.value), "num_instance": int(ell.value), "resident_bytes": int(nbytes.value)}

    def pvk_alpha_beta(self, pvk) -> bytes:
        """ark355_pvk_alpha_beta: e(alpha_g1, beta_g2) as multi_pairing returns it."""
        out = np.zeros(12 * self.sizes(self.pvk_info(pvk)["curve"])["fq"], dtype=np.uint8)
        self.check(None, self.dll.ark355_pvk_alpha_beta(pvk, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def pvk_pairings(self, ctx, pvk, which, g1: bytes, n, want_gt=True):
        """ark355_pvk_pairings: e(P_i, Q_which) for n raw G1 images.  Returns (gt, is_one) as pairing_groups does."""
        fq = self.sizes(self.pvk_info(pvk)["curve"])["fq"]
        out = np.zeros(max(1, n) * 12 * fq, dtype=np.uint8)
        one = np.zeros(max(1, n), dtype=np.uint8)
        b1, k1 = _buf(g1 if g1 else None)
        self.check(ctx, self.dll.ark355_pvk_pairings(ctx, pvk, which, b1, n, out.ctypes.data_as(C.c_void_p) if want_gt else None,
                                                     one.ctypes.data_as(C.c_void_p)))
        return (out[:n * 12 * fq].tobytes() if want_gt else None), [bool(v) for v in one[:n]]

    def verify_each_pvk(self, ctx, pvk, proofs, public_inputs: bytes):
        """ark355_verify_each_pvk: one verdict per proof against a processed key.  Returns a list of bool."""
        arr = self._proof_array(proofs)
        ib, k1 = _buf(public_inputs if len(public_inputs) else None)
        ok = np.zeros(max(1, len(proofs)), dtype=np.uint8)
        self.check(ctx, self.dll.ark355_verify_each_pvk(ctx, pvk, arr, ib, len(proofs), ok.ctypes.data_as(C.c_void_p)))
        return [bool(v) for v in ok[:len(proofs)]]

    # ---- proofs as wire bytes (include/ark355.h "proofs as wire bytes") ---------------------------------------------------
    def points_check(self, ctx, curve, group, raw: bytes, n, method=1):
        """ark355_points_check: curve + subgroup status of n raw affine images (method 0: [r]P, 1: the endomorphism tests).
        Returns a list of int (0, 2 not on the curve, 4 not in the subgroup)."""
        st = np.zeros(max(1, n), dtype=np.uint8)
        rb, k = _buf(raw if n else None)
        self.check(ctx, self.dll.ark355_points_check(ctx, curve, group, rb, n, int(method), st.ctypes.data_as(C.c_void_p)))
        return [int(v) for v in st[:n]]

    def proofs_from_bytes(self, ctx, curve, data: bytes, count, sizes, compressed=True, validate=1):
        """ark355_proofs_from_bytes: `count` proofs (a || b || c each) decoded on the device.
        Returns ([(a, b, c) raw images], [status]); the images of a proof with a non-zero status are all zero."""
        arr = (ProofRaw * max(1, count))()
        st = np.zeros(max(1, count), dtype=np.uint8)
        db, k = _buf(data if count else None)
        self.check(ctx, self.dll.ark355_proofs_from_bytes(ctx, curve, db, count, int(bool(compressed)), int(validate), arr,
                                                          st.ctypes.data_as(C.c_void_p)))
        out = [(bytes(arr[j].a)[:sizes["g1"]], bytes(arr[j].b)[:sizes["g2"]], bytes(arr[j].c)[:sizes["g1"]]) for j in range(count)]
        return out, [int(v) for v in st[:count]]

    def verify_each_bytes(self, ctx, pvk, data: bytes, count, public_inputs: bytes, compressed=True, validate=1, want_status=True):
        """ark355_verify_each_bytes: `count` serialized proofs against a processed key.  Returns (list of bool, list of int
        statuses or None with want_status=False)."""
        ok = np.zeros(max(1, count), dtype=np.uint8)
        st = np.zeros(max(1, count), dtype=np.uint8)
        db, k = _buf(data if count else None)
        ib, k1 = _buf(public_inputs if len(public_inputs) else None)
        self.check(ctx, self.dll.ark355_verify_each_bytes(ctx, pvk, db, count, int(bool(compressed)), int(validate), ib,
                                                          ok.ctypes.data_as(C.c_void_p),
                                                          st.ctypes.data_as(C.c_void_p) if want_status else None))
        return [bool(v) for v in ok[:count]], ([int(v) for v in st[:count]] if want_status else None)

    def verify_batch_pvk(self, ctx, pvk, proofs, public_inputs: bytes, rho=None) -> bool:
        """ark355_verify_batch_pvk: verify_batch against a processed key."""
        arr = self._proof_array(proofs)
        ib, k1 = _buf(public_inputs if len(public_inputs) else None)
        rb, k2 = _buf(b"".join(rho) if rho else None)
        ok = C.c_int32(0)
        self.check(ctx, self.dll.ark355_verify_batch_pvk(ctx, pvk, arr, ib, rb, len(proofs), C.byref(ok)))
        return bool(ok.value)

    def pairing_groups(self, ctx, curve, g1: bytes, g2: bytes, groups, group_len=1, want_gt=True):
        """ark355_pairing_groups over groups x group_len raw affine pairs.  Returns (gt, is_one): gt = groups x 12 Fq as bytes
        (None with want_gt=False), is_one = list of bool."""
        fq = self.sizes(curve)["fq"]
        out = np.zeros(max(1, groups) * 12 * fq, dtype=np.uint8)
        one = np.zeros(max(1, groups), dtype=np.uint8)
        b1, k1 = _buf(g1 if g1 else None)
        b2, k2 = _buf(g2 if g2 else None)
        self.check(ctx, self.dll.ark355_pairing_groups(ctx, curve, b1, b2, groups, group_len,
                                                       out.ctypes.data_as(C.c_void_p) if want_gt else None,
                                                       one.ctypes.data_as(C.c_void_p)))
        return (out[:groups * 12 * fq].tobytes() if want_gt else None), [bool(v) for v in one[:groups]]

    def multi_pairing(self, ctx, curve, g1: bytes, g2: bytes, n, want_gt=True):
        """ark355_multi_pairing over n raw affine pairs.  Returns (gt, is_one): gt = 12 Fq (Montgomery, ark-ff Fp12 order) as
        bytes, or None with want_gt=False."""
        fq = self.sizes(curve)["fq"]
        out = np.zeros(12 * fq, dtype=np.uint8)
        b1, k1 = _buf(g1 if g1 else None)
        b2, k2 = _buf(g2 if g2 else None)
        one = C.c_int32(0)
        self.check(ctx, self.dll.ark355_multi_pairing(ctx, curve, b1, b2, n, out.ctypes.data_as(C.c_void_p) if want_gt else None,
                                                      C.byref(one)))
        return (out.tobytes() if want_gt else None), bool(one.value)

    def timings(self, ctx):
        t = Timings()
        self.check(ctx, self.dll.ark355_get_timings(ctx, C.byref(t)))
        return {n: getattr(t, n) for n, _ in Timings._fields_}

    def kernel_stats(self, ctx):
        ms, l, p = C.c_float(0), C.c_uint64(0), C.c_uint64(0)
        self.check(ctx, self.dll.ark355_get_kernel_stats(ctx, C.byref(ms), C.byref(l), C.byref(p)))
        return {"accumulate_ms": ms.value, "launches": l.value, "points": p.value}
