"""GR1CS on the device: every predicate of an ``ark-relations`` constraint system, not only ``"R1CS"``.

The reference keeps a ``BTreeMap<Label, PredicateConstraintSystem>`` (relations/src/gr1cs/constraint_system.rs:44-97):
a predicate is a sparse multivariate polynomial of some arity ``t`` over ``t`` matrices
(gr1cs/predicate/polynomial_constraint.rs), ``"R1CS"`` (``x0*x1 - x2``) merely the one registered by default, and
``ConstraintSystem::to_matrices()`` returns one list of matrices per label (constraint_system.rs:768-774).
``GR1CS.from_matrices`` takes exactly that map plus each predicate's polynomial
(``PredicateConstraintSystem::get_predicate``); the device then answers ``which_is_unsatisfied``
(constraint_system.rs:652-687: labels in sorted order, rows ascending), ``mat_vec_mul`` per matrix and the polynomial's
residual per row.  Groth16 proves R1CS only: ``r1cs_handle`` hands the ``"R1CS"`` predicate to the prover and refuses
when any other predicate carries a constraint.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .params import Curve, CURVES

R1CS_PREDICATE_LABEL = "R1CS"          # predicate/polynomial_constraint.rs:69


@dataclass
class Predicate:
    """One label: the polynomial (terms = [(coeff, [(var, exp), ...]), ...], canonical ints) and its ``arity`` matrices in
    CSR (row_ptr u64[n + 1], col u32[nnz], coeff = Montgomery Fr images, 32 B per non-zero)."""
    label: str
    arity: int
    terms: List[Tuple[int, List[Tuple[int, int]]]]
    n: int
    row_ptr: List[np.ndarray]
    col: List[np.ndarray]
    coeff: List[bytes]


def csr_from_rows(curve: Curve, rows, _cache=None):
    """Matrix<F> = Vec<Vec<(F, usize)>> (canonical ints) -> (row_ptr, col, coeff bytes)."""
    cache = {} if _cache is None else _cache
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    cl, cf = [], []
    for i, row in enumerate(rows):
        for c, j in row:
            b = cache.get(c)
            if b is None:
                b = cache[c] = curve.fr_mont(c)
            cl.append(j)
            cf.append(b)
        rp[i + 1] = len(cl)
    return rp, np.array(cl, dtype=np.uint32), b"".join(cf)


@dataclass
class GR1CS:
    curve: Curve
    ell: int                                   # instance variables, the constant One included
    w: int
    predicates: List[Predicate]
    lib: object = None
    ctx: object = None
    handle: object = None
    _index: Dict[str, int] = field(default_factory=dict)

    @staticmethod
    def from_matrices(curve, ell: int, w: int, predicates) -> "GR1CS":
        """predicates: {label: (arity, terms, matrices)} with ``matrices`` shaped like ``to_matrices()[label]`` (``arity``
        lists of rows of (coeff, column) pairs, as in ``R1CS.from_rows``) and ``terms`` = [(coeff, [(var, exp), ...])]."""
        curve = CURVES[curve] if not isinstance(curve, Curve) else curve
        cache, preds = {}, []
        for label, (arity, terms, matrices) in predicates.items():
            if len(matrices) != arity:
                raise ValueError("predicate %r: %d matrices for arity %d" % (label, len(matrices), arity))
            n = len(matrices[0]) if matrices else 0
            if any(len(M) != n for M in matrices):
                raise ValueError("predicate %r: matrices of different heights" % (label,))
            csr = [csr_from_rows(curve, M, cache) for M in matrices]
            preds.append(Predicate(label, arity, [(c, list(f)) for c, f in terms], n, [a for a, _, _ in csr],
                                   [b for _, b, _ in csr], [c for _, _, c in csr]))
        return GR1CS(curve, ell, w, preds)

    @staticmethod
    def from_handle(curve, lib, ctx, handle, predicates) -> "GR1CS":
        """A ``GR1CS`` over a system that is already resident (``LcSystem.finalize``): predicates = [(label, terms)] in the order
        the handle was built with; dimensions and row counts are read from the handle (``ark355_gr1cs_dims`` / ``_pred_dims``).
        ``free()`` frees the handle."""
        curve = CURVES[curve] if not isinstance(curve, Curve) else curve
        ell, w, n_preds = lib.gr1cs_dims(handle)
        if n_preds != len(predicates):
            raise ValueError("the handle holds %d predicates, %d were named" % (n_preds, len(predicates)))
        preds = []
        for i, (label, terms) in enumerate(predicates):
            arity, n, _ = lib.gr1cs_pred_dims(handle, i)
            preds.append(Predicate(label, arity, [(c, list(f)) for c, f in terms], n, [], [], []))
        g = GR1CS(curve, ell, w, preds)
        g.lib, g.ctx, g.handle = lib, ctx, handle
        g._index = {p.label: i for i, p in enumerate(preds)}
        return g

    # ---- device ---------------------------------------------------------------------------------------------------
    def load(self, lib, ctx) -> "GR1CS":
        self.free()
        descs = []
        for p in self.predicates:
            term_ptr, var, exp = [0], [], []
            for _, factors in p.terms:
                var += [v for v, _ in factors]
                exp += [e for _, e in factors]
                term_ptr.append(len(var))
            descs.append((p.label, p.arity, p.n, b"".join(self.curve.fr_mont(c) for c, _ in p.terms),
                          np.array(term_ptr, dtype=np.uint32), np.array(var, dtype=np.uint32), np.array(exp, dtype=np.uint32),
                          list(zip(p.row_ptr, p.col, p.coeff))))
        self.handle = lib.gr1cs_load(ctx, self.curve.curve_id, self.ell, self.w, descs)
        self.lib, self.ctx = lib, ctx
        self._index = {p.label: i for i, p in enumerate(self.predicates)}
        return self

    def free(self):
        if self.handle is not None:
            self.lib.gr1cs_free(self.handle)
            self.handle = None

    def _need(self):
        if self.handle is None:
            raise RuntimeError("GR1CS.load(lib, ctx) first")

    @property
    def m(self):
        return self.ell + self.w

    def num_constraints(self) -> int:
        self._need()
        return self.lib.gr1cs_num_constraints(self.handle)

    def _z(self, z):
        """z: canonical ints, or the Montgomery images as bytes"""
        if isinstance(z, (bytes, bytearray, memoryview, np.ndarray)):
            return z, len(z) // 32
        return b"".join(self.curve.fr_mont(v) for v in z), len(z)

    def which_is_unsatisfied(self, z) -> Optional[Tuple[str, int]]:
        """(label, row) of the first unsatisfied constraint -- the two parts of the reference's "<label> - <row>" -- or None"""
        self._need()
        zb, n = self._z(z)
        got = self.lib.gr1cs_which_is_unsatisfied(self.ctx, self.handle, zb, n)
        return None if got is None else (self.predicates[got[0]].label, got[1])

    def is_satisfied(self, z) -> bool:
        return self.which_is_unsatisfied(z) is None

    def mat_vec(self, label: str, z) -> List[bytes]:
        """M_k z for the matrices of `label`: arity byte strings of n Montgomery Fr each"""
        self._need()
        i = self._index[label]
        p = self.predicates[i]
        zb, n = self._z(z)
        return self.lib.gr1cs_mat_vec(self.ctx, self.handle, i, zb, n, p.arity, p.n, 32)

    def eval(self, label: str, z) -> bytes:
        """the polynomial's value on every row of `label` (n Montgomery Fr): zero exactly where the row is satisfied"""
        self._need()
        i = self._index[label]
        zb, n = self._z(z)
        return self.lib.gr1cs_eval(self.ctx, self.handle, i, zb, n, self.predicates[i].n, 32)

    def quotient_dims(self, label: str, log_n: int = 0) -> Tuple[int, int, int, int]:
        """(degree, log_domain, log_ext, h_len) of ``quotient(label, .., log_n)``: the total degree of the polynomial, the
        evaluation domain N = 2^log_domain (``log_n = 0``: the smallest power of two >= max(n, 2)), the extension D = 2^log_ext
        (1 up to degree 2, else next_pow2(degree - 1)) and h_len = D * N.  No device work."""
        self._need()
        return self.lib.gr1cs_quotient_dims(self.handle, self._index[label], log_n)

    def quotient(self, label: str, z, log_n: int = 0) -> bytes:
        """h = P(m_0, .., m_{t-1}) / (X^N - 1) of `label`: h_len Montgomery Fr, the coefficients of the polynomial of degree
        < D N that agrees with the quotient on the coset g H_{DN} (``ark355_gr1cs_quotient``); exact for an assignment that
        satisfies all N rows, the zero rows past n included"""
        self._need()
        i = self._index[label]
        h_len = self.lib.gr1cs_quotient_dims(self.handle, i, log_n)[3]
        zb, n = self._z(z)
        return self.lib.gr1cs_quotient(self.ctx, self.handle, i, zb, n, log_n, h_len, 32)

    def quotient_dev(self, label: str, d_z: int, z_len: int, d_h: int, log_n: int = 0):
        """the same on device pointers: reads z_len Fr at d_z, writes h_len Fr (``quotient_dims``) at d_h and returns when they
        are complete -- ready for ``ark355_msm_dev`` over Montgomery scalars"""
        self._need()
        self.lib.gr1cs_quotient_dev(self.ctx, self.handle, self._index[label], d_z, z_len, log_n, d_h)

    def mat_vec_dev(self, label: str, d_z: int, z_len: int, d_out: int, log_n: int = 0):
        """the values of m_0 .. m_{t-1} of `label` over H_N on device pointers (``ark355_gr1cs_mat_vec_dev``): reads z_len Fr at
        d_z, writes arity x N Fr at d_out, matrix-major, rows n .. N-1 zero (N = 2^log_domain of ``quotient_dims``) -- ready for
        ``Evals.eval_dev`` / ``Evals.div_linear_dev``"""
        self._need()
        self.lib.gr1cs_mat_vec_dev(self.ctx, self.handle, self._index[label], d_z, z_len, log_n, d_out)

    def sumcheck_dev(self, label: str, d_tables: int, d_weight: Optional[int], num_vars: int):
        """a ``Sumcheck`` (snark_amd/poly.py) of ``sum_i W[i] P(T_0[i], .., T_{t-1}[i])`` for the polynomial P of `label`
        (``ark355_gr1cs_sumcheck_begin_dev``): d_tables holds arity x 2^num_vars Fr, matrix-major -- what ``mat_vec_dev`` writes --,
        d_weight 2^num_vars Fr or None for weight 1.  Both are borrowed until the second round returns; this system must stay
        loaded until the run is closed."""
        from .poly import Sumcheck
        self._need()
        return Sumcheck(self.lib, self.ctx, self.lib.gr1cs_sumcheck_begin_dev(self.ctx, self.handle, self._index[label], d_tables, d_weight,
                                                                              num_vars))

    def mat_vec_t(self, label: str, y) -> List[bytes]:
        """M_k^T y for the matrices of `label` (``ark355_gr1cs_mat_vec_t``): arity byte strings of m = ell + w Montgomery Fr
        each, column j the sum of c * y[i] over the stored entries (i, j, c).  y: n canonical ints or Montgomery bytes."""
        self._need()
        i = self._index[label]
        yb, n = self._z(y)
        out = self.lib.gr1cs_mat_vec_t(self.ctx, self.handle, i, yb, n, self.predicates[i].arity * self.m, 32)
        return [out[k * self.m * 32:(k + 1) * self.m * 32] for k in range(self.predicates[i].arity)]

    def mat_vec_t_dev(self, label: str, d_y: int, y_len: int, d_out: int):
        """the same on device pointers: reads y_len >= n Fr at d_y, writes arity * m Fr at d_out, returns when complete"""
        self._need()
        self.lib.gr1cs_mat_vec_t_dev(self.ctx, self.handle, self._index[label], d_y, y_len, d_out)

    def columns_at(self, label: str, tau: int, log_n: int = 0) -> List[bytes]:
        """The column polynomials of `label` at tau (``ark355_gr1cs_columns_at``): arity byte strings of m Montgomery Fr,
        column j of matrix k = sum_i M_k[i][j] L_i(tau) over N = 2^log_n points (``log_n = 0``: as ``quotient_dims``)."""
        self._need()
        i = self._index[label]
        out = self.lib.gr1cs_columns_at(self.ctx, self.handle, i, int(tau).to_bytes(32, "little"), log_n,
                                        self.predicates[i].arity * self.m, 32)
        return [out[k * self.m * 32:(k + 1) * self.m * 32] for k in range(self.predicates[i].arity)]

    def columns_at_dev(self, label: str, tau: int, d_out: int, log_n: int = 0):
        """the same into device memory: arity * m Fr at d_out, complete on return -- ready for
        ``Lib.fixed_base_mul_dev(.., scalars_mont=1)``"""
        self._need()
        self.lib.gr1cs_columns_at_dev(self.ctx, self.handle, self._index[label], int(tau).to_bytes(32, "little"), log_n, d_out)

    def matrices(self, label: str) -> List[Tuple[np.ndarray, np.ndarray, bytes]]:
        """``to_matrices()[label]`` of the resident system: its arity matrices as (row_ptr u64, col u32, coeff Montgomery bytes),
        the shape ``Lib.r1cs_load`` takes, read back from the device (``ark355_gr1cs_matrix``)"""
        self._need()
        i = self._index[label]
        arity, n, nnz = self.lib.gr1cs_pred_dims(self.handle, i)
        return [self.lib.gr1cs_matrix(self.ctx, self.handle, i, k, n, nnz[k], 32) for k in range(arity)]

    def r1cs_handle(self):
        """An ``ark355_r1cs`` handle (for ``Lib.prove``; the caller frees it with ``ark355_r1cs_free``) from the predicate
        labelled "R1CS".  Raises ``Ark355Error`` (EINVAL, naming the label) when any other predicate carries a constraint:
        a proof that silently drops constraints is not obtainable through this path."""
        self._need()
        return self.lib.gr1cs_r1cs(self.ctx, self.handle)
