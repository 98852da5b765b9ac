"""finalize() on the device: a constraint system as the reference holds it *before* ``finalize()`` -- the symbolic linear
combinations of ``LcMap`` (relations/src/gr1cs/lc_map.rs:51-56: three flat arrays), packed ``Variable``s
(utils/variable.rs:4-14) and interned coefficients (field_interner.rs:24-69) -- becomes a resident ``GR1CS``:
``ConstraintSystem::inline_all_lcs`` + ``to_matrices`` (constraint_system.rs:691-804) and, on request, instance outlining
(:826-863, instance_outliner.rs:41-81) run in ``ark355_gr1cs_from_lcs``.

    system = LcSystem.from_constraint_system(curve, cs)      # cs: before finalize()
    g = system.finalize(lib, ctx, outline="R1CS")            # a GR1CS: which_is_unsatisfied, mat_vec, matrices, r1cs_handle
    z2 = outlined_assignment(z, system.ell)                  # the assignment of the outlined system

Rows come back in canonical form (columns strictly ascending, merged, zeros dropped); see include/ark355.h.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np

from ._binding import VAR_TAG_SHIFT
from .gr1cs import GR1CS
from .params import Curve, CURVES

OUTLINE_MODES = {None: 0, 0: 0, "R1CS": 1, 1: 1, "SR1CS": 2, 2: 2}


def pack_variable(tag: int, index: int) -> int:
    """Variable::new (utils/variable.rs:4-14): the tag in the top 3 bits, the payload in the low 61"""
    return (tag << VAR_TAG_SHIFT) | index


class Interner:
    """FieldInterner (field_interner.rs:24-69): entries 0 and 1 are 1 and -1, and one always interns to 0"""

    def __init__(self, p: int):
        self.p = p
        self.vec: List[int] = [1, p - 1]
        self.map: Dict[int, int] = {1: 0, p - 1: 1}

    def get_or_intern(self, value: int) -> int:
        value %= self.p
        if value == 1:
            return 0
        i = self.map.get(value)
        if i is None:
            i = self.map[value] = len(self.vec)
            self.vec.append(value)
        return i


@dataclass
class LcPredicate:
    """One label before to_matrices: the polynomial and ``argument_lcs`` column-wise (arity arrays of packed Variables)"""
    label: str
    arity: int
    terms: List[Tuple[int, List[Tuple[int, int]]]]
    n: int
    args: List[np.ndarray]


@dataclass
class LcSystem:
    curve: Curve
    ell: int                       # instance variables, the constant One included
    w: int
    lc_offsets: np.ndarray         # u64[n_lcs + 1]
    lc_vars: np.ndarray            # u64: packed Variables
    lc_coeffs: np.ndarray          # u32: indices into pool
    pool: List[int]                # canonical integers; pool[0] = 1, pool[1] = -1
    predicates: List[LcPredicate]

    @staticmethod
    def from_constraint_system(curve, cs) -> "LcSystem":
        """cs: any object shaped like the reference's ConstraintSystem before finalize(): num_instance_variables,
        num_witness_variables, lc_map (a list of lists of (coefficient, (tag, index))) and predicates ({label: object with
        .predicate.arity, .predicate.terms, .argument_lcs (arity lists of (tag, index)), .num_constraints})."""
        curve = CURVES[curve] if not isinstance(curve, Curve) else curve
        interner = Interner(curve.r)
        offsets, vars_, coeffs = [0], [], []
        for lc in cs.lc_map:
            for c, (tag, index) in lc:
                vars_.append(pack_variable(tag, index))
                coeffs.append(interner.get_or_intern(c))
            offsets.append(len(vars_))
        preds = []
        for label, pcs in cs.predicates.items():
            arity = pcs.predicate.arity
            args = [np.array([pack_variable(t, i) for t, i in column], dtype=np.uint64) for column in pcs.argument_lcs]
            preds.append(LcPredicate(label, arity, [(c, list(f)) for c, f in pcs.predicate.terms], pcs.num_constraints, args))
        return LcSystem(curve, cs.num_instance_variables, cs.num_witness_variables, np.array(offsets, dtype=np.uint64),
                        np.array(vars_, dtype=np.uint64), np.array(coeffs, dtype=np.uint32), interner.vec, preds)

    @property
    def n_lcs(self) -> int:
        return len(self.lc_offsets) - 1

    def pool_bytes(self) -> bytes:
        return b"".join(self.curve.fr_mont(v) for v in self.pool)

    def _descs(self):
        out = []
        for p in self.predicates:
            term_ptr, var, exp = [0], [], []
            for _, factors in p.terms:
                var += [v for v, _ in factors]
                exp += [e for _, e in factors]
                term_ptr.append(len(var))
            out.append((p.label, p.arity, p.n, b"".join(self.curve.fr_mont(c) for c, _ in p.terms),
                        np.array(term_ptr, dtype=np.uint32), np.array(var, dtype=np.uint32), np.array(exp, dtype=np.uint32), p.args))
        return out

    def finalize(self, lib, ctx, outline=None) -> GR1CS:
        """outline: None, "R1CS" (outline_r1cs) or "SR1CS" (outline_sr1cs).  The caller frees the result (``GR1CS.free``)."""
        if outline not in OUTLINE_MODES:
            raise ValueError("outline must be None, 'R1CS' or 'SR1CS'")
        handle = lib.gr1cs_from_lcs(ctx, self.curve.curve_id, self.ell, self.w, self.lc_offsets, self.lc_vars, self.lc_coeffs,
                                    self.pool_bytes(), self._descs(), OUTLINE_MODES[outline])
        return GR1CS.from_handle(self.curve, lib, ctx, handle, [(p.label, p.terms) for p in self.predicates])


def outlined_assignment(z: Sequence, ell: int) -> list:
    """z' = z || 1 || z[1 .. ell): the assignment of the outlined system (instance_outliner.rs: one witness copy of One and
    of every instance variable).  z: canonical integers, or the 32-byte Montgomery images as a list."""
    z = list(z)
    return z + [z[0]] + z[1:ell]
