"""Square R1CS on the device: the reference's ``Sr1csAdapter`` (relations/src/sr1cs/mod.rs:124-265) over a resident R1CS.

``Sr1csAdapter::r1cs_to_sr1cs`` (setup) and ``r1cs_to_sr1cs_with_assignment`` (prove) rewrite an R1CS system -- and its
assignment -- into one over the ``"SR1CS"`` predicate ``x0^2 - x1``, the input of the GM17-style provers (Polymath, Garuda,
Pari).  ``SR1CS.from_r1cs`` builds that system on the device from an ``ark355_r1cs`` handle, without the matrices visiting the
host; ``assignment`` maps a full R1CS assignment to the SR1CS one in two launches.  ``system`` is an ordinary ``GR1CS`` over the
resident result: ``which_is_unsatisfied``, ``mat_vec`` and ``eval`` work on it as on any loaded system.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from .gr1cs import GR1CS, Predicate
from .params import Curve, CURVES

SR1CS_PREDICATE_LABEL = "SR1CS"        # predicate/polynomial_constraint.rs


class _BorrowedGR1CS(GR1CS):
    """The system inside an ``ark355_sr1cs`` handle: it lives and dies with that handle, so ``free`` does nothing."""

    def free(self):
        pass

    def load(self, lib, ctx):
        raise RuntimeError("the system of an SR1CS handle is already resident")


class SR1CS:
    def __init__(self, curve: Optional[Curve], lib, ctx, handle, source_m: Optional[int]):
        self.curve, self.lib, self.ctx, self.handle, self.source_m = curve, lib, ctx, handle, source_m
        self._system: Optional[GR1CS] = None

    @staticmethod
    def from_r1cs(lib, ctx, r1cs_handle, curve=None, num_variables: Optional[int] = None) -> "SR1CS":
        """r1cs_handle: an ``ark355_r1cs`` (``Lib.r1cs_load``, ``GR1CS.r1cs_handle``); it may be freed afterwards.  The handle
        is opaque, so what Python needs beyond it comes from the caller: ``curve`` to take assignments as canonical integers
        (Montgomery bytes need none), ``num_variables`` (num_instance + num_witness of the R1CS) for ``var_map``."""
        if curve is not None and not isinstance(curve, Curve):
            curve = CURVES[curve]
        return SR1CS(curve, lib, ctx, lib.sr1cs_from_r1cs(ctx, r1cs_handle), num_variables)

    def free(self):
        if self.handle is not None:
            self.lib.sr1cs_free(self.handle)
            self.handle = None
            self._system = None

    def _need(self):
        if self.handle is None:
            raise RuntimeError("this SR1CS has been freed")

    @property
    def dims(self) -> Tuple[int, int, int, Tuple[int, int]]:
        """(num_instance', num_witness', rows = 2n + P, (non-zeros of M0, of M1))"""
        self._need()
        return self.lib.sr1cs_dims(self.handle)

    def var_map(self) -> Tuple[np.ndarray, np.ndarray]:
        """(witness_col, instance_col) over the old columns: the column of each one's witness copy (0 for One, -1 when it never
        occurs) and the new input of a public that occurs (-1 otherwise)"""
        self._need()
        if self.source_m is None:
            raise RuntimeError("SR1CS.from_r1cs(..., num_variables=num_instance + num_witness) to size the maps")
        return self.lib.sr1cs_var_map(self.ctx, self.handle, self.source_m)

    def matrices(self) -> List[Tuple[np.ndarray, np.ndarray, bytes]]:
        """[M0, M1] as (row_ptr u64, col u32, coeff Montgomery bytes), the shape ``Lib.r1cs_load`` takes"""
        self._need()
        _, _, rows, nnz = self.dims
        return [self.lib.sr1cs_matrix(self.ctx, self.handle, k, rows, nnz[k], 32) for k in range(2)]

    def assignment(self, z) -> bytes:
        """the SR1CS assignment (Montgomery bytes, num_instance' + num_witness' elements) of a full R1CS assignment z
        (canonical ints, or Montgomery bytes)"""
        self._need()
        if isinstance(z, (bytes, bytearray, memoryview, np.ndarray)):
            zb, n = z, len(z) // 32
        else:
            if self.curve is None:
                raise RuntimeError("SR1CS.from_r1cs(..., curve=...) to pass an assignment as integers")
            zb, n = b"".join(self.curve.fr_mont(v) for v in z), len(z)
        ell, w, _, _ = self.dims
        return self.lib.sr1cs_assignment(self.ctx, self.handle, zb, n, ell + w, 32)

    def assignment_dev(self, d_z: int, z_len: int, d_z_out: int):
        """device pointers: z (z_len elements) -> z' (num_instance' + num_witness' elements, all written)"""
        self._need()
        self.lib.sr1cs_assignment_dev(self.ctx, self.handle, d_z, z_len, d_z_out)

    @property
    def system(self) -> GR1CS:
        """a ``GR1CS`` view over the borrowed handle (its ``free()`` does nothing; it dies with this object)"""
        self._need()
        if self._system is None:
            ell, w, rows, _ = self.dims
            terms = [(1, [(0, 2)]), (self.curve.r - 1, [(1, 1)])] if self.curve is not None else []
            pred = Predicate(SR1CS_PREDICATE_LABEL, 2, terms, rows, [], [], [])
            g = _BorrowedGR1CS(self.curve, ell, w, [pred])
            g.lib, g.ctx, g.handle = self.lib, self.ctx, self.lib.sr1cs_system(self.handle)
            g._index = {SR1CS_PREDICATE_LABEL: 0}
            self._system = g
        return self._system
