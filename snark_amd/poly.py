"""Polynomial openings on the device (``include/ark355.h`` "Polynomial openings", ``csrc/poly_impl.cuh``): what a KZG-style
prover does with a challenge once it has committed -- evaluate (ark-poly ``DensePolynomial::evaluate``), divide by ``X - x``
(ark-poly-commit ``KZG10::compute_witness_polynomial``) and combine (``DensePolynomial``'s ``Add`` / ``Mul<F>``).

Polynomials are Montgomery Fr coefficients, 32 bytes each, ``count`` polynomials of ``length`` coefficients back to back;
points and scalars are Python integers below r.  The ``_dev`` forms take device pointers (ints) of the calling process, e.g.
``torch.Tensor.data_ptr()``, and return when the output is complete, so that ``GR1CS.quotient_dev`` -> ``Poly.eval_dev`` ->
``Poly.div_linear_dev`` -> ``ark355_msm_dev`` never visits the host."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

from . import lib as _lib
from .params import CURVES, Curve


def _canon(v: int) -> bytes:
    return int(v).to_bytes(32, "little")


class Poly:
    def __init__(self, curve="bls12_381", lib=None, ctx=None, device: int = 0):
        """``lib`` / ``ctx`` are injectable so that tests drive this over the CPU emulator build, or share a context; by
        default the HIP library is loaded and a context of its own is created (and destroyed by ``close``)."""
        self.curve: Curve = CURVES[curve] if not isinstance(curve, Curve) else curve
        self.lib = lib if lib is not None else _lib()
        self._own_ctx = ctx is None
        self.ctx = self.lib.ctx_create(device) if ctx is None else ctx

    def close(self):
        if self._own_ctx and self.ctx is not None:
            self.lib.ctx_destroy(self.ctx)
        self.ctx = None

    # ---- host forms ------------------------------------------------------------------------------------------------
    def eval(self, coeffs: bytes, length: int, x: int, count: int = 1) -> bytes:
        """p_k(x) for k < count: count Montgomery Fr"""
        return self.lib.poly_eval_fr(self.ctx, self.curve.curve_id, coeffs, length, count, _canon(x))

    def div_linear(self, coeffs: bytes, length: int, x: int, count: int = 1, want_rem: bool = True) -> Tuple[bytes, Optional[bytes]]:
        """(q, rem) with p_k(X) = q_k(X) (X - x) + rem_k; q in the layout of the input"""
        return self.lib.poly_div_linear_fr(self.ctx, self.curve.curve_id, coeffs, length, count, _canon(x), want_rem)

    def lincomb(self, polys: bytes, length: int, scalars: Sequence[int]) -> bytes:
        """sum_k scalars[k] polys[k]: ``length`` Montgomery Fr"""
        return self.lib.poly_lincomb_fr(self.ctx, self.curve.curve_id, polys, length, len(scalars), b"".join(_canon(s) for s in scalars))

    # ---- device forms ----------------------------------------------------------------------------------------------
    def eval_dev(self, d_coeffs: int, length: int, x: int, d_out: int, count: int = 1) -> None:
        self.lib.poly_eval_fr_dev(self.ctx, self.curve.curve_id, d_coeffs, length, count, _canon(x), d_out)

    def div_linear_dev(self, d_coeffs: int, length: int, x: int, d_q_out: int, d_rem_out: Optional[int] = None, count: int = 1) -> None:
        """``d_q_out == d_coeffs`` divides in place; ``d_rem_out`` may be None"""
        self.lib.poly_div_linear_fr_dev(self.ctx, self.curve.curve_id, d_coeffs, length, count, _canon(x), d_q_out, d_rem_out)

    def lincomb_dev(self, d_polys: int, length: int, scalars: Sequence[int], d_out: int) -> None:
        """``d_out == d_polys`` combines in place on polynomial 0"""
        self.lib.poly_lincomb_fr_dev(self.ctx, self.curve.curve_id, d_polys, length, len(scalars), b"".join(_canon(s) for s in scalars),
                                     d_out)


class Evals:
    """The same openings for polynomials held in the evaluation basis (``include/ark355.h`` "Openings in the evaluation basis",
    ``csrc/evals_impl.cuh``): ``count`` vectors of ``2^log_n`` Montgomery values over the domain of ``ark355_ntt_fr`` (``coset``:
    over its coset), back to back.  No transform runs: ``GR1CS.mat_vec_dev`` -> ``Evals.eval_dev`` -> ``Evals.div_linear_dev`` ->
    ``ark355_msm_dev`` over a Lagrange-basis key never visits the host."""

    def __init__(self, curve="bls12_381", lib=None, ctx=None, device: int = 0):
        self.curve: Curve = CURVES[curve] if not isinstance(curve, Curve) else curve
        self.lib = lib if lib is not None else _lib()
        self._own_ctx = ctx is None
        self.ctx = self.lib.ctx_create(device) if ctx is None else ctx

    def close(self):
        if self._own_ctx and self.ctx is not None:
            self.lib.ctx_destroy(self.ctx)
        self.ctx = None

    # ---- host forms ------------------------------------------------------------------------------------------------
    def eval(self, evals: bytes, log_n: int, x: int, count: int = 1, coset: bool = False) -> bytes:
        """p_k(x) for k < count: count Montgomery Fr"""
        return self.lib.evals_eval_fr(self.ctx, self.curve.curve_id, evals, log_n, count, int(coset), _canon(x))

    def div_linear(self, evals: bytes, log_n: int, x: int, count: int = 1, coset: bool = False,
                   want_rem: bool = True) -> Tuple[bytes, Optional[bytes]]:
        """(q, rem): the values of (p_k - p_k(x)) / (X - x) over the same domain, and rem_k = p_k(x)"""
        return self.lib.evals_div_linear_fr(self.ctx, self.curve.curve_id, evals, log_n, count, int(coset), _canon(x), want_rem)

    # ---- device forms ----------------------------------------------------------------------------------------------
    def eval_dev(self, d_evals: int, log_n: int, x: int, d_out: int, count: int = 1, coset: bool = False) -> None:
        self.lib.evals_eval_fr_dev(self.ctx, self.curve.curve_id, d_evals, log_n, count, int(coset), _canon(x), d_out)

    def div_linear_dev(self, d_evals: int, log_n: int, x: int, d_q_out: int, d_rem_out: Optional[int] = None, count: int = 1,
                       coset: bool = False) -> None:
        """``d_q_out == d_evals`` divides in place; ``d_rem_out`` may be None"""
        self.lib.evals_div_linear_fr_dev(self.ctx, self.curve.curve_id, d_evals, log_n, count, int(coset), _canon(x), d_q_out, d_rem_out)


class Mle:
    """Multilinear extensions on the device (``include/ark355.h`` "Multilinear extensions", ``csrc/mle_impl.cuh``): tables of
    ``2^num_vars`` Montgomery Fr over the Boolean hypercube, variable 0 the lowest index bit (ark-poly's
    ``DenseMultilinearExtension``).  Points are sequences of Python integers below r and stay on the host; the ``_dev`` forms take
    device pointers (ints) for the tables and the outputs: ``GR1CS.mat_vec_dev`` -> ``Mle.eq_dev`` -> ``GR1CS.sumcheck_dev`` ->
    ``Mle.eval_dev`` never visits the host with a table, and ``Mle.open_dev`` opens a committed table at the point the sum-check
    ends at (PST13, ark-poly-commit's ``MultilinearPC::open``) against a key from ``Mle.commit_key``."""

    def __init__(self, curve="bls12_381", lib=None, ctx=None, device: int = 0):
        self.curve: Curve = CURVES[curve] if not isinstance(curve, Curve) else curve
        self.lib = lib if lib is not None else _lib()
        self._own_ctx = ctx is None
        self.ctx = self.lib.ctx_create(device) if ctx is None else ctx

    def close(self):
        if self._own_ctx and self.ctx is not None:
            self.lib.ctx_destroy(self.ctx)
        self.ctx = None

    @staticmethod
    def _point(point: Sequence[int]) -> bytes:
        return b"".join(_canon(v) for v in point)

    # ---- host forms ------------------------------------------------------------------------------------------------
    def eq(self, point: Sequence[int]) -> bytes:
        """eq(point, i) for i < 2^len(point): Montgomery Fr"""
        return self.lib.mle_eq_fr(self.ctx, self.curve.curve_id, len(point), self._point(point))

    def fix(self, evals: bytes, num_vars: int, point: Sequence[int], count: int = 1) -> bytes:
        """variables 0 .. len(point)-1 of ``count`` tables fixed to ``point``: count x 2^(num_vars - len(point)) Montgomery Fr"""
        return self.lib.mle_fix_fr(self.ctx, self.curve.curve_id, evals, num_vars, count, self._point(point), len(point))

    def eval(self, evals: bytes, num_vars: int, point: Sequence[int], count: int = 1) -> bytes:
        """f~_k(point) for k < count (``len(point) == num_vars``): count Montgomery Fr"""
        assert len(point) == num_vars
        return self.lib.mle_eval_fr(self.ctx, self.curve.curve_id, evals, num_vars, count, self._point(point))

    # ---- device forms ----------------------------------------------------------------------------------------------
    def eq_dev(self, point: Sequence[int], d_out: int) -> None:
        self.lib.mle_eq_fr_dev(self.ctx, self.curve.curve_id, len(point), self._point(point), d_out)

    def fix_dev(self, d_evals: int, num_vars: int, point: Sequence[int], d_out: int, count: int = 1) -> None:
        """``d_out`` may not overlap ``d_evals``"""
        self.lib.mle_fix_fr_dev(self.ctx, self.curve.curve_id, d_evals, num_vars, count, self._point(point), len(point), d_out)

    def eval_dev(self, d_evals: int, num_vars: int, point: Sequence[int], d_out: int, count: int = 1) -> None:
        assert len(point) == num_vars
        self.lib.mle_eval_fr_dev(self.ctx, self.curve.curve_id, d_evals, num_vars, count, self._point(point), d_out)


    # ---- openings (csrc/mle_open_impl.cuh) ---------------------------------------------------------------------------
    @staticmethod
    def level(num_vars: int, j: int) -> Tuple[int, int]:
        """(offset, length) in elements of quotient level ``j`` inside one table's ``2^num_vars`` output elements"""
        assert 0 <= j < num_vars
        n = 1 << num_vars
        return n - (n >> j), n >> (j + 1)

    def quotients(self, evals: bytes, num_vars: int, point: Sequence[int], count: int = 1, want_rem: bool = True) -> Tuple[bytes, Optional[bytes]]:
        """(q, rem): the PST quotient tables ``q_j[i] = f^(j)[2i+1] - f^(j)[2i]`` of ``count`` tables at ``point``, count x 2^num_vars
        Montgomery Fr -- level j of a table at ``level(num_vars, j)``, ``f~(point)`` in the table's last element -- and the values"""
        assert len(point) == num_vars
        return self.lib.mle_quotients_fr(self.ctx, self.curve.curve_id, evals, num_vars, count, self._point(point), want_rem)

    def quotients_dev(self, d_evals: int, num_vars: int, point: Sequence[int], d_q_out: int, d_rem_out: Optional[int] = None,
                      count: int = 1) -> None:
        """no two of the three ranges may overlap; ``d_rem_out`` may be None"""
        assert len(point) == num_vars
        self.lib.mle_quotients_fr_dev(self.ctx, self.curve.curve_id, d_evals, num_vars, count, self._point(point), d_q_out, d_rem_out)

    def open_dev(self, level_bases, d_evals: int, num_vars: int, point: Sequence[int], group: int = 1) -> Tuple[bytes, bytes]:
        """(proofs, value): ``num_vars`` affine points ``pi_j = <q_j, level_bases[j]>`` of group ``group`` and ``f~(point)``; the
        handles are what ``commit_key`` returns, the quotients never leave the context's scratch"""
        assert len(point) == num_vars and len(level_bases) >= num_vars
        size = self.lib.sizes(self.curve.curve_id)["g1" if group == 1 else "g2"]
        return self.lib.mle_open_dev(self.ctx, self.curve.curve_id, list(level_bases[:num_vars]), d_evals, num_vars, self._point(point), size)

    def commit_dev(self, handle, d_tables: int, num_vars: int, count: int = 1, group: int = 1) -> bytes:
        """The commitments ``<f_k, handle>`` to ``count`` resident tables of ``2^num_vars`` Montgomery Fr, back to back at
        ``d_tables``, with one key (``commit`` of ``commit_key``): ``count`` affine points of group ``group`` from ONE call of
        ``ark355_msm_batch_dev`` -- byte for byte what ``ark355_msm_dev`` returns table by table"""
        size = self.lib.sizes(self.curve.curve_id)["g1" if group == 1 else "g2"]
        n = 1 << num_vars
        return self.lib.msm_batch_dev(self.ctx, [handle] * count, [d_tables + 32 * n * k for k in range(count)], [n] * count, 1, size)

    def commit_key(self, group: int, base: bytes, t: Sequence[int], alloc=None):
        """The PST key of ``len(t)`` variables over the trapdoor ``t``: ``(commit, levels)``, resident base handles
        (``ark355_bases_free`` each).  ``commit`` holds the 2^v points ``eq(t, i) base``, so that ``ark355_msm_dev`` of a table
        against it is the commitment ``[f~(t)] base``; ``levels[j]`` holds the 2^(v-1-j) points ``eq((t_{j+1} .. t_{v-1}), i) base``
        that ``open_dev`` pairs with quotient level j.  Built from ``eq_dev``, ``fixed_base_mul_dev`` and ``bases_load``; the points
        pass through host memory, which key generation can afford.  ``alloc(nbytes) -> (device pointer, keepalive)`` supplies the
        device memory of the eq tables; by default a torch tensor."""
        if alloc is None:
            def alloc(nbytes):
                import torch
                buf = torch.empty((max(1, nbytes),), dtype=torch.uint8, device="cuda")
                return buf.data_ptr(), buf
        cid = self.curve.curve_id
        size = self.lib.sizes(cid)["g1" if group == 1 else "g2"]
        v = len(t)
        d_eq, keep = alloc(32 << v)

        def handle(suffix):
            n = 1 << len(suffix)
            self.eq_dev(suffix, d_eq)
            points = self.lib.fixed_base_mul_dev(self.ctx, cid, group, base, d_eq, n, True, size)
            return self.lib.bases_load(self.ctx, cid, group, points, n)

        handles = []
        try:
            handles.append(handle(list(t)))
            for j in range(v):
                handles.append(handle(list(t[j + 1:])))
        except Exception:
            for h in handles:
                self.lib.dll.ark355_bases_free(h)
            raise
        del keep
        return handles[0], handles[1:]


class Sumcheck:
    """One sum-check run of a predicate over resident tables (``include/ark355.h`` "Sum-check of a GR1CS predicate",
    ``csrc/sumcheck_impl.cuh``); made by ``GR1CS.sumcheck_dev``.  ``round(None)`` is round 1, ``round(r_j)`` every later one,
    ``finish(r_v)`` returns the tables and the weight at the point of the challenges.  The caller's device memory is borrowed
    until the second ``round`` returns; the GR1CS it came from must stay loaded until ``close``."""

    def __init__(self, lib, ctx, handle):
        self.lib, self.ctx, self.handle = lib, ctx, handle

    def info(self) -> Tuple[int, int, int, int]:
        """(num_vars, arity, points, rounds_done)"""
        return self.lib.sumcheck_info(self.handle)

    def round(self, challenge: Optional[int] = None) -> bytes:
        """the next round's message g(0) .. g(D): ``points`` Montgomery Fr"""
        points = self.info()[2]
        return self.lib.sumcheck_round(self.ctx, self.handle, None if challenge is None else _canon(challenge), points)

    def finish(self, challenge: Optional[int] = None) -> bytes:
        """T_0 .. T_{t-1}, W at (r_1 .. r_v): arity + 1 Montgomery Fr (``challenge`` is None exactly when num_vars = 0)"""
        arity = self.info()[1]
        return self.lib.sumcheck_finish(self.ctx, self.handle, None if challenge is None else _canon(challenge), arity)

    def close(self):
        if self.handle is not None:
            self.lib.sumcheck_free(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
