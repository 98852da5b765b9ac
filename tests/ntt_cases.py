"""Transform cases shared by the CPU-emulator tier and the GPU tier: every plan of the pass planner (ntt_radices / ntt_p_log in
csrc/ntt_impl.cuh), inputs whose transform is known in closed form, the planner's policies, and the device-pointer entry
`ark355_ntt_fr_dev`.  The reference is the C oracle (oracle/c) and Python integers, never a second call into the library; the
one "policy A == policy B" comparison comes on top of an oracle comparison."""
from __future__ import annotations

import numpy as np

import parity_cases as pc
from field_edge_cases import pattern_values
from helpers import z_bytes
from oracle import synthetic as S
from oracle.c import cbase
from oracle.ntt import Domain

MODES = ((0, 0), (1, 0), (0, 1), (1, 1))          # (inverse, coset)

# cb_ntt costs seconds from 2^22 points: one result per (curve, size, seed, mode) is kept for the cases that share an input
# (up to 2^24: 512 MiB each)
_ORACLE = {}
_ORACLE_LOGS, _ORACLE_MAX = (22, 23, 24), 6


def random_vector(C, log_n, seed):
    """2^log_n valid residues as Montgomery images (any value below r is the image of some element)"""
    n = 1 << log_n
    rng = np.random.default_rng(seed * 100 + log_n)
    raw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    raw[:, 3] &= np.uint64((1 << (C.r.bit_length() - 1 - 192)) - 1)      # < 2^(bits-1) < r
    return raw.astype("<u8").tobytes()


def oracle_ntt(C, data, log_n, seed, inv, cos):
    if log_n not in _ORACLE_LOGS:
        return cbase.ntt(C, data, log_n, bool(inv), bool(cos))
    k = (C.name, log_n, seed, inv, cos)
    if k not in _ORACLE:
        while len(_ORACLE) >= _ORACLE_MAX:
            _ORACLE.pop(next(iter(_ORACLE)))
        _ORACLE[k] = cbase.ntt(C, data, log_n, bool(inv), bool(cos))
    return _ORACLE[k]


def first_difference(got, exp):
    """(element index, count of differing elements) for an assertion message"""
    a = np.frombuffer(got, dtype=np.uint8).reshape(-1, 32)
    b = np.frombuffer(exp, dtype=np.uint8).reshape(-1, 32)
    bad = np.nonzero((a != b).any(axis=1))[0]
    return (int(bad[0]), int(bad.size)) if bad.size else None


def ntt_full_case(lib, ctx, C, log_n, modes=MODES, seed=5):
    """ark355_ntt_fr vs cb_ntt, every element"""
    data = random_vector(C, log_n, seed)
    for inv, cos in modes:
        got = lib.ntt(ctx, C.curve_id, data, log_n, inv, cos)
        exp = oracle_ntt(C, data, log_n, seed, inv, cos)
        assert got == exp, (C.name, log_n, inv, cos, first_difference(got, exp))


# ---- inputs whose transform needs no oracle -----------------------------------------------------------------------------------
def _powers(base, n, r, first=1):
    out, p = [], first % r
    for _ in range(n):
        out.append(p)
        p = p * base % r
    return out


def _batch_inverse(xs, r):
    pref, acc = [], 1
    for x in xs:
        acc = acc * x % r
        pref.append(acc)
    inv = pow(acc, -1, r)
    out = [0] * len(xs)
    for k in range(len(xs) - 1, -1, -1):
        out[k] = inv * (pref[k - 1] if k else 1) % r
        inv = inv * xs[k] % r
    return out


class ClosedForms:
    """Transforms of a few vectors in Python integers, from the definitions: X_k = sum_j x_j w^(jk); the inverse with w^-1 and
    1/N; coset forward = forward of x_j g^j; coset inverse = inverse, then times g^-k."""

    def __init__(self, C, log_n):
        self.d = Domain(C, log_n)
        self.r, self.n = C.r, 1 << log_n
        d, r, n = self.d, self.r, self.n
        # sum_j (g w^k)^j = (g^N - 1) / (g w^k - 1): the coset transform of the all-ones vector (g w^k is never 1)
        num = (pow(d.g, n, r) - 1) % r
        self.coset_of_ones = [num * v % r for v in _batch_inverse([(x - 1) % r for x in _powers(d.omega, n, r, d.g)], r)]

    def zero(self, inv, cos):
        return [0] * self.n

    def constant(self, c, inv, cos):
        if not inv and cos:
            return [c * v % self.r for v in self.coset_of_ones]
        out = [0] * self.n
        out[0] = c % self.r if inv else self.n * c % self.r
        return out

    def delta(self, v, j, inv, cos):
        d, r, n = self.d, self.r, self.n
        if not inv:
            first = v * pow(d.g, j, r) if cos else v
            return _powers(pow(d.omega, j, r), n, r, first)
        step = pow(d.omega_inv, j, r) * (d.g_inv if cos else 1) % r
        return _powers(step, n, r, v * d.n_inv)

    def alternating(self, inv, cos):
        """x_j = (-1)^j = w^(j N/2)"""
        r, n = self.r, self.n
        if not inv and cos:
            return [self.coset_of_ones[(k + n // 2) % n] for k in range(n)]
        out = [0] * n
        out[n // 2] = (pow(self.d.g_inv, n // 2, r) if cos else 1) if inv else n % r
        return out


def structured_case(lib, ctx, C, log_n):
    """Zero, constant r - 1, deltas of r - 1, alternating (1, r - 1, ..) and a cycle of the multiplier's pattern values: every
    butterfly sees a + b with a = b = r - 1, a - b = 0, products with 0 and with -1.  Four modes; against cb_ntt AND against
    the closed form in Python integers (the pattern cycle, which has none: against the Python oracle's radix-2 transform)."""
    r, n = C.r, 1 << log_n
    cf = ClosedForms(C, log_n)
    d = cf.d
    vals = pattern_values(C)
    cycle = [vals[i % len(vals)] for i in range(n)]
    python_ntt = {(0, 0): d.fft, (1, 0): d.ifft, (0, 1): d.coset_fft, (1, 1): d.coset_ifft}
    vectors = [("zero", [0] * n, cf.zero),
               ("constant r-1", [r - 1] * n, lambda inv, cos: cf.constant(r - 1, inv, cos)),
               ("alternating", [1, r - 1] * (n // 2), cf.alternating),
               ("pattern cycle", cycle, lambda inv, cos: python_ntt[(inv, cos)](cycle))]
    for j in sorted({0, 1, n // 2, n - 1}):
        vec = [0] * n
        vec[j] = r - 1
        vectors.append(("delta at %d" % j, vec, lambda inv, cos, j=j: cf.delta(r - 1, j, inv, cos)))
    for name, vec, closed in vectors:
        data = z_bytes(C, vec)
        for inv, cos in MODES:
            got = lib.ntt(ctx, C.curve_id, data, log_n, inv, cos)
            exp = cbase.ntt(C, data, log_n, bool(inv), bool(cos))
            assert got == exp, (C.name, log_n, name, inv, cos, "vs cb_ntt", first_difference(got, exp))
            exp = z_bytes(C, closed(inv, cos))
            assert got == exp, (C.name, log_n, name, inv, cos, "vs closed form", first_difference(got, exp))


# ---- planner policies -----------------------------------------------------------------------------------------------------------
POLICY_CIRCUITS = (5, 60, 250, 900, 3000, 9000)


def policy_sweep_case(lib, ctx, C, seed=1):
    """What the caller's policy (NTT_RMAX / NTT_DIRECT_MAX / NTT_NOFUSE) must not change: the four transforms at 2^1 .. 2^12
    and the R1CS operations + witness map of mulchain circuits with domains 2^3 .. 2^14, all against the Python oracle."""
    for log_n in range(1, 13):
        pc.ntt_case(lib, ctx, C, log_n, seed=seed)
    for n in POLICY_CIRCUITS:
        pc.r1cs_case(lib, ctx, C, *S.mulchain_direct(C.r, n))


def nofuse_equals_fused_case(lib, ctx, policy, C):
    """The witness map with the inverse -> coset seam fused (default) and as two transforms (NTT_NOFUSE = 1): the oracle's h,
    and the same bytes both ways."""
    for n in POLICY_CIRCUITS:
        n_, ell, w, mats, z = S.mulchain_csr(C.r, n)
        zb = S._mont_bytes(C.r, z)
        rh = lib.r1cs_load(ctx, C.curve_id, n_, ell, w, mats)
        try:
            assert lib.ctx_get_policy(ctx, "NTT_NOFUSE") == 0
            fused = lib.witness_map(ctx, rh, zb, len(z), 32)
            assert fused == cbase.witness_map(C, n_, ell, w, mats, zb), (C.name, n, "fused vs oracle/c")
            policy.setenv("ARK355_NTT_NOFUSE", "1")
            try:
                unfused = lib.witness_map(ctx, rh, zb, len(z), 32)
            finally:
                policy.setenv("ARK355_NTT_NOFUSE", "0")
            assert unfused == fused, (C.name, n, "NTT_NOFUSE=1 vs fused", first_difference(unfused, fused))
        finally:
            lib.dll.ark355_r1cs_free(rh)


# ---- ark355_ntt_fr_dev ------------------------------------------------------------------------------------------------------------
GUARD = 4096
DATA_FILL, SCRATCH_FILL = 0xA5, 0x5A


class HostBuffers:
    """The emulator's "device": host memory, one stream (the context's own), nothing to wait for.  The GPU tier has the same
    interface over torch device tensors (tests/test_gpu_shapes.py).  A buffer is GUARD bytes of `fill`, the payload, GUARD
    bytes of `fill` inside ONE allocation; ptr addresses the payload."""

    streams = (None,)

    def guarded(self, payload, nbytes, fill, stream):
        a = np.full(nbytes + 2 * GUARD, fill, dtype=np.uint8)
        if payload is not None:
            a[GUARD:GUARD + nbytes] = np.frombuffer(payload, dtype=np.uint8)
        return a.ctypes.data + GUARD, a

    def before_call(self, stream):
        pass

    def stream_handle(self, stream):
        return None

    def after_call(self, stream):
        pass

    def read(self, buf, stream):
        return buf


def ntt_dev_case(lib, ctx, C, log_n, dev, modes=MODES, seed=5):
    """ark355_ntt_fr_dev: in place on device pointers, on each stream of `dev`.  d_data must hold the oracle's vector (for the
    tiny kernel and for odd pass counts the passes end on the scratch side and are copied back); the guard bytes around BOTH
    buffers must be untouched; the content of d_scratch is unspecified and not looked at."""
    data = random_vector(C, log_n, seed)
    nbytes = len(data)
    for inv, cos in modes:
        exp = oracle_ntt(C, data, log_n, seed, inv, cos)
        for stream in dev.streams:
            d_ptr, d_buf = dev.guarded(data, nbytes, DATA_FILL, stream)
            s_ptr, s_buf = dev.guarded(None, nbytes, SCRATCH_FILL, stream)
            dev.before_call(stream)
            lib.ntt_dev(ctx, C.curve_id, d_ptr, s_ptr, log_n, inv, cos, stream=dev.stream_handle(stream))
            dev.after_call(stream)
            d = dev.read(d_buf, stream)
            s = dev.read(s_buf, stream)
            where = (C.name, log_n, inv, cos, "stream" if stream is not None else "context stream")
            got = d[GUARD:GUARD + nbytes].tobytes()
            assert got == exp, where + ("d_data vs cb_ntt", first_difference(got, exp))
            assert (d[:GUARD] == DATA_FILL).all() and (d[GUARD + nbytes:] == DATA_FILL).all(), where + ("guards of d_data",)
            assert (s[:GUARD] == SCRATCH_FILL).all() and (s[GUARD + nbytes:] == SCRATCH_FILL).all(), where + ("guards of d_scratch",)
