"""Call SEQUENCES on dirty scratch, shared by the CPU-emulator tier (tests/test_emul_dirty.py) and the GPU tier
(tests/test_gpu_dirty.py).

Every scratch buffer of the library grows and is never shrunk or cleared as a whole (DevBuf::ensure): a small call after a large
one runs on the large call's residue -- plausible keys, counts, bucket slots, verdict and status bytes -- and what has to be
cleared is listed by hand in the host drivers.  The other modules check each operation at its own edge shapes in a context whose
history nobody chose; here ONE fresh context per module (policy POISON_ALLOC set, so that no first use passes on zero pages) runs
each family as large, small, small with other data, large again, plus the degenerate sizes and one host-side refusal followed
by a good call.  Every step is compared with the oracle (oracle/, oracle/c, or a known discrete log), never with another run of
the library."""
from __future__ import annotations

import random

import gr1cs_cases as gc
import lcmap_cases as lc
import ntt_cases as nc
import o3_cases as O
import pairing_cases as pg
import pairing_each_cases as pe
import pvk_cases as pv
import quotient_cases as qc
import setup_cases as su
import sr1cs_cases as sc
import verify_bytes_cases as vb
from helpers import fr_vec_from_mont, z_bytes
from oracle import r1cs as R, serialize as Z, synthetic as S
from oracle.c import cbase
from oracle.curves import g1, g2
from snark_amd._binding import Ark355Error, EINVAL, ENOMEM

POISON = 0xA5
E_ASSIGNMENT_MISSING, E_UNSATISFIABLE = -16, -17


class Policy:
    """monkeypatch.setenv-shaped access to the context's policy, as the `*_policy` fixtures of conftest.py give it"""

    def __init__(self, lib, ctx):
        self.lib, self.ctx, self.saved = lib, ctx, []

    def setenv(self, name, value):
        assert name.startswith("ARK355_")
        name = name[len("ARK355_"):]
        self.saved.append((name, self.lib.ctx_get_policy(self.ctx, name)))
        self.lib.ctx_set_policy(self.ctx, name, int(value))

    def set(self, **kw):
        for k, v in kw.items():
            self.setenv("ARK355_" + k, v)

    def restore(self):
        for name, old in reversed(self.saved):
            self.lib.ctx_set_policy(self.ctx, name, old)
        self.saved = []


class Tier:
    """library, the module's fresh context, how bytes reach "device" memory, and the sizes of the tier"""

    def __init__(self, lib, ctx, io, ntt_buffers, emul):
        self.lib, self.ctx, self.io, self.ntt_buffers, self.emul = lib, ctx, io, ntt_buffers, emul
        self.policy = Policy(lib, ctx)

    def to_dev(self, b):
        return self.io.to_dev(b)


def fresh_context(lib):
    """The module fixture's body: POISON_ALLOC is process-wide, so it is set through a context that exists only for that, BEFORE
    the context under test makes its first allocation; the caller destroys the context and calls unpoison."""
    setter = lib.ctx_create(0)
    try:
        lib.ctx_set_policy(setter, "POISON_ALLOC", POISON)
    finally:
        lib.ctx_destroy(setter)
    ctx = lib.ctx_create(0)
    assert lib.ctx_get_policy(ctx, "POISON_ALLOC") == POISON
    return ctx


def unpoison(lib):
    setter = lib.ctx_create(0)
    try:
        lib.ctx_set_policy(setter, "POISON_ALLOC", -1)
        assert lib.ctx_get_policy(setter, "POISON_ALLOC") == -1
    finally:
        lib.ctx_destroy(setter)


def refused(code, needle=None):
    """context manager: the call is refused with this status and the context stays usable"""
    class _R:
        def __enter__(self):
            return self

        def __exit__(self, et, ev, tb):
            assert ev is not None and isinstance(ev, Ark355Error) and ev.code < 0 and code in (None, ev.code), (et, ev)
            assert needle is None or needle in str(ev), str(ev)
            return True
    return _R()


def _group(lib, C, group):
    sz = lib.sizes(C.curve_id)
    return (g1(C) if group == 1 else g2(C)), (Z.g1_raw if group == 1 else Z.g2_raw), (Z.g1_from_raw if group == 1 else Z.g2_from_raw), \
        (sz["g1"] if group == 1 else sz["g2"])


def _scalars(C, kind, n, rnd):
    if kind == "equal":
        return [rnd.randrange(C.r)] * n
    if kind == "boolean":
        return [rnd.randrange(2) if rnd.random() < 0.9 else rnd.randrange(C.r) for _ in range(n)]
    return [rnd.randrange(C.r) for _ in range(n)]


def _canon(C, ks):
    return b"".join(Z.fr_canon(C, k) for k in ks)


# ---- proofs ------------------------------------------------------------------------------------------------------------------
def proofs_sequence(t, C):
    """Two keys and two R1CS handles of different sizes (on the GPU a third above the 1024-row floor of the window policy) bound in
    ONE context and proven alternately under changing schedules; ark355_prove_batch with 3 in flight, then a single proof.  Keys
    and expected bytes from the C oracle."""
    lib, ctx, pol = t.lib, t.ctx, t.policy
    sizes = lib.sizes(C.curve_id)
    insts = {"big": S.mulchain_csr(C.r, 300), "small": S.mulchain_csr(C.r, 9), "small2": S.mulchain_csr(C.r, 9, seed=0xD1B7)}
    if not t.emul:
        insts["floor"] = S.mulchain_csr(C.r, 1500)
    keys = {k: O.oracle_key(C, v) for k, v in insts.items() if k != "small2"}
    keys["small2"] = keys["small"]                       # same matrices, another assignment
    handles = {k: O.load(lib, ctx, C, insts[k], keys[k]) for k in keys if k != "small2"}
    handles["small2"] = handles["small"]
    step = [0]

    def prove(which, **knobs):
        step[0] += 1
        pol.set(**knobs)
        n, ell, w, mats, z = insts[which]
        zb = S._mont_bytes(C.r, z)
        r_, s_ = 0x1234 + 77 * step[0], 0x9999 + 131 * step[0]
        pkh, rh = handles[which]
        got = lib.prove(ctx, pkh, rh, zb, len(z), Z.fr_canon(C, r_), Z.fr_canon(C, s_), sizes)
        assert got == cbase.prove(C, n, ell, w, mats, zb, keys[which], r_, s_), (C.name, which, step[0], knobs)

    try:
        order = ["big", "small", "small2", "big"] + ([] if t.emul else ["floor", "small", "floor"])
        knobs = [dict(SCHED=0), dict(SCHED=1), dict(SCHED=0, BATCH_TAILS=0), dict(SIDE_G2_TAILS=0), dict(SCHED=1, BATCH_TAILS=1),
                 dict(SCHED=0, SIDE_G2_TAILS=1), dict(BATCH_TAILS=0)]
        for which, kn in zip(order, knobs):
            prove(which, **kn)
        # a refusal between two proofs: the assignment one element short
        n, ell, w, mats, z = insts["big"]
        zb = S._mont_bytes(C.r, z)
        with refused(E_ASSIGNMENT_MISSING):
            lib.prove(ctx, handles["big"][0], handles["big"][1], zb[:-32], len(z) - 1, Z.fr_canon(C, 1), Z.fr_canon(C, 2), sizes)
        prove("small", SCHED=0, BATCH_TAILS=1)
        # three in flight on the large key, then one proof alone on the small one
        rs = [(0xABC + 5 * k, 0xDEF + 9 * k) for k in range(3)]
        outs = lib.prove_batch(ctx, handles["big"][0], handles["big"][1], [zb] * 3, len(z), [Z.fr_canon(C, a) for a, _ in rs],
                               [Z.fr_canon(C, b) for _, b in rs], sizes, inflight=3)
        for (r_, s_), got in zip(rs, outs):
            assert got == cbase.prove(C, n, ell, w, mats, zb, keys["big"], r_, s_), (C.name, "ark355_prove_batch")
        prove("small2", SCHED=1)
        # the planner's refusal: no window layout of the largest key fits one MiB; the keys already loaded prove on
        pol.set(HBM_BUDGET_MB=1)
        huge = S.mulchain_csr(C.r, 5000 if t.emul else 20000)
        with refused(ENOMEM, "do not fit"):
            O.load(lib, ctx, C, huge, O.oracle_key(C, huge))
        pol.set(HBM_BUDGET_MB=0)
        prove("big", SCHED=0)
    finally:
        pol.restore()
        for k in set(handles) - {"small2"}:
            O.free(lib, *handles[k])


def check_satisfied_sequence(t, C):
    """CHECK_SATISFIED = 1: unsatisfied (ARK355_E_UNSATISFIABLE naming the oracle's row), satisfied (the oracle's bytes), unsatisfied
    at ANOTHER, earlier row: the verdict word of the first refusal must not decide the second or the third call."""
    lib, ctx, pol = t.lib, t.ctx, t.policy
    sizes = lib.sizes(C.curve_id)
    nrows = 300
    inst = S.mulchain_csr(C.r, nrows)
    n, ell, w, mats, z = inst
    A, B, Cm, z2, ell2 = S.mulchain_direct(C.r, nrows)
    assert list(z2) == list(z) and ell2 == ell
    pk = O.oracle_key(C, inst)
    pkh, rh = O.load(lib, ctx, C, inst, pk)
    try:
        pol.set(CHECK_SATISFIED=1, SCHED=0)

        def bad(k):
            zb = list(z)
            zb[k] = (zb[k] + 1) % C.r
            row = R.first_unsatisfied_r1cs(A, B, Cm, zb, C.r)
            assert row is not None and row >= 0
            with refused(E_UNSATISFIABLE, "constraint %d " % row):
                lib.prove(ctx, pkh, rh, S._mont_bytes(C.r, zb), len(z), Z.fr_canon(C, 7), Z.fr_canon(C, 9), sizes)
            return row

        def good(r_, s_):
            zb = S._mont_bytes(C.r, z)
            assert lib.prove(ctx, pkh, rh, zb, len(z), Z.fr_canon(C, r_), Z.fr_canon(C, s_), sizes) == \
                cbase.prove(C, n, ell, w, mats, zb, pk, r_, s_)

        first = bad(ell + 250)
        good(77, 99)
        second = bad(ell + 40)
        assert second < first
        good(78, 100)
        third = bad(ell + 290)
        assert third > first
    finally:
        pol.restore()
        O.free(lib, pkh, rh)


# ---- MSMs --------------------------------------------------------------------------------------------------------------------
def _known_bases(C, group, n, seed):
    """s_i G from the C oracle's fixed-base routine; rows 0 and 1 are opposite, so that a prefix can sum to infinity"""
    rnd = random.Random("dirty-bases/%s/%d/%d/%d" % (C.name, group, n, seed))
    ss = [rnd.getrandbits(64) + 1 for _ in range(n)]
    if n >= 2:
        ss[1] = C.r - ss[0]
    gen = Z.g1_raw(C, C.g1_gen) if group == 1 else Z.g2_raw(C, C.g2_gen)
    return ss, cbase.fixed_base(C, group, gen, _canon(C, ss), n)


def resident_msm_sequence(t, C, group):
    """One resident base set (MSM_C = 11, TABLE_STRIDE = 1, MSM_SEG = 16: the merge designs' policy) under uniform, all-equal (one
    run per segment: the heavy merge), boolean scalars, a prefix of 8 that sums to infinity, count 1, count 0, uniform again; a
    second, smaller set with another window size; the first set again.  Expected: the known discrete log, and cbase.msm."""
    lib, ctx, pol = t.lib, t.ctx, t.policy
    G_, raw, fromraw, psz = _group(lib, C, group)
    n = 1100
    rnd = random.Random("dirty-resident/%s/%d" % (C.name, group))
    ss, pts = _known_bases(C, group, n, 1)
    ss2, pts2 = _known_bases(C, group, 70, 2)

    def run(h, ss_, pts_, ks, what):
        count = len(ks)
        sb = _canon(C, ks) if ks else bytes(32)
        ptr, keep = t.to_dev(sb)
        got = lib.msm_dev(ctx, h, ptr, count, 0, psz)
        expect = G_.mul(G_.gen, sum(k * s for k, s in zip(ks, ss_)) % C.r)
        assert fromraw(C, got) == expect, (C.name, group, what)
        if count:
            assert got == cbase.msm(C, group, pts_[:count * psz], sb, count), (C.name, group, what, "cbase.msm")
        return got

    h = h2 = None
    try:
        pol.set(MSM_C=11, TABLE_STRIDE=1, MSM_SEG=16)
        h = lib.bases_load(ctx, C.curve_id, group, pts, n)
        run(h, ss, pts, _scalars(C, "uniform", n, rnd), "uniform")
        run(h, ss, pts, _scalars(C, "equal", n, rnd), "equal")
        run(h, ss, pts, _scalars(C, "boolean", n, rnd), "boolean")
        k = rnd.randrange(1, C.r)
        assert fromraw(C, run(h, ss, pts, [k, k] + [0] * 6, "prefix of 8 summing to infinity")) is None
        run(h, ss, pts, [rnd.randrange(C.r)], "count 1")
        assert fromraw(C, run(h, ss, pts, [], "count 0")) is None
        run(h, ss, pts, _scalars(C, "uniform", n, rnd), "uniform again")
        # refusal: more scalars than the table has rows
        ptr, keep = t.to_dev(bytes(32 * (n + 1)))
        with refused(EINVAL):
            lib.msm_dev(ctx, h, ptr, n + 1, 0, psz)
        run(h, ss, pts, _scalars(C, "boolean", n, rnd), "boolean after the refusal")
        pol.set(MSM_C=7, MSM_SEG=0)
        h2 = lib.bases_load(ctx, C.curve_id, group, pts2, 70)
        run(h2, ss2, pts2, _scalars(C, "uniform", 70, rnd), "second set")
        run(h2, ss2, pts2, _scalars(C, "equal", 70, rnd), "second set, equal")
        run(h2, ss2, pts2, _scalars(C, "uniform", 5, rnd), "second set, prefix 5")
        pol.set(MSM_C=11, MSM_SEG=16)
        run(h, ss, pts, _scalars(C, "equal", n, rnd), "first set again, equal")
        run(h, ss, pts, _scalars(C, "uniform", n, rnd), "first set again")
        run(h2, ss2, pts2, _scalars(C, "uniform", 70, rnd), "second set under the first set's segment length")
    finally:
        pol.restore()
        for x in (h, h2):
            if x is not None:
                lib.dll.ark355_bases_free(x)


def oneshot_msm_sequence(t, C, group):
    """ark355_msm with n = 2000, 16, 1, 0, 5, 2000; before the n = 5 step an argument refusal (a curve id the library does not know:
    the header documents no point validation for the one-shot entries, so there is no off-curve refusal to provoke here)"""
    lib, ctx = t.lib, t.ctx
    G_, raw, fromraw, psz = _group(lib, C, group)
    rnd = random.Random("dirty-oneshot/%s/%d" % (C.name, group))
    big = 700 if t.emul else 2000
    ss, pts = _known_bases(C, group, big, 3)
    for step, n in enumerate((big, 16, 1, 0, 5, big)):
        ks = _scalars(C, ("uniform", "boolean", "uniform", "uniform", "equal", "uniform")[step], n, rnd)
        if n == big and step:
            ks[3], ks[4] = 0, C.r - 1
        sb = _canon(C, ks)
        if n == 5:
            with refused(EINVAL, "unknown curve id"):
                lib.msm(ctx, 99, group, pts[:n * psz], sb, n, psz)
        got = lib.msm(ctx, C.curve_id, group, pts[:n * psz], sb, n, psz)
        assert fromraw(C, got) == G_.mul(G_.gen, sum(k * s for k, s in zip(ks, ss)) % C.r), (C.name, group, step, n)
        if n:
            assert got == cbase.msm(C, group, pts[:n * psz], sb, n), (C.name, group, step, n, "cbase.msm")


# ---- transforms --------------------------------------------------------------------------------------------------------------
def ntt_sequence(t, C):
    """ark355_ntt_fr and ark355_ntt_fr_dev: log_n = 14, 3, 9, 1, 14, four modes each, against cb_ntt"""
    top = 12 if t.emul else 14
    for step, log_n in enumerate((top, 3, 9, 1, top)):
        nc.ntt_full_case(t.lib, t.ctx, C, log_n, seed=5 + step)
    # refusal: a domain the field has no root of unity for (PolynomialDegreeTooLarge)
    with refused(None):
        t.lib.ntt(t.ctx, C.curve_id, bytes(64), 60, 0, 0)
    for step, log_n in enumerate((top, 3, 9, 1, top)):
        nc.ntt_dev_case(t.lib, t.ctx, C, log_n, t.ntt_buffers, seed=11 + step)


def witness_map_sequence(t, C):
    """ark355_witness_map, ark355_r1cs_mat_vec and ark355_is_satisfied at N = 2^10, then 2^3, then 2^10 again, both handles alive; an
    unsatisfied assignment followed by a satisfied one answers -1 (the first-bad word is cleared per call)."""
    lib, ctx = t.lib, t.ctx
    loaded = []
    try:
        for rows in (1000, 5):
            n, ell, w, mats, z = S.mulchain_csr(C.r, rows)
            A, B, Cm, z2, _ = S.mulchain_direct(C.r, rows)
            assert list(z) == list(z2)
            loaded.append((lib.r1cs_load(ctx, C.curve_id, n, ell, w, mats), (n, ell, w, mats, z), (A, B, Cm)))
        for which, bump in ((0, 900), (1, 3), (1, 4), (0, 17)):
            rh, (n, ell, w, mats, z), (A, B, Cm) = loaded[which]
            m = len(z)
            zb = S._mont_bytes(C.r, z)
            zbad = list(z)
            zbad[ell + bump] = (zbad[ell + bump] + 1 + bump) % C.r
            zbb = S._mont_bytes(C.r, zbad)
            want_bad = R.first_unsatisfied_r1cs(A, B, Cm, zbad, C.r)
            assert want_bad is not None and want_bad >= 0
            assert lib.is_satisfied(ctx, rh, zbb, m) == want_bad, (C.name, n, "unsatisfied")
            assert lib.is_satisfied(ctx, rh, zb, m) == -1, (C.name, n, "satisfied after unsatisfied")
            assert lib.witness_map(ctx, rh, zbb, m, 32) == cbase.witness_map(C, n, ell, w, mats, zbb), (C.name, n, "map, unsatisfied")
            assert lib.witness_map(ctx, rh, zb, m, 32) == cbase.witness_map(C, n, ell, w, mats, zb), (C.name, n, "map")
            az, bz, cz = lib.mat_vec(ctx, rh, zbb, m, n, 32)
            for got, M in ((az, A), (bz, B), (cz, Cm)):
                assert fr_vec_from_mont(C, got) == R.mat_vec_mul(M, zbad, C.r), (C.name, n, "mat_vec")
            if which == 0:
                # refusal: an assignment one element short, then the same handle again
                with refused(E_ASSIGNMENT_MISSING):
                    lib.witness_map(ctx, rh, zb[:-32], m - 1, 32)
                assert lib.is_satisfied(ctx, rh, zb, m) == -1
    finally:
        for rh, _, _ in loaded:
            lib.dll.ark355_r1cs_free(rh)


# ---- GR1CS and the quotient ----------------------------------------------------------------------------------------------------
def _quotient_of(C, g, spec, label, z):
    arity, terms, mats = spec[label]
    dims = g.quotient_dims(label, 0)
    assert dims == qc.dims_ref(len(mats[0]), terms, 0), (label, dims)
    h = g.quotient(label, z, 0)
    want = qc.mont(C, qc.r_def(C, terms, qc.mat_vecs(C, mats, z), dims[1], dims[2]))
    assert h == want, (C.name, label, dims, qc.first_difference(h, want))
    return dims


def quotient_sequence(t, C):
    """One system with predicates of degree 5, 3 and 2 (extension D = 4, 2, 1): ark355_gr1cs_quotient in that order, then reversed
    (the padding above N of the D = 4 call lies under the D = 2 and D = 1 calls), then a system with a smaller domain; all against
    the definition (quotient_cases.r_def)."""
    lib, ctx = t.lib, t.ctx
    shapes = qc.shapes(C)
    rnd = random.Random("dirty-quotient/%d" % C.curve_id)
    m = 9
    spec = {}
    for label, shape, n in (("a-deg5", "deg5-N8", 100), ("b-deg3", "arity4-deg3-N16", 100), ("c-deg2", "arity2-N4", 100)):
        arity, terms = shapes[shape][0], shapes[shape][1]
        spec.update(qc.random_spec(C, rnd, label, arity, terms, n, m))
    small = {}
    for label, shape, n in (("a-deg5", "deg5-N8", 5), ("c-deg2", "arity2-N4", 3)):
        small.update(qc.random_spec(C, rnd, label, shapes[shape][0], shapes[shape][1], n, m))
    z1, z2 = qc.random_z(C, rnd, m), qc.random_z(C, rnd, m)
    g = gc.load(lib, ctx, C, 2, m - 2, spec)
    gs = None
    try:
        exts = [_quotient_of(C, g, spec, label, z1)[2] for label in ("a-deg5", "b-deg3", "c-deg2")]
        assert exts == [2, 1, 0]
        for label in ("c-deg2", "b-deg3", "a-deg5"):
            _quotient_of(C, g, spec, label, z2)
        # refusal: a predicate index out of range, then the smaller system
        with refused(EINVAL):
            lib.gr1cs_quotient(ctx, g.handle, 7, z_bytes(C, z1), m, 0, 8, 32)
        gs = gc.load(lib, ctx, C, 2, m - 2, small)
        for label in ("a-deg5", "c-deg2", "a-deg5"):
            _quotient_of(C, gs, small, label, z1)
        _quotient_of(C, g, spec, "b-deg3", z1)
    finally:
        g.free()
        if gs is not None:
            gs.free()


def which_is_unsatisfied_sequence(t, C):
    """ark355_gr1cs_which_is_unsatisfied failing in predicate 2, then passing, then failing in predicate 0; the refusals of
    ark355_gr1cs_load (gr1cs_cases.refusal_case), then a smaller system"""
    b = gc.Builder(C, 0xD127 + C.curve_id)
    rnd = b.rnd
    rows = 70
    for label, arity in (("p0", 2), ("p1", 4), ("p2", 3)):
        b.add(label, arity, gc.random_polynomial(rnd, C.r, arity, max_deg=5), rows)
    zs = [b.violated("p2", rows - 1), b.z(), b.violated("p0", 3), b.z()]
    gc.check_system(t.lib, t.ctx, C, b.ell, len(b.wit), b.spec, zs, expect=[("p2", rows - 1), None, ("p0", 3), None])
    gc.refusal_case(t.lib, t.ctx, C)
    small = gc.Builder(C, 0xD128 + C.curve_id)
    small.add("q", 3, gc.r1cs_terms(C.r), 5)
    gc.check_system(t.lib, t.ctx, C, small.ell, len(small.wit), small.spec, [small.violated("q", 4), small.z()], expect=[("q", 4), None])


# ---- Square R1CS, finalize(), setup ----------------------------------------------------------------------------------------------
def sr1cs_sequence(t, C):
    """5000-row source, then 20 rows: adapter, assignment, `_dev` assignment; a refusal between them"""
    big = 600 if t.emul else 5000
    sc.random_case(t.lib, t.ctx, C, t.io, big, seed=0xD1)
    sc.random_case(t.lib, t.ctx, C, t.io, 20, seed=0xD2)
    sc.refusal_case(t.lib, t.ctx, C)
    sc.random_case(t.lib, t.ctx, C, t.io, 20, seed=0xD3)
    sc.random_case(t.lib, t.ctx, C, t.io, big, seed=0xD4)


def finalize_sequence(t, C):
    """random system with 5000 LCs, circuit2 (and, beyond the issue, circuit1: four predicates, no R1CS rows), the hand-made system
    with LCS_ROW_LDS_MAX at its default and at 8 (handmade_case runs both and compares their read-backs), the random one again"""
    big = 600 if t.emul else 5000
    try:
        lc.random_case(t.lib, t.ctx, C, big, seed=0xD1A)
        lc.reference_circuit_case(t.lib, t.ctx, C, 0)          # circuit2
        lc.reference_circuit_case(t.lib, t.ctx, C, 1)          # circuit1
        lc.handmade_case(t.lib, t.ctx, C, t.policy)
        t.policy.restore()
        lc.refusal_case(t.lib, t.ctx, C)
        lc.random_case(t.lib, t.ctx, C, big, seed=0xD1A)
    finally:
        t.policy.restore()


def setup_sequence(t, C):
    """ark355_setup at n = 70, then 9, a refusal, n = 1, then 70 under another trapdoor: every key vector against the oracle's
    generator"""
    su.whole_key_case(t.lib, t.ctx, C, "mulchain70")
    su.whole_key_case(t.lib, t.ctx, C, "mulchain9")
    su.argument_errors_case(t.lib, t.ctx, C)
    su.whole_key_case(t.lib, t.ctx, C, "n1")
    su.whole_key_case(t.lib, t.ctx, C, "mulchain70", tau=0x5EED5EED5EED)


# ---- pairings and verification (device route forced) ---------------------------------------------------------------------------
def pairing_sequence(t, C):
    """ark355_multi_pairing with many pairs, then 3, both against e(G1, G2)^(sum a_i b_i); a refusal between them"""
    try:
        t.policy.set(PAIRING_DEVICE=1)
        pg.gt_case(t.lib, t.ctx, C, 70 if t.emul else 300, seed=0xD1)
        pg.refusals_case(t.lib, t.ctx, C, Ark355Error, EINVAL)
        pg.gt_case(t.lib, t.ctx, C, 3, seed=0xD2)
    finally:
        t.policy.restore()


def verify_each_sequence(t, C):
    """ark355_verify_each with 70 proofs, bad ones at 0, 33 and 69, then 2 good proofs; the same through a processed key"""
    batch = pg.oracle_batch(C, 8)
    total = 9 if t.emul else 70
    tamper = dict(other_c=(0,), wrong_input=(total // 2 - 2,), b_off=(total // 2,), swapped=(total - 1,))
    vk = batch[0]
    try:
        t.policy.set(PAIRING_DEVICE=1)
        ps, xs, want = pe.tampered_batch(C, batch, total, **tamper)
        assert want.count(False) == 4
        assert t.lib.verify_each(t.ctx, C.curve_id, vk, ps, b"".join(xs)) == want
        # refusal after the device has checked the key's points: gamma_g2 poked off its curve
        bad = bytearray(vk[2])
        bad[len(bad) // 2] ^= 1
        with refused(EINVAL, "gamma_g2"):
            t.lib.verify_each(t.ctx, C.curve_id, (vk[0], vk[1], bytes(bad), vk[3], vk[4]), ps, b"".join(xs))
        ps2, xs2, want2 = pe.tampered_batch(C, batch, 2)
        assert want2 == [True, True]
        assert t.lib.verify_each(t.ctx, C.curve_id, batch[0], ps2, b"".join(xs2)) == want2
        with pv.processed(t.lib, t.ctx, C, batch[0]) as h:
            assert t.lib.verify_each_pvk(t.ctx, h, ps, b"".join(xs)) == want
            assert t.lib.verify_each_pvk(t.ctx, h, ps2, b"".join(xs2)) == want2
    finally:
        t.policy.restore()


def verify_each_bytes_sequence(t, C):
    """ark355_verify_each_bytes with 96 proofs, then 5 good ones (all verdicts 1, all status 0), then 96 with the bad ones elsewhere.
    verify_each_bytes_case plants one wire defect per (point, kind of damage) on every third proof: 96 proofs hold all of
    them on A, B and C (asserted below; 64 would reach only the first kinds on C).  The emulator runs 12 proofs, which hold the
    first three kinds on A only -- its tier has every kind in tests/test_emul_verify_bytes.py and keeps the order of calls here."""
    total = 12 if t.emul else 96
    kinds = sum(len(vb.damages(C, 2 if pos == 1 else 1, True)) for pos in range(3))
    for tampered in ((0, total // 2, total - 1), (3, total - 2)):
        assert t.emul or len([j for j in range(2, total, 3) if j not in tampered]) >= kinds, (total, kinds)
    try:
        vb.verify_each_bytes_case(t.lib, t.ctx, t.policy, C, True, vb.FULL, total, tamper=dict(other_c=(0,), wrong_input=(total // 2,), a_inf=(total - 1,)))
        t.policy.restore()
        t.policy.set(PAIRING_DEVICE=1)
        batch = vb.oracle_proofs(C)[0]
        ps, xs, want = pe.tampered_batch(C, batch, 5)
        blob = b"".join(vb.raw_to_wire(C, p, True) for p in ps)
        with pv.processed(t.lib, t.ctx, C, batch[0]) as h:
            ok, status = t.lib.verify_each_bytes(t.ctx, h, blob, 5, b"".join(xs), True, vb.FULL)
        assert list(status) == [0] * 5 and list(ok) == [True] * 5, (ok, status)
        t.policy.restore()
        vb.verify_each_bytes_case(t.lib, t.ctx, t.policy, C, True, vb.FULL, total, tamper=dict(other_c=(3,), swapped=(total - 2,)))
    finally:
        t.policy.restore()
