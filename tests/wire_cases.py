"""ark-serialize wire formats THROUGH the C ABI against the oracle's encoders (oracle/serialize.py), shared by the
CPU-emulator tier and the GPU tier: point codecs (ark355_points_decode/_encode), proof bytes, and the end-to-end
path bytes of an ark_groth16::ProvingKey -> ark355_pk_load_bytes -> ark355_prove -> proof bytes == oracle; and the decoders
against the oracle's own DECODER (oracle/serialize.py g1_decode / g2_decode, written from the specification in
include/ark355.h): constructed edge points, a seeded fuzz, batch counts, the smallest failing index, damaged key streams."""
import random
import re

import pytest

from helpers import csr_from_rows, z_bytes
from oracle import groth16 as G, serialize as Z, synthetic as S
from oracle.curves import g1, g2


def points_case(lib, ctx, C, n=9, seed=3):
    rnd = random.Random(seed)
    sz = lib.sizes(C.curve_id)
    for group, Gp, gen, raw, encs in ((1, g1(C), C.g1_gen, Z.g1_raw, (Z.g1_compressed, Z.g1_uncompressed)),
                                      (2, g2(C), C.g2_gen, Z.g2_raw, (Z.g2_compressed, Z.g2_uncompressed))):
        pts = [None, gen] + [Gp.mul(gen, rnd.randrange(C.r)) for _ in range(n - 2)]
        pts += [Gp.neg(p) for p in pts[1:4]]                       # both signs of y
        raws = b"".join(raw(C, p) for p in pts)
        rsz = sz["g1"] if group == 1 else sz["g2"]
        for comp, enc in ((True, encs[0]), (False, encs[1])):
            wire = b"".join(enc(C, p) for p in pts)
            assert lib.point_size(C.curve_id, group, comp) * len(pts) == len(wire)
            assert lib.points_encode(ctx, C.curve_id, group, raws, len(pts), comp) == wire
            assert lib.points_decode(ctx, C.curve_id, group, wire, len(pts), comp, True, rsz) == raws
        # an off-curve uncompressed point and a non-residue compressed x must be rejected with the index
        bad = bytearray(b"".join(encs[1](C, p) for p in pts))
        psz = lib.point_size(C.curve_id, group, False)
        bad[2 * psz + psz // 2 + 1] ^= 1
        with pytest.raises(Exception) as ei:
            lib.points_decode(ctx, C.curve_id, group, bytes(bad), len(pts), False, True, rsz)
        assert "[2]" in str(ei.value) and "curve" in str(ei.value)
        assert len(lib.points_decode(ctx, C.curve_id, group, bytes(bad), len(pts), False, False, rsz)) == len(raws)


def key_stream_case(lib, ctx, C, n=24, compressed=False):
    A, B, Cm, z, ell = S.cs_to_instance(S.bench_lc_cs(C.r, n))
    m, w = len(z), len(z) - ell
    opk = G.setup(C, A, B, Cm, ell, m, G.Trapdoor(tau=0xABCDEF123, alpha=3, beta=5, gamma=7, delta=11))
    stream = Z.pk_bytes(C, opk, compressed)
    pkh = lib.pk_load_bytes(ctx, C.curve_id, stream, compressed=compressed, validate=True)
    rh = lib.r1cs_load(ctx, C.curve_id, len(A), ell, w, [csr_from_rows(C, M) for M in (A, B, Cm)])
    try:
        assert lib.pk_dims(pkh) == (ell, w, 1 << opk.domain_log)
        sizes = lib.sizes(C.curve_id)
        r_, s_ = 0x1234567, 0x7654321
        a, b, c = lib.prove(ctx, pkh, rh, z_bytes(C, z), m, Z.fr_canon(C, r_), Z.fr_canon(C, s_), sizes)
        exp = G.prove_closed_form(C, opk, z, ell, r_, s_)
        for comp in (True, False):
            wire = lib.proof_to_bytes(C.curve_id, a, b, c, comp)
            assert wire == Z.proof_bytes(C, exp, comp)
            assert lib.proof_from_bytes(C.curve_id, wire, sizes, comp) == (a, b, c)
    finally:
        lib.dll.ark355_pk_free(pkh)
        lib.dll.ark355_r1cs_free(rh)
    # malformed streams fail in the loader
    for broken in (stream[:-3], stream + b"\0", stream[:40]):
        with pytest.raises(Exception):
            lib.pk_load_bytes(ctx, C.curve_id, broken, compressed=compressed)


VALIDATE_NONE, VALIDATE_FULL, VALIDATE_CURVE = 0, 1, 2


def validation_case(lib, ctx, C, seed=17):
    """What ark-serialize's Validate::Yes refuses and the on-curve-only mode lets through: points on
    the curve but outside the prime-order subgroup, infinity flags with a payload, flag combinations upstream rejects in
    every mode; and the same on a proof (three points, host path of ark355_proof_from_bytes)."""
    rnd = random.Random(seed)
    sz = lib.sizes(C.curve_id)
    q = C.q
    stray = {}
    for group, Gp, comp_enc, unc_enc, from_raw, rsz in ((1, g1(C), Z.g1_compressed, Z.g1_uncompressed, Z.g1_from_raw, sz["g1"]),
                                                        (2, g2(C), Z.g2_compressed, Z.g2_uncompressed, Z.g2_from_raw, sz["g2"])):
        # random x: the compressed decoder (curve-only mode) hands back the oracle's point where x^3 + b has a root and
        # answers "not on curve" where it has none -- the oracle decoder says which, for every x tried
        P, seen = None, set()
        for _ in range(16):
            x = rnd.randrange(q) if group == 1 else (rnd.randrange(q), rnd.randrange(q))
            wire = comp_enc(C, (x, 1 if group == 1 else (1, 0)))
            status, Q = Z.verdict(C, group, wire, True, VALIDATE_CURVE)
            assert status in (0, Z.NOT_ON_CURVE)
            seen.add(status)
            if status == 0:
                got = lib.points_decode(ctx, C.curve_id, group, wire, 1, True, VALIDATE_CURVE, rsz)
                assert from_raw(C, got) == Q and Q[0] == x
                if P is None:
                    P, raw = Q, got
            else:
                with pytest.raises(Exception) as ei:
                    lib.points_decode(ctx, C.curve_id, group, wire, 1, True, VALIDATE_CURVE, rsz)
                assert "point[0]: point not on curve" in str(ei.value)
        assert seen == {0, Z.NOT_ON_CURVE}, "16 random x give both a residue and a non-residue"
        assert P is not None and Gp.is_on_curve(P)
        in_subgroup = Gp.add(Gp.mul(P, C.r - 1), P) is None         # [r]P == O  (Group.mul reduces its scalar mod r)
        cofactor_one = C.bn_like and group == 1
        assert in_subgroup == cofactor_one, "a random curve point lies outside the subgroup unless the cofactor is 1"
        for comp, enc in ((True, comp_enc), (False, unc_enc)):
            w = enc(C, P)
            assert lib.points_decode(ctx, C.curve_id, group, w, 1, comp, VALIDATE_CURVE, rsz) == raw
            assert lib.points_decode(ctx, C.curve_id, group, w, 1, comp, VALIDATE_NONE, rsz) == raw
            if cofactor_one:
                assert lib.points_decode(ctx, C.curve_id, group, w, 1, comp, VALIDATE_FULL, rsz) == raw
            else:
                with pytest.raises(Exception) as ei:
                    lib.points_decode(ctx, C.curve_id, group, w, 1, comp, VALIDATE_FULL, rsz)
                assert "subgroup" in str(ei.value)
        stray[group] = P
        # subgroup members pass the full check
        good = Gp.mul(Gp.gen, rnd.randrange(1, C.r))
        for comp, enc in ((True, comp_enc), (False, unc_enc)):
            lib.points_decode(ctx, C.curve_id, group, enc(C, good), 1, comp, VALIDATE_FULL, rsz)
        # infinity flag with a payload
        for comp, enc in ((True, comp_enc), (False, unc_enc)):
            inf = bytearray(enc(C, None))
            assert from_raw(C, lib.points_decode(ctx, C.curve_id, group, bytes(inf), 1, comp, VALIDATE_FULL, rsz)) is None
            inf[len(inf) // 2] ^= 0x10
            for mode in (VALIDATE_FULL, VALIDATE_CURVE, VALIDATE_NONE):
                if C.bn_like:
                    # ark-ec's generic reader: the coordinates under an infinity flag are parsed (reduced) and ignored
                    assert from_raw(C, lib.points_decode(ctx, C.curve_id, group, bytes(inf), 1, comp, mode, rsz)) is None
                else:
                    # ark-bls12-381's readers refuse a payload under the infinity flag, whatever the validation mode
                    with pytest.raises(Exception) as ei:
                        lib.points_decode(ctx, C.curve_id, group, bytes(inf), 1, comp, mode, rsz)
                    assert "flag" in str(ei.value)
            if C.bn_like:
                big = bytearray(enc(C, None))
                for i in range(C.fq_bytes - 1):
                    big[i] = 0xFF                                          # first coordinate >= q under the infinity flag
                big[C.fq_bytes - 1] |= 0x3F if (group == 1 and comp) else 0xFF
                with pytest.raises(Exception):
                    lib.points_decode(ctx, C.curve_id, group, bytes(big), 1, comp, VALIDATE_NONE, rsz)
        # flag combinations upstream refuses in every mode
        if C.bn_like:
            both = bytearray(comp_enc(C, good))
            both[-1] |= 0xC0                                               # SWFlags::from_u8(0b11) is None
            bad_flags = [(True, bytes(both))]
        else:
            unc = bytearray(unc_enc(C, good))
            unc[0] |= 0x20                                                 # sort bit without the compressed bit
            infs = bytearray(comp_enc(C, None))
            infs[0] |= 0x20                                                # sort bit with the infinity bit
            mism = bytearray(unc_enc(C, good))
            mism[0] |= 0x80                                                # compressed bit on an uncompressed encoding
            bad_flags = [(False, bytes(unc)), (True, bytes(infs)), (False, bytes(mism))]
        for comp, w in bad_flags:
            for mode in (VALIDATE_NONE, VALIDATE_FULL, VALIDATE_CURVE):
                with pytest.raises(Exception) as ei:
                    lib.points_decode(ctx, C.curve_id, group, w, 1, comp, mode, rsz)
                assert "flag" in str(ei.value)
    # a proof whose B (and, where G1 has a cofactor, A) left the subgroup: refused by the default mode of
    # ark355_proof_from_bytes, accepted only by the explicit curve-only mode
    G1, G2 = g1(C), g2(C)
    a, b, c = G1.mul(G1.gen, 5), G2.mul(G2.gen, 7), G1.mul(G1.gen, 11)
    for comp in (True, False):
        e1, e2 = (Z.g1_compressed, Z.g2_compressed) if comp else (Z.g1_uncompressed, Z.g2_uncompressed)
        ok = e1(C, a) + e2(C, b) + e1(C, c)
        assert lib.proof_from_bytes(C.curve_id, ok, sz, comp) == (Z.g1_raw(C, a), Z.g2_raw(C, b), Z.g1_raw(C, c))
        evil = [e1(C, a) + e2(C, stray[2]) + e1(C, c)]
        if not C.bn_like:
            evil.append(e1(C, stray[1]) + e2(C, b) + e1(C, c))
        for w in evil:
            with pytest.raises(Exception):
                lib.proof_from_bytes(C.curve_id, w, sz, comp)
            lib.proof_from_bytes(C.curve_id, w, sz, comp, validate=VALIDATE_CURVE)


# ---- differential tests against the oracle's DECODER (oracle/serialize.py g1_decode / g2_decode) ------------------------------------
# Every comparison below is exact: the raw bytes of an accepted point, the status (and, in a batch, the index) of a refusal.
MODES = (VALIDATE_NONE, VALIDATE_FULL, VALIDATE_CURVE)
STATUS_TEXT = {"coordinate not reduced": Z.NOT_REDUCED, "point not on curve": Z.NOT_ON_CURVE, "bad flag bits": Z.BAD_FLAGS,
               "point not in the prime-order subgroup": Z.NOT_IN_SUBGROUP}
_REPORT = re.compile(r"(\w+)\[(\d+)\]: (.+)$")


class Format:
    """One of the eight formats: curve, group, form."""

    def __init__(self, lib, C, group, comp):
        self.lib, self.C, self.group, self.comp = lib, C, group, comp
        self.G = g1(C) if group == 1 else g2(C)
        self.enc = {(1, True): Z.g1_compressed, (1, False): Z.g1_uncompressed,
                    (2, True): Z.g2_compressed, (2, False): Z.g2_uncompressed}[(group, comp)]
        self.raw = Z.g1_raw if group == 1 else Z.g2_raw
        self.rsz = lib.sizes(C.curve_id)["g1" if group == 1 else "g2"]
        self.psz = lib.point_size(C.curve_id, group, comp)
        self.nb = C.fq_bytes
        self.ncoord = group * (1 if comp else 2)
        assert self.psz == self.ncoord * self.nb
        self.name = "%s G%d %s" % (C.name, group, "compressed" if comp else "uncompressed")
        self.cofactor_one = C.bn_like and group == 1
        # the statuses this format can answer in each mode
        self.statuses = {}
        for mode in MODES:
            st = {Z.BAD_FLAGS, Z.NOT_REDUCED}
            if comp or mode != VALIDATE_NONE:
                st.add(Z.NOT_ON_CURVE)
            if mode == VALIDATE_FULL and not self.cofactor_one:
                st.add(Z.NOT_IN_SUBGROUP)
            self.statuses[mode] = st

    def encode(self, P):
        return self.enc(self.C, P)

    def oracle(self, w, mode):
        """(status, raw image of the point): the oracle decoder's verdict"""
        st, P = Z.verdict(self.C, self.group, w, self.comp, mode)
        return st, (self.raw(self.C, P) if st == 0 else None)

    def decode(self, ctx, wire, n, mode):
        """The library's answer to a batch: (None, raw images) or ((index, status), None)."""
        from snark_amd._binding import EINVAL, Ark355Error
        try:
            return None, self.lib.points_decode(ctx, self.C.curve_id, self.group, wire, n, self.comp, mode, self.rsz)
        except Ark355Error as e:
            m = _REPORT.search(str(e))
            assert e.code == EINVAL and m and m.group(1) == "point" and m.group(3) in STATUS_TEXT, str(e)
            return (int(m.group(2)), STATUS_TEXT[m.group(3)]), None

    def decode_one(self, ctx, w, mode):
        """(status, raw image) of a single encoding, the shape of Format.oracle"""
        bad, raws = self.decode(ctx, w, 1, mode)
        if bad is None:
            return 0, raws
        assert bad[0] == 0
        return bad[1], None

    def with_coordinate(self, w, slot, value):
        """encoding `w` with the integer `value` written into coordinate slot `slot`, the flag bits kept"""
        b = bytearray(w)
        nb = self.nb
        if self.C.bn_like:
            flags = b[-1] & 0xC0
            b[slot * nb:(slot + 1) * nb] = value.to_bytes(nb, "little")
            if slot == self.ncoord - 1:
                assert value < 1 << (8 * nb - 2)
            b[-1] = (b[-1] & 0x3F) | flags
        else:
            flags = b[0] & 0xE0
            b[slot * nb:(slot + 1) * nb] = value.to_bytes(nb, "big")
            if slot == 0:
                assert value < 1 << (8 * nb - 3)
            b[0] = (b[0] & 0x1F) | flags
        return bytes(b)

    def slot_bits(self, slot):
        """bits of coordinate slot `slot` below the flag bits"""
        if self.C.bn_like:
            return 8 * self.nb - (2 if slot == self.ncoord - 1 else 0)
        return 8 * self.nb - (3 if slot == 0 else 0)

    def flag_values(self):
        """(read, write) of the flag field as a small integer"""
        if self.C.bn_like:
            return (lambda w: w[-1] >> 6), (lambda w, f: w[:-1] + bytes([(w[-1] & 0x3F) | (f << 6)])), 4
        return (lambda w: w[0] >> 5), (lambda w, f: bytes([(w[0] & 0x1F) | (f << 5)]) + w[1:]), 8


def formats(lib, C):
    return [Format(lib, C, group, comp) for group in (1, 2) for comp in (True, False)]


def compare_with_oracle(F, ctx, encodings, what, verdicts=None):
    """Every encoding, alone, in all three modes: the oracle's status, and the oracle's point byte for byte where it accepts.
    Then per mode one batch of everything the oracle accepts (a clean return with the same bytes) and one batch of all of
    them (the index and status of the first one the oracle refuses).  Returns {mode: [(status, raw)]} of the oracle."""
    if verdicts is None:
        verdicts = {mode: [F.oracle(w, mode) for w in encodings] for mode in MODES}
    for mode in MODES:
        exp = verdicts[mode]
        for i, (w, e) in enumerate(zip(encodings, exp)):
            assert F.decode_one(ctx, w, mode) == e, (F.name, what, "mode %d" % mode, i, w.hex())
        good = [i for i, e in enumerate(exp) if e[0] == 0]
        bad, raws = F.decode(ctx, b"".join(encodings[i] for i in good), len(good), mode)
        assert bad is None and raws == b"".join(exp[i][1] for i in good), (F.name, what, "mode %d" % mode, "accepted batch")
        first = next((i for i, e in enumerate(exp) if e[0] != 0), None)
        bad, raws = F.decode(ctx, b"".join(encodings), len(encodings), mode)
        if first is None:
            assert bad is None and raws == b"".join(e[1] for e in exp)
        else:
            assert bad == (first, exp[first][0]), (F.name, what, "mode %d" % mode, "whole batch")
    return verdicts


def encode_matches_oracle(F, ctx, points):
    raws = b"".join(F.raw(F.C, P) for P in points)
    wire = b"".join(F.encode(P) for P in points)
    assert F.lib.points_encode(ctx, F.C.curve_id, F.group, raws, len(points), F.comp) == wire, (F.name, "encode")


def real_rhs_points(C):
    """Points of the twist whose x^3 + b' is REAL, one of each kind and both signs of y: {"real": [(x, (r, 0)), (x, (-r, 0))],
    "imaginary": [(x, (0, r)), (x, (0, -r))]}.  Random points never give one, and it is the only way into the `c1 == 0` branch of
    the Fq2 square root and into the c0 tie-break of the Fq2 ordering.  With x = (a, beta) the imaginary part of x^3 + b' is
    3 a^2 beta - beta^3 + b1: solve a^2 = (beta^3 - b1) / (3 beta) over small beta."""
    q = C.q
    G2 = g2(C)
    F = G2.F
    b0, b1 = G2.b
    out = {}
    for beta in range(1, 200):
        a = Z.fq_sqrt(C, (beta ** 3 - b1) * pow(3 * beta, -1, q))
        if a is None:
            continue
        x = (a, beta)
        rhs = F.add(F.mul(F.sqr(x), x), G2.b)
        assert rhs[1] == 0 and rhs[0] != 0
        y = Z.fq2_sqrt(C, rhs)
        assert y is not None, "every element of Fq is a square in Fq2"
        kind = "real" if y[1] == 0 else "imaginary"
        assert (y[0] == 0) == (kind == "imaginary") and y != (0, 0)
        if kind not in out:
            P = (x, y)
            assert G2.is_on_curve(P) and not Z.has_order_dividing_r(G2, P, C.r), "on the twist, outside the r-torsion"
            out[kind] = [P, G2.neg(P)]
        if len(out) == 2:
            return out
    raise AssertionError("no real-rhs point of both kinds below beta = 200")


def edge_points_case(lib, ctx, C, seed=23):
    """Constructed points and encodings that sampling never produces, through decode (three modes), encode and the host path
    of the proof codecs, against the oracle's decoder and encoder."""
    rnd = random.Random(seed)
    q = C.q
    G1, G2 = g1(C), g2(C)
    sz = lib.sizes(C.curve_id)
    real = real_rhs_points(C)
    assert set(real) == {"real", "imaginary"}
    # x = 0: BLS12-381 G1 has y^2 = 4; no other group of the two curves has such a point
    zero_x = {1: Z.fq_sqrt(C, G1.b), 2: Z.fq2_sqrt(C, G2.b)}
    assert (zero_x[1] is not None) == (not C.bn_like) and zero_x[2] is None
    host = {}                                             # (group, comp) -> [(encoding, oracle verdicts by mode)]
    for F in formats(lib, C):
        Gp = F.G
        zero = 0 if F.group == 1 else (0, 0)
        one = 1 if F.group == 1 else (1, 0)
        good = [Gp.mul(Gp.gen, rnd.randrange(1, C.r)) for _ in range(2)]
        points, encodings, kinds = [], [], []
        if F.group == 2:
            for kind in ("real", "imaginary"):
                points += real[kind]
                kinds += [kind + " root"] * 2
        if zero_x[F.group] is not None:
            y0 = zero_x[F.group]
            points += [(zero, y0), (zero, Gp.F.neg(y0))]
            kinds += ["x = 0"] * 2
        points += [None, good[1], Gp.neg(good[1])]
        kinds += ["valid"] * 3
        encodings += [F.encode(P) for P in points]
        encode_matches_oracle(F, ctx, points)
        if zero_x[F.group] is None:
            # x = 0 as a refusal: the compressed form with either sign bit, the uncompressed form with y = 1
            if F.comp:
                w = F.encode((zero, one))
                read, write, _ = F.flag_values()
                sign_bit = 2 if C.bn_like else 1
                cand = [write(w, read(w) & ~sign_bit), write(w, read(w) | sign_bit)]
            else:
                cand = [F.encode((zero, one))]
            for w in cand:
                assert F.oracle(w, VALIDATE_CURVE)[0] == Z.NOT_ON_CURVE, (F.name, "x = 0 is on no curve here")
            encodings += cand
            kinds += ["x = 0 refused"] * len(cand)
        # q - 1, q, q + 1 and all ones below the flag bits, in each coordinate slot of a valid non-infinity encoding
        base = F.encode(good[0])
        for slot in range(F.ncoord):
            for v, reduced in ((q - 1, True), (q, False), (q + 1, False), ((1 << F.slot_bits(slot)) - 1, False)):
                w = F.with_coordinate(base, slot, v)
                for mode in MODES:
                    assert (F.oracle(w, mode)[0] != Z.NOT_REDUCED) == reduced, (F.name, slot, hex(v))
                encodings.append(w)
                kinds.append("slot %d = %s" % (slot, "q - 1" if reduced else "not reduced"))
        if C.bn_like and not F.comp:
            # the sign bit of the uncompressed form is not looked at: the same point
            for P in good:
                w = F.encode(P)
                flipped = w[:-1] + bytes([w[-1] ^ 0x80])
                for mode in MODES:
                    assert F.oracle(flipped, mode) == (0, F.raw(C, P))
                encodings.append(flipped)
                kinds.append("sign bit flipped")
        verdicts = compare_with_oracle(F, ctx, encodings, "edge encodings")
        # on the oracle's side: each kind was produced, and answered as the construction intends
        for i, kind in enumerate(kinds):
            by_mode = {mode: verdicts[mode][i][0] for mode in MODES}
            if kind.endswith(" root"):
                assert by_mode == {VALIDATE_NONE: 0, VALIDATE_CURVE: 0, VALIDATE_FULL: Z.NOT_IN_SUBGROUP}, (F.name, kind)
            elif kind == "x = 0":
                assert by_mode[VALIDATE_NONE] == by_mode[VALIDATE_CURVE] == 0
            elif kind == "valid":
                assert set(by_mode.values()) == {0}
            elif kind == "x = 0 refused":
                assert by_mode[VALIDATE_CURVE] == by_mode[VALIDATE_FULL] == Z.NOT_ON_CURVE
                assert by_mode[VALIDATE_NONE] == (Z.NOT_ON_CURVE if F.comp else 0)
            elif kind.endswith("not reduced"):
                assert set(by_mode.values()) == {Z.NOT_REDUCED}
        want = {"slot %d = q - 1" % s for s in range(F.ncoord)} | {"slot %d = not reduced" % s for s in range(F.ncoord)}
        if F.group == 2:
            want |= {"real root", "imaginary root"}
        want.add("x = 0" if zero_x[F.group] is not None else "x = 0 refused")
        if C.bn_like and not F.comp:
            want.add("sign bit flipped")
        assert want <= set(kinds), (F.name, want - set(kinds))
        host[(F.group, F.comp)] = [(w, {mode: verdicts[mode][i] for mode in MODES}) for i, w in enumerate(encodings)]
    proof_host_path(lib, C, sz, host)


def proof_host_path(lib, C, sz, host):
    """The same templates as portable C++ on the host: every G1 encoding as a and as c, every G2 encoding as B of a proof
    whose other two points are accepted ones, through ark355_proof_from_bytes: refused exactly where the oracle refuses
    that encoding (the entry point has no context to leave a status text in), else the oracle's three points -- and back
    through ark355_proof_to_bytes.
    host: {(group, compressed): [(encoding, {mode: (status, raw)})]}"""
    for comp in (True, False):
        e1, e2 = host[(1, comp)], host[(2, comp)]
        for mode in MODES:
            ok1 = [e for e in e1 if e[1][mode][0] == 0]
            ok2 = [e for e in e2 if e[1][mode][0] == 0]
            assert ok1 and ok2
            triples = [(e, ok2[i % len(ok2)], ok1[i % len(ok1)]) for i, e in enumerate(e1)]
            triples += [(ok1[i % len(ok1)], ok2[(i + 1) % len(ok2)], e) for i, e in enumerate(e1)]
            triples += [(ok1[i % len(ok1)], e, ok1[(i + 1) % len(ok1)]) for i, e in enumerate(e2)]
            accepted = refused = 0
            for i, abc in enumerate(triples):
                wire = b"".join(e[0] for e in abc)
                exp = [e[1][mode] for e in abc]
                if all(st == 0 for st, _ in exp):
                    got = lib.proof_from_bytes(C.curve_id, wire, sz, comp, validate=mode)
                    assert got == tuple(raw for _, raw in exp), (C.name, comp, mode, i)
                    back = lib.proof_to_bytes(C.curve_id, got[0], got[1], got[2], comp)
                    assert lib.proof_from_bytes(C.curve_id, back, sz, comp, validate=mode) == got, (C.name, comp, mode, i)
                    accepted += 1
                else:
                    with pytest.raises(Exception) as ei:
                        lib.proof_from_bytes(C.curve_id, wire, sz, comp, validate=mode)
                    assert getattr(ei.value, "code", 0) == -1, ei.value
                    refused += 1
            assert accepted and refused, (C.name, comp, mode)


# ---- seeded differential fuzz -------------------------------------------------------------------------------------------------------
FUZZ_MIX = {"valid": 100, "random x": 56, "random bytes": 40, "random payload": 30, "coordinate >= q": 20, "bit flip": 44,
            "flags": 50}


def fuzz_encodings(F, rnd, scale=1.0):
    """Encodings of one format, from: valid points as they are (the only source of acceptances under VALIDATE_FULL where the
    group has a cofactor); random reduced x with either sign bit (uncompressed: with a root of the curve equation, or with
    a random y); random full-width bytes -- all of them, under flag bits that promise a point, or in one coordinate of a
    valid encoding and at least q; valid encodings with one random bit flipped; valid encodings with every other value of
    the flag bits."""
    C, Gp, q = F.C, F.G, F.C.q
    read, write, nflags = F.flag_values()

    def valid():
        if rnd.randrange(12) == 0:
            return F.encode(None)
        return F.encode(Gp.mul(Gp.gen, rnd.randrange(1, C.r)))

    def rand_fq():
        return rnd.randrange(q)

    def random_x():
        while True:
            x = rand_fq() if F.group == 1 else (rand_fq(), rand_fq())
            if F.comp:
                y = 1 if F.group == 1 else (1, 0)
                w = F.encode((x, y))
                sign_bit = 2 if C.bn_like else 1
                return write(w, (read(w) & ~sign_bit) | (sign_bit * rnd.randrange(2)))
            if rnd.randrange(3) == 0:
                y = rand_fq() if F.group == 1 else (rand_fq(), rand_fq())
                return F.encode((x, y))
            rhs = Gp.F.add(Gp.F.mul(Gp.F.sqr(x), x), Gp.b)
            y = Z.fq_sqrt(C, rhs) if F.group == 1 else Z.fq2_sqrt(C, rhs)
            if y is not None:
                return F.encode((x, y if rnd.randrange(2) else Gp.F.neg(y)))

    def random_bytes():
        return bytes(rnd.randrange(256) for _ in range(F.psz))

    def random_payload():
        w = random_bytes()
        if C.bn_like:
            return write(w, rnd.choice((0, 2)))
        return write(w, rnd.choice((4, 5)) if F.comp else 0)

    def coordinate_ge_q():
        slot = rnd.randrange(F.ncoord)
        return F.with_coordinate(valid_point(), slot, rnd.randrange(q, 1 << F.slot_bits(slot)))

    def valid_point():
        return F.encode(Gp.mul(Gp.gen, rnd.randrange(1, C.r)))

    def bit_flip():
        w = bytearray(valid())
        k = rnd.randrange(8 * len(w))
        w[k >> 3] ^= 1 << (k & 7)
        return bytes(w)

    def flags():
        w = valid()
        others = [f for f in range(nflags) if f != read(w)]
        if C.bn_like:
            others += [3, 3]                  # of BN254's four flag values only "both bits" is refused: make it half the draws
        return write(w, rnd.choice(others))

    make = {"valid": valid, "random x": random_x, "random bytes": random_bytes, "random payload": random_payload,
            "coordinate >= q": coordinate_ge_q, "bit flip": bit_flip, "flags": flags}
    out = []
    for source, count in FUZZ_MIX.items():
        out += [make[source]() for _ in range(max(1, int(count * scale)))]
    rnd.shuffle(out)
    return out


def fuzz_case(lib, ctx, C, seed=29, scale=1.0, host_triples=48):
    """A few hundred encodings per format against the oracle decoder: every single verdict, in all three modes.  Before the
    library is touched the oracle's own verdicts show that the set cannot pass vacuously: accepted and refused encodings are
    each at least a quarter of it, and every status the format can answer occurs at least 8 times -- in every mode."""
    sz = lib.sizes(C.curve_id)
    host = {}
    for F in formats(lib, C):
        rnd = random.Random(seed * 1000 + F.group * 10 + int(F.comp))
        encodings = fuzz_encodings(F, rnd, scale)
        n = len(encodings)
        verdicts = {mode: [F.oracle(w, mode) for w in encodings] for mode in MODES}
        for mode in MODES:
            statuses = [st for st, _ in verdicts[mode]]
            accepted = statuses.count(0)
            assert 4 * accepted >= n and 4 * (n - accepted) >= n, (F.name, mode, accepted, n)
            for st in F.statuses[mode]:
                assert statuses.count(st) >= 8, (F.name, mode, Z.STATUS_NAMES[st], statuses.count(st))
            assert set(statuses) <= F.statuses[mode] | {0}
        compare_with_oracle(F, ctx, encodings, "fuzz", verdicts)
        host[(F.group, F.comp)] = [(w, {mode: verdicts[mode][i] for mode in MODES}) for i, w in enumerate(encodings[:host_triples])]
    proof_host_path(lib, C, sz, host)


# ---- batches ------------------------------------------------------------------------------------------------------------------------
BATCH_COUNTS = (1, 63, 64, 65, 127, 128, 129, 1000, (1 << 16) + 1)


def known_points(lib, ctx, C, group, n, seed):
    """n raw points k_i G with known k_i from ark355_fixed_base_mul (k_0 = 0: the point at infinity), three of them against
    the Python group law."""
    rnd = random.Random(seed)
    Gp = g1(C) if group == 1 else g2(C)
    raw = Z.g1_raw if group == 1 else Z.g2_raw
    rsz = lib.sizes(C.curve_id)["g1" if group == 1 else "g2"]
    ks = [0] + [rnd.randrange(1, C.r) for _ in range(n - 1)]
    out = lib.fixed_base_mul(ctx, C.curve_id, group, raw(C, Gp.gen), b"".join(Z.fr_canon(C, k) for k in ks), n, rsz)
    for i in sorted({0, n // 2, n - 1}):
        assert out[i * rsz:(i + 1) * rsz] == raw(C, Gp.mul(Gp.gen, ks[i]) if ks[i] else None)
    return out


def batch_counts_case(lib, ctx, C, group, comp, counts=BATCH_COUNTS, modes=(VALIDATE_FULL, VALIDATE_CURVE), seed=31):
    """Whole and partial workgroups of the one-lane-per-point kernels (128 lanes, 64 per wavefront): n points both ways
    against the C oracle's encoder."""
    from oracle.c import cbase
    F = Format(lib, C, group, comp)
    raws = known_points(lib, ctx, C, group, max(counts), seed)
    wire = cbase.points_serialize(C, group, raws, comp)
    for i in (0, 1, len(raws) // F.rsz - 1):                  # the C encoder against the Python one
        assert wire[i * F.psz:(i + 1) * F.psz] == F.encode((Z.g1_from_raw if group == 1 else Z.g2_from_raw)(C, raws[i * F.rsz:(i + 1) * F.rsz]))
    for n in counts:
        r, w = raws[:n * F.rsz], wire[:n * F.psz]
        assert lib.points_encode(ctx, C.curve_id, group, r, n, comp) == w, (F.name, n, "encode")
        for mode in modes:
            assert F.decode(ctx, w, n, mode) == (None, r), (F.name, n, "decode, mode %d" % mode)


def off_subgroup_point(F, rnd):
    """a point of the curve outside the prime-order subgroup (None where the cofactor is 1)"""
    if F.cofactor_one:
        return None
    C, Gp = F.C, F.G
    while True:
        x = rnd.randrange(C.q) if F.group == 1 else (rnd.randrange(C.q), rnd.randrange(C.q))
        rhs = Gp.F.add(Gp.F.mul(Gp.F.sqr(x), x), Gp.b)
        y = Z.fq_sqrt(C, rhs) if F.group == 1 else Z.fq2_sqrt(C, rhs)
        if y is not None and not Z.has_order_dividing_r(Gp, (x, y), C.r):
            return (x, y)


def first_failure_case(lib, ctx, C, group, comp, n=1000, seed=37):
    """Three failures of three statuses among n = 1000 points, in three workgroups, the last of them the last point.  The one
    at the SMALLEST index is the one a lane finds last (the subgroup test is a 255-bit scalar multiplication; where the
    cofactor is 1, the curve equation) and the one at the last index returns first (its flag bits), so on the device the word
    that keeps the failure is written in descending order of index and has to be replaced twice.  The report is the smallest
    index; with that failure repaired the next one, and so on, and with all three repaired the batch decodes."""
    from oracle.c import cbase
    F = Format(lib, C, group, comp)
    rnd = random.Random(seed)
    raws = known_points(lib, ctx, C, group, n, seed)
    good = [F.encode((Z.g1_from_raw if group == 1 else Z.g2_from_raw)(C, raws[i * F.rsz:(i + 1) * F.rsz])) for i in (130, 517, n - 1)]
    read, write, nflags = F.flag_values()
    stray = off_subgroup_point(F, rnd)
    slow = F.encode(stray) if stray is not None else None
    # not on the curve: random reduced values in the coordinate that carries the flag bits (x or an element of it; BN254
    # uncompressed: of y) until the oracle says so
    slot = F.ncoord - 1 if C.bn_like else 0
    off_curve = good[1]
    while F.oracle(off_curve, VALIDATE_FULL)[0] != Z.NOT_ON_CURVE:
        off_curve = F.with_coordinate(good[1], slot, rnd.randrange(1 << (F.slot_bits(slot) - 2)))
    not_reduced = F.with_coordinate(good[1], rnd.randrange(F.ncoord), C.q)
    bad_flags = write(good[2], 3 if C.bn_like else (7 if comp else 1))
    if slow is not None:
        plan = [(130, slow, Z.NOT_IN_SUBGROUP), (517, off_curve, Z.NOT_ON_CURVE), (n - 1, bad_flags, Z.BAD_FLAGS)]
    else:
        plan = [(130, off_curve, Z.NOT_ON_CURVE), (517, not_reduced, Z.NOT_REDUCED), (n - 1, bad_flags, Z.BAD_FLAGS)]
    assert len({i // 128 for i, _, _ in plan}) == 3 and len({st for _, _, st in plan}) == 3
    for _, w, st in plan:
        assert F.oracle(w, VALIDATE_FULL)[0] == st, (F.name, Z.STATUS_NAMES[st])
    clean = cbase.points_serialize(C, group, raws, comp)
    assert [clean[i * F.psz:(i + 1) * F.psz] for i in (130, 517, n - 1)] == good
    wire = bytearray(clean)
    for i, w, _ in plan:
        wire[i * F.psz:(i + 1) * F.psz] = w
    for k, (i, _, st) in enumerate(plan):
        assert F.decode(ctx, bytes(wire), n, VALIDATE_FULL) == ((i, st), None), (F.name, "failures left: %d" % (3 - k))
        wire[i * F.psz:(i + 1) * F.psz] = clean[i * F.psz:(i + 1) * F.psz]
    assert F.decode(ctx, bytes(wire), n, VALIDATE_FULL) == (None, raws)


# ---- key streams: the loader names the vector and the index of a bad point ---------------------------------------------------------
def key_stream_damage_case(lib, ctx, C, n=12, compressed=False):
    """One damaged point in each vector of an ark_groth16::ProvingKey stream in turn -- a_query, b_g1_query, b_g2_query, h_query,
    l_query and the verifying key's gamma_abc_g1 -- at its last index and at one in the middle: ark355_pk_load_bytes refuses
    the stream with EINVAL and a text that names that vector, that index and the status the oracle decoder gives the bytes."""
    from snark_amd._binding import EINVAL, Ark355Error
    A, B, Cm, z, ell = S.cs_to_instance(S.bench_lc_cs(C.r, n))
    opk = G.setup(C, A, B, Cm, ell, len(z), G.Trapdoor(tau=0xABCDEF123, alpha=3, beta=5, gamma=7, delta=11))
    stream = Z.pk_bytes(C, opk, compressed)
    s1, s2 = lib.point_size(C.curve_id, 1, compressed), lib.point_size(C.curve_id, 2, compressed)
    # where each vector's points start (oracle/serialize.py pk_bytes)
    off = s1 + 3 * s2
    starts = {}
    for name, group, pts in (("gamma_abc_g1", 1, opk.vk.gamma_abc_g1), (None, 1, [0, 0]), ("a_query", 1, opk.a_query),
                             ("b_g1_query", 1, opk.b_g1_query), ("b_g2_query", 2, opk.b_g2_query), ("h_query", 1, opk.h_query),
                             ("l_query", 1, opk.l_query)):
        if name is None:
            off += 2 * s1                                        # beta_g1, delta_g1
            continue
        assert int.from_bytes(stream[off:off + 8], "little") == len(pts)
        starts[name] = (off + 8, group, len(pts))
        off += 8 + len(pts) * (s1 if group == 1 else s2)
    assert off == len(stream) and len(starts) == 6
    lib.dll.ark355_pk_free(lib.pk_load_bytes(ctx, C.curve_id, stream, compressed=compressed, validate=VALIDATE_FULL))
    for name, (start, group, count) in starts.items():
        F = Format(lib, C, group, compressed)
        for idx in sorted({count // 2, count - 1}):
            at = start + idx * F.psz
            w = bytearray(stream[at:at + F.psz])
            # the lowest bit of the encoding's last coordinate (BLS12-381: big-endian, its last byte; BN254: the first byte
            # of the last coordinate): a neighbouring x / y, or a payload under an infinity flag
            w[F.psz - 1 if not C.bn_like else F.psz - F.nb] ^= 1
            status = F.oracle(bytes(w), VALIDATE_FULL)[0]
            if status == 0:                                      # (a neighbouring x that is on the curve and in the subgroup: BN254 G1)
                w = bytearray(F.with_coordinate(bytes(w), 0, C.q))
                status = F.oracle(bytes(w), VALIDATE_FULL)[0]
            assert status != 0
            bad = stream[:at] + bytes(w) + stream[at + F.psz:]
            with pytest.raises(Ark355Error) as ei:
                lib.pk_load_bytes(ctx, C.curve_id, bad, compressed=compressed, validate=VALIDATE_FULL)
            text = "%s[%d]: %s" % (name, idx, {v: k for k, v in STATUS_TEXT.items()}[status])
            assert ei.value.code == EINVAL and str(ei.value).endswith(text), (str(ei.value), text)
