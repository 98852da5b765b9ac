"""Known answers that do NOT come from this repository: constants published by other implementations of the same curves,
checked against the oracle (and, where the product has the same object, against libark355 through the emulator / the GPU).
They pin conventions the Groth16 boundary depends on -- the group law of both G1 groups, and the generator / two-adic
root of unity of both scalar fields, which fix the order of every NTT domain (ark-poly's Radix2EvaluationDomain takes
group_gen = TWO_ADIC_ROOT_OF_UNITY^(2^(S - log2 N))).

Sources (quoted from memory of the public specifications; a wrong digit would fail these tests, it cannot silently pass):
  * generators:         G1 / G2 of BLS12-381 as fixed by the zcash / IETF pairing-friendly-curves text, G2 of alt_bn128 as
                        in EIP-197,
  * wire format:        the zcash compressed encodings of the BLS12-381 generators (96 / 192 hex digits) and of the point at
                        infinity (0xc0 00 ..), which ark-serialize's BLS12-381 implementation follows,
  * alt_bn128 / BN254:  (1, 2) + (1, 2) of EIP-196's test vectors ("chfast1"),
  * BLS12-381:          2 * G1 as listed with EIP-2537's G1 test vectors,
  * BLS12-381 Fr:       ROOT_OF_UNITY of zkcrypto/bls12_381 (generator 7, two-adicity 32),
  * BN254 Fr:           FrConfig::TWO_ADIC_ROOT_OF_UNITY of ark-bn254 (generator 5, two-adicity 28).
"""
import pytest

from helpers import z_bytes
from oracle.curves import g1, g2
from oracle.ntt import Domain
from oracle.fields import BLS12_381, BN254
from helpers import fr_vec_from_mont

BN254_2G = (0x030644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd3,
            0x15ed738c0e0a7c92e7845f96b2ae9c0a68a6a449e3538fc7ff3ebf7a5a18a2c4)
BLS_2G = (0x0572cbea904d67468808c8eb50a9450c9721db309128012543902d0ac358a62ae28f75bb8f1c7c42c39a8c5529bf0f4e,
          0x166a9d8cabc673a322fda673779d8e3822ba3ecb8670e461f73bb9021d5fd76a4c56d9d4cd16bd1bba86881979749d28)
BLS_FR_ROOT_2_32 = 0x16a2a19edfe81f20d09b681922c813b4b63683508c2280b93829971f439f0d2b
BN_FR_ROOT_2_28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904
BLS_G1 = (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
          0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)
BLS_G2 = ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
           0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
          (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
           0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))
BN_G2 = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed,
          0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
         (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa,
          0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))
ROOTS = {"bls12_381": (7, 32, BLS_FR_ROOT_2_32), "bn254": (5, 28, BN_FR_ROOT_2_28)}


def test_oracle_generators_are_the_published_ones():
    assert tuple(g1(BLS12_381).gen) == BLS_G1
    H = g2(BLS12_381).gen
    assert (tuple(H[0]), tuple(H[1])) == BLS_G2
    H = g2(BN254).gen
    assert (tuple(H[0]), tuple(H[1])) == BN_G2
    for C in (BLS12_381, BN254):          # and they have order r
        assert g1(C).mul(g1(C).gen, C.r) is None and g2(C).mul(g2(C).gen, C.r) is None


def test_oracle_wire_format_against_the_zcash_generator_encodings():
    from oracle import serialize as Z
    assert Z.g1_compressed(BLS12_381, g1(BLS12_381).gen).hex() == (
        "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
    assert Z.g2_compressed(BLS12_381, g2(BLS12_381).gen).hex() == (
        "93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
        "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")
    assert Z.g1_compressed(BLS12_381, None) == bytes([0xC0]) + bytes(47)
    assert Z.g2_compressed(BLS12_381, None) == bytes([0xC0]) + bytes(95)


def test_oracle_decoder_against_the_zcash_generator_encodings():
    """The oracle's DECODER (oracle/serialize.py g1_decode / g2_decode) on the published encodings: the compressed strings
    above, the uncompressed form (x || y, G2 c1 || c0, big-endian, no flag bit) of the published coordinates, and the two
    infinity encodings of either form -- in every validation mode."""
    from oracle import serialize as Z
    C = BLS12_381
    g1c = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
    g2c = bytes.fromhex("93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                        "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")
    g1u = b"".join(v.to_bytes(48, "big") for v in BLS_G1)
    g2u = b"".join(v.to_bytes(48, "big") for v in (BLS_G2[0][1], BLS_G2[0][0], BLS_G2[1][1], BLS_G2[1][0]))
    for mode in (Z.VALIDATE_NONE, Z.VALIDATE_FULL, Z.VALIDATE_CURVE):
        assert Z.g1_decode(C, g1c, True, mode) == BLS_G1 == tuple(g1(C).gen)
        assert Z.g1_decode(C, g1u, False, mode) == BLS_G1
        assert Z.g2_decode(C, g2c, True, mode) == BLS_G2
        assert Z.g2_decode(C, g2u, False, mode) == BLS_G2
        assert Z.g1_decode(C, bytes([0xC0]) + bytes(47), True, mode) is None
        assert Z.g2_decode(C, bytes([0xC0]) + bytes(95), True, mode) is None
        assert Z.g1_decode(C, bytes([0x40]) + bytes(95), False, mode) is None
        assert Z.g2_decode(C, bytes([0x40]) + bytes(191), False, mode) is None
        # the other sign of y is the negated generator
        flipped = bytes([g1c[0] ^ 0x20]) + g1c[1:]
        assert Z.g1_decode(C, flipped, True, mode) == (BLS_G1[0], C.q - BLS_G1[1])
    # alt_bn128: EIP-197's G2 generator and (1, 2), ark-ec SWFlags (little-endian, flags in the last byte)
    B = BN254
    assert Z.g1_decode(B, (1).to_bytes(32, "little"), True) == (1, 2)               # 2 < q - 2: the sign bit is clear
    assert Z.g1_decode(B, (1).to_bytes(31, "little") + b"\x80", True) == (1, B.q - 2)
    g2u = b"".join(v.to_bytes(32, "little") for v in (BN_G2[0][0], BN_G2[0][1], BN_G2[1][0], BN_G2[1][1]))
    assert Z.g2_decode(B, g2u, False) == BN_G2
    assert Z.g2_decode(B, Z.g2_compressed(B, BN_G2), True) == BN_G2
    for size, dec, comp in ((32, Z.g1_decode, True), (64, Z.g1_decode, False), (64, Z.g2_decode, True), (128, Z.g2_decode, False)):
        assert dec(B, bytes(size - 1) + b"\x40", comp) is None


def test_oracle_group_law_against_published_doublings():
    G = g1(BN254)
    assert G.gen == (1, 2)
    assert G.add(G.gen, G.gen) == BN254_2G and G.mul(G.gen, 2) == BN254_2G
    G = g1(BLS12_381)
    assert G.add(G.gen, G.gen) == BLS_2G and G.mul(G.gen, 2) == BLS_2G


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_oracle_two_adic_roots_of_unity(C):
    gen, s, root = ROOTS[C.name]
    assert pow(gen, (C.r - 1) >> s, C.r) == root
    assert pow(root, 1 << s, C.r) == 1 and pow(root, 1 << (s - 1), C.r) == C.r - 1
    # the oracle's domains are generated by exactly that root
    for log_n in (1, 5, 21):
        d = Domain(C, log_n)
        assert d.omega == pow(root, 1 << (s - log_n), C.r)


def _ntt_of_delta(lib, ctx, C, log_n):
    n = 1 << log_n
    xs = [0] * n
    xs[1] = 1
    return fr_vec_from_mont(C, lib.ntt(ctx, C.curve_id, z_bytes(C, xs), log_n, 0, 0))


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_product_ntt_uses_the_published_root(emul_lib, emul_ctx, C):
    """NTT of the unit vector e_1 is (1, w, w^2, ...): w must be the published root raised to 2^(S - log2 N)."""
    gen, s, root = ROOTS[C.name]
    for log_n in (2, 7):
        w = pow(root, 1 << (s - log_n), C.r)
        assert _ntt_of_delta(emul_lib, emul_ctx, C, log_n) == [pow(w, k, C.r) for k in range(1 << log_n)]


@pytest.mark.gpu
@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_device_ntt_uses_the_published_root(gpu_lib, gpu_ctx, C):
    gen, s, root = ROOTS[C.name]
    log_n = 12
    w = pow(root, 1 << (s - log_n), C.r)
    assert _ntt_of_delta(gpu_lib, gpu_ctx, C, log_n) == [pow(w, k, C.r) for k in range(1 << log_n)]
