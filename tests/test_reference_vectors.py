"""Byte strings the reference project itself holds (tests/golden/reference_vectors.json: its ALICE_SK / ALICE_PK test
constants): the scalar codec of the C ABI on the secret key, the public key as a JubJub point recovered on Python integers, and
(GPU) the curve equation of that point evaluated with the library's Bls381Fr vector kernels."""
import json
import os

import numpy as np
import pytest

from oracle import pyref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.json")
R = pyref.FIELDS["Bls381Fr"][0]                 # BLS12-381 Fr = the JubJub base field
A = R - 1                                        # JubJub (ark-ed-on-bls12-381 0.3): a = -1, d = -(10240 / 10241)
D = (-10240 * pow(10241, -1, R)) % R
JUBJUB_ORDER = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7   # the prime-order subgroup (cofactor 8)


def _vec():
    return json.load(open(GOLD))


def _sqrt(v):
    """Tonelli-Shanks in BLS12-381 Fr (p - 1 = 2^32 t)"""
    s, t = pyref.two_adicity(R)
    z = pyref.FIELDS["Bls381Fr"][1]                 # a non-residue: the multiplicative generator
    m, c, x, b = s, pow(z, t, R), pow(v, (t + 1) // 2, R), pow(v, t, R)
    while b != 1:
        i, b2 = 0, b
        while b2 != 1:
            b2, i = b2 * b2 % R, i + 1
        cc = pow(c, 1 << (m - i - 1), R)
        m, c, x, b = i, cc * cc % R, x * cc % R, b * cc * cc % R
    assert x * x % R == v
    return x


def _te_add(P, Q):
    (x1, y1), (x2, y2) = P, Q
    t = D * x1 * x2 % R * y1 * y2 % R
    return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, R) % R, (y1 * y2 - A * x1 * x2) * pow(1 - t, -1, R) % R)


def _te_mul(k, P):
    acc = (0, 1)
    while k:
        if k & 1:
            acc = _te_add(acc, P)
        P, k = _te_add(P, P), k >> 1
    return acc


def _pk_point():
    """ark-ec 0.3 writes a twisted Edwards point compressed as x with EdwardsFlags::from_y_sign(y > -y) in bit 7 of the last
    byte (bit 6 unused): recover y from x on the curve and take the root the flag names"""
    b = bytes.fromhex(_vec()["ALICE_PK"]["hex"])
    flags = b[31] >> 6
    x = int.from_bytes(b, "little") & ((1 << 255) - 1)
    assert flags == 2 and x < R                # the y-sign flag is set; x is canonical once it is cleared
    y2 = (1 - A * x * x) * pow(1 - D * x * x, -1, R) % R
    assert pow(y2, (R - 1) // 2, R) == 1, "y^2 is not a square: the bytes are not a JubJub point"
    y = _sqrt(y2)
    if y < R - y:
        y = R - y
    return x, y


@pytest.fixture(scope="module")
def zk():
    import contangle_zkcp_amd as zk
    zk._lib = None
    zk.load()
    return zk


def test_secret_key_through_the_scalar_codec(zk):
    az = zk.ark_serialize
    sk = bytes.fromhex(_vec()["ALICE_SK"]["hex"])
    v = int.from_bytes(sk, "little")
    assert v < R
    got = az.scalars_from_bytes("Bls381Fr", sk, 1)
    want = pyref.mont("Bls381Fr", v)
    assert [int(w) for w in got[0]] == [(want >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    assert az.scalars_to_bytes("Bls381Fr", got) == sk


def test_public_key_is_a_jubjub_point_of_the_prime_order_subgroup():
    x, y = _pk_point()
    assert (A * x * x + y * y - 1 - D * x * x * y * y) % R == 0
    assert _te_mul(JUBJUB_ORDER, (x, y)) == (0, 1)
    assert _te_mul(8, (x, y)) != (0, 1)        # not of small order
    # the other root differs by the 2-torsion point (0, -1): on the curve, outside the subgroup -- the flag is what selects
    assert _te_mul(JUBJUB_ORDER, (x, R - y)) == (0, R - 1)
    # the bytes read as y (the later ark-serialize convention) also give a curve point, but not one of the subgroup
    yy = x
    xx = _sqrt((1 - yy * yy) * pow(A - D * yy * yy, -1, R) % R)
    assert _te_mul(JUBJUB_ORDER, (xx, yy)) != (0, 1)


def test_scalar_decoder_refuses_the_flagged_public_key_bytes(zk):
    """include/zkcp_amd_prover.h: Fr elements are canonical 32 bytes; the PK's flag bit puts its integer above the modulus"""
    pk = bytes.fromhex(_vec()["ALICE_PK"]["hex"])
    assert int.from_bytes(pk, "little") >= R
    with pytest.raises(zk.ZkError):
        zk.ark_serialize.scalars_from_bytes("Bls381Fr", pk, 1)


@pytest.mark.gpu
def test_public_key_curve_equation_on_the_device():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    import contangle_zkcp_amd as zk
    zk._lib = None
    zk.load()
    zk.init(0)
    try:
        x, y = _pk_point()
        F = "Bls381Fr"
        limbs = lambda v: np.array([[(pyref.mont(F, v % R) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]], dtype=np.uint64)
        dev = lambda v: torch.from_numpy(limbs(v).view(np.int64)).cuda()
        val = lambda t: pyref.unmont(F, sum(int(w) << (64 * i) for i, w in enumerate(t.cpu().numpy().view(np.uint64)[0].tolist())))

        def check(t, want, what):
            torch.cuda.synchronize()
            got = t.cpu().numpy().view(np.uint64)
            assert (got == limbs(want)).all(), (what, hex(val(t)), hex(want % R))

        xx, yy = dev(x), dev(y)
        zk.vec_op(F, "mul", xx, b=dev(x))
        check(xx, x * x, "x^2")
        zk.vec_op(F, "mul", yy, b=dev(y))
        check(yy, y * y, "y^2")
        dxy = xx.clone()
        zk.vec_op(F, "mul", dxy, b=yy)
        check(dxy, x * x * y * y, "x^2 y^2")
        zk.vec_op(F, "scale", dxy, scalar=limbs(D)[0])
        check(dxy, D * x * x * y * y, "d x^2 y^2")
        lhs = xx.clone()
        zk.vec_op(F, "scale", lhs, scalar=limbs(A)[0])
        check(lhs, A * x * x, "a x^2")
        zk.vec_op(F, "add", lhs, b=yy)
        check(lhs, A * x * x + y * y, "a x^2 + y^2")
        zk.vec_op(F, "sub", lhs, b=dev(1))
        check(lhs, A * x * x + y * y - 1, "a x^2 + y^2 - 1")
        zk.vec_op(F, "sub", lhs, b=dxy)
        check(lhs, 0, "a x^2 + y^2 - 1 - d x^2 y^2")
    finally:
        zk.shutdown()
