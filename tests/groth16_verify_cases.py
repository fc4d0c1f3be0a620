"""TEST INFRASTRUCTURE shared by tests/test_groth16_verify_emu.py (CPU tier, emulator build) and tests/test_groth16_verify_gpu.py
(-m gpu): Groth16 verification -- the checked point decode on the device, prepare_inputs, the pairing and the public verify --
against the library's own encoder, the host checked decoder, Python-integer curve arithmetic (oracle.pyref), the independent
pairing of tests/pairing_ref.py and oracle.pyref_groth16.verify_logs.  Every comparison of field elements is bit for bit."""
import ctypes

import numpy as np

import groth16_setup_cases as gc
import pairing_ref as pr
from oracle import pyref
from oracle import pyref_groth16 as g16
from oracle import zk_oracle as orc
from parity_suite import to_device, to_host

PAIRINGS = gc.PAIRINGS
G1 = {"Bls381": "Bls381G1", "Bn254": "Bn254G1"}
G2 = {"Bls381": "Bls381G2", "Bn254": "Bn254G2"}
# one partial wave, exactly one wave, one wave and a lane, the same around a 256-lane workgroup, several grid strides
DECODE_SIZES = [1, 63, 64, 65, 255, 256, 257, 4099]
NONCANONICAL, FLAGS, NOT_ON_CURVE, NOT_IN_SUBGROUP = 1, 2, 3, 4
ZK_ERR_INVALID_ARG = -1


# ---------------------------------------------------------------- helpers
def base_field(curve):
    return pyref.CURVES[curve][0]


def multiples(curve, ks):
    """[k] G for every k, affine Montgomery limbs (k = 0 gives the identity, (0, 0))"""
    r = pyref.FIELDS[pyref.CURVES[curve][1]][0]
    return orc.fixed_base_mul(curve, gc.ints_to_arr([k % r for k in ks]), threads=8)


def seeded_points(curve, n, seed):
    r = pyref.FIELDS[pyref.CURVES[curve][1]][0]
    rng = pyref.Rng(seed)
    return multiples(curve, [1 + rng.below(r - 1) for _ in range(n)])


def coord_len(curve):
    return 8 * pyref.FIELDS[base_field(curve)][2]          # the encoded length of an Fq element of both base fields: the limb array


def enc_fq(curve, v, flags=0):
    b = bytearray(v.to_bytes(coord_len(curve), "little"))
    b[-1] |= flags
    return bytes(b)


def enc_point(curve, P, compressed):
    """ark-serialize 0.3 of an affine integer point of a G1 curve, written out here (not the library's encoder)"""
    p = pyref.FIELDS[base_field(curve)][0]
    x, y = P
    if compressed:
        return enc_fq(curve, x, 0x80 if y > p - y else 0)
    return enc_fq(curve, x) + enc_fq(curve, y)


def device_decode(zk, curve, buf, n, compressed):
    d_out = to_device(zk, np.ones((n, 2 * zk.base_limbs(curve)), dtype=np.uint64))
    zk.ark_serialize.points_from_bytes_checked_device(curve, buf, n, d_out, compressed=compressed)
    return to_host(zk, d_out)


def refused(zk, fn):
    try:
        fn()
    except zk.ark_serialize.PointDecodeError as e:
        return e.status, e.index, e.reason
    raise AssertionError("accepted")


# ---------------------------------------------------------------- 1. decode parity
def check_decode_parity(zk, curve, n, compressed, seed=0xDEC0DE):
    az = zk.ark_serialize
    pts = seeded_points(curve, n, seed + n)
    for i in {0, n // 2, n - 1} if n > 1 else ():                    # the infinity encoding at the first, a middle and the last index
        pts[i] = 0
    buf = az.points_to_bytes(curve, pts, compressed)
    ps = az.point_size(curve, compressed)
    assert len(buf) == n * ps
    if compressed and n >= 63:                                       # both y signs
        signs = {buf[i * ps + ps - 1] & 0x80 for i in range(n) if pts[i].any()}
        assert signs == {0, 0x80}
    if n > 1:
        assert buf[ps - 1] & 0x40 and buf[(n // 2) * ps + ps - 1] & 0x40 and buf[n * ps - 1] & 0x40
    got = device_decode(zk, curve, buf, n, compressed)
    assert (got == pts).all(), (curve, n, compressed, "device decode")
    assert (az.points_from_bytes_checked(curve, buf, n, compressed) == pts).all(), (curve, n, compressed, "host decode")
    if n == 1:                                                       # ... and a single infinity
        inf = az.points_to_bytes(curve, np.zeros_like(pts), compressed)
        assert not device_decode(zk, curve, inf, 1, compressed).any() and not az.points_from_bytes_checked(curve, inf, 1, compressed).any()


# ---------------------------------------------------------------- 2. decode refusals
def non_residue_x(curve):
    p, b = pyref.FIELDS[base_field(curve)][0], pyref.CURVES[curve][2]
    for x in range(1, 48):
        if pow((x ** 3 + b) % p, (p - 1) // 2, p) == p - 1:
            return x
    raise AssertionError("no small x off the curve")


def outside_subgroup_point(curve="Bls381G1"):
    """the first small x whose x^3 + 4 is a square: a point of E(Fq) that [r] does not kill (the cofactor of BLS12-381 G1 is ~2^126)"""
    p, b = pyref.FIELDS[base_field(curve)][0], pyref.CURVES[curve][2]
    r = pyref.FIELDS[pyref.CURVES[curve][1]][0]
    for x in range(1, 48):
        rhs = (x ** 3 + b) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p == rhs:
            P = (x, y)
            assert pyref.ec_on_curve(curve, P)
            assert pyref.ec_mul(curve, r, P) is not None, "[r] P != O"
            return P
    raise AssertionError("no small x on the curve")          # fails, never skips


def bad_encodings(curve, good, compressed):
    """(name, the bytes of one bad point, expected reason) for every refusal class of this curve and format; `good` = the encoding
    of a valid point"""
    p = pyref.FIELDS[base_field(curve)][0]
    cl = coord_len(curve)
    out = []
    x_ge_p = enc_fq(curve, p) if compressed else enc_fq(curve, p) + good[cl:]
    out.append(("x >= p", x_ge_p, NONCANONICAL))
    both = bytearray(good)
    both[-1] |= 0xC0
    out.append(("both flag bits", bytes(both), FLAGS))
    if compressed:
        out.append(("x^3 + b a non-residue", enc_fq(curve, non_residue_x(curve)), NOT_ON_CURVE))
    else:
        y = int.from_bytes(good[cl:], "little")
        out.append(("wrong y", good[:cl] + enc_fq(curve, (y + 1) % p), NOT_ON_CURVE))
        out.append(("y >= p", good[:cl] + enc_fq(curve, p + 1), NONCANONICAL))
    if curve == "Bls381G1":
        out.append(("outside the subgroup", enc_point(curve, outside_subgroup_point(curve), compressed), NOT_IN_SUBGROUP))
    # BN254 G1 has cofactor 1: every point of the curve is in the r-order subgroup, so that class does not exist there
    return out


def check_decode_refusals(zk, curve, compressed, n=257, seed=0xBAD):
    az = zk.ark_serialize
    pts = seeded_points(curve, n, seed)
    buf = az.points_to_bytes(curve, pts, compressed)
    ps = az.point_size(curve, compressed)
    classes = bad_encodings(curve, buf[5 * ps: 6 * ps], compressed)
    assert len(classes) == (4 if compressed else 5) - (curve != "Bls381G1")

    def planted(where):
        b = bytearray(buf)
        for i, enc in where:
            b[i * ps:(i + 1) * ps] = enc
        return bytes(b)

    for name, enc, reason in classes:
        assert len(enc) == ps
        for i in (0, n - 1, n // 2):
            b = planted([(i, enc)])
            assert refused(zk, lambda: device_decode(zk, curve, b, n, compressed)) == (ZK_ERR_INVALID_ARG, i, reason), (curve, name, i, "device")
            assert refused(zk, lambda: az.points_from_bytes_checked(curve, b, n, compressed)) == (ZK_ERR_INVALID_ARG, i, reason), (curve, name, i, "host")
    # two bad points: the smaller index wins, whichever reason it carries
    (_, e0, r0), (_, e1, r1) = classes[0], classes[1]
    for lo, hi in ((77, 200), (3, 256)):
        b = planted([(hi, e0), (lo, e1)])
        assert refused(zk, lambda: device_decode(zk, curve, b, n, compressed)) == (ZK_ERR_INVALID_ARG, lo, r1)
        assert refused(zk, lambda: az.points_from_bytes_checked(curve, b, n, compressed)) == (ZK_ERR_INVALID_ARG, lo, r1)
        b = planted([(lo, e0), (hi, e1)])
        assert refused(zk, lambda: device_decode(zk, curve, b, n, compressed)) == (ZK_ERR_INVALID_ARG, lo, r0)
    # the unchecked decoder keeps its behaviour: it takes the point outside the subgroup
    if curve == "Bls381G1":
        b = planted([(9, classes[-1][1])])
        assert az.points_from_bytes(curve, b, n, compressed=compressed, check_on_curve=True)[9].any()
    # the library is still usable
    assert (device_decode(zk, curve, buf, n, compressed) == pts).all()


def check_decode_arguments(zk):
    az = zk.ark_serialize
    lib = az._lib()
    pts = seeded_points("Bn254G1", 4, 1)
    buf = az.points_to_bytes("Bn254G1", pts, True)
    d_out = to_device(zk, np.zeros((5, 8), dtype=np.uint64))
    ptr = d_out.ctypes.data if isinstance(d_out, np.ndarray) else d_out.data_ptr()
    idx, why = ctypes.c_uint64(7), ctypes.c_uint64(7)
    call = lambda c, b, n, out: lib.zk_ark_points_decode_checked_device(c, b, n, 1, out, ctypes.byref(idx), ctypes.byref(why), None)
    for c in (zk.PALLAS, zk.VESTA, zk.BN254_G2, zk.BLS12_381_G2):
        assert call(c, buf, 4, ptr) == -6                              # ZK_ERR_UNSUPPORTED
    assert call(zk.BN254_G1, buf, 0, None) == 0
    assert call(zk.BN254_G1, None, 4, ptr) == -1 and call(zk.BN254_G1, buf, 4, None) == -1 and call(zk.BN254_G1, buf, 4, ptr + 8) == -1
    assert (idx.value, why.value) == (0, 0)
    assert not to_host(zk, d_out).any(), "refused calls write nothing"
    assert call(zk.BN254_G1, buf, 4, ptr) == 0 and (to_host(zk, d_out)[:4] == pts).all()
    for c in ("Pallas", "Vesta"):
        assert lib.zk_ark_points_decode_checked(zk.curve_id(c), buf, 1, 1, ptr, None, None) == -6


# ---------------------------------------------------------------- 3. pairing
def gt_ints(pairing, gt):
    """zk_pairing_product's 12 Montgomery coefficients -> integers, still in tower order"""
    fq = base_field(G1[pairing])
    return [pyref.unmont(fq, orc.limbs_to_int(row)) for row in np.ascontiguousarray(gt, dtype=np.uint64)]


def gt_poly(pairing, gt):
    return pr.Fq12(pairing).from_tower(gt_ints(pairing, gt))


def check_pairing(zk, pairing, seed=0xE):
    g16z = zk.groth16
    g1, g2 = G1[pairing], G2[pairing]
    F = pr.Fq12(pairing)
    r = pr.PARAMS[pairing]["r"]
    P, Q = multiples(g1, [1]), multiples(g2, [1])
    Pi, Qi = gc.py_points(g1, P)[0], gc.py_points(g2, Q)[0]
    assert Pi == tuple(pyref.CURVES[g1][3:5]) and Qi == tuple(pyref.CURVES[g2][3:5])
    e = gt_poly(pairing, g16z.pairing_product(pairing, P, Q))
    e_ref = pr.pairing(pairing, Pi, Qi)                                   # reference pairing 1
    assert e == e_ref, "e(G1, G2) against the polynomial-ring reference"
    assert e != F.one and F.pow(e, r) == F.one
    rng = pyref.Rng(seed)
    singles = []
    pairs = [(1 + rng.below(r - 1), 1 + rng.below(r - 1)) for _ in range(2)]
    for a, b in pairs:
        aP, bQ = multiples(g1, [a]), multiples(g2, [b])
        got = gt_poly(pairing, g16z.pairing_product(pairing, aP, bQ))
        assert got == F.pow(e_ref, a * b % r), "e(aP, bQ) = e(P, Q)^(ab)"
        singles.append((aP, bQ, got))
    a, b = pairs[0]                                                       # reference pairing 2: away from the generators
    assert singles[0][2] == pr.pairing(pairing, gc.py_points(g1, singles[0][0])[0], gc.py_points(g2, singles[0][1])[0])
    # a product of pairs = the product of the single pairings (one final exponentiation over three Miller loops)
    prod = g16z.pairing_product(pairing, np.concatenate([P, singles[0][0], singles[1][0]]), np.concatenate([Q, singles[0][1], singles[1][1]]))
    assert gt_poly(pairing, prod) == F.mul(F.mul(e, singles[0][2]), singles[1][2])
    # the identity in either slot gives 1; so does the empty product
    one = g16z.pairing_product(pairing, np.zeros_like(P), Q)
    assert gt_poly(pairing, one) == F.one and gt_ints(pairing, one) == [1] + [0] * 11
    assert gt_poly(pairing, g16z.pairing_product(pairing, P, np.zeros_like(Q))) == F.one
    assert gt_poly(pairing, g16z.pairing_product(pairing, P[:0], Q[:0])) == F.one
    mixed = g16z.pairing_product(pairing, np.concatenate([np.zeros_like(P), P]), np.concatenate([Q, Q]))
    assert gt_poly(pairing, mixed) == e
    # e(-P, Q) e(P, Q) = 1
    negP = multiples(g1, [r - 1])
    assert gt_poly(pairing, g16z.pairing_product(pairing, np.concatenate([negP, P]), np.concatenate([Q, Q]))) == F.one


# ---------------------------------------------------------------- 4. prepare_inputs
def synthetic_vk(zk, pairing, n_abc, seed):
    """a key of seeded multiples of the generators, gamma_abc_g1 on the device"""
    r = pr.PARAMS[pairing]["r"]
    rng = pyref.Rng(seed)
    k1 = [1 + rng.below(r - 1) for _ in range(n_abc + 1)]
    k2 = [1 + rng.below(r - 1) for _ in range(3)]
    p1, p2 = multiples(G1[pairing], k1), multiples(G2[pairing], k2)
    return zk.groth16.VerifyingKey(pairing, p1[0], p2[0], p2[1], p2[2], to_device(zk, p1[1:])), p1[1:]


def check_prepare_inputs(zk, pairing, n_inputs, seed=0x1C):
    g16z = zk.groth16
    field, g1 = gc.FIELD[pairing], G1[pairing]
    r = pr.PARAMS[pairing]["r"]
    vk, abc = synthetic_vk(zk, pairing, n_inputs + 1, seed + n_inputs)
    pvk = g16z.PreparedVerifyingKey(vk, None)
    rng = pyref.Rng(seed)
    xs = ([r - 1, 0, 1] + [rng.below(r) for _ in range(n_inputs)])[:n_inputs]        # the edge scalars first
    pts = gc.py_points(g1, abc)
    exp = pyref.ec_add(g1, pts[0], pyref.msm_naive(g1, xs, pts[1:]))
    for inputs in (gc.monts(field, xs), to_device(zk, gc.monts(field, xs))):         # host limbs, or a device buffer
        got = g16z.prepare_inputs(pvk, inputs)
        assert gc.py_points(g1, got.reshape(1, -1))[0] == exp, (pairing, n_inputs)
    # a length mismatch is upstream's MalformedVerifyingKey
    for bad in (n_inputs + 1, n_inputs - 1):
        if bad < 0:
            continue
        try:
            g16z.prepare_inputs(pvk, gc.monts(field, [5] * bad))
        except g16z.MalformedVerifyingKey:
            pass
        else:
            raise AssertionError("accepted %d inputs for %d" % (bad, n_inputs))
    out = np.zeros(2 * zk.base_limbs(g1), dtype=np.uint64)
    d_x = to_device(zk, gc.monts(field, [1] * (n_inputs + 2)))
    lib = g16z._lib()
    assert lib.zk_groth16_prepare_inputs(zk.curve_id(g1), vk.tail.handle if vk.tail else 0, vk.gamma_abc0.ctypes.data, vk.n,
                                         zk._ptr(d_x), n_inputs + 2, out.ctypes.data, None) == ZK_ERR_INVALID_ARG
    assert not out.any()
    vk.free()


# ---------------------------------------------------------------- 5. setup -> prove -> verify
def check_round_trip(zk, pairing, num_inputs=4, num_constraints=40, seed=0x60, long_rows=(17,)):
    """generate_random_parameters -> Prover.prove -> verify, the reference's idiom (circuits-ark/src/encryption.rs:407-410), then
    every single change that must turn the verdict"""
    g16z, az = zk.groth16, zk.ark_serialize
    field, g1, g2 = gc.FIELD[pairing], G1[pairing], G2[pairing]
    p = pyref.FIELDS[field][0]
    r1cs, z = g16.random_r1cs(field, seed, num_inputs=num_inputs, num_constraints=num_constraints, long_rows=long_rows)
    n_vars = len(z)
    dev = lambda arr: to_device(zk, arr)
    rng = pyref.Rng(seed + 1)

    def setup_and_prove():
        mats = gc.matrices(zk, field, r1cs, n_vars)
        params = g16z.generate_random_parameters(pairing, mats[0], mats[1], mats[2], num_inputs, n_vars)
        prover = g16z.Prover(pairing, params, mats[0], mats[1], mats[2], num_inputs, dev)
        proof, proof_bytes = prover.prove(gc.monts(field, z), gc.mont1(field, rng.below(p)), gc.mont1(field, rng.below(p)))
        return params, prover, proof, proof_bytes

    params, prover, (A, B, C), proof_bytes = setup_and_prove()
    public = z[1:num_inputs]                                   # z[0] = 1 is gamma_abc_g1[0]'s wire
    x = gc.monts(field, public)
    vk = g16z.VerifyingKey.from_parameters(params)
    pvk = g16z.prepare_verifying_key(vk)
    assert g16z.verify(vk, x, (A, B, C)) is True, pairing
    assert g16z.verify(pvk, x, proof_bytes) is True
    # one public input off by one; two public inputs swapped
    for i in {0, len(public) - 1}:
        off = list(public)
        off[i] = (off[i] + 1) % p
        assert g16z.verify(pvk, gc.monts(field, off), (A, B, C)) is False, ("input", i)
    if len(public) >= 2:
        sw = list(public)
        assert sw[0] != sw[-1]
        sw[0], sw[-1] = sw[-1], sw[0]
        assert g16z.verify(pvk, gc.monts(field, sw), (A, B, C)) is False, "swapped"
    # A, B or C replaced by another point of its subgroup
    other1, other2 = multiples(g1, [rng.below(p)])[0], multiples(g2, [rng.below(p)])[0]
    assert g16z.verify(pvk, x, (other1, B, C)) is False and g16z.verify(pvk, x, (A, other2, C)) is False
    assert g16z.verify(pvk, x, (A, B, other1)) is False
    assert g16z.verify(pvk, x, az.proof_to_bytes(pairing, A, B, other1)) is False
    # the key through its file: verifying_key_bytes -> VerifyingKey.deserialize (checked; gamma_abc_g1 decoded on the device)
    vk_bytes = params.verifying_key_bytes()
    vk2 = g16z.VerifyingKey.deserialize(pairing, vk_bytes)
    assert (to_host(zk, vk2.d_gamma_abc_g1) == params.points("gamma_abc_g1")).all()
    for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert (getattr(vk2, name) == params.points(name)[0]).all(), name
    assert g16z.verify(vk2, x, proof_bytes) is True
    # a proof made under other parameters
    params3, prover3, _, proof3 = setup_and_prove()
    assert g16z.verify(pvk, x, proof3) is False
    assert g16z.verify(g16z.VerifyingKey.from_parameters(params3), x, proof3) is True
    # a key whose gamma_abc_g1 holds a point outside the subgroup is refused when it is read (BN254 G1 has cofactor 1: there the
    # planted point is off the curve)
    s1, s2 = az.point_size(g1, True), az.point_size(g2, True)
    at = s1 + 3 * s2 + 8 + (num_inputs - 1) * s1
    if pairing == "Bls381":
        bad, reason = enc_point(g1, outside_subgroup_point(g1), True), NOT_IN_SUBGROUP
    else:
        bad, reason = enc_fq(g1, non_residue_x(g1)), NOT_ON_CURVE
    assert refused(zk, lambda: g16z.VerifyingKey.deserialize(pairing, vk_bytes[:at] + bad + vk_bytes[at + s1:])) == (ZK_ERR_INVALID_ARG, num_inputs - 1, reason)
    b2 = bytearray(vk_bytes)
    b2[s1 + s2 - 1] |= 0xC0                                     # beta_g2: the host decoder's share of the key
    assert refused(zk, lambda: g16z.VerifyingKey.deserialize(pairing, bytes(b2)))[2] == FLAGS
    for bad_len in (vk_bytes[:-1], vk_bytes + b"\0"):
        try:
            g16z.VerifyingKey.deserialize(pairing, bad_len)
        except ValueError:
            pass
        else:
            raise AssertionError("accepted a key of the wrong length")
    assert g16z.verify(vk2, x, proof_bytes) is True             # still usable
    for v in (vk, vk2):
        v.free()
    prover.free()
    prover3.free()


# ---------------------------------------------------------------- 6. agreement with the check in the exponent
def check_agrees_with_logs(zk, pairing, seed=0x10, num_inputs=3, num_constraints=40):
    g16z = zk.groth16
    field, g1, g2 = gc.FIELD[pairing], G1[pairing], G2[pairing]
    p = pyref.FIELDS[field][0]
    r1cs, z = g16.random_r1cs(field, seed, num_inputs=num_inputs, num_constraints=num_constraints, long_rows=(7,))
    key = g16.setup(r1cs, seed + 100)
    rng = pyref.Rng(seed + 200)
    r, s = rng.below(p), rng.below(p)
    a, b, c = g16.prove_logs(r1cs, key, z, r, s)
    mats = gc.matrices(zk, field, r1cs, len(z))
    params = gc.generate(zk, pairing, mats, num_inputs, len(z), gc.trapdoor_of(key))
    prover = g16z.Prover(pairing, params, mats[0], mats[1], mats[2], num_inputs, lambda arr: to_device(zk, arr))
    (A, B, C), _ = prover.prove(gc.monts(field, z), gc.mont1(field, r), gc.mont1(field, s))
    assert (A == multiples(g1, [a])[0]).all() and (B == multiples(g2, [b])[0]).all() and (C == multiples(g1, [c])[0]).all()
    pvk = g16z.prepare_verifying_key(g16z.VerifyingKey.from_parameters(params))
    pub = z[:num_inputs]
    assert g16.verify_logs(r1cs, key, pub, a, b, c) is True and g16z.verify(pvk, gc.monts(field, pub[1:]), (A, B, C)) is True
    c_bad = (c + 1) % p
    assert g16.verify_logs(r1cs, key, pub, a, b, c_bad) is False
    assert g16z.verify(pvk, gc.monts(field, pub[1:]), (A, B, multiples(g1, [c_bad])[0])) is False
    pub_bad = pub[:1] + [(pub[1] + 1) % p] + pub[2:]
    assert g16.verify_logs(r1cs, key, pub_bad, a, b, c) is False
    assert g16z.verify(pvk, gc.monts(field, pub_bad[1:]), (A, B, C)) is False
    # a forged proof that satisfies the equation in the exponent is accepted by both: a' = 2a, b' = b / 2 leave a b unchanged
    a2, b2 = 2 * a % p, b * pow(2, -1, p) % p
    assert g16.verify_logs(r1cs, key, pub, a2, b2, c) is True
    assert g16z.verify(pvk, gc.monts(field, pub[1:]), (multiples(g1, [a2])[0], multiples(g2, [b2])[0], C)) is True
    pvk.vk.free()
    prover.free()
