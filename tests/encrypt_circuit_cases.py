"""TEST INFRASTRUCTURE shared by tests/test_encrypt_circuit_emu.py (CPU tier: emulator build, and the host-only checks without any
device) and tests/test_encrypt_circuit_gpu.py (-m gpu): JubJub on the host, the R1CS of EncryptCircuit, the per-element witness kernel,
the plaintext kernel, the first-unsatisfied-row check and the whole path plaintext -> proof -> verify -- against RefEncrypt, a
restatement on Python integers that shares no code with the library: its own twisted-Edwards addition, RefPoseidon of
tests/poseidon_cases.py, and its own row-by-row evaluation of a CSR triple.  Every comparison is exact.

Geometry of the witness kernel (csrc/zk_encrypt_kernels.h): a workgroup of 64 lanes covers a tile of 1024 elements, lane t owns the
16 elements tile + t + 64 j (interleaved, so that the wave's loads and stores are coalesced), and the grid is not capped -- one tile
per workgroup, no grid-stride loop, hence no "second trip" size.  WITNESS_NS therefore holds, next to 1, 15 .. 17 and 1023 .. 1025 (the
end inside a lane's first element row, and one workgroup's share +- 1), the edges of this geometry: 63 .. 65, where the first lane gets
its second element.  "First, middle and last element of a lane's share" are j = 0, 8, 15 of lane 5; lane 7's whole share is zeros."""
import ctypes
import functools
import json
import os
import random

import numpy as np

from halo2_mock_cases import FIELD_IDS, dev, host, limbs_of, modulus, mont, ptr, unmont
from poseidon_cases import RefPoseidon, filled, reference_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
FIELD = "Bls381Fr"
FIELDS = ["PallasFp", "PallasFq", "Bn254Fr", "Bls381Fr"]
P = modulus(FIELD)
D = (-10240 * pow(10241, -1, P)) % P
ORDER = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
GEN = (8076246640662884909881801758704306714034609987455869804520522091855516602923,
       13262374693698910701929044844600465831413122818447359594527400194675274060458)
LANES, SHARE, TILE = 64, 16, 1024                 # csrc/zk_encrypt_kernels.h: ENC_WG, ENC_K, ENC_TILE
WITNESS_NS = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]
PLAINTEXT_NS = [1, 255, 256, 257]
UNSAT_NS = [1, 17]
FULL = 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------- the restatement
def ref_on_curve(pt):
    x, y = pt
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def ref_add(p1, p2):
    """a = -1: x3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), y3 = (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2)"""
    (x1, y1), (x2, y2) = p1, p2
    t = D * x1 * x2 * y1 * y2 % P
    return (x1 * y2 + y1 * x2) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P


def ref_mul(k, pt):
    acc = (0, 1)
    for bit in bin(k)[2:] if k else "":
        acc = ref_add(acc, acc)
        if bit == "1":
            acc = ref_add(acc, pt)
    return acc


class RefEncrypt:
    """encryption.rs on Python integers: encrypt, the per-element witness of its circuit, and the evaluation of an R1CS row by row"""

    def __init__(self):
        d, ark, mds = reference_constants()
        self.poseidon = RefPoseidon(P, 2, 1, d["full_rounds"], d["partial_rounds"], d["alpha"], ark, mds)
        self.shape = (d["full_rounds"], d["partial_rounds"], d["alpha"], mds, ark)

    def dh(self, point):
        return self.poseidon.hash([point[0], point[1]])

    def encrypt(self, pk, msg, r, base=GEN):
        dh = self.dh(ref_mul(r, pk))
        return ref_mul(r, base), [(m + dh) % P for m in msg]

    @staticmethod
    def witness(msg, msg_len, n, dh, p=P):
        """-> (c2, m, b, k), n integers each"""
        m = [msg[i] % p if i < msg_len else 0 for i in range(n)]
        c2 = [(m[i] + dh) % p if i < msg_len else 0 for i in range(n)]
        b = [1 if x else 0 for x in c2]
        k = [pow(x, p - 2, p) if x else 1 for x in c2]
        return c2, m, b, k

    @staticmethod
    def first_unsatisfied(csr, z):
        """csr: [(row_ptr, col, val words)] for A, B, C; z: integers -> the smallest row with <A, z> <B, z> != <C, z>, or None"""
        coeff = {}

        def side(ptrs, cols, vals, i):
            acc = 0
            for q in range(int(ptrs[i]), int(ptrs[i + 1])):
                w = vals[q].tobytes()
                if w not in coeff:
                    coeff[w] = unmont(FIELD, vals[q:q + 1])[0]
                acc += coeff[w] * z[int(cols[q])]
            return acc % P

        for i in range(len(csr[0][0]) - 1):
            if side(*csr[0], i) * side(*csr[1], i) % P != side(*csr[2], i):
                return i
        return None


@functools.lru_cache(maxsize=None)
def ref():
    return RefEncrypt()


def alice():
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))
    return bytes.fromhex(v["ALICE_SK"]["hex"]), bytes.fromhex(v["ALICE_PK"]["hex"])


_circuits = {}


def circuit(zk, n, bits):
    """zk.encryption.EncryptCircuit over the reference's Poseidon set, one per library instance, n and scalar_bits"""
    key = (id(zk._lib), n, bits)
    if key not in _circuits:
        rf, rp, alpha, mds, ark = ref().shape
        prm = zk.poseidon.PoseidonParameters(FIELD, rf, rp, alpha, mds, ark)
        _circuits[key] = zk.encryption.EncryptCircuit(zk.encryption.Parameters(n, prm), scalar_bits=bits)
    return _circuits[key]


def seeded_key(seed):
    sk = random.Random("encrypt key %s" % seed).randrange(1, ORDER)
    return sk, ref_mul(sk, GEN)


def z_ints(circ, head, c2, fixed, m, b, k):
    z = list(head) + list(c2) + list(fixed) + list(m) + list(b) + list(k)
    assert len(z) == circ.n_vars
    return z


# ---------------------------------------------------------------- 1. JubJub on the host
def check_jubjub(zk):
    jj = zk.jubjub
    assert (jj.P, jj.D, jj.ORDER, jj.GENERATOR, jj.A) == (P, D, ORDER, GEN, P - 1)
    assert ref_on_curve(GEN) and jj.is_on_curve(GEN)
    assert ref_mul(ORDER, GEN) == (0, 1) and jj.mul(ORDER, GEN) == (0, 1) and jj.in_prime_subgroup(GEN)
    assert ref_mul(8, GEN) != (0, 1)
    assert GEN != (0, 1) and pow(2, ORDER - 1, ORDER) == 1 and 8 * ORDER == jj.COFACTOR * jj.ORDER      # ORDER passes a Fermat test
    rng = random.Random("jubjub")
    pts = [ref_mul(rng.randrange(1, ORDER), GEN) for _ in range(6)]
    two_torsion = (0, P - 1)
    for pt in pts:
        assert jj.is_on_curve(pt) and jj.mul(ORDER, pt) == (0, 1)
        assert jj.add(pt, pt) == ref_add(pt, pt) == ref_mul(2, pt)
        assert jj.add(pt, jj.neg(pt)) == (0, 1)
        assert jj.add(pt, (0, 1)) == pt and jj.add((0, 1), pt) == pt
        assert jj.add(pt, two_torsion) == ref_add(pt, two_torsion) == ((P - pt[0]) % P, (P - pt[1]) % P)
        k = rng.randrange(1 << 256)
        assert jj.mul(k, pt) == ref_mul(k, pt) == ref_mul(k % ORDER, pt)
        assert jj.from_bytes(jj.to_bytes(pt)) == pt and jj.from_bytes(jj.to_bytes(jj.neg(pt))) == jj.neg(pt)
        other = (pt[0], (P - pt[1]) % P)                  # the other root: same x, the flag differs
        assert jj.to_bytes(other)[:31] == jj.to_bytes(pt)[:31] and jj.to_bytes(other)[31] ^ jj.to_bytes(pt)[31] == 0x80
    for a, b in zip(pts, pts[1:]):
        assert jj.add(a, b) == ref_add(a, b) == jj.add(b, a) and ref_on_curve(jj.add(a, b))
    assert jj.mul(0, GEN) == (0, 1) and jj.add((0, 1), (0, 1)) == (0, 1)
    assert jj.from_bytes(jj.to_bytes((0, 1))) == (0, 1)
    sk, pk = jj.keygen(12345)
    assert (sk, pk) == (12345, ref_mul(12345, GEN))
    # the reference's ALICE_PK, as tests/test_reference_vectors.py finds it: x from the bytes, on the curve, y the greater root, in the subgroup
    sk_bytes, pk_bytes = alice()
    pt = jj.from_bytes(pk_bytes)
    assert pt[0] == int.from_bytes(pk_bytes, "little") & ((1 << 255) - 1) and ref_on_curve(pt) and pt[1] > P - pt[1]
    assert ref_mul(ORDER, pt) == (0, 1) and jj.to_bytes(pt) == pk_bytes
    # the pair is not a key pair over GENERATOR (upstream's generator is unpinned)
    assert jj.keygen(int.from_bytes(sk_bytes, "little"))[1] != pt
    # refusals of the decoder
    good = bytearray(jj.to_bytes(pts[0]))
    for bad in (bytes(good[:31]), bytes(good) + b"\0", (P).to_bytes(32, "little"), ((1 << 255) - 1).to_bytes(32, "little"),
                jj.to_bytes(two_torsion)):
        try:
            jj.from_bytes(bad)
        except jj.PointDecodeError:
            continue
        raise AssertionError("decoded %s" % bad.hex())
    x = next(x for x in range(2, 100) if pow((1 + x * x) * pow(1 - D * x * x, P - 2, P) % P, (P - 1) // 2, P) != 1)
    try:
        jj.from_bytes(x.to_bytes(32, "little"))
        raise AssertionError("decoded an x that is on no curve point")
    except jj.PointDecodeError:
        pass
    assert jj.from_bytes(jj.to_bytes(two_torsion), check_subgroup=False) == two_torsion


# ---------------------------------------------------------------- 2. the matrices
def csr_bytes(csr):
    return b"".join(np.ascontiguousarray(a).tobytes() for side in csr for a in side)


def check_csr(zk, n=3, bits=8):
    """shape, coverage, and independence of the witness: two valued passes with different keys, messages and r lay out the same rows"""
    circ = circuit(zk, n, bits)
    csr = circ.csr()
    rows = circ.num_constraints()
    assert circ.num_inputs == n + 3 and circ.n_vars == 4 * n + 3 + circ.num_fixed and rows == circ.num_fixed_rows + 4 * n
    seen = np.zeros(circ.n_vars, dtype=bool)
    terms = np.zeros(rows, dtype=np.int64)
    for row_ptr, col, val in csr:
        assert row_ptr.dtype == np.uint64 and col.dtype == np.uint32 and val.dtype == np.uint64
        assert row_ptr.shape == (rows + 1,) and row_ptr[0] == 0 and int(row_ptr[-1]) == col.shape[0] and val.shape == (col.shape[0], 4)
        assert (np.diff(row_ptr.astype(np.int64)) >= 0).all() and int(col.max()) < circ.n_vars
        seen[col] = True
        terms += np.diff(row_ptr.astype(np.int64))
    assert seen.all(), "a variable occurs in no row: %s" % np.nonzero(~seen)[0][:8].tolist()
    assert (terms > 0).all(), "a row is empty on all three sides"
    rng = random.Random("csr %d %d" % (n, bits))
    layouts = [circ.fixed_section(None, None, None).rows]
    for seed in (1, 2):
        _, pk = seeded_key(seed)
        r = rng.randrange(1 << bits)
        layouts.append(circ.fixed_section(pk, r, ref_mul(r, GEN)).rows)
    assert layouts[0] == layouts[1] == layouts[2]
    fresh = zk.encryption.EncryptCircuit(circ.params, scalar_bits=bits)
    fresh.fixed_assignment(seeded_key(3)[1], rng.randrange(1 << bits))
    assert csr_bytes(fresh.csr()) == csr_bytes(csr)


def check_reference_size(zk):
    """the reference's own test size fits the 2^20 domain: rows + num_inputs <= 2^20 at n = 196608, scalar_bits = 256"""
    n = 196608
    circ = circuit(zk, n, 256)
    assert circ.num_constraints() + n + 3 <= 1 << 20, circ.num_constraints()
    csr = circ.csr()
    assert all(side[0].shape[0] == circ.num_constraints() + 1 for side in csr)
    assert int(max(side[1].max() for side in csr)) == circ.n_vars - 1


# ---------------------------------------------------------------- 3. satisfaction on Python integers
def r_values(bits, seed):
    return [0, 1, (1 << bits) - 1, random.Random("r %d %s" % (bits, seed)).randrange(1 << bits)]


def check_satisfied_host(zk, bits, n=3):
    circ = circuit(zk, n, bits)
    csr = circ.csr()
    rng = random.Random("sat %d" % bits)
    for which, r in enumerate(r_values(bits, "sat")):
        pk = zk.jubjub.from_bytes(alice()[1]) if which == 0 else seeded_key(which)[1]
        msg = [rng.randrange(P) for _ in range(n - which % 2)]
        c1, dh, head, fixed = circ.fixed_assignment(pk, r)
        want_c1, want_c2 = ref().encrypt(pk, msg, r)
        assert c1 == want_c1 == tuple(head[1:]) and dh == ref().dh(ref_mul(r, pk)) and len(fixed) == circ.num_fixed
        c2, m, b, k = RefEncrypt.witness(msg, len(msg), n, dh)
        assert c2[:len(msg)] == want_c2
        z = z_ints(circ, head, c2, fixed, m, b, k)
        assert z[1:3] == list(want_c1) and z[3:3 + len(msg)] == want_c2 and z[circ.dh_col] == dh
        assert RefEncrypt.first_unsatisfied(csr, z) is None, (bits, r)
        z[circ.m0] = (z[circ.m0] + 1) % P                     # the reference evaluation does notice a wrong plaintext
        assert RefEncrypt.first_unsatisfied(csr, z) == circ.num_fixed_rows + 3
    try:
        circ.fixed_assignment(seeded_key(1)[1], 1 << bits)
        raise AssertionError("an r of more than scalar_bits bits was accepted")
    except ValueError:
        pass


# ---------------------------------------------------------------- 4. the witness kernel
def elib(zk):
    return zk.encryption._elib()


def witness_message(p, n, dh, seed):
    """n canonical integers with c2 = 0 (m = -dh) at the first, a middle and the last element of lane 5's share, over the whole share of
    lane 7, and at both ends of the vector; 0, 1, p - 1 among the rest"""
    rng = random.Random("witness %s" % seed)
    msg = [rng.choice([0, 1, p - 1]) if rng.random() < 0.1 else rng.randrange(p) for _ in range(n)]
    zeros = [5 + LANES * j for j in (0, 8, 15)] + [7 + LANES * j for j in range(SHARE)] + [0, n - 1, TILE + 5]
    for i in zeros:
        if i < n:
            msg[i] = (-dh) % p
    return msg


def call_witness(zk, field, msg_words, msg_len, n, dh, expect=0):
    """the C entry on four separate output buffers of n + 1 elements of 0xFF bytes -> (c2, m, b, k) words, after the guard checks"""
    d_msg = dev(zk, msg_words) if len(msg_words) else None
    outs = [dev(zk, filled(n + 1)) for _ in range(4)]
    dh_words = mont(field, [dh])
    st = elib(zk).zk_encrypt_witness_device(FIELD_IDS[field], ptr(d_msg) if d_msg is not None else None, msg_len, n, ptr(dh_words),
                                            *[ptr(o) for o in outs], None)
    assert st == expect, st
    got = [host(o) for o in outs]
    if d_msg is not None:
        assert (host(d_msg) == msg_words).all(), "the message changed"
    for g in got:
        assert (g[n] == FULL).all(), "written past the end"
    return [g[:n] for g in got]


def check_witness(zk, field, n):
    p = modulus(field)
    rng = random.Random("witness dh %s %d" % (field, n))
    for dh in (0, 1, p - 1, rng.randrange(p)):
        msg = witness_message(p, n, dh, "%s %d" % (field, n))
        words = mont(field, msg)
        for msg_len in sorted({0, 1, n - 1, n}):
            want = RefEncrypt.witness(msg, msg_len, n, dh, p)
            got = call_witness(zk, field, words, msg_len, n, dh)
            for name, g, w in zip(("c2", "m", "b", "k"), got, want):
                bad = np.nonzero((g != mont(field, w)).any(axis=1))[0]
                assert bad.size == 0, (field, n, msg_len, dh, name, bad[:8].tolist())
    # the outputs as adjacent segments of one buffer, as assign lays them out, with the message shorter than its buffer
    msg_len = n // 2
    d_msg, d_z = dev(zk, words), dev(zk, filled(4 * n + 2))
    seg = lambda q: ctypes.c_void_p(ptr(d_z).value + 32 * (1 + q * n))      # noqa: E731
    dh_words = mont(field, [dh])
    assert elib(zk).zk_encrypt_witness_device(FIELD_IDS[field], ptr(d_msg), msg_len, n, ptr(dh_words), seg(0), seg(1), seg(2), seg(3), None) == 0
    got = host(d_z)
    want = RefEncrypt.witness(msg, msg_len, n, dh, p)
    assert (got[0] == FULL).all() and (got[-1] == FULL).all()
    assert (got[1:-1] == np.concatenate([mont(field, w) for w in want])).all(), (field, n)


def check_witness_large(zk, n=196608):
    """GPU: the reference's size with its all-bytes plaintext shape; dh = -3, so every byte 3 gives an empty element.  k o c2 == b and
    b o b == b on the device over the whole vectors, then 256 seeded positions and both ends against Python integers."""
    enc = zk.encryption
    data = bytes((i * 7 + i // 256) % 256 for i in range(n))
    d_msg = enc.bytes_to_plaintext_chunks_direct(data, n)
    dh = P - 3
    d_out = dev(zk, filled(4 * n))
    c2, m, b, k = (d_out[q * n:(q + 1) * n] for q in range(4))
    enc.encrypt_witness(d_msg, n, n, dh, c2, m, b, k)
    prod, sq = k.clone(), b.clone()
    zk.vec_op(FIELD, "mul", prod, b=c2)
    zk.vec_op(FIELD, "sub", prod, b=b)
    zk.vec_op(FIELD, "mul", sq, b=b)
    zk.vec_op(FIELD, "sub", sq, b=b)
    assert not host(prod).any(), "k o c2 != b somewhere"
    assert not host(sq).any(), "b is not boolean somewhere"
    rng = random.Random("large")
    pos = sorted({0, n - 1, data.index(3), data.rindex(3)} | {rng.randrange(n) for _ in range(256)})
    msg = [data[i] for i in pos]
    want = RefEncrypt.witness(msg, len(msg), len(msg), dh)
    assert 0 in want[0]
    for g, w in zip((c2, m, b, k), want):
        assert (host(g)[pos] == mont(FIELD, w)).all()
    assert (host(d_msg)[pos] == mont(FIELD, msg)).all()


def check_witness_refusals(zk, n=17):
    lib, f, p = elib(zk), FIELD_IDS[FIELD], P
    words = mont(FIELD, witness_message(p, n, 9, "refusals"))
    d_msg = dev(zk, words)
    d_out = dev(zk, filled(4 * n + 4))
    at = lambda buf, elems, extra=0: ctypes.c_void_p(ptr(buf).value + 32 * elems + extra)      # noqa: E731
    o = [at(d_out, q * (n + 1)) for q in range(4)]
    dh_words, dh_p, dh_max = mont(FIELD, [9]), limbs_of([p]), limbs_of([(1 << 256) - 1])      # (kept alive: the calls take their addresses)
    dh = ptr(dh_words)
    for which, st in enumerate((
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, dh, at(d_out, 0, 8), o[1], o[2], o[3], None),          # misaligned outputs
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, dh, o[0], o[1], o[2], at(d_out, 3 * (n + 1), 4), None),
            lambda: lib.zk_encrypt_witness_device(f, at(d_msg, 0, 8), n - 1, n, dh, o[0], o[1], o[2], o[3], None),            # misaligned message
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, dh, o[0], at(d_out, n - 1), o[2], o[3], None),         # m begins at c2's last element
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, dh, o[0], o[1], o[2], o[2], None),                     # k = b
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, dh, o[3], o[1], o[2], at(d_out, 3 * (n + 1) + 1), None),
            lambda: lib.zk_encrypt_witness_device(f, at(d_out, n - 1), n, n, dh, o[0], o[1], o[2], o[3], None),               # the message inside c2
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n + 1, n, dh, o[0], o[1], o[2], o[3], None),                 # msg_len > n
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, ptr(dh_p), o[0], o[1], o[2], o[3], None),                # dh = p
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, ptr(dh_max), o[0], o[1], o[2], o[3], None),
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, None, o[0], o[1], o[2], o[3], None),
            lambda: lib.zk_encrypt_witness_device(f, None, n, n, dh, o[0], o[1], o[2], o[3], None),
            lambda: lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, dh, o[0], None, o[2], o[3], None),
            lambda: lib.zk_encrypt_witness_device(9, ptr(d_msg), n, n, dh, o[0], o[1], o[2], o[3], None))):
        assert st() == INVALID_ARG, which
        assert (host(d_out) == FULL).all(), ("a refused call wrote", which)
        assert (host(d_msg) == words).all()
    # and the good call on the same buffers
    assert lib.zk_encrypt_witness_device(f, ptr(d_msg), n, n, dh, o[0], o[1], o[2], o[3], None) == 0
    want = RefEncrypt.witness(witness_message(p, n, 9, "refusals"), n, n, 9)
    got = host(d_out)
    for q in range(4):
        assert (got[q * (n + 1):q * (n + 1) + n] == mont(FIELD, want[q])).all() and (got[q * (n + 1) + n] == FULL).all()


# ---------------------------------------------------------------- 5. the plaintext kernel
def check_plaintext(zk, field, n):
    lib = elib(zk)
    rng = random.Random("plaintext %d" % n)
    data = bytes(range(256)) * (n // 256) + bytes(rng.randrange(256) for _ in range(n % 256)) if n >= 256 else bytes(rng.randrange(256) for _ in range(n))
    d_bytes = dev(zk, np.frombuffer(data + b"\xee", dtype=np.uint8))
    for length in sorted({0, 1, n - 1, n, n + 1}):          # n + 1: the byte past n is dropped
        d_out = dev(zk, filled(n + 1))
        assert lib.zk_plaintext_from_bytes_device(FIELD_IDS[field], ptr(d_bytes), length, ptr(d_out), n, None) == 0
        got = host(d_out)
        want = [data[i] if i < length else 0 for i in range(n)]
        assert (got[:n] == mont(field, want)).all() and (got[n] == FULL).all(), (field, n, length)
    assert host(d_bytes).tobytes() == data + b"\xee"


def check_plaintext_mirror(zk):
    """every byte value through zk.encryption.bytes_to_plaintext_chunks_direct; a size below and above the length; refusals"""
    enc, lib = zk.encryption, elib(zk)
    data = bytes(range(256))
    for size in (256, 100, 300, 1):
        got = host(enc.bytes_to_plaintext_chunks_direct(data, size))
        assert got.shape == (size, 4) and (got == mont(FIELD, [data[i] if i < 256 else 0 for i in range(size)])).all(), size
    assert (host(enc.bytes_to_plaintext_chunks_direct(b"", 5)) == 0).all()
    d_bytes, d_out = dev(zk, np.frombuffer(data, dtype=np.uint8)), dev(zk, filled(8))
    f = FIELD_IDS[FIELD]
    for st in (lib.zk_plaintext_from_bytes_device(f, ptr(d_bytes), 4, None, 4, None),
               lib.zk_plaintext_from_bytes_device(f, None, 4, ptr(d_out), 4, None),
               lib.zk_plaintext_from_bytes_device(f, ptr(d_bytes), 4, ctypes.c_void_p(ptr(d_out).value + 8), 4, None),
               lib.zk_plaintext_from_bytes_device(f, ctypes.c_void_p(ptr(d_out).value + 40), 4, ptr(d_out), 4, None),
               lib.zk_plaintext_from_bytes_device(9, ptr(d_bytes), 4, ptr(d_out), 4, None)):
        assert st == INVALID_ARG
    assert (host(d_out) == FULL).all()


# ---------------------------------------------------------------- 6. the first unsatisfied row
def honest(zk, circ, seed, msg_len=None):
    """-> (pk, sk, r, msg integers, msg device buffer, d_z) for a seeded witness"""
    n = circ.n
    rng = random.Random("honest %s %d" % (seed, n))
    sk, pk = seeded_key(seed)
    r = rng.randrange(1 << circ.scalar_bits)
    msg = [rng.randrange(1, P) for _ in range(n if msg_len is None else msg_len)]
    d_msg = dev(zk, mont(FIELD, msg))
    return pk, sk, r, msg, d_msg, circ.assign(pk, r, d_msg)


def z_words_to_ints(words):
    return unmont(FIELD, words)


def check_first_unsatisfied(zk, n, bits=8):
    g16 = zk.groth16
    circ = circuit(zk, n, bits)
    csr = circ.csr()
    A, B, C = circ.matrices()
    pk, _, r, msg, d_msg, d_z = honest(zk, circ, "unsat")
    z0 = host(d_z).copy()
    zi = z_words_to_ints(z0)
    # the device assignment is RefEncrypt's, element for element
    c1, c2 = ref().encrypt(pk, msg, r)
    dh = ref().dh(ref_mul(r, pk))
    assert zi[0] == 1 and tuple(zi[1:3]) == c1 and zi[3:3 + n] == c2 and zi[circ.dh_col] == dh
    assert zi[circ.m0:] == [x for part in RefEncrypt.witness(msg, n, n, dh)[1:] for x in part]
    assert g16.first_unsatisfied(A, B, C, d_z) is None and RefEncrypt.first_unsatisfied(csr, zi) is None
    assert (host(d_z) == z0).all(), "the check changed z"
    i, f0 = n - 1, circ.num_fixed_rows
    bit_col = circ.num_inputs + min(3, bits - 1)               # a bit of r: the first fixed witnesses

    def planted(changes, want_row=None):
        z = list(zi)
        for col, v in changes:
            z[col] = v % P
        want = RefEncrypt.first_unsatisfied(csr, z)
        if want_row is not None:
            assert want == want_row, (want, want_row)
        got = g16.first_unsatisfied(A, B, C, dev(zk, mont(FIELD, z)))
        assert got == want, (n, changes, got, want)
        return got

    other_c2 = next(v for v in (zi[3 + i] + 1, zi[3 + i] + 2) if v % P)
    assert planted([(3 + i, other_c2)], f0 + 4 * i + 1) is not None         # k_i is no longer its inverse: the element's row 2 ...
    assert planted([(3 + i, other_c2), (circ.k0 + i, pow(other_c2 % P, P - 2, P))], f0 + 4 * i + 3) is not None   # ... and with k mended, exactly row 4
    assert planted([(circ.b0 + i, 1 - zi[circ.b0 + i])], f0 + 4 * i + 1) is not None       # b_i flipped: 0 is boolean, so row 2 names it
    assert planted([(circ.b0 + i, 2)], f0 + 4 * i) is not None                              # b_i not boolean: row 1
    assert planted([(circ.k0 + i, zi[circ.k0 + i] + 1)], f0 + 4 * i + 1) is not None
    low = planted([(bit_col, 1 - zi[bit_col])])
    assert low is not None and low < f0
    c1_row = planted([(1, zi[1] + 1)], f0 - 2)                                              # c1' == c1 closes the fixed section
    assert planted([(circ.m0 + i, zi[circ.m0 + i] + 1)], f0 + 4 * i + 3) is not None
    # two faults: the lower row wins, whichever is planted first
    assert planted([(circ.k0 + i, 5), (1, zi[1] + 1)]) == c1_row
    assert planted([(circ.k0 + i, 5), (circ.b0, 2)]) == f0
    # the documented quirk: an empty ciphertext element (c2_i = 0, b_i = 0) leaves m_i and k_i free
    assert planted([(3 + i, 0), (circ.b0 + i, 0), (circ.m0 + i, 12345), (circ.k0 + i, 777)]) is None
    for mtx in (A, B, C):
        mtx.free()


def check_first_unsatisfied_refusals(zk, n=1, bits=8):
    g16 = zk.groth16
    circ = circuit(zk, n, bits)
    A, B, C = circ.matrices()
    lib, f = g16._lib(), FIELD_IDS[FIELD]
    d_z = honest(zk, circ, "unsat refusals")[-1]
    rows, need = A.n_rows, 3 * A.n_rows + g16.R1CS_CHECK_SCRATCH_ELEMS
    d_s = dev(zk, filled(need))
    out = ctypes.c_uint64(7)
    call = lambda z=ptr(d_z), zl=circ.n_vars, s=ptr(d_s), sl=need, o=ctypes.byref(out), fld=f, a=A.handle: \
        lib.zk_r1cs_first_unsatisfied_device(fld, a, B.handle, C.handle, z, zl, s, sl, o, None)      # noqa: E731
    for st in (call(z=None), call(s=None), call(o=None), call(zl=circ.n_vars - 1), call(sl=need - 1), call(fld=2),
               call(z=ctypes.c_void_p(ptr(d_z).value + 8)), call(s=ctypes.c_void_p(ptr(d_s).value + 8)), call(s=ptr(d_z), sl=circ.n_vars)):
        assert st == INVALID_ARG, st
    assert call(a=1 << 40) == -7
    assert out.value == 7 and (host(d_s) == FULL).all()
    assert call() == 0 and out.value == FULL and rows == circ.num_constraints()
    for mtx in (A, B, C):
        mtx.free()


# ---------------------------------------------------------------- 7. plaintext -> proof -> verify
def check_end_to_end(zk, n, bits):
    g16, enc, jj = zk.groth16, zk.encryption, zk.jubjub
    circ = circuit(zk, n, bits)
    params = circ.params
    A, B, C = circ.matrices()
    key = g16.generate_random_parameters("Bls381", A, B, C, circ.num_inputs, circ.n_vars)
    prover = g16.Prover("Bls381", key, A, B, C, circ.num_inputs, lambda arr: dev(zk, np.ascontiguousarray(arr, dtype=np.uint64)))
    vk = g16.VerifyingKey.from_parameters(key)
    pvk = g16.prepare_verifying_key(vk)
    rng = random.Random("e2e %d" % n)
    blinds = mont(FIELD, [rng.randrange(P), rng.randrange(P)])
    short = max(n - 2, 1)                                          # a message shorter than n
    pk, sk, r, msg, d_msg, d_z = honest(zk, circ, "e2e", msg_len=short)
    assert jj.keygen(sk)[1] == pk
    cipher = enc.encrypt(pk, d_msg, r, params)
    want_c1, want_c2 = ref().encrypt(pk, msg, r)
    assert cipher[0] == want_c1 and (host(cipher[1]) == mont(FIELD, want_c2)).all()
    assert (host(enc.decrypt(cipher, sk, params)) == mont(FIELD, msg)).all(), "decrypt(encrypt(m)) != m"
    full_msg = [rng.randrange(P) for _ in range(n)]
    d_full = dev(zk, mont(FIELD, full_msg))
    assert (host(enc.decrypt(enc.encrypt(pk, d_full, r, params), sk, params)) == mont(FIELD, full_msg)).all()
    public = enc.get_public_inputs(cipher, params)
    pub_host = host(public).copy()
    assert (pub_host == mont(FIELD, list(want_c1) + want_c2 + [0] * (n - short))).all()
    assert (host(d_z)[1:circ.num_inputs] == pub_host).all(), "the instance segment of z is not get_public_inputs"
    assert g16.first_unsatisfied(A, B, C, d_z) is None
    z_before = host(d_z).copy()
    (pa, pb, pc), proof = prover.prove_device(d_z, blinds[0], blinds[1])
    assert (host(d_z) == z_before).all(), "prove_device changed z"
    (qa, qb, qc), proof_host = prover.prove(z_before, blinds[0], blinds[1])
    assert proof == proof_host and (pa == qa).all() and (pb == qb).all() and (pc == qc).all()
    assert g16.verify(pvk, public, proof) is True
    assert g16.verify(pvk, pub_host, proof) is True
    # one ciphertext element changed
    bad = pub_host.copy()
    bad[2] = mont(FIELD, [want_c2[0] + 1])[0]
    assert g16.verify(pvk, bad, proof) is False
    bad = pub_host.copy()
    bad[1 + n] = mont(FIELD, [1])[0]                               # a padding element that is no longer empty
    assert g16.verify(pvk, bad, proof) is False
    # c1 replaced by another subgroup point
    bad = pub_host.copy()
    bad[0:2] = mont(FIELD, list(ref_mul(r + 1, GEN)))
    assert g16.verify(pvk, bad, proof) is False
    # the proof of M presented for the ciphertext of M'
    other = [(m + 1) % P for m in msg]
    other_cipher = enc.encrypt(pk, dev(zk, mont(FIELD, other)), r, params)
    assert g16.verify(pvk, enc.get_public_inputs(other_cipher, params), proof) is False
    # ... which has a proof of its own
    d_z2 = circ.assign(pk, r, dev(zk, mont(FIELD, other)))
    _, proof2 = prover.prove_device(d_z2, blinds[1], blinds[0])
    assert g16.verify(pvk, enc.get_public_inputs(other_cipher, params), proof2) is True
    assert g16.verify(pvk, public, proof2) is False
    vk.free()
    prover.free()
