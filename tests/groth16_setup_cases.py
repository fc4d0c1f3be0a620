"""TEST INFRASTRUCTURE shared by tests/test_groth16_setup_emu.py (CPU tier, emulator build) and tests/test_groth16_setup_gpu.py
(-m gpu): Groth16 key generation on the device (zk.groth16.generate_parameters and the entry points under it) against
Python integers, oracle.pyref_groth16.setup, the oracle's fixed-base points and oracle.pyref_ark's encoder.  Every comparison
is bit for bit."""
import random

import numpy as np

from oracle import pyref, pyref_ark
from oracle import pyref_groth16 as g16
from oracle import zk_oracle as orc
from parity_suite import to_device, to_host

PAIRINGS = ["Bls381", "Bn254"]
FIELD = {"Bls381": "Bls381Fr", "Bn254": "Bn254Fr"}
TRAPDOOR = ("alpha", "beta", "gamma", "delta", "tau")


# ---------------------------------------------------------------- conversions (bulk: the GPU tier moves 2^20-element vectors)
def ints_to_arr(xs):
    """Python integers < 2^256 -> u64 limbs [n, 4]"""
    if not len(xs):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def arr_to_ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    raw = a.tobytes()
    w = a.shape[-1] * 8
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def monts(field, xs):
    return orc.to_mont(field, ints_to_arr(xs)) if len(xs) else np.zeros((0, 4), dtype=np.uint64)


def unmonts(field, a):
    return arr_to_ints(orc.from_mont(field, np.ascontiguousarray(a, dtype=np.uint64)))


def mont1(field, x):
    return monts(field, [x])[0]


def py_points(curve, arr):
    """affine Montgomery limbs [n, 2L] -> the Python-integer points of oracle.pyref_ark (None = infinity; an Fq2 coordinate is (c0, c1))"""
    bf = pyref.CURVES[curve][0]
    nl = pyref.FIELDS[bf][2]
    k = 2 if pyref.is_g2(curve) else 1
    out = []
    for row in np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 2 * k * nl):
        if not row.any():
            out.append(None)
            continue
        v = [pyref.unmont(bf, orc.limbs_to_int(row[i * nl:(i + 1) * nl])) for i in range(2 * k)]
        out.append((v[0], v[1]) if k == 1 else ((v[0], v[1]), (v[2], v[3])))
    return out


# ---------------------------------------------------------------- systems
def matrices(zk, field, r1cs, n_vars):
    """the three resident matrices of a pyref_groth16-style system (CSR arrays built in bulk)"""
    out = []
    for k in "ABC":
        rows = r1cs[k]
        row_ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
        row_ptr[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
        col = np.array([j for r in rows for _, j in r], dtype=np.uint32)
        val = monts(field, [c for r in rows for c, _ in r])
        if not len(col):
            col, val = np.zeros(1, dtype=np.uint32), np.zeros((1, 4), dtype=np.uint64)
        out.append(zk.groth16.R1csMatrix(field, n_cols=n_vars, csr=(row_ptr, col, val)))
    return out


def fast_r1cs(field, seed, num_inputs, num_constraints):
    """a satisfied system like pyref_groth16.random_r1cs, generated quickly enough for 2^20 constraints: constraint i defines
    a fresh witness variable w = <LA, z> <LB, z>.  Variable 0 (the constant one) is in the A row of every fourth constraint, so
    its column is dense, and one A row near the end -- the packing row -- spans every variable defined before it."""
    p = pyref.FIELDS[field][0]
    rnd = random.Random(seed)
    bits = rnd.getrandbits
    z = [1] + [bits(256) % p for _ in range(num_inputs - 1 + 4)]
    A, B, C = [], [], []
    pack = num_constraints - 3
    coeffs = (1, p - 1, 1, 2)

    def lin(nterms, with_one):
        idx = {0} if with_one else set()
        n = len(z)
        for _ in range(nterms):
            r = bits(32)
            idx.add(n - 1 - r % min(n, 64) if r & (1 << 31) else r % n)      # recent variables or any earlier one
        out = []
        for j in sorted(idx):
            k = bits(3)
            out.append((coeffs[k] if k < 4 else (bits(256) % p if k == 4 else 1), j))
        return out

    for i in range(num_constraints):
        if i == pack:
            la = [(1 if bits(1) else bits(256) % p, j) for j in range(len(z))]
        else:
            la = lin(1 + bits(2) % 3, i % 4 == 0)
        lb = lin(1 + bits(1), False)
        va = sum(c * z[j] for c, j in la) % p
        vb = sum(c * z[j] for c, j in lb) % p
        z.append(va * vb % p)
        A.append(la)
        B.append(lb)
        C.append([(1, len(z) - 1)])
    return {"field": field, "num_inputs": num_inputs, "A": A, "B": B, "C": C}, z


def lagrange_expected(field, log_m, tau):
    """L_i(tau) = (tau^m - 1)/m * w^i / (tau - w^i) and zt, with ONE modular inversion (Montgomery's trick)"""
    p = pyref.FIELDS[field][0]
    m = 1 << log_m
    w = pyref.root_of_unity(field, log_m)
    zt = (pow(tau, m, p) - 1) % p
    wi, den, pre, run = [], [], [], 1
    x = 1
    for _ in range(m):
        wi.append(x)
        d = (tau - x) % p
        den.append(d)
        pre.append(run)
        run = run * d % p
        x = x * w % p
    inv = pow(run, -1, p)
    s = zt * pow(m, -1, p) % p
    L = [0] * m
    for i in range(m - 1, -1, -1):
        L[i] = inv * pre[i] % p * wi[i] % p * s % p
        inv = inv * den[i] % p
    return L, zt


def setup_expected(r1cs, trap, n_vars):
    """generate_parameters on Python integers for a GIVEN trapdoor: the dictionary of pyref_groth16.setup plus "w" and "zt"
    (pinned to pyref_groth16.setup itself by the small-system tests)"""
    field = r1cs["field"]
    p = pyref.FIELDS[field][0]
    nc, ni = len(r1cs["A"]), r1cs["num_inputs"]
    m, _ = g16.domain(field, nc, ni)
    L, zt = lagrange_expected(field, m.bit_length() - 1, trap["tau"])
    u, v, wv = [0] * n_vars, [0] * n_vars, [0] * n_vars
    for j in range(ni):
        u[j] = L[nc + j]
    for vec, rows in ((u, r1cs["A"]), (v, r1cs["B"]), (wv, r1cs["C"])):
        for i, row in enumerate(rows):
            li = L[i]
            for c, j in row:
                vec[j] += c * li
    u, v, wv = [x % p for x in u], [x % p for x in v], [x % p for x in wv]
    dinv, ginv = pow(trap["delta"], -1, p), pow(trap["gamma"], -1, p)
    al, be = trap["alpha"], trap["beta"]
    abc = [(be * a + al * b + c) % p for a, b, c in zip(u, v, wv)]
    h, x, s = [], 1, zt * dinv % p
    for _ in range(m - 1):
        h.append(x * s % p)
        x = x * trap["tau"] % p
    key = dict(trap)
    key.update(m=m, num_inputs=ni, a_query=u, b_query=v, w=wv, abc=abc, zt=zt, h_query=h,
               l_query=[x * dinv % p for x in abc[ni:]], gamma_abc=[x * ginv % p for x in abc[:ni]])
    return key


def trapdoor_of(key):
    return {k: key[k] for k in TRAPDOOR}


def generate(zk, pairing, mats, ni, n_vars, trap, **kw):
    f = FIELD[pairing]
    return zk.groth16.generate_parameters(pairing, mats[0], mats[1], mats[2], ni, n_vars, *[mont1(f, trap[k]) for k in TRAPDOOR], **kw)


def oracle_members(pairing, key, k1=1, k2=1):
    """the key's members as the oracle's fixed-base points over the logarithms (times k1 in G1, k2 in G2), as
    parity_suite.check_groth16_prove builds them"""
    g1, g2 = pyref_ark.PAIRINGS[pairing]
    p = pyref.FIELDS[FIELD[pairing]][0]
    pts = lambda curve, logs, k: orc.fixed_base_mul(curve, ints_to_arr([v * k % p for v in logs]), threads=8)
    one = lambda curve, v, k: pts(curve, [v], k)
    return {"alpha_g1": one(g1, key["alpha"], k1), "beta_g2": one(g2, key["beta"], k2), "gamma_g2": one(g2, key["gamma"], k2),
            "delta_g2": one(g2, key["delta"], k2), "gamma_abc_g1": pts(g1, key["gamma_abc"], k1), "beta_g1": one(g1, key["beta"], k1),
            "delta_g1": one(g1, key["delta"], k1), "a_query": pts(g1, key["a_query"], k1), "b_g1_query": pts(g1, key["b_query"], k1),
            "b_g2_query": pts(g2, key["b_query"], k2), "h_query": pts(g1, key["h_query"], k1), "l_query": pts(g1, key["l_query"], k1)}


def pyref_ark_key(pairing, members):
    g1, g2 = pyref_ark.PAIRINGS[pairing]
    cv = lambda name: g2 if name in ("beta_g2", "gamma_g2", "delta_g2", "b_g2_query") else g1
    conv = {name: py_points(cv(name), a) for name, a in members.items()}
    single = lambda name: conv[name][0]
    vk = {"alpha_g1": single("alpha_g1"), "beta_g2": single("beta_g2"), "gamma_g2": single("gamma_g2"), "delta_g2": single("delta_g2"),
          "gamma_abc_g1": conv["gamma_abc_g1"]}
    pk = {"vk": vk, "beta_g1": single("beta_g1"), "delta_g1": single("delta_g1")}
    pk.update({k: conv[k] for k in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")})
    return pk


# ---------------------------------------------------------------- 1. transposed mat-vec
def transposed_expected(field, rows, x, x_len, out_len):
    p = pyref.FIELDS[field][0]
    out = [0] * out_len
    for i, row in enumerate(rows[:x_len]):
        for c, j in row:
            out[j] += c * x[i]
    return [v % p for v in out]


def check_matvec_transposed(zk, field, seed, num_constraints=120, long_rows=(17,)):
    p = pyref.FIELDS[field][0]
    r1cs, z = g16.random_r1cs(field, seed, num_inputs=3, num_constraints=num_constraints, long_rows=long_rows)
    n_vars, nc = len(z), num_constraints
    rng = pyref.Rng(seed + 1)
    x = [rng.below(p) for _ in range(nc)]
    d_x = to_device(zk, monts(field, x))
    mats = matrices(zk, field, r1cs, n_vars)
    other = matrices(zk, field, r1cs, n_vars)
    ones = lambda n: to_device(zk, np.ones((n, 4), dtype=np.uint64))
    for mtx, k in zip(mats, "ABC"):
        for x_len, out_len in ((nc, n_vars), (nc, n_vars + 37), (nc - 11, n_vars), (0, n_vars + 1)):     # the later calls reuse the companion
            got = to_host(zk, mtx.matvec_transposed(d_x, ones(out_len), x_len=x_len))
            assert (got == monts(field, transposed_expected(field, r1cs[k], x, x_len, out_len))).all(), (field, k, x_len, out_len)
    # a handle is freed; the others (and their cached companions) are untouched
    other[1].matvec_transposed(d_x, ones(n_vars))
    for mtx in other:
        mtx.free()
    got = to_host(zk, mats[1].matvec_transposed(d_x, ones(n_vars)))
    assert (got == monts(field, transposed_expected(field, r1cs["B"], x, nc, n_vars))).all()
    for mtx in mats:
        mtx.free()


def check_matvec_transposed_shapes(zk, field, seed=3, n_rows=200, n_cols=90):
    """a dense column (every row: the long-column kernel), an empty column, a column with exactly R1CS_LONG_ROW and one more
    terms, +-1 and general coefficients, an empty row; and a matrix with no terms at all"""
    p = pyref.FIELDS[field][0]
    rng = pyref.Rng(seed)
    coef = lambda: (1, p - 1, 2, rng.below(p))[rng.below(4)]
    rows = []
    for i in range(n_rows):
        if i == 7:
            rows.append([])
            continue
        row = [(coef(), 5)]                                   # column 5 is dense
        if i < 64:
            row.append((coef(), 11))                          # exactly 64 terms (row 7 is empty: 63) -> the short kernel
        if i < 66:
            row.append((coef(), 12))                          # 65 terms -> the long kernel
        for _ in range(rng.below(3)):
            j = 20 + rng.below(n_cols - 20)
            if j != 33 and all(j != jj for _, jj in row):     # column 33 stays empty
                row.append((coef(), j))
        rows.append(sorted(row, key=lambda t: t[1]))
    x = [rng.below(p) for _ in range(n_rows)]
    d_x = to_device(zk, monts(field, x))
    r1cs = {"A": rows, "B": [[] for _ in rows], "C": rows}
    mats = matrices(zk, field, r1cs, n_cols)
    for x_len in (n_rows, 65, 1):
        exp = transposed_expected(field, rows, x, x_len, n_cols + 3)
        assert exp[33] == 0
        for mtx in (mats[0], mats[2]):
            got = to_host(zk, mtx.matvec_transposed(d_x, to_device(zk, np.ones((n_cols + 3, 4), dtype=np.uint64)), x_len=x_len))
            assert (got == monts(field, exp)).all(), (field, x_len)
    got = to_host(zk, mats[1].matvec_transposed(d_x, to_device(zk, np.ones((n_cols, 4), dtype=np.uint64))))
    assert not got.any()
    for mtx in mats:
        mtx.free()


# ---------------------------------------------------------------- 2. Lagrange coefficients
def check_lagrange(zk, field, log_m, seed=9):
    p = pyref.FIELDS[field][0]
    rng = pyref.Rng(seed + log_m)
    tau = 1 + rng.below(p - 1)
    m = 1 << log_m
    while pow(tau, m, p) == 1:
        tau = 1 + rng.below(p - 1)
    w = pyref.root_of_unity(field, log_m)
    zt = (pow(tau, m, p) - 1) % p
    if m <= 2048:      # the formula as pyref_groth16.setup writes it
        exp = [zt * pow(m, -1, p) % p * pow(w, i, p) % p * pow((tau - pow(w, i, p)) % p, -1, p) % p for i in range(m)]
        assert exp == lagrange_expected(field, log_m, tau)[0]
    else:
        exp = lagrange_expected(field, log_m, tau)[0]
    assert sum(exp) % p == 1
    d_out = to_device(zk, np.ones((m, 4), dtype=np.uint64))
    got_zt = zk.groth16.lagrange_coefficients(field, log_m, mont1(field, tau), d_out)
    got = to_host(zk, d_out)
    assert (got == monts(field, exp)).all(), (field, log_m)
    assert (got_zt == mont1(field, zt)).all()
    assert sum(unmonts(field, got)) % p == 1
    # the ark-poly mirror
    dom = zk.ark.Radix2EvaluationDomain(field, m)
    d2 = to_device(zk, np.zeros((m, 4), dtype=np.uint64))
    assert (dom.evaluate_all_lagrange_coefficients(mont1(field, tau), d2) == got_zt).all() and (to_host(zk, d2) == got).all()


# ---------------------------------------------------------------- 3. u, v, w, abc, h
def check_key_scalars(zk, pairing, r1cs, z, key, mats=None):
    """qap_at + key_scalars against the lists of a setup dictionary (pyref_groth16.setup's, or setup_expected's at size)"""
    field = FIELD[pairing]
    p = pyref.FIELDS[field][0]
    n_vars, ni, m = len(z), r1cs["num_inputs"], key["m"]
    log_m = m.bit_length() - 1
    own = mats is None
    mats = matrices(zk, field, r1cs, n_vars) if own else mats
    full = lambda: to_device(zk, np.ones((n_vars, 4), dtype=np.uint64))
    d_u, d_v, d_w = full(), full(), full()
    zt = zk.groth16.qap_at(field, mats[0], mats[1], mats[2], ni, log_m, mont1(field, key["tau"]), d_u, d_v, d_w)
    assert (zt == mont1(field, (pow(key["tau"], m, p) - 1) % p)).all()
    w_exp = key["w"] if "w" in key else [(a - key["beta"] * u - key["alpha"] * v) % p for a, u, v in zip(key["abc"], key["a_query"], key["b_query"])]
    assert (to_host(zk, d_u) == monts(field, key["a_query"])).all(), "u"
    assert (to_host(zk, d_v) == monts(field, key["b_query"])).all(), "v"
    assert (to_host(zk, d_w) == monts(field, w_exp)).all(), "w"
    d_abc, d_h = full(), to_device(zk, np.ones((m - 1, 4), dtype=np.uint64))
    t = [mont1(field, key[k]) for k in TRAPDOOR]
    zk.groth16.key_scalars(field, d_u, d_v, d_w, ni, log_m, t[0], t[1], t[2], t[3], t[4], zt, d_abc, d_h)
    abc = unmonts(field, to_host(zk, d_abc))
    assert abc == key["gamma_abc"] + key["l_query"], "abc / gamma | abc / delta"
    assert [x * key["gamma"] % p for x in abc[:ni]] + [x * key["delta"] % p for x in abc[ni:]] == key["abc"], "abc"
    assert (to_host(zk, d_h) == monts(field, key["h_query"])).all(), "h"
    assert (to_host(zk, d_u) == monts(field, key["a_query"])).all(), "the inputs are left alone"
    # in place over w, as generate_parameters calls it
    zk.groth16.key_scalars(field, d_u, d_v, d_w, ni, log_m, t[0], t[1], t[2], t[3], t[4], zt, d_w, d_h)
    assert (to_host(zk, d_w) == to_host(zk, d_abc)).all()
    if own:
        for mtx in mats:
            mtx.free()


# ---------------------------------------------------------------- 4. the whole key
def check_whole_key(zk, pairing, seed=5, num_constraints=40, long_rows=(17,), num_inputs=3, zero_b=None):
    field = FIELD[pairing]
    az = zk.ark_serialize
    r1cs, z = g16.random_r1cs(field, seed, num_inputs=num_inputs, num_constraints=num_constraints, long_rows=long_rows)
    key = g16.setup(r1cs, seed + 100)
    n_vars = len(z)
    assert setup_expected(r1cs, trapdoor_of(key), n_vars)["h_query"] == key["h_query"]
    mats = matrices(zk, field, r1cs, n_vars)
    params = generate(zk, pairing, mats, num_inputs, n_vars, trapdoor_of(key))
    members = oracle_members(pairing, key)
    if zero_b is not None:          # the infinity encodings
        assert (len(key["b_query"]), key["b_query"].count(0)) == zero_b
    for name in az.PK_MEMBERS:
        assert (params.points(name) == members[name]).all(), (pairing, name)
    blob = params.serialize_unchecked()
    assert blob == pyref_ark.encode_pk_unchecked(pairing, pyref_ark_key(pairing, members)), "key file bytes"
    pk = az.ProvingKey.deserialize_unchecked(pairing, blob)              # zk_ark_proving_key_index accepts them
    assert [pk.count(n) for n in az.PK_MEMBERS] == [params.count(n) for n in az.PK_MEMBERS]
    assert params.verifying_key_bytes() == pyref_ark.encode_vk(pairing, pyref_ark_key(pairing, members)["vk"])
    for mtx in mats:
        mtx.free()


# ---------------------------------------------------------------- 5. setup -> prove -> verify
def check_setup_prove_verify(zk, pairing, seed=5, num_constraints=40, long_rows=(17,), num_inputs=3):
    field = FIELD[pairing]
    az = zk.ark_serialize
    g1, g2 = az.PAIRING_CURVES[az.pairing_id(pairing)]
    p = pyref.FIELDS[field][0]
    r1cs, z = g16.random_r1cs(field, seed, num_inputs=num_inputs, num_constraints=num_constraints, long_rows=long_rows)
    key = g16.setup(r1cs, seed + 100)
    n_vars = len(z)
    z_mont = monts(field, z)
    point = lambda curve, v: orc.fixed_base_mul(curve, ints_to_arr([v % p]), threads=1)[0]
    rng = pyref.Rng(seed + 200)
    r, s = rng.below(p), rng.below(p)
    a, b, c = g16.prove_logs(r1cs, key, z, r, s)
    assert g16.verify_logs(r1cs, key, z[:num_inputs], a, b, c)
    dev = lambda arr: to_device(zk, arr)
    proofs = []
    mats = matrices(zk, field, r1cs, n_vars)
    params = generate(zk, pairing, mats, num_inputs, n_vars, trapdoor_of(key))
    for through_bytes in (True, False):          # the key file's bytes, then the resident vectors adopted as they are
        pk = az.ProvingKey.deserialize_unchecked(pairing, params.serialize_unchecked()) if through_bytes else params
        prover = zk.groth16.Prover(pairing, pk, mats[0], mats[1], mats[2], num_inputs, dev)
        (A, B, C), proof_bytes = prover.prove(z_mont, mont1(field, r), mont1(field, s))
        assert (A == point(g1, a)).all() and (B == point(g2, b)).all() and (C == point(g1, c)).all(), (pairing, through_bytes)
        proofs.append(proof_bytes)
        prover.free()                            # frees the matrices too
        mats = matrices(zk, field, r1cs, n_vars)
    assert proofs[0] == proofs[1]
    # negative control: one trapdoor scalar changed -> a different key -> a different A
    bad = trapdoor_of(key)
    bad["delta"] = (bad["delta"] + 1) % p
    prover = zk.groth16.Prover(pairing, generate(zk, pairing, mats, num_inputs, n_vars, bad), mats[0], mats[1], mats[2], num_inputs, dev)
    (A2, _, _), _ = prover.prove(z_mont, mont1(field, r), mont1(field, s))
    assert not (A2 == point(g1, a)).all()
    prover.free()


# ---------------------------------------------------------------- 6. other generators
def check_random_generators(zk, pairing, seed=6, num_constraints=50, k1=7919, k2=104729):
    field = FIELD[pairing]
    az = zk.ark_serialize
    g1, g2 = az.PAIRING_CURVES[az.pairing_id(pairing)]
    r1cs, z = g16.random_r1cs(field, seed, num_inputs=2, num_constraints=num_constraints, long_rows=(9,))
    key = g16.setup(r1cs, seed + 100)
    base1 = orc.scalar_mul(g1, orc.curve_generator(g1), orc.int_to_limbs(k1, 4))
    base2 = orc.scalar_mul(g2, orc.curve_generator(g2), orc.int_to_limbs(k2, 4))
    mats = matrices(zk, field, r1cs, len(z))
    params = generate(zk, pairing, mats, 2, len(z), trapdoor_of(key), g1=base1, g2=base2)
    members = oracle_members(pairing, key, k1, k2)
    for name in az.PK_MEMBERS:
        assert (params.points(name) == members[name]).all(), (pairing, name)
    for mtx in mats:
        mtx.free()


# ---------------------------------------------------------------- 7. refusals
def check_refusals(zk, pairing="Bls381", seed=8):
    field = FIELD[pairing]
    p = pyref.FIELDS[field][0]
    fid = zk.field_id(field)
    lib = zk.groth16._lib()
    r1cs, z = g16.random_r1cs(field, seed, num_inputs=3, num_constraints=40, long_rows=(5,))
    key = g16.setup(r1cs, seed + 100)
    n_vars, ni, m, log_m = len(z), 3, 64, 6
    mats = matrices(zk, field, r1cs, n_vars)
    short = {"field": field, "num_inputs": 3, "A": r1cs["A"][:30], "B": r1cs["B"][:30], "C": r1cs["C"][:30]}
    mats_short = matrices(zk, field, short, n_vars)
    bufs = to_device(zk, np.zeros((4 * n_vars + 2 * m + 8, 4), dtype=np.uint64))        # one allocation carved into aligned vectors
    base = bufs.ctypes.data if isinstance(bufs, np.ndarray) else bufs.data_ptr()
    assert base % 16 == 0
    at = lambda k: base + 32 * k
    u, v, w, abc, h, L = at(0), at(n_vars), at(2 * n_vars), at(3 * n_vars), at(4 * n_vars), at(4 * n_vars + m)
    t = {k: mont1(field, key[k]) for k in TRAPDOOR}
    ptr = lambda a: a.ctypes.data
    zero = np.zeros(4, dtype=np.uint64)
    in_domain = mont1(field, pow(pyref.root_of_unity(field, log_m), 5, p))
    zt = np.zeros(4, dtype=np.uint64)
    ha, hb, hc = (mtx.handle for mtx in mats)
    qap = lambda a=ha, b=hb, c=hc, n_in=ni, lm=log_m, tau=ptr(t["tau"]), uu=u, vv=v, ww=w, nv=n_vars: \
        lib.zk_groth16_qap_at_device(fid, a, b, c, n_in, lm, tau, uu, vv, ww, nv, ptr(zt), None)
    assert qap(tau=ptr(in_domain)) == -1                                   # tau^m = 1
    assert qap(tau=ptr(mont1(field, 1))) == -1
    assert qap(a=mats_short[0].handle) == -1 and qap(c=mats_short[2].handle) == -1          # different row counts
    assert qap(lm=5) == -1                                                 # 40 + 3 > 32
    assert qap(nv=n_vars - 1) == -1                                        # n_vars below a matrix's n_cols
    assert qap(n_in=n_vars + 1, lm=10) == -1
    assert qap(tau=None) == -1 and qap(uu=None) == -1 and qap(vv=None) == -1 and qap(ww=None) == -1
    assert qap(uu=u + 8) == -1 and qap(vv=v + 8) == -1 and qap(ww=w + 8) == -1
    assert qap(lm=31) == -1 and qap(lm=33) == -1
    assert lib.zk_groth16_qap_at_device(fid ^ 1, ha, hb, hc, ni, log_m, ptr(t["tau"]), u, v, w, n_vars, ptr(zt), None) == -1   # another field's matrices
    assert qap(a=0xDEAD) == -7                                             # not a handle
    lag = lambda lm=log_m, tau=ptr(t["tau"]), out=L: lib.zk_lagrange_coefficients_device(fid, lm, tau, out, ptr(zt), None)
    assert lag(tau=ptr(in_domain)) == -1 and lag(tau=None) == -1 and lag(out=None) == -1 and lag(out=L + 8) == -1 and lag(lm=40) == -1
    assert lib.zk_lagrange_coefficients_device(9, log_m, ptr(t["tau"]), L, ptr(zt), None) == -1
    d_x = at(0)
    mvt = lambda x=d_x, x_len=40, out=abc, out_len=n_vars: lib.zk_r1cs_matvec_transposed_device(ha, x, x_len, out, out_len, None)
    assert mvt(x=None) == -1 and mvt(out=None) == -1 and mvt(x=d_x + 4) == -1 and mvt(out=abc + 8) == -1 and mvt(out_len=n_vars - 1) == -1
    assert lib.zk_r1cs_matvec_transposed_device(0xDEAD, d_x, 40, abc, n_vars, None) == -7
    good_zt = mont1(field, (pow(key["tau"], m, p) - 1) % p)
    ks = lambda gamma=ptr(t["gamma"]), delta=ptr(t["delta"]), z_=ptr(good_zt), uu=u, out=abc, hh=h, n_in=ni: \
        lib.zk_groth16_key_scalars_device(fid, uu, v, w, n_vars, n_in, log_m, ptr(t["alpha"]), ptr(t["beta"]), gamma, delta, ptr(t["tau"]), z_, out, hh, None)
    assert ks(gamma=ptr(zero)) == -1 and ks(delta=ptr(zero)) == -1 and ks(z_=ptr(zero)) == -1
    assert ks(gamma=None) == -1 and ks(uu=None) == -1 and ks(out=None) == -1 and ks(hh=None) == -1 and ks(uu=u + 8) == -1 and ks(hh=h + 8) == -1
    assert ks(n_in=n_vars + 1) == -1
    assert not to_host(zk, bufs).any(), "refused calls write nothing"
    # the same refusals through generate_parameters
    for bad in ({"tau": pow(pyref.root_of_unity(field, log_m), 3, p)}, {"gamma": 0}, {"delta": 0}):
        trap = trapdoor_of(key)
        trap.update(bad)
        try:
            generate(zk, pairing, mats, ni, n_vars, trap)
        except zk.ZkError as e:
            assert e.status == -1
        else:
            raise AssertionError("accepted %r" % bad)
    # ... and the library is still usable: one good run of everything
    assert qap() == 0 and ks() == 0 and lag() == 0 and mvt() == 0
    check_key_scalars(zk, pairing, r1cs, z, key, mats=mats)
    for mtx in mats + mats_short:
        mtx.free()


# ---------------------------------------------------------------- the GPU tier, at size
def check_at_size(zk, pairing, log_nc, seed=0x51E7, samples=64):
    """Key generation for 2^log_nc constraints: every scalar vector in full against Python integers; the six point vectors by
    their zero entries, sampled entries and one random linear combination through the library's own variable-base MSM; a proof
    from the key (adopted device vectors), verified in the exponent without the O(m^2) quotient."""
    field = FIELD[pairing]
    az = zk.ark_serialize
    g1, g2 = az.PAIRING_CURVES[az.pairing_id(pairing)]
    p = pyref.FIELDS[field][0]
    ni, nc = 3, 1 << log_nc
    r1cs, z = fast_r1cs(field, seed, ni, nc)
    n_vars = len(z)
    rnd = random.Random(seed + 1)
    trap = {k: 1 + rnd.getrandbits(256) % (p - 1) for k in TRAPDOOR}
    key = setup_expected(r1cs, trap, n_vars)
    m = key["m"]
    assert m == 2 * nc                      # 2^log_nc constraints + the input rows: the next power of two
    assert max(len(r) for r in r1cs["A"]) >= nc - 3 and sum(1 for r in r1cs["A"] if r[0][1] == 0) >= nc // 4, "packing row, dense variable 0"
    mats = matrices(zk, field, r1cs, n_vars)
    check_key_scalars(zk, pairing, r1cs, z, key, mats=mats)
    params = generate(zk, pairing, mats, ni, n_vars, trap)
    # ---- points
    scalars = {"a_query": key["a_query"], "b_g1_query": key["b_query"], "b_g2_query": key["b_query"], "h_query": key["h_query"],
               "l_query": key["l_query"], "gamma_abc_g1": key["gamma_abc"]}
    gens = {g1: orc.curve_generator(g1), g2: orc.curve_generator(g2)}
    mul = lambda curve, k: orc.scalar_mul(curve, gens[curve], orc.int_to_limbs(k % p, 4))
    for name, sc in scalars.items():
        curve = g2 if name == "b_g2_query" else g1
        pts = params.points(name)
        n = len(sc)
        assert pts.shape[0] == n, name
        zero = np.array([s == 0 for s in sc])
        assert (pts.any(axis=1) != zero).all(), (name, "a zero scalar gives (0, 0) and nothing else does")
        for i in sorted({0, n - 1} | {rnd.getrandbits(32) % n for _ in range(samples)}):
            assert (pts[i] == mul(curve, sc[i])).all(), (name, i)
        rho = np.frombuffer(random.Random(seed + 2).randbytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
        rho[:, 3] &= np.uint64((1 << 58) - 1)                  # canonical: below 2^250
        dot = sum(r * s for r, s in zip(arr_to_ints(rho), sc)) % p
        bases = params.upload(name)
        got = zk.point_to_affine(curve, zk.msm(bases, to_device(zk, rho)))
        bases.free()
        assert (got == mul(curve, dot)).all(), (name, "random linear combination")
    for name, k in (("alpha_g1", "alpha"), ("beta_g1", "beta"), ("delta_g1", "delta"), ("beta_g2", "beta"), ("gamma_g2", "gamma"), ("delta_g2", "delta")):
        assert (params.points(name)[0] == mul(g2 if name.endswith("g2") else g1, key[k])).all(), name
    # ---- a proof from the key, in the exponent
    prover = zk.groth16.Prover(pairing, params, mats[0], mats[1], mats[2], ni, lambda a: to_device(zk, a))
    r, s = rnd.getrandbits(256) % p, rnd.getrandbits(256) % p
    (A, B, C), _ = prover.prove(monts(field, z), mont1(field, r), mont1(field, s))
    dot = lambda xs, ys: sum(x * y for x, y in zip(xs, ys)) % p
    zu, zv, zw = dot(z, key["a_query"]), dot(z, key["b_query"]), dot(z, key["w"])
    dinv = pow(key["delta"], -1, p)
    a = (key["alpha"] + zu + r * key["delta"]) % p
    b = (key["beta"] + zv + s * key["delta"]) % p
    c = (dot(z[ni:], key["abc"][ni:]) * dinv + (zu * zv - zw) * dinv + s * a + r * b - r * s * key["delta"]) % p
    assert (A == mul(g1, a)).all() and (B == mul(g2, b)).all() and (C == mul(g1, c)).all(), pairing
    assert g16.verify_logs(r1cs, key, z[:ni], a, b, c)
    prover.free()
