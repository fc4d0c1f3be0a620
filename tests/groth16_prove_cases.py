"""TEST INFRASTRUCTURE shared by tests/test_groth16_prove_emu.py (CPU tier, emulator build) and tests/test_groth16_prove_gpu.py
(-m gpu): the Groth16 prove path from the assignment to the proof bytes -- zk_r1cs_matrix_upload, the two row-major mat-vec
kernels, the witness map, the five MSMs and the assembly -- at the row lengths, long-row-list layouts, operand values, domain
sizes and assignments where it can go wrong.  Every reference is Python integers mod p (the Montgomery form included: x 2^256
mod p); every comparison is word for word on canonical Montgomery limbs or canonical affine points.

  1. R1csMatrix.matvec against sum(c * z[j]) % p, row by row
  2. witness_map against pyref_groth16.h_coefficients and against a sampled-tau identity that shares nothing with it
  3. Prover.prove against pyref_groth16.prove_logs, and the proof bytes through the project's own groth16.verify"""
import functools
import random

import numpy as np

import groth16_setup_cases as gc
import groth16_verify_cases as vc
from oracle import pyref
from oracle import pyref_groth16 as g16
from parity_suite import to_device, to_host

PAIRINGS = gc.PAIRINGS
FIELD = gc.FIELD
FIELDS = ["Bls381Fr", "Bn254Fr"]
LONG_ROW = 64                     # R1CS_LONG_ROW of zk_r1cs_kernels.h: a row of more terms goes to the workgroup-per-row kernel
ROW_LENGTHS = [0, 1, 2, 63, 64, 65, 66, 255, 256, 257, 511, 513, 1000]
N_COLS = 1100
SENTINEL = 0xFFFFFFFFFFFFFFFF     # every output buffer starts as all-ones bits: not a canonical element, so a missed write shows


def modulus(field):
    return pyref.FIELDS[field][0]


def mont_rows(field, xs):
    """Python integers -> Montgomery limbs [n, 4], in Python integers (no oracle call)"""
    return gc.ints_to_arr([pyref.mont(field, x % modulus(field)) for x in xs])


def sentinel(zk, n):
    return to_device(zk, np.full((n, 4), SENTINEL, dtype=np.uint64))


# ---------------------------------------------------------------- 1. the row-major mat-vec
def upload(zk, field, rows, n_cols):
    row_ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
    row_ptr[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    col = np.array([j for r in rows for _, j in r], dtype=np.uint32)
    val = mont_rows(field, [c for r in rows for c, _ in r])
    if not len(col):
        col, val = np.zeros(1, dtype=np.uint32), np.zeros((1, 4), dtype=np.uint64)
    return zk.groth16.R1csMatrix(field, n_cols=n_cols, csr=(row_ptr, col, val))


def matvec_expected(field, rows, z, out_len):
    p = modulus(field)
    return [sum(c * z[j] for c, j in row) % p for row in rows] + [0] * (out_len - len(rows))


def run_matvec(zk, field, rows, z, n_cols, out_len):
    """-> (device result, expected), both [out_len, 4] Montgomery limbs; the output buffer starts as the sentinel"""
    assert len(z) == n_cols
    mtx = upload(zk, field, rows, n_cols)
    got = to_host(zk, mtx.matvec(to_device(zk, mont_rows(field, z)), sentinel(zk, out_len))).copy()
    mtx.free()
    return got, mont_rows(field, matvec_expected(field, rows, z, out_len))


def assert_rows(got, exp, rows, what):
    """row by row; the message names the lengths of the rows that differ, and the positions past the last row that are not zero"""
    assert got.shape == exp.shape
    bad = np.nonzero((got != exp).any(axis=1))[0].tolist()
    assert not bad, (what, [("row %d" % i, "%d terms" % len(rows[i])) if i < len(rows) else ("zero-fill", i) for i in bad[:8]])
    assert not got[len(rows):].any(), (what, "zero-fill")


def coefficient(rng, p, kind):
    return (0, 1, p - 1, 2, p - 2, rng.randrange(3, p - 2))[kind]


def random_row(rng, p, length, n_cols):
    """`length` distinct columns; coefficients 1, p - 1 (the shortcut branches of r1cs_term), 2, p - 2, 0 and random"""
    cols = sorted(rng.sample(range(n_cols), length))
    return [(coefficient(rng, p, rng.randrange(6)), j) for j in cols]


def random_z(rng, p, n):
    z = [rng.randrange(p) for _ in range(n)]
    for i in range(0, n, 7):
        z[i] = (0, 1, p - 1)[(i // 7) % 3]
    return z


def run_row_lengths(zk, field, seed=0x2047):
    """one matrix whose row i has ROW_LENGTHS[i] terms -> (got, expected, rows)"""
    p = modulus(field)
    rng = random.Random(seed)
    rows = [random_row(rng, p, n, N_COLS) for n in ROW_LENGTHS]
    z = random_z(rng, p, N_COLS)
    got, exp = run_matvec(zk, field, rows, z, N_COLS, len(rows) + 3)
    return got, exp, rows


def check_row_length(result, length):
    got, exp, rows = result
    i = ROW_LENGTHS.index(length)
    assert len(rows[i]) == length
    assert (got[i] == exp[i]).all(), "the row of %d terms" % length
    assert not got[len(rows):].any(), "zero-fill"


# the long-row list zk_r1cs_matrix_upload builds: row lengths per layout (a row is long from LONG_ROW + 1 terms on)
LAYOUTS = {
    "no_long_row": [3, 64, 1, 64, 0, 2, 63],
    "only_long_rows": [65, 300, 66, 257],
    "long_row_first": [70, 2, 3, 1, 64],
    "long_row_last": [2, 64, 3, 1, 70],
    "two_adjacent_long_rows": [2, 65, 300, 3],
    "long_alternating_with_empty": [0, 65, 0, 130, 0, 257, 0, 600, 0],
    "nnz_zero": [0, 0, 0, 0, 0],
    "no_rows": [],
}


def check_layout(zk, field, name, seed=0x1A70):
    p = modulus(field)
    rng = random.Random(seed + len(name))
    n_cols = 700
    rows = [random_row(rng, p, n, n_cols) for n in LAYOUTS[name]]
    longs = [i for i, r in enumerate(rows) if len(r) > LONG_ROW]
    if name == "no_long_row" or name in ("nnz_zero", "no_rows"):
        assert not longs
    if name == "only_long_rows":
        assert longs == list(range(len(rows)))
    z = random_z(rng, p, n_cols)
    # zk_r1cs_matrix_upload takes n_rows = 0 (row_ptr = {0}); the product is then the zero-fill alone
    got, exp = run_matvec(zk, field, rows, z, n_cols, len(rows) + 3)
    assert_rows(got, exp, rows, (field, name))
    if rows:                                              # out_len = n_rows exactly: nothing to fill
        got, exp = run_matvec(zk, field, rows, z, n_cols, len(rows))
        assert_rows(got, exp, rows, (field, name, "out_len = n_rows"))


EDGES = ["coefficients", "z_values", "column_ends", "all_one", "all_minus_one", "sums_to_zero", "duplicate_columns"]
EDGE_ROW = {"short": 24, "long": 288}                     # one lane's loop; the workgroup kernel with a second stride iteration


def edge_case(field, edge, length, seed=0xED6E):
    """-> (rows, z, n_cols): row 1 of three carries the edge (rows 0 and 2 are random short rows around it)"""
    p = modulus(field)
    rng = random.Random(seed + length + EDGES.index(edge))
    n_cols = 400
    z = [rng.randrange(2, p - 1) for _ in range(n_cols)]
    cols = sorted(rng.sample(range(1, n_cols - 1), length))
    if edge == "coefficients":                            # 0, 1, p - 1, 2, p - 2, random next to one another
        row = [(coefficient(rng, p, i % 6), j) for i, j in enumerate(cols)]
    elif edge == "z_values":                              # every coefficient kind against z = 0, 1, p - 1 and random
        row = []
        for i, j in enumerate(cols):
            kc, kz = i % 6, (i // 6) % 4
            z[j] = (0, 1, p - 1, z[j])[kz]
            row.append((coefficient(rng, p, kc), j))
        assert length % 24 == 0
    elif edge == "column_ends":
        cols[0], cols[-1] = 0, n_cols - 1
        row = [(coefficient(rng, p, 1 + i % 5), j) for i, j in enumerate(cols)]
    elif edge == "all_one":
        row = [(1, j) for j in cols]
    elif edge == "all_minus_one":
        row = [(p - 1, j) for j in cols]
    elif edge == "sums_to_zero":                          # +c and -c on two variables of the same value; c = 1 takes both shortcuts
        row = []
        for i in range(0, length, 2):
            c = 1 if i % 8 == 0 else p - 1 if i % 8 == 2 else rng.randrange(2, p - 1)
            z[cols[i + 1]] = z[cols[i]]
            row += [(c, cols[i]), (p - c, cols[i + 1])]
    elif edge == "duplicate_columns":                     # upstream's evaluate_constraint sums every term; so does the product
        half = cols[:length // 2]
        row = [(coefficient(rng, p, 1 + i % 5), j) for i, j in enumerate(half + half)]
        row[1] = (row[1][0], half[0])                     # ... and two equal neighbours
    rows = [random_row(rng, p, 5, n_cols), row, random_row(rng, p, 3, n_cols)]
    return rows, z, n_cols


def check_edge(zk, field, edge, kind):
    length = EDGE_ROW[kind]
    assert (length > 256) == (kind == "long") and (length <= LONG_ROW) == (kind == "short")
    rows, z, n_cols = edge_case(field, edge, length)
    assert len(rows[1]) == length
    exp_ints = matvec_expected(field, rows, z, len(rows))
    if edge == "sums_to_zero":
        assert exp_ints[1] == 0
    if edge == "duplicate_columns":
        assert len({j for _, j in rows[1]}) < length
    got, exp = run_matvec(zk, field, rows, z, n_cols, len(rows) + 1)
    assert_rows(got, exp, rows, (field, edge, "%d terms" % length))


def check_zero_fill(zk, field, fill, seed=0xF111, n_rows=300):
    """out_len = n_rows, n_rows + 1, 2 n_rows over a sentinel buffer: more than one workgroup of the row kernel, a long last row"""
    p = modulus(field)
    rng = random.Random(seed)
    n_cols = 500
    rows = [random_row(rng, p, rng.randrange(0, 5), n_cols) for _ in range(n_rows)]
    rows[255], rows[256], rows[n_rows - 1] = random_row(rng, p, 64, n_cols), random_row(rng, p, 65, n_cols), random_row(rng, p, 300, n_cols)
    out_len = {"exact": n_rows, "plus_one": n_rows + 1, "double": 2 * n_rows}[fill]
    got, exp = run_matvec(zk, field, rows, random_z(rng, p, n_cols), n_cols, out_len)
    assert_rows(got, exp, rows, (field, "out_len = %d" % out_len))


def check_matvec_refusals(zk, field="Bn254Fr"):
    """the documented refusals around the product: out_len < n_rows, a column index >= n_cols, a decreasing row_ptr"""
    p = modulus(field)
    rng = random.Random(5)
    rows = [random_row(rng, p, 3, 50) for _ in range(4)]
    mtx = upload(zk, field, rows, 50)
    d_z, d_out = to_device(zk, mont_rows(field, random_z(rng, p, 50))), sentinel(zk, 4)
    lib = zk.groth16._lib()
    assert lib.zk_r1cs_matvec_device(mtx.handle, zk._ptr(d_z), zk._ptr(d_out), 3, None) == vc.ZK_ERR_INVALID_ARG
    assert (to_host(zk, d_out) == SENTINEL).all(), "a refused call writes nothing"
    mtx.free()
    for bad in ([[(1, 50)]], [[(1, 3), (1, 2 ** 31)]]):
        try:
            upload(zk, field, bad, 50)
        except zk.ZkError as e:
            assert e.status == vc.ZK_ERR_INVALID_ARG
        else:
            raise AssertionError("accepted a column index past n_cols")
    try:
        zk.groth16.R1csMatrix(field, n_cols=50, csr=(np.array([0, 2, 1], dtype=np.uint64), np.zeros(2, dtype=np.uint32), np.zeros((2, 4), dtype=np.uint64)))
    except zk.ZkError as e:
        assert e.status == vc.ZK_ERR_INVALID_ARG
    else:
        raise AssertionError("accepted a decreasing row_ptr")


# ---------------------------------------------------------------- 2. the witness map at domain edges
# (constraints, inputs): the sum is 2^k - 1, 2^k, 2^k + 1 -- the domain is the smallest power of two >= the sum
DOMAIN_EDGES = {
    "k5_one_under": (28, 3), "k5_exact": (29, 3), "k5_one_over": (30, 3),
    "k10_one_under": (1019, 4), "k10_exact": (1020, 4), "k10_one_over": (1021, 4),
    "smallest": (1, 1), "one_input": (44, 1),
}
SMALL_DOMAIN_EDGES = [k for k in DOMAIN_EDGES if not k.startswith("k10")]


def domain_size(total):
    m = 1
    while m < total:
        m *= 2
    return m


def fft(p, a, w):
    """[sum_j a[j] w^(jk)]_k, recursive radix 2 on Python integers"""
    n = len(a)
    if n == 1:
        return list(a)
    w2 = w * w % p
    even, odd = fft(p, a[0::2], w2), fft(p, a[1::2], w2)
    out, x = [0] * n, 1
    for k in range(n // 2):
        t = x * odd[k] % p
        out[k], out[k + n // 2] = (even[k] + t) % p, (even[k] - t) % p
        x = x * w % p
    return out


def h_coefficients_fft(r1cs, z):
    """pyref_groth16.h_coefficients with its O(m^2) DFTs and schoolbook product replaced by radix-2 transforms (the naive one
    takes 40 s at m = 1024): interpolate a, b, c, multiply on a domain of 2m, subtract c, divide by X^m - 1 exactly.  Pinned to
    pyref_groth16.h_coefficients by every small case (check_witness_map, fast=False)."""
    field = r1cs["field"]
    p = modulus(field)
    a, b, c = g16.evaluations(r1cs, z)
    m = len(a)
    log_m = m.bit_length() - 1
    w, w2 = pyref.root_of_unity(field, log_m), pyref.root_of_unity(field, log_m + 1)
    minv = pow(m, -1, p)
    coef = lambda e: [x * minv % p for x in fft(p, e, pow(w, -1, p))]
    ca, cb, cc = coef(a), coef(b), coef(c)
    ea, eb = fft(p, ca + [0] * m, w2), fft(p, cb + [0] * m, w2)
    m2inv = pow(2 * m, -1, p)
    prod = [x * m2inv % p for x in fft(p, [x * y % p for x, y in zip(ea, eb)], pow(w2, -1, p))]
    assert prod[2 * m - 1] == 0
    prod = [(x - y) % p for x, y in zip(prod, cc + [0] * m)][:2 * m - 1]
    q = [0] * (m - 1)
    for k in range(m - 2, -1, -1):
        q[k] = (prod[k + m] + (q[k + m] if k + m < m - 1 else 0)) % p
    rem = [(prod[k] + q[k]) % p if k < m - 1 else prod[k] for k in range(m)]
    assert not any(rem), "the assignment does not satisfy the system"
    return q + [0]


def at_tau(field, evals, tau):
    """the polynomial of degree < m through `evals` on the domain {w^i}, at tau: barycentric weights, integers only
         P(tau) = (tau^m - 1) / m * sum_i evals[i] w^i / (tau - w^i)"""
    p, g, _ = pyref.FIELDS[field]
    m = len(evals)
    w = pow(g, (p - 1) // m, p)
    assert pow(w, m, p) == 1 and (m == 1 or pow(w, m // 2, p) == p - 1)
    acc, x = 0, 1
    for e in evals:
        if e:
            acc += e * x * pow(tau - x, -1, p)
        x = x * w % p
    return acc % p * (pow(tau, m, p) - 1) % p * pow(m, -1, p) % p


def horner(p, coeffs, tau):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * tau + c) % p
    return acc


def quotient_identity(field, evals, h, tau):
    """A(tau) B(tau) - C(tau) == h(tau) (tau^m - 1)"""
    p = modulus(field)
    a, b, c = (at_tau(field, e, tau) for e in evals)
    m = len(evals[0])
    return (a * b - c) % p == horner(p, h, tau) * (pow(tau, m, p) - 1) % p


def device_witness_map(zk, field, r1cs, z, mats=None):
    """-> (the three evaluation vectors as the mat-vecs and the input rows leave them, h), Python integers"""
    nc, ni = len(r1cs["A"]), r1cs["num_inputs"]
    m = domain_size(nc + ni)
    own = mats is None
    mats = [upload(zk, field, r1cs[k], len(z)) for k in "ABC"] if own else mats
    z_mont = mont_rows(field, z)
    d_z = to_device(zk, z_mont)
    evals = [to_host(zk, mtx.matvec(d_z, sentinel(zk, m))).copy() for mtx in mats]
    evals[0][nc:nc + ni] = z_mont[:ni]                   # the input-consistency rows, which the witness map adds
    bufs = [sentinel(zk, m) for _ in range(3)]
    h = to_host(zk, zk.groth16.witness_map(field, mats[0], mats[1], mats[2], d_z, ni, *bufs)).copy()
    if own:
        for mtx in mats:
            mtx.free()
    return evals, h


def check_witness_map(zk, field, r1cs, z, fast, seed=0x7A0, corrupt=None):
    """h of the device against the coefficient reference and against the sampled-tau identity over the REFERENCE's evaluations;
    the identity fails for a corrupted h and for a witness with one entry changed"""
    p = modulus(field)
    nc, ni = len(r1cs["A"]), r1cs["num_inputs"]
    m = domain_size(nc + ni)
    assert m // 2 < nc + ni <= m or m == 1
    ref_evals = g16.evaluations(r1cs, z)
    assert len(ref_evals[0]) == m
    h_ref = h_coefficients_fft(r1cs, z)
    if not fast:
        assert h_ref == g16.h_coefficients(r1cs, z), "the radix-2 reference against pyref_groth16.h_coefficients"
    evals, h = device_witness_map(zk, field, r1cs, z)
    for name, e, ref in zip("abc", evals, ref_evals):
        assert (e == mont_rows(field, ref)).all(), (field, nc, ni, "evaluations of " + name)
    assert h.shape == (m, 4), "h has the domain's length"
    assert not h[m - 1].any(), "deg h <= m - 2: the top coefficient is zero"
    assert (h == mont_rows(field, h_ref)).all(), (field, nc, ni, "h")
    h_ints = [pyref.unmont(field, v) for v in gc.arr_to_ints(h)]
    rng = random.Random(seed + nc)
    tau = rng.randrange(2, p)
    while pow(tau, m, p) == 1:
        tau = rng.randrange(2, p)
    assert quotient_identity(field, ref_evals, h_ints, tau), (field, nc, ni, "A(tau) B(tau) - C(tau) = h(tau) Z(tau)")
    # the check is not vacuous: one coefficient of h changed
    for i in sorted({0, (m - 1) // 2, m - 1}):
        bad = list(h_ints)
        bad[i] = (bad[i] + 1) % p
        assert not quotient_identity(field, ref_evals, bad, tau), ("a corrupted h passed", i)
    # one witness entry changed: the quotient no longer divides, whatever the device returns for it
    z_bad = list(z)
    z_bad[-1] = (z_bad[-1] + 1) % p
    _, h_bad = device_witness_map(zk, field, r1cs, z_bad)
    h_bad = [pyref.unmont(field, v) for v in gc.arr_to_ints(h_bad)]
    assert not quotient_identity(field, g16.evaluations(r1cs, z_bad), h_bad, tau), "a wrong witness passed"


@functools.lru_cache(maxsize=None)
def domain_edge_system(field, name):
    nc, ni = DOMAIN_EDGES[name]
    long_rows = (nc // 2, nc - 1) if nc > 4 else ()      # at k = 10: rows of ~520 and ~1028 terms inside the witness map
    return g16.random_r1cs(field, 0xD0 + nc, num_inputs=ni, num_constraints=nc, long_rows=long_rows)


def check_domain_edge(zk, field, name):
    nc, ni = DOMAIN_EDGES[name]
    k = {"k5": 5, "k10": 10}.get(name.split("_")[0])
    if k is not None:
        assert nc + ni - (1 << k) == {"one_under": -1, "exact": 0, "one_over": 1}[name.split("_", 1)[1]]
        assert domain_size(nc + ni) == (2 << k if name.endswith("over") else 1 << k)
    r1cs, z = domain_edge_system(field, name)
    check_witness_map(zk, field, r1cs, z, fast=nc > 100)


def zero_quotient_system(field, seed=0x20, num_inputs=3, num_constraints=29):
    """Every constraint has <A, z> = 0 (a pair +c, -c over two variables of the same value), <B, z> = 0 and an empty C row.
    The input-consistency rows give a(X) the values z[j] != 0, so a(X) is never the zero polynomial: a(X) b(X) - c(X) vanishes
    identically -- and h with it -- only because b(X) does."""
    p = modulus(field)
    rng = random.Random(seed)
    vals = [rng.randrange(2, p) for _ in range(12)]
    z = [1] + [rng.randrange(2, p) for _ in range(num_inputs - 1)] + [v for v in vals for _ in range(2)]
    first = num_inputs
    pair = lambda: first + 2 * rng.randrange(len(vals))

    def cancelling(n_pairs):
        row = []
        for _ in range(n_pairs):
            c, j = (1, p - 1, rng.randrange(2, p - 1))[rng.randrange(3)], pair()
            row += [(c, j), (p - c, j + 1)]
        return row

    A = [cancelling(1 + rng.randrange(3)) for _ in range(num_constraints)]
    B = [cancelling(rng.randrange(3)) for _ in range(num_constraints)]      # some B rows have no term at all
    C = [[] for _ in range(num_constraints)]
    return {"field": field, "num_inputs": num_inputs, "A": A, "B": B, "C": C}, z


def check_zero_quotient(zk, field):
    r1cs, z = zero_quotient_system(field)
    p = modulus(field)
    a, b, c = g16.evaluations(r1cs, z)
    nc = len(r1cs["A"])
    assert not any(a[:nc]) and a[nc] == 1 and not any(b) and not any(c)
    assert not any(g16.h_coefficients(r1cs, z))
    evals, h = device_witness_map(zk, field, r1cs, z)
    assert (evals[0] == mont_rows(field, a)).all() and not evals[1].any() and not evals[2].any()
    assert h.shape == (len(a), 4) and not h.any(), "h is identically zero"
    assert quotient_identity(field, (a, b, c), [0] * len(a), 12345 % p)


# ---------------------------------------------------------------- 3. whole proofs at witness edges
ASSIGNMENTS = ["zero_witness", "boolean", "minus_one"]
BLINDINGS = ["zero", "one_minus_one", "random"]


def edge_system(field, kind, seed=0xA551, num_inputs=3, num_constraints=24, n_vars=40, long_row=False):
    """A satisfied system around a CHOSEN assignment: z is fixed first, the A and B rows are drawn, and the C row of a constraint
    is made to equal <A, z> <B, z> (a witness variable plus a multiple of the constant one).  `kind`:
      zero_witness  every witness variable 0; z[0] = 1 and the public inputs are what is left
      boolean       at least 80 % of z in {0, 1}, with the booleanity constraints b (1 - b) = 0 of a bit decomposition (empty C rows)
      minus_one     p - 1 at a public input and at witness variables
    long_row: constraint 1's A row spans every variable (n_vars terms)."""
    p = modulus(field)
    rng = random.Random(seed + ASSIGNMENTS.index(kind) + n_vars)
    ni = num_inputs
    z = [1] + [rng.randrange(2, p - 1) for _ in range(ni - 1)]
    if kind == "zero_witness":
        z += [0] * (n_vars - ni)
    elif kind == "boolean":
        z += [rng.randrange(2, p - 1) if i % 8 == 7 else rng.randrange(2) for i in range(n_vars - ni)]
        assert sum(1 for v in z if v in (0, 1)) >= 0.8 * n_vars
    else:
        z += [rng.randrange(2, p - 1) for _ in range(n_vars - ni)]
        z[1] = z[ni] = z[n_vars - 1] = z[n_vars // 2] = p - 1
    assert len(z) == n_vars

    def lin(nterms):
        return [((1, p - 1, 2, rng.randrange(p))[rng.randrange(4)], j) for j in sorted(rng.sample(range(n_vars), nterms))]

    A, B, C = [], [], []
    bits = [j for j in range(ni, n_vars) if z[j] in (0, 1)] if kind == "boolean" else []
    for i in range(num_constraints):
        if i % 3 == 2 and bits:                          # b (1 - b) = 0
            j = bits.pop()
            A.append([(1, j)])
            B.append([(1, 0), (p - 1, j)])
            C.append([])
            continue
        la = [(1 if rng.randrange(2) else rng.randrange(p), j) for j in range(n_vars)] if long_row and i == 1 else lin(1 + rng.randrange(4))
        lb = lin(1 + rng.randrange(3))
        prod = sum(c * z[j] for c, j in la) % p * (sum(c * z[j] for c, j in lb) % p) % p
        k = n_vars - 1 - i % (n_vars - ni)               # constraint 0 names the last variable
        rest = (prod - z[k]) % p
        A.append(la)
        B.append(lb)
        C.append([(rest, 0), (1, k)] if rest else [(1, k)])
    return {"field": field, "num_inputs": ni, "A": A, "B": B, "C": C}, z


@functools.lru_cache(maxsize=None)
def proof_case(pairing, kind, long_row=False):
    """-> (r1cs, z, the key's logarithms, the key's members as the oracle's fixed-base points)"""
    field = FIELD[pairing]
    r1cs, z = edge_system(field, kind, n_vars=300 if long_row else 40, long_row=long_row)
    if long_row:
        assert max(len(r) for r in r1cs["A"]) > 256
    key = g16.setup(r1cs, 0x5E7 + len(z))
    assert len(key["a_query"]) == len(z)
    return r1cs, z, key, gc.oracle_members(pairing, key)


def blinding(field, name):
    p = modulus(field)
    rng = random.Random(0xB11D)
    return {"zero": (0, 0), "one_minus_one": (1, p - 1), "random": (rng.randrange(p), rng.randrange(p))}[name]


def check_proof(zk, pairing, kind, blindings, long_row=False):
    g16z, az = zk.groth16, zk.ark_serialize
    field, g1, g2 = FIELD[pairing], vc.G1[pairing], vc.G2[pairing]
    p = modulus(field)
    r1cs, z, key, members = proof_case(pairing, kind, long_row)
    ni = r1cs["num_inputs"]
    pk = az.ProvingKey.deserialize_unchecked(pairing, az.ProvingKey.serialize_unchecked(pairing, members))
    mats = [upload(zk, field, r1cs[k], len(z)) for k in "ABC"]
    prover = g16z.Prover(pairing, pk, mats[0], mats[1], mats[2], ni, lambda arr: to_device(zk, arr))
    vk = g16z.VerifyingKey(pairing, members["alpha_g1"][0], members["beta_g2"][0], members["gamma_g2"][0], members["delta_g2"][0],
                           to_device(zk, members["gamma_abc_g1"]))
    pvk = g16z.prepare_verifying_key(vk)
    public = z[1:ni]
    off = [(public[0] + 1) % p] + public[1:]
    for name in blindings:
        r, s = blinding(field, name)
        (A, B, C), proof_bytes = prover.prove(mont_rows(field, z), mont_rows(field, [r])[0], mont_rows(field, [s])[0])
        a, b, c = g16.prove_logs(r1cs, key, z, r, s)
        assert g16.verify_logs(r1cs, key, z[:ni], a, b, c)
        assert (A == vc.multiples(g1, [a])[0]).all(), (pairing, kind, name, "A")
        assert (B == vc.multiples(g2, [b])[0]).all(), (pairing, kind, name, "B")
        assert (C == vc.multiples(g1, [c])[0]).all(), (pairing, kind, name, "C")
        assert len(proof_bytes) == (192 if pairing == "Bls381" else 128)
        assert g16z.verify(pvk, mont_rows(field, public), proof_bytes) is True, (pairing, kind, name, "verify")
        assert g16z.verify(pvk, mont_rows(field, off), proof_bytes) is False, (pairing, kind, name, "one public input changed")
    vk.free()
    prover.free()
