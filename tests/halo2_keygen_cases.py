"""TEST INFRASTRUCTURE shared by tests/test_halo2_keygen_emu.py (CPU tier, emulator build) and tests/test_halo2_keygen_gpu.py
(-m gpu): halo2 key generation on the device (zk.halo2.Assembly, permutation_sigmas, keygen_vk, keygen_pk) against a restatement
of halo2_proofs 0.2 plonk/permutation/keygen.rs and plonk/keygen.rs on Python integers: the Assembly, sigma = delta^col omega^row,
the key columns, and every coefficient / extended form by direct evaluation of the interpolant.  Every comparison is exact."""
import random

import numpy as np

from oracle import pyref
from oracle import zk_oracle as orc
from parity_suite import to_device, to_host
from points_fft_cases import arr_to_ints, ints_to_arr, points_of_logs, seeded_scalars

CURVES = ["Pallas", "Vesta"]
# (k, ncols) of the sigma checks: n below a wave, exactly one wave, just above one, several workgroups, more than one tile of the
# omega tables (k > 10), column counts that are a multiple of nothing
SIGMA_SHAPES = [(1, 1), (2, 3), (3, 16), (5, 2), (6, 1), (6, 17), (7, 3), (10, 16), (13, 5)]
CLOSE_SHAPES = [s for s in SIGMA_SHAPES if s[0] >= 3]


def field_of(curve):
    return pyref.CURVES[curve][1]


def modulus(field):
    return pyref.FIELDS[field][0]


def monts(field, xs):
    return orc.to_mont(field, ints_to_arr(xs)) if len(xs) else np.zeros((0, 4), dtype=np.uint64)


def unmonts(field, a):
    return arr_to_ints(orc.from_mont(field, np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)))


def mont1(field, x):
    return monts(field, [x])[0]


def delta_int(field):
    """FieldExt::DELTA = GENERATOR^(2^S)"""
    p, g, _ = pyref.FIELDS[field]
    return pow(g, 1 << pyref.two_adicity(p)[0], p)


def zeta_int(field):
    """FieldExt::ZETA = GENERATOR^((p - 1) / 3)"""
    p, g, _ = pyref.FIELDS[field]
    return pow(g, (p - 1) // 3, p)


# ---------------------------------------------------------------- the restatement
class RefAssembly:
    """plonk/permutation/keygen.rs Assembly on Python tuples"""

    def __init__(self, n, ncols):
        self.n, self.ncols = n, ncols
        self.mapping = [[(c, r) for r in range(n)] for c in range(ncols)]
        self.aux = [[(c, r) for r in range(n)] for c in range(ncols)]
        self.sizes = [[1] * n for _ in range(ncols)]

    def copy(self, lc, lr, rc, rr):
        if not (0 <= lc < self.ncols and 0 <= rc < self.ncols and 0 <= lr < self.n and 0 <= rr < self.n):
            return False                               # Error::BoundsFailure
        left, right = (lc, lr), (rc, rr)
        get = lambda t, cell: t[cell[0]][cell[1]]
        if get(self.aux, left) == get(self.aux, right):
            return True
        if get(self.sizes, get(self.aux, left)) < get(self.sizes, get(self.aux, right)):
            left, right = right, left
        al, ar = get(self.aux, left), get(self.aux, right)
        self.sizes[al[0]][al[1]] += self.sizes[ar[0]][ar[1]]
        i = right
        while True:
            self.aux[i[0]][i[1]] = al
            i = get(self.mapping, i)
            if i == right:
                break
        tmp = get(self.mapping, left)
        self.mapping[left[0]][left[1]] = get(self.mapping, right)
        self.mapping[right[0]][right[1]] = tmp
        return True

    def mapping_array(self):
        return np.array([[(c << 32) | r for c, r in col] for col in self.mapping], dtype=np.uint64).reshape(self.ncols, self.n)


def both(zk, n, ncols, copies, many=False):
    """the same copies through the library and the restatement -> (Assembly, RefAssembly), mappings compared cell for cell"""
    asm, ref = zk.halo2.Assembly(n, ncols), RefAssembly(n, ncols)
    if many:
        assert asm.copy_many(copies) == len(copies)
    for q in copies:
        if not many:
            asm.copy(*q)
        assert ref.copy(*q)
    assert (asm.mapping() == ref.mapping_array()).all(), (n, ncols, copies[:8])
    return asm, ref


def random_copies(n, ncols, count, seed):
    rnd = random.Random(seed)
    return [(rnd.randrange(ncols), rnd.randrange(n), rnd.randrange(ncols), rnd.randrange(n)) for _ in range(count)]


def cycles_of(mapping):
    """the cycles of a [ncols, n] mapping array, as lists of (column, row)"""
    ncols, n = mapping.shape
    seen = np.zeros((ncols, n), dtype=bool)
    out = []
    for c in range(ncols):
        for r in range(n):
            if seen[c, r]:
                continue
            cyc, cell = [], (c, r)
            while not seen[cell]:
                seen[cell] = True
                cyc.append(cell)
                m = int(mapping[cell])
                cell = (m >> 32, m & 0xFFFFFFFF)
            out.append(cyc)
    return out


# ---------------------------------------------------------------- 1. the Assembly
def check_assembly(zk):
    a, b, c, d = (0, 0), (0, 1), (1, 2), (2, 3)
    ident = both(zk, 4, 3, [])
    assert (ident[0].mapping() == np.array([[(col << 32) | r for r in range(4)] for col in range(3)], dtype=np.uint64)).all()
    ident[0].free()
    scenarios = {
        "self": [a + a],
        "inside one cycle": [a + b, b + a, a + b],
        "left larger": [a + b, a + c],
        "right larger (swap)": [a + b, c + a],
        "equal sizes": [a + b, c + d, b + d],
        "equal then right larger": [a + b, c + d, b + d, (1, 0) + c, (2, 0) + (2, 1), (2, 0) + a],
    }
    for name, copies in scenarios.items():
        asm, ref = both(zk, 4, 3, copies)
        asm.free()
    # a chain that ends as one cycle through every column
    ncols, n = 7, 5
    chain = [(col, col % n, col + 1, (col + 1) % n) for col in range(ncols - 1)]
    asm, ref = both(zk, n, ncols, chain)
    longest = max(cycles_of(asm.mapping()), key=len)
    assert sorted(cell[0] for cell in longest) == list(range(ncols))
    asm.free()
    # the order of the calls matters, and the restatement agrees with each order
    first, second = [a + b, b + c], [b + c, a + b]
    asm1, _ = both(zk, 4, 3, first)
    asm2, _ = both(zk, 4, 3, second)
    assert (asm1.mapping() != asm2.mapping()).any()
    assert sorted(map(sorted, cycles_of(asm1.mapping()))) == sorted(map(sorted, cycles_of(asm2.mapping())))      # the same cycles, another walk
    asm1.free()
    asm2.free()
    # random copies one by one, in one call, and as an array
    copies = random_copies(16, 5, 60, seed=1)
    one, _ = both(zk, 16, 5, copies)
    many, _ = both(zk, 16, 5, copies, many=True)
    arr = zk.halo2.Assembly(16, 5)
    assert arr.copy_many(np.array(copies, dtype=np.int64)) == 60
    assert (one.mapping() == many.mapping()).all() and (one.mapping() == arr.mapping()).all()
    for x in (one, many, arr):
        x.free()
    # out of bounds: the error, the earlier copies applied, the later ones untouched, the count reported
    for bad in ((0, 4, 1, 1), (1, 1, 3, 0), (0, 1, 0, (1 << 32) + 1), (-1, 0, 0, 0), (1 << 32, 0, 0, 0)):
        asm, ref = zk.halo2.Assembly(4, 3), RefAssembly(4, 3)
        good = [a + b, c + d]
        try:
            asm.copy_many(good + [bad, b + d])
        except zk.halo2.BoundsFailure as e:
            assert e.applied == 2
        else:
            raise AssertionError("accepted %r" % (bad,))
        for q in good:
            ref.copy(*q)
        assert not ref.copy(*bad)
        assert (asm.mapping() == ref.mapping_array()).all()
        asm.copy(*(b + d))                               # still usable
        ref.copy(*(b + d))
        assert (asm.mapping() == ref.mapping_array()).all()
        asm.free()


# ---------------------------------------------------------------- 2. sigma
def sigma_expected(field, k, mapping):
    """delta^col omega^row for every cell of a [ncols, n] mapping array -> Montgomery limbs [ncols, n, 4]"""
    p = modulus(field)
    ncols, n = mapping.shape
    w, dl = pyref.root_of_unity(field, k), delta_int(field)
    wp, dp = [1], [1]
    for _ in range(n - 1):
        wp.append(wp[-1] * w % p)
    for _ in range(ncols - 1):
        dp.append(dp[-1] * dl % p)
    flat = mapping.reshape(-1).tolist()
    return monts(field, [dp[m >> 32] * wp[m & 0xFFFFFFFF] % p for m in flat]).reshape(ncols, n, 4)


def check_sigmas(zk, curve, k, ncols, seed=3):
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    assert (zk.halo2.delta(field) == mont1(field, delta_int(field))).all()
    # the identity mapping: sigma_c[j] = delta^c omega^j
    asm = zk.halo2.Assembly(n, ncols)
    got = to_host(zk, zk.halo2.permutation_sigmas(field, k, asm.mapping()))
    w, dl = pyref.root_of_unity(field, k), delta_int(field)
    assert (got == monts(field, [pow(dl, c, p) * pow(w, j, p) % p for c in range(ncols) for j in range(n)]).reshape(ncols, n, 4)).all()
    asm.free()
    # random copies, through the library and the restatement
    asm, ref = both(zk, n, ncols, random_copies(n, ncols, max(1, n * ncols // 2), seed + 7 * k + ncols), many=True)
    mapping = asm.mapping()
    identity = (np.arange(ncols, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    assert n * ncols < 4 or (mapping != identity).any()
    out = to_device(zk, np.full((ncols, n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
    got = to_host(zk, zk.halo2.permutation_sigmas(field, k, to_device(zk, mapping), sigmas=out))
    assert (got == sigma_expected(field, k, ref.mapping_array())).all(), (curve, k, ncols)
    asm.free()


def check_sigmas_grid_stride(zk, curve, k=16, ncols=17, seed=5):
    """more cells than one sweep of the kernel's grid covers (4096 workgroups of 256): the second trip of the grid-stride loop.
    The mapping comes from the library's Assembly (pinned to the restatement by the small shapes) over 2^18 random copies."""
    field = field_of(curve)
    n = 1 << k
    assert n * ncols > 4096 * 256
    rng = np.random.default_rng(seed)
    quads = np.stack([rng.integers(0, ncols, 1 << 18), rng.integers(0, n, 1 << 18), rng.integers(0, ncols, 1 << 18), rng.integers(0, n, 1 << 18)], axis=1)
    asm = zk.halo2.Assembly(n, ncols)
    assert asm.copy_many(quads) == 1 << 18
    mapping = asm.mapping()
    asm.free()
    got = to_host(zk, zk.halo2.permutation_sigmas(field, k, mapping))
    assert (got == sigma_expected(field, k, mapping)).all(), (curve, k, ncols)


# ---------------------------------------------------------------- 3. the permutation argument closes
def run_product(zk, field, k, d_cols, sigmas, beta, gamma, delta):
    """Z over chunks of <= 8 columns chained through z_first -> the value after the last row of the last chunk"""
    n = 1 << k
    z_out = to_device(zk, np.zeros((n, 4), dtype=np.uint64))
    zf = None
    for lo in range(0, len(d_cols), 8):
        hi = min(lo + 8, len(d_cols))
        zf = zk.halo2.permutation_product(field, d_cols[lo:hi], sigmas[lo:hi], beta, gamma, delta, k, z_out, first_column_index=lo, z_first=zf)
    return zf


def check_argument_closes(zk, curve, k, ncols, seed=11):
    """independent of the restatement: with the generated sigma the grand product over a witness that respects the copies ends at
    exactly 1; with one copied cell changed, or with seeded random sigma (what the bench uses as key material), it does not"""
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    rnd = random.Random(seed + 31 * k + ncols)
    asm = zk.halo2.Assembly(n, ncols)
    asm.copy_many(random_copies(n, ncols, max(2, n * ncols // 3), seed + k))
    mapping = asm.mapping()
    asm.free()
    cyc = cycles_of(mapping)
    long_cycle = next(c for c in cyc if len(c) >= 2)
    val = [[0] * n for _ in range(ncols)]
    for cells in cyc:
        v = rnd.randrange(p)
        for c, r in cells:
            val[c][r] = v
    one = mont1(field, 1)
    beta, gamma = mont1(field, rnd.randrange(p)), mont1(field, rnd.randrange(p))
    sigmas = zk.halo2.permutation_sigmas(field, k, mapping)
    d_cols = [to_device(zk, monts(field, col)) for col in val]
    delta = zk.halo2.delta(field)
    assert (run_product(zk, field, k, d_cols, sigmas, beta, gamma, delta) == one).all(), (curve, k, ncols, "a satisfied permutation closes")
    c, r = long_cycle[0]
    val[c][r] = (val[c][r] + 1) % p
    d_cols[c] = to_device(zk, monts(field, val[c]))
    assert not (run_product(zk, field, k, d_cols, sigmas, beta, gamma, delta) == one).all(), "a broken copy does not"
    val[c][r] = (val[c][r] - 1) % p
    d_cols[c] = to_device(zk, monts(field, val[c]))
    seeded = to_device(zk, monts(field, [rnd.randrange(p) for _ in range(ncols * n)]).reshape(ncols, n, 4))
    assert not (run_product(zk, field, k, d_cols, seeded, beta, gamma, delta) == one).all(), "seeded random sigma is not a key"


# ---------------------------------------------------------------- 4. coefficient and extended forms
def batch_inverse(xs, p):
    pre, run = [], 1
    for x in xs:
        pre.append(run)
        run = run * x % p
    inv = pow(run, -1, p)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % p
        inv = inv * xs[i] % p
    return out


class Interpolant:
    """the polynomials of degree < n through columns of n values on the powers of omega, evaluated directly at points outside the
    domain: P(x) = (x^n - 1) / n * sum_j v_j omega^j / (x - omega^j)"""

    def __init__(self, field, k):
        self.p, self.n = modulus(field), 1 << k
        w = pyref.root_of_unity(field, k)
        self.wp = [1]
        for _ in range(self.n - 1):
            self.wp.append(self.wp[-1] * w % self.p)
        self.ninv = pow(self.n, -1, self.p)

    def at(self, x, columns):
        p = self.p
        inv = batch_inverse([(x - wj) % p for wj in self.wp], p)
        weights = [wj * iv % p for wj, iv in zip(self.wp, inv)]
        s = (pow(x, self.n, p) - 1) * self.ninv % p
        return [s * sum(v * wt for v, wt in zip(col, weights)) % p for col in columns]


def make_key(zk, curve, k, degree, bf, ncols, nfixed, seed, cosets="mont", params=None):
    """-> (params, vk, pk, fixed (Python integers), sigma (Python integers, from the restatement), asm)"""
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    rnd = random.Random(seed)
    own = params is None
    if own:
        params = zk.halo2.Params.from_g(curve, k, points_of_logs(curve, seeded_scalars(curve, n, seed + 1)))
    fixed = [[rnd.randrange(p) if rnd.randrange(4) else rnd.randrange(2) for _ in range(n)] for _ in range(nfixed)]     # some 0 / 1 selector cells
    asm, ref = both(zk, n, ncols, random_copies(n, ncols, n * ncols // 2, seed + 2), many=True)
    sigma = [unmonts(field, col) for col in sigma_expected(field, k, ref.mapping_array())]
    cols = [monts(field, col) if i % 2 else to_device(zk, monts(field, col)) for i, col in enumerate(fixed)]        # device and host inputs
    vk = zk.halo2.keygen_vk(params, degree, cols, asm, bf)
    pk = zk.halo2.keygen_pk(params, vk, cols, asm, cosets=cosets)
    return params, vk, pk, fixed, sigma, asm


def check_forms(zk, curve, k, degree, bf, ncols=3, nfixed=2, seed=17, samples=None):
    """polys and cosets of the permutation and fixed columns, l0, l_last, l_active_row: k <= 6 at every position, otherwise at
    `samples` seeded positions"""
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    params, vk, pk, fixed, sigma, asm = make_key(zk, curve, k, degree, bf, ncols, nfixed, seed + k + degree + bf)
    dom = vk.domain
    assert dom.k == k and dom.quotient_poly_degree == degree - 1 and dom.extended_k - k == (degree - 2).bit_length()
    ext = dom.extended_len()
    assert (to_host(zk, pk.permutation.permutations) == np.stack([monts(field, c) for c in sigma])).all()
    assert (to_host(zk, pk.fixed_values) == np.stack([monts(field, c) for c in fixed])).all()
    w = pyref.root_of_unity(field, k)
    if samples is None:
        # the coefficient forms, evaluated at every omega^j by Horner, give back the Lagrange values
        for name, polys, values in (("permutation", pk.permutation.polys, sigma), ("fixed", pk.fixed_polys, fixed)):
            for coeffs, col in zip(to_host(zk, polys), values):
                cs = unmonts(field, coeffs)
                for j in range(n):
                    x, acc = pow(w, j, p), 0
                    for cf in reversed(cs):
                        acc = (acc * x + cf) % p
                    assert acc == col[j], (name, j)
    ind = lambda rows: [1 if r in rows else 0 for r in range(n)]
    l0, l_last, l_blind = ind({0}), ind({n - bf - 1}), ind(set(range(n - bf, n)))
    columns = sigma + fixed + [l0, l_last, l_blind]
    got = [unmonts(field, a) for a in list(to_host(zk, pk.permutation.cosets)) + list(to_host(zk, pk.fixed_cosets)) +
           [to_host(zk, pk.l0), to_host(zk, pk.l_last), to_host(zk, pk.l_active_row)]]
    assert all(len(g) == ext for g in got)
    rnd = random.Random(seed)
    positions = range(ext) if samples is None else sorted({0, ext - 1} | {rnd.randrange(ext) for _ in range(samples)})
    zeta, we = zeta_int(field), pyref.root_of_unity(field, dom.extended_k)
    interp = Interpolant(field, k)
    for i in positions:
        exp = interp.at(zeta * pow(we, i, p) % p, columns)
        exp[-1] = (1 - (exp[-2] + exp[-1])) % p                     # l_active_row = 1 - (l_last + l_blind), upstream's pass
        assert [g[i] for g in got] == exp, (curve, k, degree, bf, i)
    # l_active_row + l_last + l_blind == 1 at EVERY extended row, l_blind through the domain's own transforms
    d_blind = to_device(zk, monts(field, l_blind))
    dom.lagrange_to_coeff(d_blind)
    d_ext = to_device(zk, np.zeros((ext, 4), dtype=np.uint64))
    dom.coeff_to_extended(d_ext, coeffs=d_blind)
    blind_ext = unmonts(field, to_host(zk, d_ext))
    assert all((a + b + c) % p == 1 for a, b, c in zip(got[-1], got[-2], blind_ext))
    # the lazy radix, and no extended forms at all
    lazy = zk.halo2.keygen_pk(params, vk, [monts(field, c) for c in fixed], asm, cosets="lazy")
    for a, b in ((lazy.permutation.cosets, pk.permutation.cosets), (lazy.fixed_cosets, pk.fixed_cosets), (lazy.l0, pk.l0),
                 (lazy.l_last, pk.l_last), (lazy.l_active_row, pk.l_active_row)):
        flat = to_device(zk, to_host(zk, b).reshape(-1, 4).copy())
        assert (to_host(zk, a).reshape(-1, 4) == to_host(zk, zk.halo2.to_lazy_form(field, flat))).all()
    assert (to_host(zk, lazy.permutation.polys) == to_host(zk, pk.permutation.polys)).all()
    bare = zk.halo2.keygen_pk(params, vk, [monts(field, c) for c in fixed], asm, cosets=None)
    assert bare.fixed_cosets is None and bare.permutation.cosets is None and bare.l0 is None and bare.l_active_row is None
    assert (to_host(zk, bare.l_active_row_poly) == to_host(zk, pk.l_active_row_poly)).all()
    assert (to_host(zk, bare.fixed_polys) == to_host(zk, pk.fixed_polys)).all()
    for key in (pk, lazy, bare):
        key.free()
    assert pk.fixed_values is None and pk.l0 is None
    asm.free()
    params.free()


# ---------------------------------------------------------------- 5. fixed columns as rationals
def check_rationals(zk, curve, k=5, seed=23):
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    rnd = random.Random(seed)
    num = [rnd.randrange(p) for _ in range(n)]
    den = [1 + rnd.randrange(p - 1) for _ in range(n)]
    num[3] = 0
    den[5] = 0                    # a zero denominator gives 0
    num[7], den[7] = 0, 0
    den[n - 1] = 0
    value = [a * pow(d, -1, p) % p if d else 0 for a, d in zip(num, den)]
    assert value[3] == 0 and value[5] == 0 and value[n - 1] == 0
    plain = [rnd.randrange(p) for _ in range(n)]
    params = zk.halo2.Params.from_g(curve, k, points_of_logs(curve, seeded_scalars(curve, n, seed + 1)))
    asm = zk.halo2.Assembly(n, 2)
    m = lambda xs: monts(field, xs)
    keys = []
    for pair in ((m(num), m(den)), (to_device(zk, m(num)), to_device(zk, m(den))), m(value)):
        vk = zk.halo2.keygen_vk(params, 4, [pair, m(plain)], asm, 2)
        pk = zk.halo2.keygen_pk(params, vk, [pair, m(plain)], asm, cosets=None)
        assert (to_host(zk, pk.fixed_values) == np.stack([m(value), m(plain)])).all()
        keys.append((vk.fixed_commitments.copy(), to_host(zk, pk.fixed_polys).copy()))
    for c, q in keys[1:]:
        assert (c == keys[0][0]).all() and (q == keys[0][1]).all()
    if not isinstance(to_device(zk, m(num)), np.ndarray):      # device inputs are left as they were
        d_num, d_den = to_device(zk, m(num)), to_device(zk, m(den))
        zk.halo2.keygen_vk(params, 4, [(d_num, d_den)], asm, 2)
        assert (to_host(zk, d_num) == m(num)).all() and (to_host(zk, d_den) == m(den)).all()
    asm.free()
    params.free()


# ---------------------------------------------------------------- 6. commitments
def py_point(curve, aff):
    """affine Montgomery limbs (x, y) -> Python integers, None = the identity"""
    bf = pyref.CURVES[curve][0]
    aff = np.ascontiguousarray(aff, dtype=np.uint64)
    if not aff.any():
        return None
    return tuple(pyref.unmont(bf, orc.limbs_to_int(aff[4 * i:4 * i + 4])) for i in range(2))


def check_commitments(zk, curve, k, seed=29, ncols=3, nfixed=2):
    field = field_of(curve)
    params, vk, pk, fixed, sigma, asm = make_key(zk, curve, k, 5, 1, ncols, nfixed, seed + k, cosets=None)
    aff = lambda jac: zk.point_to_affine(curve, jac)
    assert vk.fixed_commitments.shape == (nfixed, 12) and vk.permutation.commitments.shape == (ncols, 12)
    gl = [py_point(curve, row) for row in to_host(zk, params.d_g_lagrange)] if k <= 4 else None
    for commitments, values, polys in ((vk.fixed_commitments, pk.fixed_values, pk.fixed_polys),
                                       (vk.permutation.commitments, pk.permutation.permutations, pk.permutation.polys)):
        ints = fixed if values is pk.fixed_values else sigma
        for i in range(int(values.shape[0])):
            got = aff(commitments[i])
            assert (got == aff(params.commit_lagrange(values[i]))).all(), (curve, k, i, "commit_lagrange of the column")
            assert (got == aff(params.commit(polys[i]))).all(), (curve, k, i, "commit of the coefficient form")
            if gl is not None:          # double-and-add on Python integers
                assert py_point(curve, got) == pyref.msm_naive(curve, ints[i], gl), (curve, k, i)
    pk.free()
    asm.free()
    params.free()


# ---------------------------------------------------------------- 7. refusals
def check_refusals(zk, curve="Pallas", seed=37):
    field = field_of(curve)
    fid = zk.field_id(field)
    lib = zk.halo2._plib()
    k, ncols = 5, 3
    n = 1 << k
    p = modulus(field)
    asm, ref = both(zk, n, ncols, random_copies(n, ncols, 40, seed), many=True)
    mapping = asm.mapping()
    # one allocation carved into the mapping (8 B a cell) and the output (32 B a cell), both 32-byte aligned
    buf = to_device(zk, np.zeros((ncols * n // 4 + ncols * n + 2, 4), dtype=np.uint64))
    base = buf.ctypes.data if isinstance(buf, np.ndarray) else buf.data_ptr()
    assert base % 16 == 0
    d_map, d_out = base, base + 8 * ncols * n
    flat = buf.reshape(-1)
    def put(m):
        words = np.ascontiguousarray(m, dtype=np.uint64).reshape(-1)
        if isinstance(flat, np.ndarray):
            flat[:words.size] = words
        else:
            import torch
            flat[:words.size] = torch.from_numpy(words.view(np.int64)).to(flat.device)
    put(mapping)
    dl = zk.halo2.delta(field)
    ptr = lambda a: a.ctypes.data
    call = lambda f=fid, kk=k, nc=ncols, m=d_map, d=ptr(dl), out=d_out: lib.zk_halo2_permutation_sigmas_device(f, kk, nc, m, d, out, None)
    assert call(m=None) == -1 and call(d=None) == -1 and call(out=None) == -1
    assert call(m=d_map + 8) == -1 and call(out=d_out + 8) == -1                 # misaligned
    assert call(nc=0) == -1
    assert call(kk=33) == -1 and call(kk=31) == -1                               # above the two-adicity; above the library's sizes
    assert call(f=9) == -1
    assert call(out=d_map) == -1 and call(out=d_map + 16) == -1                  # output over the mapping
    out_words = lambda: to_host(zk, buf).reshape(-1)[ncols * n:]
    assert not out_words().any(), "refused calls write nothing"
    # a well-formed buffer whose CONTENT names cells outside the grid: refused by the kernel's own check, nothing read through them
    bad = mapping.copy()
    bad[1, 7] = (np.uint64(1) << np.uint64(32)) | np.uint64(n)                   # row = n
    bad[2, 30] = (np.uint64(ncols) << np.uint64(32)) | np.uint64(3)              # column = ncols
    put(bad)
    assert call() == -1
    got = out_words()[:ncols * n * 4].reshape(ncols, n, 4)
    exp = sigma_expected(field, k, ref.mapping_array())
    ok = np.ones((ncols, n), dtype=bool)
    ok[1, 7] = ok[2, 30] = False
    assert (got[ok] == exp[ok]).all() and not got[1, 7].any() and not got[2, 30].any(), "the bad cells wrote only their own slots"
    try:
        zk.halo2.permutation_sigmas(field, k, bad)
    except zk.ZkError as e:
        assert e.status == -1
    else:
        raise AssertionError("accepted a mapping outside the grid")
    # ... and a following good call is right
    put(mapping)
    assert call() == 0
    assert (out_words()[:ncols * n * 4].reshape(ncols, n, 4) == exp).all()
    # assembly handles
    h = ctypes_u64()
    assert lib.zk_halo2_assembly_new(n, 0, h[1]) == -1 and lib.zk_halo2_assembly_new(0, 3, h[1]) == -1 and lib.zk_halo2_assembly_new(n, 3, None) == -1
    assert lib.zk_halo2_assembly_new(1 << 20, 1 << 12, h[1]) == -1               # 2^32 cells
    quad = np.array([0, 0, 1, 1], dtype=np.uint32)
    assert lib.zk_halo2_assembly_copy(0xDEAD, quad.ctypes.data, 1, None) == -7 and lib.zk_halo2_assembly_mapping(0xDEAD, d_out) == -7
    assert lib.zk_halo2_assembly_copy(asm.handle, None, 1, None) == -1 and lib.zk_halo2_assembly_mapping(asm.handle, None) == -1
    stale = zk.halo2.Assembly(n, ncols)
    handle = stale.handle
    stale.free()
    stale.free()                                                                 # a second free of the object is a no-op
    assert lib.zk_halo2_assembly_free(handle) == -7 and lib.zk_halo2_assembly_copy(handle, quad.ctypes.data, 1, None) == -7
    assert (asm.mapping() == mapping).all()
    # keygen: too few rows, a column of the wrong length, an assembly of another size
    params = zk.halo2.Params.from_g(curve, k, points_of_logs(curve, seeded_scalars(curve, n, seed + 1)))
    col = monts(field, [random.Random(seed).randrange(p) for _ in range(n)])
    for bf in (n - 2, n):
        try:
            zk.halo2.keygen_vk(params, 4, [col], asm, bf)
        except ValueError as e:
            assert "NotEnoughRowsAvailable" in str(e)
        else:
            raise AssertionError("accepted n < blinding_factors + 3")
    for wrong in (col[:n - 1], np.concatenate([col, col]), (col, col[:n // 2])):
        for gen in (lambda: zk.halo2.keygen_vk(params, 4, [col, wrong], asm, 2),
                    lambda: zk.halo2.keygen_pk(params, zk.halo2.keygen_vk(params, 4, [col], asm, 2), [wrong], asm)):
            try:
                gen()
            except AssertionError as e:
                assert "assertion failed: a.values.len() == 1 << self.k" in str(e)
            else:
                raise AssertionError("accepted a fixed column of the wrong length")
    small = zk.halo2.Assembly(n // 2, ncols)
    try:
        zk.halo2.keygen_vk(params, 4, [col], small, 2)
    except AssertionError as e:
        assert "assembly.n == params.n" in str(e)
    else:
        raise AssertionError("accepted an assembly of another size")
    small.free()
    vk = zk.halo2.keygen_vk(params, 4, [col], asm, n - 3)                        # n == blinding_factors + 3 is the smallest accepted
    try:
        zk.halo2.keygen_pk(params, vk, [col], asm, cosets="r29")
    except zk.ZkError as e:
        assert e.status == -1
    else:
        raise AssertionError("accepted an unknown coset form")
    # ... and the library is still usable: a whole key
    pk = zk.halo2.keygen_pk(params, vk, [col], asm)
    assert (to_host(zk, pk.permutation.permutations) == exp).all()
    assert (zk.point_to_affine(curve, vk.fixed_commitments[0]) == zk.point_to_affine(curve, params.commit_lagrange(to_device(zk, col)))).all()
    pk.free()
    asm.free()
    params.free()


def ctypes_u64():
    import ctypes
    v = ctypes.c_uint64(0)
    return v, ctypes.byref(v)
