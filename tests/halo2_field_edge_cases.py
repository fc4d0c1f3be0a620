"""The field-side kernels of the halo2 prover (csrc/zk_poly_kernels.h, launched from csrc/zk_poly.inl) at the launch and operand edges:
past one grid of a grid-capped kernel, scans deep enough for scan_totals_kernel to own several tiles per lane, zeros through the shared
inversion, small and odd lengths, a batch evaluation whose stride is not its length, and the aliasing the headers document.

The reference is written here, on Python integers, from the definition of each operation: running products, Horner, the fold
formulas of the kernel comments / halo2_proofs 0.2, the inverse as pow(x, p - 2, p) (0 -> 0, as upstream's BatchInvert leaves it).
Nothing of oracle/pyref_halo2.py is called.  Every comparison is exact, word for word, on Montgomery limbs; the one exception is
check_permutation_relation (k = 21), which checks the local relation z[i+1] den_i = z[i] num_i on a fixed set of rows.

Where a reference needs an inverse per element at a length past 2^16 (the lookup product past one grid) the inverses come from
inv_many: Montgomery's trick on Python integers around ONE pow(t, p - 2, p), every result then checked against the definition
(x * x^-1 = 1 mod p) before it is used -- 10^6 Fermat powers in Python are a minute and a half.

Large inputs are random Montgomery limbs straight from numpy (any canonical four-word value below p is the Montgomery form of some
element) and reach Python integers through the oracle's from_mont; they are drawn once per field and shared (base_vector)."""
import functools

import numpy as np

from oracle import pyref
from oracle import zk_oracle as orc
from parity_suite import to_device, to_host

SCAN_WG = 256                  # lanes of a scan workgroup = lanes of scan_totals_kernel
TILE = SCAN_WG * 16            # SCAN_WG * SCAN_K elements per scan workgroup
G = 4096 * 256                 # one grid of the kernels capped at 4096 workgroups of 256 lanes
G_WIDE = 8192 * 256            # vec_muladd and vec_fold_many are capped at 8192 workgroups (zk_poly.inl)
G_IP = 1024 * 256              # inner_product
NB = G_WIDE + 2 * 257          # length of the shared base vectors: two halves of G + 257, or one of G_WIDE + 257
ZK_ERR_INVALID_ARG = -1        # include/zkcp_amd.h
SENTINEL = 0xA5A5A5A5A5A5A5A5  # what an output buffer holds before the call: an element never written shows


def P(name):
    return pyref.FIELDS[name][0]


# ---------------------------------------------------------------- integers <-> limbs, fast enough for 2^21 elements
def limbs_of(vals):
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def ints_of(limbs):
    b = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def monts(name, vals):
    p = P(name)
    return orc.to_mont(name, limbs_of([v % p for v in vals])) if len(vals) else np.zeros((0, 4), dtype=np.uint64)


def m1(name, v):
    return monts(name, [v])[0]


def ints(name, arr):
    return ints_of(orc.from_mont(name, np.ascontiguousarray(arr, dtype=np.uint64))) if len(arr) else []


def rand_limbs(name, n, seed):
    """n random elements as Montgomery limbs: below 2^253, which is below every scalar modulus here"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(3)
    assert P(name) >> 253
    return a


def same(got, exp, what):
    got = np.asarray(got)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero((got != exp).any(axis=1))
        raise AssertionError("%s: %d of %d elements differ, the first at %d" % (what, len(bad), len(exp), int(bad[0])))


def blank(zk, n):
    return to_device(zk, np.full((n, 4), SENTINEL, dtype=np.uint64))


def inv(x, p):
    return pow(x, p - 2, p) if x else 0


def inv_many(xs, p):
    """1 / x for every x (0 -> 0): prefix products, one Fermat power, back-substitution; each result checked by x * x^-1 = 1"""
    pre, run = [], 1
    for x in xs:
        pre.append(run)
        if x:
            run = run * x % p
    t = pow(run, p - 2, p)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        x = xs[i]
        if x:
            out[i] = t * pre[i] % p
            t = t * x % p
    assert all(x * y % p == (1 if x else 0) for x, y in zip(xs, out))
    return out


@functools.lru_cache(maxsize=None)
def base_vector(name, which):
    """shared random vector `which` of the field: (Montgomery limbs [NB, 4], the same as Python integers); never written"""
    limbs = rand_limbs(name, NB, 0xF1E1D + 977 * which + sum(name.encode()))
    limbs.setflags(write=False)
    return limbs, ints(name, limbs)


def take(name, which, n, off=0, edges=True):
    """n elements of a base vector from `off` on, as (limbs, integers), own copies; edges: 0 at index 0, p - 1 at the last index"""
    limbs, vals = base_vector(name, which)
    assert off + n <= NB
    limbs, vals = limbs[off:off + n].copy(), vals[off:off + n]
    if edges and n:
        vals[0] = 0
        limbs[0] = 0
        if n > 1:
            vals[n - 1] = P(name) - 1
            limbs[n - 1] = m1(name, P(name) - 1)
    return limbs, vals


def small_values(name, n, seed, kind="random"):
    """n integers: random, or made only of {0, 1, p - 1}"""
    p, rng = P(name), pyref.Rng(seed)
    if kind == "edge":
        return [(0, 1, p - 1)[rng.below(3)] for _ in range(n)]
    return [rng.below(p) for _ in range(n)]


def expect_invalid(zk, fn):
    try:
        fn()
    except zk.ZkError as e:
        assert e.status == ZK_ERR_INVALID_ARG, e
        return
    raise AssertionError("the call must be refused with ZK_ERR_INVALID_ARG")


# ---------------------------------------------------------------- A. scan depth
# nblocks = ceil(n / TILE) tile totals go through scan_totals_kernel, lane t owning [t per, (t + 1) per) with
# per = ceil(nblocks / SCAN_WG): 256 tiles is the last per = 1; 257 -> per = 2 and lanes 129 .. 255 empty; 511 -> per = 2 and the
# last lane owns one tile; 513 -> per = 3 and lanes from 171 on empty.
SCAN_NS = (0, 1, TILE, TILE + 1, SCAN_WG * TILE, SCAN_WG * TILE + 1, 511 * TILE - 7, 513 * TILE - 7)
SCAN_EMU_MAX = 257 * TILE
SCAN_NS_EMU = tuple(n for n in SCAN_NS if n <= SCAN_EMU_MAX)
SCAN_ALIAS_N = SCAN_WG * TILE + 1         # 257 tiles (F: in == out as documented)
SCAN_ZERO_N = 511 * TILE - 7


@functools.lru_cache(maxsize=None)
def _scan_reference(name, n_max):
    """(f as limbs, first, [first * prod_{j<i} f[j] for i <= n_max] as limbs): one running product serves every n <= n_max"""
    p = P(name)
    f = rand_limbs(name, n_max, 0x5CA9 + sum(name.encode()))
    first = pyref.Rng(0x5CA9F).below(p - 1) + 1
    z, acc = [0] * (n_max + 1), first
    for i, x in enumerate(ints(name, f)):
        z[i] = acc
        acc = acc * x % p
    z[n_max] = acc
    f.setflags(write=False)
    return f, first, monts(name, z)


def check_scan(zk, name, n, in_place):
    f, first, z = _scan_reference(name, SCAN_EMU_MAX if n <= SCAN_EMU_MAX else max(SCAN_NS))
    d_in = to_device(zk, f[:n].copy())
    if in_place:
        out, total = zk.halo2.prefix_product(name, d_in, first=m1(name, first), want_total=True)
    else:
        out, total = zk.halo2.prefix_product(name, d_in, out=blank(zk, n), first=m1(name, first), want_total=True)
        same(to_host(zk, d_in), f[:n], "prefix_product left its input alone (%s, n = %d)" % (name, n))
    same(to_host(zk, out), z[:n], "prefix_product(%s, n = %d, %s)" % (name, n, "in place" if in_place else "out of place"))
    assert (total == z[n]).all(), (name, n, "total")


def check_scan_zero_in_last_tile(zk, name, n=SCAN_ZERO_N):
    """a 0 in the last tile: everything after it is 0 and so is the total"""
    f, first, z = _scan_reference(name, SCAN_EMU_MAX if n <= SCAN_EMU_MAX else max(SCAN_NS))
    at = n - 1000
    assert at // TILE == (n - 1) // TILE and at % TILE
    f, exp = f[:n].copy(), z[:n].copy()
    f[at] = 0
    exp[at + 1:] = 0
    out, total = zk.halo2.prefix_product(name, to_device(zk, f), out=blank(zk, n), first=m1(name, first), want_total=True)
    same(to_host(zk, out), exp, "prefix_product with a zero at %d of %d" % (at, n))
    assert not total.any()


# ---------------------------------------------------------------- B. the second grid-stride trip
def case_lookup_product(zk, name="PallasFp", n=G + 257):
    p, rng = P(name), pyref.Rng(0xB001)
    beta, gamma = rng.below(p), rng.below(p)
    (dA, A), (dS, S), (dAp, Ap), (dSp, Sp) = take(name, 0, n), take(name, 1, n), take(name, 2, n), take(name, 0, n, off=NB - n)
    den = [(x + beta) * (y + gamma) % p for x, y in zip(Ap, Sp)]
    assert all(den)
    z, acc = [0] * n, 1
    for i, (a, s, d) in enumerate(zip(A, S, inv_many(den, p))):
        z[i] = acc
        acc = acc * ((a + beta) * (s + gamma) % p * d % p) % p
    z_out = blank(zk, n)
    last = zk.halo2.lookup_product(name, *[to_device(zk, v) for v in (dA, dS, dAp, dSp)], m1(name, beta), m1(name, gamma), z_out)
    same(to_host(zk, z_out), monts(name, z), "lookup_product(n = %d)" % n)
    assert (last == m1(name, acc)).all()


def case_vec_muladd(zk, name="PallasFp", n=G_WIDE + 257, out=False):
    p = P(name)
    s = pyref.Rng(0xB002).below(p)
    (la, a), (lb, b) = take(name, 0, n), take(name, 1, n)
    lb[0], b[0], lb[n - 1], b[n - 1] = m1(name, p - 1), p - 1, 0, 0            # the second operand mirrored: p - 1 first, 0 last
    exp = monts(name, [(x * s + y) % p for x, y in zip(a, b)])
    d_a, d_b = to_device(zk, la), to_device(zk, lb)
    if out:
        got = zk.halo2.vec_muladd(name, d_a, d_b, m1(name, s), out=blank(zk, n))
        same(to_host(zk, d_a), la, "vec_muladd(out=) left a alone")
    else:
        got = zk.halo2.vec_muladd(name, d_a, d_b, m1(name, s))
    same(to_host(zk, got), exp, "vec_muladd(n = %d, out = %s)" % (n, out))
    same(to_host(zk, d_b), lb, "vec_muladd left b alone")


def case_vec_fold(zk, name="PallasFp", half=G + 257):
    p = P(name)
    c = pyref.Rng(0xB003).below(p)
    la, a = take(name, 0, 2 * half)
    exp = [(a[i] + c * a[i + half]) % p for i in range(half)] + a[half:]          # the upper half stays
    got = zk.halo2.vec_fold(name, to_device(zk, la), half, m1(name, c))
    same(to_host(zk, got), monts(name, exp), "vec_fold(half = %d)" % half)


def fold_many_reference(polys, s, p, reverse):
    order = polys[::-1] if reverse else polys
    acc = list(order[0])
    for q in order[1:]:
        acc = [(e * s + v) % p for e, v in zip(acc, q)]
    return acc


def case_vec_fold_many(zk, name="PallasFp", n=G_WIDE + 257, reverse=False):
    p = P(name)
    s = pyref.Rng(0xB004).below(p)
    parts = [take(name, w, n) for w in range(3)]
    host = np.stack([l for l, _ in parts])
    exp = monts(name, fold_many_reference([v for _, v in parts], s, p, reverse))
    d_polys = to_device(zk, host)
    got = zk.halo2.vec_fold_many(name, blank(zk, n), d_polys, m1(name, s), reverse=reverse)
    same(to_host(zk, got), exp, "vec_fold_many(n = %d, reverse = %s)" % (n, reverse))
    assert np.array_equal(to_host(zk, d_polys), host), "vec_fold_many left its sources alone"


def case_vec_powers(zk, name="PallasFp", n=G + 257, x=None):
    p = P(name)
    x = pyref.Rng(0xB005).below(p) if x is None else x % p
    exp, acc = [0] * n, 1
    for i in range(n):
        exp[i] = acc
        acc = acc * x % p
    got = zk.halo2.vec_powers(name, blank(zk, n), m1(name, x))
    same(to_host(zk, got), monts(name, exp), "vec_powers(n = %d)" % n)


def fold_round_reference(pv, bv, w, half, m0, u, p):
    ui = inv(u, p)
    pv, bv = list(pv), list(bv)
    for i in range(half):
        pv[i] = (pv[i] + ui * pv[i + half]) % p
        bv[i] = (bv[i] + u * bv[i + half]) % p
    if w is not None:
        w = [x * u % p if i & half else x for i, x in enumerate(w[:m0])] + list(w[m0:])
    return pv, bv, w


def case_ipa_fold_round(zk, name="PallasFp", half=G + 257, m0=0):
    """m0 = 0: without the weights; otherwise W over m0 generators (half and m0 powers of two, half < m0)"""
    p = P(name)
    u = pyref.Rng(0xB006).below(p - 1) + 1
    (lp, pv), (lb, bv) = take(name, 0, 2 * half), take(name, 1, 2 * half)
    lw, w = take(name, 2, m0) if m0 else (None, None)
    ep, eb, ew = fold_round_reference(pv, bv, w, half, m0, u, p)
    d_p, d_b, d_w = to_device(zk, lp), to_device(zk, lb), to_device(zk, lw) if m0 else None
    zk.halo2.ipa_fold_round(name, d_p, d_b, half, m1(name, u), w=d_w, m0=m0)
    same(to_host(zk, d_p), monts(name, ep), "ipa_fold_round p (half = %d, m0 = %d)" % (half, m0))
    same(to_host(zk, d_b), monts(name, eb), "ipa_fold_round b (half = %d, m0 = %d)" % (half, m0))
    if m0:
        same(to_host(zk, d_w), monts(name, ew), "ipa_fold_round W (half = %d, m0 = %d)" % (half, m0))


def ipa_virtual_scalars(zk, name, d_p, d_w, m0, cur, d_sl, d_sr):
    st = zk.halo2._plib().zk_ipa_virtual_scalars_device(zk.field_id(name), zk._ptr(d_p), zk._ptr(d_w), m0, cur, zk._ptr(d_sl), zk._ptr(d_sr), None)
    zk._check(st, "zk_ipa_virtual_scalars_device")


def ipa_update_weights(zk, name, d_w, m0, bit, u_mont):
    uu = np.ascontiguousarray(u_mont, dtype=np.uint64)
    zk._check(zk.halo2._plib().zk_ipa_update_weights_device(zk.field_id(name), zk._ptr(d_w), m0, bit, zk._ptr(uu), None), "zk_ipa_update_weights_device")


def check_virtual_scalars(zk, name, lp, pv, lw, w, m0, cur):
    """S_L[idx] = p[i + cur/2] W[idx] for i = idx mod cur < cur/2, else 0; S_R[idx] = p[i - cur/2] W[idx] for i >= cur/2, else 0"""
    p, half = P(name), cur // 2
    sl, sr = [0] * m0, [0] * m0
    for idx in range(m0):
        i = idx % cur
        if i < half:
            sl[idx] = pv[i + half] * w[idx] % p
        else:
            sr[idx] = pv[i - half] * w[idx] % p
    d_sl, d_sr = blank(zk, m0), blank(zk, m0)
    ipa_virtual_scalars(zk, name, to_device(zk, lp), to_device(zk, lw), m0, cur, d_sl, d_sr)
    same(to_host(zk, d_sl), monts(name, sl), "ipa_virtual_scalars S_L (m0 = %d, cur = %d)" % (m0, cur))
    same(to_host(zk, d_sr), monts(name, sr), "ipa_virtual_scalars S_R (m0 = %d, cur = %d)" % (m0, cur))


def case_ipa_virtual_scalars(zk, name="PallasFp", m0=1 << 21, cur=2):
    (lp, pv), (lw, w) = take(name, 0, cur), take(name, 1, m0)
    check_virtual_scalars(zk, name, lp, pv, lw, w, m0, cur)


def check_update_weights(zk, name, lw, w, m0, bit, u):
    p = P(name)
    exp = [x * u % p if idx & bit else x for idx, x in enumerate(w[:m0])] + list(w[m0:])
    d_w = to_device(zk, lw)
    ipa_update_weights(zk, name, d_w, m0, bit, m1(name, u))
    same(to_host(zk, d_w), monts(name, exp), "ipa_update_weights (m0 = %d, bit = %d)" % (m0, bit))


def case_ipa_update_weights(zk, name="PallasFp", m0=1 << 21, cur=2):
    lw, w = take(name, 1, m0)
    check_update_weights(zk, name, lw, w, m0, cur // 2, pyref.Rng(0xB007).below(P(name)))


def case_inner_product(zk, name="PallasFp", n=G_IP + 257):
    p = P(name)
    (la, a), (lb, b) = take(name, 0, n), take(name, 1, n, edges=False)
    got = zk.halo2.inner_product(name, to_device(zk, la), to_device(zk, lb))
    assert (got == m1(name, sum(x * y for x, y in zip(a, b)) % p)).all(), ("inner_product", name, n)


def halo2_delta(name):
    p = P(name)
    return pow(pyref.FIELDS[name][1], 1 << pyref.two_adicity(p)[0], p)        # halo2's DELTA = generator^(2^S)


def permutation_relation_rows(n, seed=0xB008):
    """the fixed row set of the k = 21 case: both sides of every tile boundary, the 600 rows around one grid, the first and the last
    32 rows, 1000 seeded random rows"""
    rng = pyref.Rng(seed)
    rows = set(range(min(32, n))) | set(range(max(0, n - 32), n)) | {rng.below(n) for _ in range(1000)}
    for j in range(1, (n + TILE - 1) // TILE):
        rows |= {TILE * j - 1, TILE * j}
    rows |= {r for r in range(G - 300, G + 300) if 0 <= r < n}
    return sorted(rows)


def case_permutation_relation(zk, name="PallasFp", k=21, first_col=3):
    """permutation_product at 2^k rows, two columns: the local relation z[i + 1] den_i = z[i] num_i on permutation_relation_rows, with
    num_i = prod_c (v_c[i] + beta delta^(first_col + c) omega^i + gamma), den_i = prod_c (v_c[i] + beta sigma_c[i] + gamma) from
    Python integers; z[0] = z_first; the returned value = z[n - 1] num_(n-1) / den_(n-1).  (An error shows only at the row where it is
    made: the row set is fixed, not sampled at will.)"""
    p, n, rng = P(name), 1 << k, pyref.Rng(0xB009)
    assert n + 514 <= NB
    beta, gamma, z_first = rng.below(p), rng.below(p), rng.below(p - 1) + 1
    delta, omega = halo2_delta(name), pyref.root_of_unity(name, k)
    cols = [take(name, 0, n)[0], take(name, 1, n, edges=False)[0]]
    sigs = [take(name, 2, n, edges=False)[0], take(name, 0, n, off=514, edges=False)[0]]
    d_cols, d_sigs, z_out = [to_device(zk, c) for c in cols], [to_device(zk, s) for s in sigs], blank(zk, n)
    last = zk.halo2.permutation_product(name, d_cols, d_sigs, m1(name, beta), m1(name, gamma), m1(name, delta), k, z_out,
                                        first_column_index=first_col, z_first=m1(name, z_first))
    z = to_host(zk, z_out)
    assert (z[0] == m1(name, z_first)).all(), "z[0] = z_first"
    rows = permutation_relation_rows(n)
    at = np.array(rows, dtype=np.int64)
    nxt = np.minimum(at + 1, n - 1)
    assert all(v < p for v in ints_of(z[at])) and all(v < p for v in ints_of(z[nxt])), "canonical words"
    z_i, z_n = ints(name, z[at]), ints(name, z[nxt])
    v = [ints(name, c[at]) for c in cols]
    s = [ints(name, c[at]) for c in sigs]
    for j, i in enumerate(rows):
        w = pow(omega, i, p)
        num = den = 1
        for c in range(2):
            num = num * ((v[c][j] + beta * pow(delta, first_col + c, p) % p * w + gamma) % p) % p
            den = den * ((v[c][j] + beta * s[c][j] + gamma) % p) % p
        assert den, i
        if i + 1 < n:
            assert z_n[j] * den % p == z_i[j] * num % p, ("permutation_product: z[i + 1] den_i != z[i] num_i", i)
        else:
            assert (last == m1(name, z_i[j] * num % p * inv(den, p) % p)).all(), "returned last = z[n - 1] f[n - 1]"


# name -> (function, keyword arguments): every case runs on the GPU tier; SECOND_TRIP_EMU names the ones the emulator finishes in time
SECOND_TRIP = {
    "lookup_product": (case_lookup_product, {}),
    "vec_muladd": (case_vec_muladd, {}),
    "vec_muladd_narrow_grid": (case_vec_muladd, {"n": G + 257}),
    "vec_muladd_out": (case_vec_muladd, {"out": True}),
    "vec_fold": (case_vec_fold, {}),
    "vec_fold_many": (case_vec_fold_many, {}),
    "vec_fold_many_reverse": (case_vec_fold_many, {"reverse": True}),
    "vec_powers": (case_vec_powers, {}),
    "vec_powers_minus_one": (case_vec_powers, {"x": -1}),
    "ipa_fold_round": (case_ipa_fold_round, {}),
    "ipa_fold_round_w_half_2e18": (case_ipa_fold_round, {"half": 1 << 18, "m0": 1 << 21}),
    "ipa_fold_round_w_half_2e20": (case_ipa_fold_round, {"half": 1 << 20, "m0": 1 << 21}),
    "ipa_virtual_scalars_cur_2": (case_ipa_virtual_scalars, {"cur": 2}),
    "ipa_virtual_scalars_cur_2e19": (case_ipa_virtual_scalars, {"cur": 1 << 19}),
    "ipa_virtual_scalars_cur_2e21": (case_ipa_virtual_scalars, {"cur": 1 << 21}),
    "ipa_update_weights_cur_2": (case_ipa_update_weights, {"cur": 2}),
    "ipa_update_weights_cur_2e19": (case_ipa_update_weights, {"cur": 1 << 19}),
    "ipa_update_weights_cur_2e21": (case_ipa_update_weights, {"cur": 1 << 21}),
    "inner_product_grid_minus_1": (case_inner_product, {"n": G_IP - 1}),
    "inner_product_grid": (case_inner_product, {"n": G_IP}),
    "inner_product_grid_plus_1": (case_inner_product, {"n": G_IP + 1}),
    "inner_product_grid_plus_257": (case_inner_product, {"n": G_IP + 257}),
    "permutation_product_k21": (case_permutation_relation, {}),
}


SECOND_TRIP_EMU = tuple(sorted(SECOND_TRIP))         # the slowest in the emulator: permutation_product_k21 12 s, lookup_product 10 s


def run_second_trip(zk, case):
    fn, kw = SECOND_TRIP[case]
    fn(zk, **kw)


# ---------------------------------------------------------------- C. zeros in batch inversion
INVERT_FIELDS = ("PallasFp", "Bn254Fr")
INVERT_NS = (1, 15, 16, 17, 1023, 1024, 1025, 1041)
INV_K = 16                     # elements that share one inversion


def zero_patterns(n):
    """name -> the indices set to zero"""
    pats = {
        "all zero": range(n),
        "chunk [16, 32) zero": range(min(INV_K, n), min(2 * INV_K, n)),
        "first of every chunk": range(0, n, INV_K),
        "last of every chunk": sorted(set(range(INV_K - 1, n, INV_K)) | {n - 1}),
        "odd indices": range(1, n, 2),
        "ragged last chunk: its last element (the whole chunk where n = 1 mod 16)": [n - 1],
    }
    for j in range(INV_K):
        pats["only position %d of a chunk nonzero" % j] = [i for i in range(n) if i % INV_K != j]
    return pats


def check_batch_invert_zeros(zk, name, n):
    p, rng = P(name), pyref.Rng(0xC001 + n)
    base = [(1, p - 1)[(i // 3) % 2] if i % 3 == 1 else rng.below(p - 1) + 1 for i in range(n)]      # nonzero, 1 and p - 1 among them
    if n > 1:
        base[n - 2] = p - 1
    inverse = {x: inv(x, p) for x in set(base)}
    inverse[0] = 0
    for what, zeros in zero_patterns(n).items():
        a = list(base)
        for i in zeros:
            a[i] = 0
        got = zk.halo2.batch_invert(name, to_device(zk, monts(name, a)))
        same(to_host(zk, got), monts(name, [inverse[x] for x in a]), "batch_invert(%s, n = %d, %s)" % (name, n, what))


def grand_product(f, first, p):
    z, acc = [], first
    for x in f:
        z.append(acc)
        acc = acc * x % p
    return z, acc


def _assert_dies_after(zk, name, z_out, last, z_exp, last_exp, r, what):
    n = len(z_exp)
    got = to_host(zk, z_out)
    same(got, monts(name, z_exp), what)
    assert all(z_exp[:r + 1]), "the reference is nonzero up to and including the row"
    assert not got[r + 1:].any() and not last.any() and last_exp == 0 and not any(z_exp[r + 1:]), (what, "Z is 0 after row %d of %d" % (r, n))


def check_lookup_zero_denominator(zk, name, n=100, rows=(0, 17, 99)):
    """A'_r + beta = 0: the inverse of 0 is 0, so f_r = 0, Z is the reference up to and including r and 0 from r + 1 on"""
    p, rng = P(name), pyref.Rng(0xC002)
    beta, gamma = rng.below(p - 1) + 1, rng.below(p)
    A, S, Ap, Sp = (small_values(name, n, 0xC010 + q) for q in range(4))
    for r in rows:
        ap = list(Ap)
        ap[r] = (p - beta) % p
        f = [(a + beta) * (s + gamma) % p * inv((x + beta) * (y + gamma) % p, p) % p for a, s, x, y in zip(A, S, ap, Sp)]
        assert f[r] == 0 and all(f[:r]) and all(f[r + 1:])
        z_exp, last_exp = grand_product(f, 1, p)
        z_out = blank(zk, n)
        last = zk.halo2.lookup_product(name, *[to_device(zk, monts(name, v)) for v in (A, S, ap, Sp)], m1(name, beta), m1(name, gamma), z_out)
        _assert_dies_after(zk, name, z_out, last, z_exp, last_exp, r, "lookup_product(%s) with a zero denominator at row %d" % (name, r))


def check_permutation_zero_denominator(zk, name, k=6, rows=(0, 17, 63)):
    """v + beta sigma + gamma = 0 in one column at row r"""
    p, n, rng = P(name), 1 << k, pyref.Rng(0xC003)
    beta, gamma = rng.below(p - 1) + 1, rng.below(p)
    delta, omega = halo2_delta(name), pyref.root_of_unity(name, k)
    cols = [small_values(name, n, 0xC020 + c) for c in range(2)]
    sigs = [small_values(name, n, 0xC030 + c) for c in range(2)]
    for r in rows:
        sg = [list(s) for s in sigs]
        sg[1][r] = (p - gamma - cols[1][r]) * inv(beta, p) % p
        f = []
        for i in range(n):
            num = den = 1
            for c in range(2):
                num = num * ((cols[c][i] + beta * pow(delta, c, p) * pow(omega, i, p) + gamma) % p) % p
                den = den * ((cols[c][i] + beta * sg[c][i] + gamma) % p) % p
            f.append(num * inv(den, p) % p)
        assert f[r] == 0 and all(f[:r]) and all(f[r + 1:])
        z_exp, last_exp = grand_product(f, 1, p)
        z_out = blank(zk, n)
        last = zk.halo2.permutation_product(name, [to_device(zk, monts(name, c)) for c in cols], [to_device(zk, monts(name, s)) for s in sg],
                                            m1(name, beta), m1(name, gamma), m1(name, delta), k, z_out)
        _assert_dies_after(zk, name, z_out, last, z_exp, last_exp, r, "permutation_product(%s) with a zero denominator at row %d" % (name, r))


# ---------------------------------------------------------------- D. small and odd lengths, edge operands
SMALL_NS = (0, 1, 2, 255, 256, 257, 1000)
SMALL_FIELDS = ("PallasFp", "PallasFq")
GUARD = 3                      # elements past the end of a buffer that a call must leave alone


def check_inner_product_small(zk, name, n):
    p = P(name)
    for kind in ("random", "edge"):
        a, b = small_values(name, n, 0xD001 + n, kind), small_values(name, n, 0xD002 + n, kind)
        got = zk.halo2.inner_product(name, to_device(zk, monts(name, a)), to_device(zk, monts(name, b)))
        assert (got == m1(name, sum(x * y for x, y in zip(a, b)) % p)).all(), ("inner_product", name, n, kind)      # n = 0: 0


def check_inner_product_minus_ones(zk, name, n=257):
    p = P(name)
    d = to_device(zk, monts(name, [p - 1] * n))
    assert (zk.halo2.inner_product(name, d, d) == m1(name, n % p)).all(), ("257 copies of (p - 1)(p - 1)", name)
    assert (zk.halo2.inner_product(name, d, to_device(zk, monts(name, [p - 1] * n))) == m1(name, n % p)).all()


def check_vec_fold_small(zk, name, half):
    p, rng = P(name), pyref.Rng(0xD003 + half)
    for kind in ("random", "edge"):
        for c in (rng.below(p), 0, 1, p - 1):
            a = small_values(name, 2 * half + GUARD, 0xD004 + half, kind)
            exp = [(a[i] + c * a[i + half]) % p for i in range(half)] + a[half:]
            got = zk.halo2.vec_fold(name, to_device(zk, monts(name, a)), half, m1(name, c))
            same(to_host(zk, got), monts(name, exp), "vec_fold(%s, half = %d, %s, c = %d)" % (name, half, kind, c))


def check_ipa_fold_round_small(zk, name, half):
    p, rng = P(name), pyref.Rng(0xD005 + half)
    for kind in ("random", "edge"):
        for u in (rng.below(p - 1) + 1, 1, p - 1):
            pv, bv = (small_values(name, 2 * half + GUARD, 0xD006 + half + q, kind) for q in range(2))
            ep, eb, _ = fold_round_reference(pv, bv, None, half, 0, u, p)
            d_p, d_b = to_device(zk, monts(name, pv)), to_device(zk, monts(name, bv))
            zk.halo2.ipa_fold_round(name, d_p, d_b, half, m1(name, u))
            same(to_host(zk, d_p), monts(name, ep), "ipa_fold_round p (%s, half = %d, %s)" % (name, half, kind))
            same(to_host(zk, d_b), monts(name, eb), "ipa_fold_round b (%s, half = %d, %s)" % (name, half, kind))


def check_ipa_fold_round_weights_small(zk, name, m0=512):
    """with W: half a power of two below m0, half < one workgroup and past it"""
    p, rng = P(name), pyref.Rng(0xD007)
    for half in (1, 2, 256):
        for kind in ("random", "edge"):
            u = rng.below(p - 1) + 1
            pv, bv = (small_values(name, 2 * half + GUARD, 0xD008 + half + q, kind) for q in range(2))
            w = small_values(name, m0 + GUARD, 0xD009 + half, kind)
            ep, eb, ew = fold_round_reference(pv, bv, w, half, m0, u, p)
            d_p, d_b, d_w = (to_device(zk, monts(name, v)) for v in (pv, bv, w))
            zk.halo2.ipa_fold_round(name, d_p, d_b, half, m1(name, u), w=d_w, m0=m0)
            for d, e, what in ((d_p, ep, "p"), (d_b, eb, "b"), (d_w, ew, "W")):
                same(to_host(zk, d), monts(name, e), "ipa_fold_round %s (%s, half = %d, m0 = %d, %s)" % (what, name, half, m0, kind))


def check_ipa_fold_round_refuses_zero(zk, name, half=17):
    pv = small_values(name, 2 * half, 0xD00A)
    d_p, d_b = to_device(zk, monts(name, pv)), to_device(zk, monts(name, pv))
    expect_invalid(zk, lambda: zk.halo2.ipa_fold_round(name, d_p, d_b, half, m1(name, 0)))
    same(to_host(zk, d_p), monts(name, pv), "a refused call leaves p alone")
    same(to_host(zk, d_b), monts(name, pv), "a refused call leaves b alone")


def check_ipa_scalar_helpers_small(zk, name):
    """ipa_virtual_scalars needs powers of two (m0 = 512: two workgroups); ipa_update_weights takes any m0"""
    p, rng = P(name), pyref.Rng(0xD00B)
    for kind in ("random", "edge"):
        m0 = 512
        w = small_values(name, m0, 0xD00C, kind)
        for cur in (2, 64, 512):
            pv = small_values(name, cur, 0xD00D + cur, kind)
            check_virtual_scalars(zk, name, monts(name, pv), pv, monts(name, w), w, m0, cur)
        for m0, bit in ((2, 1), (257, 1), (257, 256), (1000, 8), (1000, 512)):
            w = small_values(name, m0 + GUARD, 0xD00E + m0, kind)
            for u in (rng.below(p), 0, 1, p - 1):
                check_update_weights(zk, name, monts(name, w), w, m0, bit, u)


# ---------------------------------------------------------------- E. batch evaluation with a stride that is not the length
EVAL_NS = (17, 5000)


def poly_eval_batch(zk, name, d_buf, n, count, stride, x_mont):
    out = np.zeros((count, 4), dtype=np.uint64)
    xx = np.ascontiguousarray(x_mont, dtype=np.uint64)
    st = zk.halo2._plib().zk_poly_eval_batch_device(zk.field_id(name), zk._ptr(d_buf), n, count, stride, zk._ptr(xx), zk._ptr(out), None)
    return st, out


def check_eval_batch_stride(zk, name, n, count=3):
    """the polynomials `stride` elements apart in one buffer, the gaps filled with p - 1 so that a wrong stride changes the value"""
    p, rng = P(name), pyref.Rng(0xE001 + n)
    polys = [small_values(name, n, 0xE002 + n + q) for q in range(count)]
    x = rng.below(p)
    exp = []
    for c in polys:
        acc = 0
        for v in reversed(c):
            acc = (acc * x + v) % p
        exp.append(acc)
    for stride in (n, n + 3, 2 * n):
        buf = [p - 1] * (count * stride)
        for q in range(count):
            buf[q * stride:q * stride + n] = polys[q]
        st, got = poly_eval_batch(zk, name, to_device(zk, monts(name, buf)), n, count, stride, m1(name, x))
        assert st == 0, st
        same(got, monts(name, exp), "zk_poly_eval_batch_device(%s, n = %d, stride = %d)" % (name, n, stride))
    st, _ = poly_eval_batch(zk, name, to_device(zk, monts(name, buf)), n, count, n - 1, m1(name, x))
    assert st == ZK_ERR_INVALID_ARG, st


# ---------------------------------------------------------------- F. aliasing as the headers document it
def check_muladd_into_b(zk, name, n=1000):
    p = P(name)
    a, b, s = small_values(name, n, 0xF001), small_values(name, n, 0xF002), pyref.Rng(0xF003).below(p)
    a[0], b[0], a[n - 1], b[n - 1] = 0, p - 1, p - 1, 0
    d_a, d_b = to_device(zk, monts(name, a)), to_device(zk, monts(name, b))
    got = zk.halo2.vec_muladd(name, d_a, d_b, m1(name, s), out=d_b)
    same(to_host(zk, got), monts(name, [(x * s + y) % p for x, y in zip(a, b)]), "vec_muladd(a, b, s, out=b) (%s)" % name)
    same(to_host(zk, d_a), monts(name, a), "vec_muladd(out=b) left a alone")


def check_fold_many_into_source(zk, name, n=1000, count=3):
    p = P(name)
    polys, s = [small_values(name, n, 0xF010 + q) for q in range(count)], pyref.Rng(0xF004).below(p)
    host = np.stack([monts(name, c) for c in polys])
    for reverse, target in ((False, 0), (True, count - 1), (False, 1), (True, 1), (False, count - 1), (True, 0)):
        d_polys = to_device(zk, host)
        got = zk.halo2.vec_fold_many(name, d_polys[target], d_polys, m1(name, s), reverse=reverse)
        exp = host.copy()
        exp[target] = monts(name, fold_many_reference(polys, s, p, reverse))
        same(to_host(zk, got), exp[target], "vec_fold_many(out = polys[%d], reverse = %s) (%s)" % (target, reverse, name))
        assert np.array_equal(to_host(zk, d_polys), exp), "the other sources stay"


def check_fold_many_refuses_partial_overlap(zk, name, n=1000, count=3):
    """out = polys[0] shifted by one element: neither a source nor disjoint from them"""
    flat = monts(name, small_values(name, count * n + 1, 0xF005))
    d = to_device(zk, flat)
    d_polys = d[:count * n].reshape(count, n, 4)
    for reverse in (False, True):
        expect_invalid(zk, lambda: zk.halo2.vec_fold_many(name, d[1:n + 1], d_polys, m1(name, 5), reverse=reverse))
    same(to_host(zk, d), flat, "a refused call writes nothing")
