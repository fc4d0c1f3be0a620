"""TEST INFRASTRUCTURE shared by tests/test_msm_collisions_emu.py (CPU tier, emulator build) and tests/test_msm_collisions_gpu.py
(-m gpu): multi-scalar multiplications whose operands COLLIDE -- equal points, opposite points, identities -- so that the
exceptional branches of every point addition in the Pippenger pipeline run where the kernels call them, after a real
accumulation history (ZZ != 1), on every path of the pipeline (oversized buckets, bucket splitting, the precomputed table,
batches, window shares, both bucket reductions, the host tail), and the same for halo2's generator fold.

Reference: a case is a list of integer logarithms k_i (base i = [k_i mod r] G from the oracle's fixed_base_mul; k_i = 0 is the
identity (0, 0)) and integer scalars s_i.  The expected point is [sum k_i s_i mod r] G: the sum in Python integers, then ONE
double-and-add of the generator on the oracle (0 -> the identity).  No Pippenger, no buckets, no digit recoding enter it.
Every comparison is word for word on the canonical affine point, and a result other than the identity must be on the curve."""
import os
import random

import numpy as np

from oracle import pyref
from oracle import zk_oracle as orc
from parity_suite import affine_of, to_device, to_host


def order(curve):
    return pyref.FIELDS[pyref.CURVES[curve][1]][0]


def ints_to_arr(xs):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


THREADS = min(8, os.cpu_count() or 1)      # of the oracle's fixed_base_mul


def points_of_logs(curve, ks):
    r = order(curve)
    return orc.fixed_base_mul(curve, ints_to_arr([k % r for k in ks]), threads=THREADS)


def point_of_log(curve, e):
    """[e mod r] G by one double-and-add of the generator; the identity is (0, 0)"""
    e %= order(curve)
    g = orc.curve_generator(curve)
    return np.zeros_like(g) if e == 0 else orc.scalar_mul(curve, g, orc.int_to_limbs(e, 4))


def rand_scalar(rnd, r):
    """uniform in [1, r)"""
    return 1 + rnd.randrange(r - 1)


class Case:
    """bases [k_i] G, canonical scalars s_i mod r and the expected sum"""

    def __init__(self, curve, name, ks, ss):
        assert len(ks) == len(ss)
        r = order(curve)
        self.curve, self.name, self.n = curve, name, len(ks)
        self.ks = [k % r for k in ks]
        self.ss = [s % r for s in ss]
        self.pts = points_of_logs(curve, self.ks)
        assert (self.pts.any(axis=1) == np.array([k != 0 for k in self.ks], dtype=bool)).all()
        self.sc = ints_to_arr(self.ss)
        self.log = sum(k * s for k, s in zip(self.ks, self.ss)) % r
        self.exp = point_of_log(curve, self.log)


_cases = {}


def case(builder, curve, *args):
    """the reference of a case is computed once per process and shared (args: numbers, strings and booleans only)"""
    assert all(isinstance(a, (int, str, bool, type(None))) for a in args), args
    key = (builder.__name__, curve) + args
    if key not in _cases:
        _cases[key] = builder(curve, *args)
    return _cases[key]


# ---------------------------------------------------------------- families
def all_equal(curve, n, seed=1):
    """1: one point n times under one full-width scalar: every bucket of every window holds n copies of it"""
    r = order(curve)
    rnd = random.Random(seed)
    k, s = rand_scalar(rnd, r), rand_scalar(rnd, r)
    return Case(curve, "all equal n=%d" % n, [k] * n, [s] * n)


def alternating(curve, n, extra, seed=2):
    """2: P, -P by index parity under one scalar (n even: the identity); `extra` appends one more P: [s] P"""
    assert n % 2 == 0
    r = order(curve)
    rnd = random.Random(seed)
    k, s = rand_scalar(rnd, r), rand_scalar(rnd, r)
    ks = [k if i % 2 == 0 else r - k for i in range(n)] + ([k] if extra else [])
    cs = Case(curve, "alternating n=%d%s" % (n, " + P" if extra else ""), ks, [s] * len(ks))
    assert cs.log == (k * s % r if extra else 0)
    return cs


def zero_sum_triples(curve, triples, c, extra, seed=3):
    """3: bases a, b, -(a + b) under one small scalar d in [1, 2^(c-1) - 1]: one bucket, whose third mixed add meets acc = -q with
    ZZ != 1 whatever the order; `extra` appends a random base under a random scalar (otherwise the total is the identity)"""
    r = order(curve)
    rnd = random.Random(seed + 100 * c)
    ks, ss = [], []
    for _ in range(triples):
        a, b = rand_scalar(rnd, r), rand_scalar(rnd, r)
        d = rnd.randint(1, max(1, (1 << (c - 1)) - 1))
        ks += [a, b, -(a + b)]
        ss += [d] * 3
    perm = list(range(len(ks)))
    rnd.shuffle(perm)
    ks, ss = [ks[i] for i in perm], [ss[i] for i in perm]
    if extra:
        ks.append(rand_scalar(rnd, r))
        ss.append(rand_scalar(rnd, r))
    cs = Case(curve, "zero-sum triples x%d c=%d%s" % (triples, c, " + base" if extra else ""), ks, ss)
    assert extra or cs.log == 0
    return cs


def identities(curve, n, edge_scalars, seed=4):
    """4: the identity at a third of the indices, index 0 and n - 1 among them, random points and scalars elsewhere;
    `edge_scalars`: the identity bases carry the scalars 1 and r - 1"""
    r = order(curve)
    rnd = random.Random(seed)
    ks = [0 if (i % 3 == 0 or i == n - 1) else rand_scalar(rnd, r) for i in range(n)]
    ss = [rand_scalar(rnd, r) for _ in range(n)]
    if edge_scalars:
        zeros = [i for i in range(n) if ks[i] == 0]
        for t, i in enumerate(zeros):
            ss[i] = 1 if t % 2 == 0 else r - 1
    assert ks[0] == 0 and ks[n - 1] == 0
    return Case(curve, "identities n=%d%s" % (n, " scalars 1, r-1" if edge_scalars else ""), ks, ss)


REDUCE_SHAPES = ("doubling", "top only", "run cancels", "window cancels")


def reduce_collisions(curve, c, shape, top=None, seed=5):
    """5: single-window scalars j in [1, top] (top = 2^(c-1) - 1 unless given; 2^(c-1) is the last positive digit) with the
    logarithms chosen so that the bucket of weight j sums to a_j Q, Q = [q] G; every populated bucket holds two or three
    distinct bases (ZZ != 1 when the reduction reads it).  From the top bucket downward:
      doubling         a = 1, 1, 2, 4, 8, ...: run += B_j doubles at every step
      top only         a populated top bucket over empty ones: wsum += run meets wsum == run
      run cancels      a_j = -(a_(j+1) + ...) at two places: run becomes the identity mid-scan and restarts; the bucket below
                       each of them is P + (-P), an identity that was accumulated
      window cancels   a_1 = -sum_(j >= 2) j a_j: the window's last addition meets wsum == -run"""
    r = order(curve)
    rnd = random.Random(seed + 100 * c + 7 * REDUCE_SHAPES.index(shape))
    T = (1 << (c - 1)) - 1 if top is None else top
    assert 1 <= T <= 1 << (c - 1)
    q = rand_scalar(rnd, r)
    a = {}
    if shape == "doubling":
        for i in range(T):
            a[T - i] = 1 if i == 0 else 1 << (i - 1)
    elif shape == "top only":
        a[T] = 1
    elif shape == "run cancels":
        cancel = {j for j in (2 * T // 3, T // 3) if 1 <= j < T}
        above = 0
        for j in range(T, 0, -1):
            if j in cancel:
                a[j] = -above
            elif j + 1 in cancel:
                a[j] = 0
            else:
                a[j] = rand_scalar(rnd, r)
            above += a[j]
    elif shape == "window cancels":
        for j in range(T, 1, -1):
            a[j] = rand_scalar(rnd, r)
        a[1] = -sum(j * x for j, x in a.items())
    else:
        raise ValueError(shape)
    ks, ss = [], []
    for j, aj in a.items():
        m = 2 + j % 2
        part = [rand_scalar(rnd, r) for _ in range(m - 1)]
        part.append((aj * q - sum(part)) % r)
        assert len(set(part)) == m and 0 not in part
        ks += part
        ss += [j] * m
    perm = list(range(len(ks)))
    rnd.shuffle(perm)
    cs = Case(curve, "reduce: %s c=%d top=%d" % (shape, c, T), [ks[i] for i in perm], [ss[i] for i in perm])
    assert cs.log == q * sum(j * x for j, x in a.items()) % r and (shape != "window cancels" or cs.log == 0)
    return cs


def digit_edge_scalars(curve, c):
    """6: the scalars at which the signed c-bit digits change form"""
    r = order(curve)
    top = r.bit_length() - 1                     # 2^top < r < 2^(top + 1)
    full = top // c                              # whole c-bit digits below 2^top
    out = [1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1, (1 << (2 * c)) - 1,
           sum(1 << (c * w + c - 1) for w in range(full)),        # every digit at the positive maximum 2^(c-1)
           (1 << (c * full)) - 1,                                   # every digit 2^c - 1: the carry ripples into the next window
           (1 << top) - 1,                                          # ... and through a ragged top digit
           r - 1, r - 2, 1 << top]
    assert all(0 < s < r for s in out)
    return out


def digit_edges(curve, c, seed=6):
    r = order(curve)
    rnd = random.Random(seed + 100 * c)
    ss = digit_edge_scalars(curve, c)
    return Case(curve, "digit edges c=%d" % c, [rand_scalar(rnd, r) for _ in ss], ss)


# ---------------------------------------------------------------- running a case
def assert_point(zk, cs, jac, what):
    got = affine_of(zk, cs.curve, jac)
    assert (got == cs.exp).all(), (cs.curve, cs.name, what)
    assert not cs.exp.any() or orc.on_curve(cs.curve, got), (cs.curve, cs.name, what, "off the curve")


def check(zk, cs, configs):
    """the case under every configuration (keyword arguments of zk.msm) over one upload of its bases"""
    bases = zk.Bases(cs.curve, cs.pts)
    try:
        for opts in configs:
            assert_point(zk, cs, zk.msm(bases, cs.sc, **opts), opts)
    finally:
        bases.free()


# ---------------------------------------------------------------- configurations
N_SMALL = 96          # more than one wave of lanes; every bucket of family 1 / 2 holds all of them
TRIPLES = 60


def default_families(curve, c):
    return [case(all_equal, curve, N_SMALL), case(alternating, curve, N_SMALL, False), case(alternating, curve, N_SMALL, True),
            case(zero_sum_triples, curve, TRIPLES, c, False), case(zero_sum_triples, curve, TRIPLES, c, True),
            case(identities, curve, N_SMALL + 3, False), case(identities, curve, N_SMALL + 3, True)]


def check_default_path(zk, curve, c):
    """families 1 - 4 through the default pipeline at window width c"""
    for cs in default_families(curve, c):
        check(zk, cs, [dict(window_bits=c)])


def check_digit_edges(zk, curve, c, singles=True):
    """family 6: canonical scalars at width c, Montgomery scalars at width c and through halo2.best_multiexp; `singles`: every
    edge scalar again as an MSM of its own"""
    sf = pyref.CURVES[curve][1]
    cs = case(digit_edges, curve, c)
    check(zk, cs, [dict(window_bits=c)])
    mont = orc.to_mont(sf, cs.sc)
    bases = zk.Bases(curve, cs.pts)
    try:
        assert_point(zk, cs, zk.msm(bases, mont, montgomery=True, window_bits=c), "montgomery")
        assert_point(zk, cs, zk.halo2.best_multiexp(mont, bases), "best_multiexp")
    finally:
        bases.free()
    # every edge scalar alone: a wrong digit cannot hide behind another term
    for i in range(cs.n if singles else 0):
        one = case(_single_edge, curve, c, i)
        check(zk, one, [dict(window_bits=c)])


def _single_edge(curve, c, i):
    full = case(digit_edges, curve, c)
    return Case(curve, "digit edge c=%d #%d" % (c, i), [full.ks[i]], [full.ss[i]])


def slice_lengths(c):
    return sorted({1, 2, 3, 8, 1 << (c - 1)})


def reduce_cases(curve, c, tops=True):
    """the four shapes below 2^(c-1), and (`tops`) the first two again with the last positive digit 2^(c-1) as the top bucket"""
    if c == 2:         # two buckets
        return [case(reduce_collisions, curve, c, s, 2) for s in REDUCE_SHAPES] + [case(reduce_collisions, curve, c, "window cancels", 1)]
    return [case(reduce_collisions, curve, c, s, None) for s in REDUCE_SHAPES] + \
           ([case(reduce_collisions, curve, c, s, 1 << (c - 1)) for s in REDUCE_SHAPES[:2]] if tops else [])


def check_reduce_collisions(zk, curve, c, limb_bits=0, slices=None, tops=True):
    """family 5 through the row / column reduction and through the slice kernel (one add site, one doubling site) at every
    slice length: 1 (run = one bucket, the multiplier phase sees acc == Y and run = identity), 2, 3 (no power of two), 8,
    2^(c-1) (one slice: the properties above hold over the whole window)"""
    for cs in reduce_cases(curve, c, tops):
        configs = [dict(window_bits=c, limb_bits=limb_bits)]
        configs += [dict(window_bits=c, limb_bits=limb_bits, slice_reduce=True, slice_len=L) for L in (slices or slice_lengths(c))]
        check(zk, cs, configs)


BIG = dict(window_bits=4, big_threshold=100)


def check_oversized_buckets(zk, curve, n=600):
    """families 1 and 2, every bucket far over big_threshold: segments of one point (every tree level, every combine step a
    doubling with ZZ != 1) and of +mP / -mP by lane parity (the tree cancels and goes on adding identities)"""
    for cs in (case(all_equal, curve, n), case(alternating, curve, n, False), case(alternating, curve, n, True)):
        check(zk, cs, [BIG])


def check_oversized_ragged(zk, curve, n=5200):
    """n above one segment with a ragged remainder: msm_combine_big_kernel adds equal segment sums (and a short last one)"""
    check(zk, case(all_equal, curve, n), [BIG, dict(window_bits=4)])
    check(zk, case(alternating, curve, n, True), [BIG])


def check_bucket_splitting(zk, curve, c=4, splits=(1, 2, 4)):
    """2, 4 and 16 pieces per bucket (big_threshold out of reach: the split path takes every bucket), families 1 - 3"""
    configs = [dict(window_bits=c, split_log=k, big_threshold=1 << 30) for k in splits]
    for cs in (case(all_equal, curve, N_SMALL), case(alternating, curve, N_SMALL, False), case(alternating, curve, N_SMALL, True),
               case(zero_sum_triples, curve, TRIPLES, c, False), case(zero_sum_triples, curve, TRIPLES, c, True)):
        check(zk, cs, configs)
        assert zk.msm_last_profile()["limb_bits"] == 29


def check_saturated_limbs(zk, curve, c=4, slices=None, tops=True, paths=3):
    """limb_bits = 32: the zk_curve.h twins of the same branches, families 1, 2, 3 and 5; the first `paths` of the default path,
    oversized buckets and bucket splitting"""
    configs = [dict(window_bits=c, limb_bits=32), dict(window_bits=c, limb_bits=32, big_threshold=20),
               dict(window_bits=c, limb_bits=32, split_log=1, big_threshold=1 << 30)][:paths]
    for cs in (case(all_equal, curve, N_SMALL), case(alternating, curve, N_SMALL, False), case(alternating, curve, N_SMALL, True),
               case(zero_sum_triples, curve, TRIPLES, c, False), case(zero_sum_triples, curve, TRIPLES, c, True)):
        check(zk, cs, configs)
        assert zk.msm_last_profile()["limb_bits"] == 32
    check_reduce_collisions(zk, curve, c, limb_bits=32, slices=slices, tops=tops)


def check_precomputed_table(zk, curve, c=7, n=256, also_default=True):
    """the table rows [2^(c w)] P_i in one bucket set: families 1, 2 and 4 (an identity base stays the identity in every row;
    [2^(c w)] P of window w meets the copies of other windows in one bucket)"""
    for cs in (case(all_equal, curve, n), case(alternating, curve, n, False), case(alternating, curve, n - 2, True),
               case(identities, curve, n, False), case(identities, curve, n, True)):
        if cs.n != n:          # the table tiles into whole scalar blocks
            cs = case(padded_alternating, curve, n)
        bases = zk.Bases(curve, cs.pts)
        try:
            bases.precompute(c)
            assert_point(zk, cs, zk.msm(bases, to_device(zk, cs.sc), window_bits=c, precomputed=True), "precomputed")
            if also_default:
                assert_point(zk, cs, zk.msm(bases, to_device(zk, cs.sc), window_bits=c), "same handle, default form")
        finally:
            bases.free()


def padded_alternating(curve, n):
    """family 2 with one more P, filled up to n with an identity base under the scalar r - 2"""
    cs = case(alternating, curve, n - 2, True)
    return Case(curve, cs.name + " padded", cs.ks + [0] * (n - cs.n), cs.ss + [order(curve) - 2] * (n - cs.n))


def batch_case(curve, c, which):
    """one bases vector [family 1 | family 2 | family 3]; vector v of the batch has its family's scalars and zeros elsewhere.
    which = 0: family 2 sums to the identity (a whole vector whose result is the identity), family 3 to a point; 1: the reverse"""
    parts = [case(all_equal, curve, N_SMALL), case(alternating, curve, N_SMALL, which == 1), case(zero_sum_triples, curve, TRIPLES, c, which == 0)]
    ks = sum((p.ks for p in parts), [])
    out, at = [], 0
    for p in parts:
        ss = [0] * len(ks)
        ss[at:at + p.n] = p.ss
        at += p.n
        out.append(Case(curve, "batch: " + p.name, ks, ss))
        assert out[-1].log == p.log
    return out


def check_batch(zk, curve, c=4):
    """msm_batch, count = 3, twice: one vector each of families 1, 2 and 3 over the same bases"""
    for which in (0, 1):
        vec = case(batch_case, curve, c, which)
        assert len(vec) == 3 and sum(1 for v in vec if v.log == 0) == 1
        bases = zk.Bases(curve, vec[0].pts)
        try:
            got = zk.msm_batch(bases, to_device(zk, np.stack([v.sc for v in vec])), window_bits=c)
            for i, v in enumerate(vec):
                assert_point(zk, v, got[i], "batch %d vector %d" % (which, i))
        finally:
            bases.free()


def check_window_shares(zk, curve, c=4):
    """the two halves of the windows added with zk.point_add: related multiples of one point (family 1), one or both shares the
    identity (family 2)"""
    nl = zk.base_limbs(curve)
    # (case, the lower share is the identity, the upper share is the identity): Z = 0
    for cs, lo_inf, hi_inf in ((case(all_equal, curve, N_SMALL), False, False), (case(alternating, curve, N_SMALL, False), True, True),
                               (case(alternating, curve, N_SMALL, True), False, False), (case(_low_half, curve, c), False, True)):
        W = zk.msm_window_count(curve, cs.n, c)
        bases = zk.Bases(curve, cs.pts)
        try:
            lo = zk.msm(bases, cs.sc, window_bits=c, windows=(0, W // 2))
            hi = zk.msm(bases, cs.sc, window_bits=c, windows=(W // 2, W))
        finally:
            bases.free()
        assert lo[2 * nl:].any() != lo_inf and hi[2 * nl:].any() != hi_inf, (curve, cs.name, "which shares are the identity")
        assert_point(zk, cs, zk.point_add(curve, lo, hi), "shares")
        assert_point(zk, cs, zk.point_add(curve, hi, lo), "shares, swapped")


def _low_half(curve, c):
    """one point under a scalar below 2^(c - 1): every window above the first is empty, the upper share is the identity"""
    r = order(curve)
    rnd = random.Random(77)
    return Case(curve, "low half", [rand_scalar(rnd, r)] * 5, [(1 << (c - 1)) - 1] * 5)


def check_device_partials(zk, curve, c=4, widths=(4, 7)):
    """families 1 and 2 with the per-window partial sums converted on the device: the two conversions agree (reserved == 0)"""
    for cs in (case(all_equal, curve, N_SMALL), case(alternating, curve, N_SMALL, False), case(alternating, curve, N_SMALL, True)):
        bases = zk.Bases(curve, cs.pts)
        try:
            for wb in widths:
                jac = zk.msm(bases, cs.sc, window_bits=wb, device_partials=True)
                prof = zk.msm_last_profile()
                assert prof["reserved"] == 0, (curve, cs.name, wb, "device / host conversions differ: %#x" % prof["reserved"])
                assert_point(zk, cs, jac, "device partials")
        finally:
            bases.free()


def check_deferred(zk, curve, c=4):
    """family 3 through zk_msm_submit / zk_msm_collect"""
    for extra in (False, True):
        cs = case(zero_sum_triples, curve, TRIPLES, c, extra)
        bases = zk.Bases(curve, cs.pts)
        try:
            t = zk.msm_submit(bases, to_device(zk, cs.sc), window_bits=c)
            assert_point(zk, cs, t.collect(), "deferred")
        finally:
            bases.free()


# ---------------------------------------------------------------- halo2's generator fold and the batched normalisation
def mont_limbs(field, x):
    return orc.int_to_limbs(pyref.mont(field, x % pyref.FIELDS[field][0]), 4)


def fold_inputs(curve, half, seed=8):
    """-> [(name, k_lo, k_hi, u)]: g_hi == g_lo under u = 1 (every lane doubles), r - 1 (every output the identity: a batch of
    identities only), 0 and a random u; g_hi == -g_lo under 1; identities in either half and in both; outputs that are the
    identity in whole, alternate and no lane groups of the normalisation (8 points per inversion) and at the last index"""
    r = order(curve)
    rnd = random.Random(seed + half)
    k = [rand_scalar(rnd, r) for _ in range(half)]
    k2 = [rand_scalar(rnd, r) for _ in range(half)]
    u = rand_scalar(rnd, r)
    out = [("equal halves u=1", k, k, 1), ("equal halves u=r-1", k, k, r - 1), ("equal halves u=0", k, k, 0), ("equal halves u random", k, k, u),
           ("opposite halves u=1", k, [r - x for x in k], 1)]
    lo = [0 if i % 3 == 0 else k[i] for i in range(half)]
    hi = [0 if (i % 3 == 1 or i % 7 == 0) else k2[i] for i in range(half)]
    out.append(("identities in either half", lo, hi, u))
    uinv = pow(u, -1, r)

    def cancels(i):          # lane group i // 8: 0 whole, 1 none, 2 alternate, 3 whole, ... and the last index
        g = i // 8
        return i == half - 1 or g % 4 in (0, 3) or (g % 4 == 2 and i % 2 == 0)
    hi = [(-k[i] * uinv) % r if cancels(i) else k2[i] for i in range(half)]
    out.append(("identity outputs by lane group", k, hi, u))
    return out


def check_ipa_fold(zk, curve, half):
    """halo2.ipa_fold_bases: g[i] <- affine(g[i] + [u] g[i + half]) == [k_lo + u k_hi] G at every index; the upper half stays"""
    sf = pyref.CURVES[curve][1]
    r = order(curve)
    for name, k_lo, k_hi, u in fold_inputs(curve, half):
        src = points_of_logs(curve, list(k_lo) + list(k_hi))
        exp = points_of_logs(curve, [(a + u * b) % r for a, b in zip(k_lo, k_hi)])
        if name in ("equal halves u=r-1", "opposite halves u=1"):
            assert not exp.any()
        g = to_device(zk, src)
        zk.halo2.ipa_fold_bases(curve, g, half, mont_limbs(sf, u))
        got = to_host(zk, g)
        bad = np.nonzero((got[:half] != exp).any(axis=1))[0]
        assert not len(bad), (curve, half, name, bad[:8])
        assert (got[half:] == src[half:]).all(), (curve, half, name, "the upper half was written")
