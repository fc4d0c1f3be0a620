"""TEST INFRASTRUCTURE shared by tests/test_ntt_options_emu.py (CPU tier, emulator build) and tests/test_ntt_options_gpu.py
(-m gpu): the switches of the NTT launch sequence (ntt_run in csrc/zk_ntt.inl) against each other -- the pass plan, lazy or
saturated limbs, the fused g_pre / g_post shifts, zero extension (log_in), the n^-1 scaling, ZK_NTT_OUT_R29,
ZK_NTT_OUT_SUBCOSETS(lp), in place or out of place -- at log n = 0 .. 12, and (GPU tier) the default plan at sizes no other
test runs it at, checked in closed form on a geometric input.

Reference: Python integers only (no oracle.zk_oracle).  `expected` pads the 2^log_in input integers with zeros, multiplies
element i by g_pre^i, applies a recursive radix-2 DFT, multiplies by n^-1 (flag bit 0), by g_post^k, by 2^5 = R'/R
(ZK_NTT_OUT_R29; include/zkcp_amd.h: R' = 2^261) and stores result k at (k mod P)(n / P) + k / P, P = 2^lp.  Every comparison
is word for word on the canonical Montgomery words.  The recursive DFT is pinned against pyref.dft_naive (n <= 64) and
`expected` as a whole against the defining sum (n = 8) by check_reference."""
import itertools
from collections import namedtuple

import numpy as np

from oracle import pyref
from parity_suite import NTT_FIELDS as FIELDS, to_device, to_host

OUT_R29 = 2                  # ZK_NTT_OUT_R29
R29_FACTOR = 1 << 5          # R' / R = 2^261 / 2^256


def out_subcosets(lp):       # ZK_NTT_OUT_SUBCOSETS(lp)
    return (lp & 15) << 4


def modulus(field):
    return pyref.FIELDS[field][0]


# ---------------------------------------------------------------- reference
def dft(p, a, w):
    """sum_j a[j] w^(j k) for every k, by the recursive radix-2 split (w: a primitive len(a)-th root of unity)"""
    n = len(a)
    if n == 1:
        return [a[0] % p]
    w2 = w * w % p
    ev, od = dft(p, a[0::2], w2), dft(p, a[1::2], w2)
    h = n // 2
    out = [0] * n
    t = 1
    for k in range(h):
        x = od[k] * t % p
        out[k] = (ev[k] + x) % p
        out[k + h] = (ev[k] - x) % p
        t = t * w % p
    return out


def out_index(n, lp, k):
    """where result k lands under ZK_NTT_OUT_SUBCOSETS(lp)"""
    parts = 1 << lp
    return (k % parts) * (n // parts) + k // parts


def expected(field, a, n, omega, g_pre, g_post, flags):
    """the n output integers (times 2^5 under ZK_NTT_OUT_R29: the Montgomery words of x 2^5 are x R') at their stored places;
    a: the 2^log_in input integers; g_pre / g_post: an integer or None"""
    p = modulus(field)
    assert n >= len(a) >= 1 and n & (n - 1) == 0 and not flags & ~0xf3
    x = [v % p for v in a] + [0] * (n - len(a))
    if g_pre is not None:
        t = 1
        for i in range(len(a)):
            x[i] = x[i] * t % p
            t = t * g_pre % p
    y = dft(p, x, omega)
    s = pow(n, -1, p) if flags & 1 else 1
    if flags & OUT_R29:
        s = s * R29_FACTOR % p
    lp = (flags >> 4) & 15
    assert (1 << lp) <= n
    out = [0] * n
    t = 1
    for k in range(n):
        out[out_index(n, lp, k)] = y[k] * s % p * t % p
        if g_post is not None:
            t = t * g_post % p
    return out


def check_reference():
    """the reference itself: the recursive DFT against the O(n^2) sum of pyref.dft_naive at every n <= 64 on every field, and
    `expected` with every option on against the defining sum at n = 8, log_in = 2, lp = 1"""
    rng = pyref.Rng(0xD0F7)
    for field in FIELDS:
        p = modulus(field)
        for logn in range(7):
            w = pyref.root_of_unity(field, logn)
            a = [rng.below(p) for _ in range(1 << logn)]
            assert dft(p, a, w) == pyref.dft_naive(field, a, w), (field, logn)
        n, m, lp = 8, 4, 1
        w, gp, gq = pyref.root_of_unity(field, 3), 1 + rng.below(p - 1), 1 + rng.below(p - 1)
        a = [rng.below(p) for _ in range(m)]
        got = expected(field, a, n, w, gp, gq, 1 | OUT_R29 | out_subcosets(lp))
        for k in range(n):
            v = sum(a[j] * pow(gp, j, p) * pow(w, j * k, p) for j in range(m)) * pow(n, -1, p) * pow(gq, k, p) * 32 % p
            assert got[(k % 2) * 4 + k // 2] == v, (field, k)
        assert expected(field, a, n, w, None, None, 0) == pyref.dft_naive(field, a + [0] * 4, w)


def mont_rows(field, xs):
    """integers -> their Montgomery words (R = 2^256), uint64 [len, 4]"""
    p = modulus(field)
    assert pyref.FIELDS[field][2] == 4
    return np.frombuffer(b"".join((x % p * (1 << 256) % p).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def ints_of_rows(field, rows):
    """Montgomery words -> integers; every row must be canonical (< p)"""
    p = modulus(field)
    rinv = pow(1 << 256, -1, p)
    raw = np.ascontiguousarray(rows, dtype=np.uint64).tobytes()
    words = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    assert all(v < p for v in words), (field, "a result is not canonical")
    return [v * rinv % p for v in words]


def garbage(rows):
    """what a correct run never reads (the padding of a zero-extended input) or overwrites in full (dst): no field element"""
    return np.full((rows, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


# ---------------------------------------------------------------- plans (keyword arguments of zk.ntt_configure)
PLANS = {
    "default": dict(),
    "radix3": dict(max_log_radix=3),
    "radix2": dict(max_log_radix=2),                      # four passes at log n = 7, 8
    "radix5_tile0": dict(max_log_radix=5, log_tile=0),
    "radix7_tile3": dict(max_log_radix=7, log_tile=3),
    "radix4_tile4": dict(max_log_radix=4, log_tile=4),
    "saturated": dict(limb_bits=32),
    "saturated_radix3": dict(limb_bits=32, max_log_radix=3),
    "block64": dict(block=64),
    "block1024": dict(block=1024),
}
MAX_LOGN = 12
RANGES = [(0, 4), (5, 8), (9, 12)]           # every pair of option values occurs within each of these ranges of log n
FULL_PRODUCT_MAX = 4


def plan_of(logn, max_log_radix=0, log_tile=None, block=0, limb_bits=0):
    """ntt_plan and the launch shape of ntt_run restated: [(log_r, log_t, tiles, lanes per tile)] pass by pass"""
    max_r = max_log_radix if 1 <= max_log_radix <= 10 else 10
    nd = max(1, -(-logn // max_r))
    rd, rem = [], logn
    for i in range(nd):
        rd.append(-(-rem // (nd - i)))
        rem -= rd[-1]
    out, log_m = [], 0
    for i, r in enumerate(rd):
        lt = min(2 if log_tile is None else log_tile, 11 - r)
        lt = min(lt, logn - log_m - r) if i < nd - 1 else (0 if nd == 1 else min(lt, rd[0]))
        lt = max(lt, 0)
        out.append((r, lt, (1 << logn) >> (r + lt), min(max((1 << (r + lt)) // 2, 64), block or 512)))
        log_m += r
    return out


def passes(plan, logn):
    return len(plan_of(logn, **PLANS[plan]))


def runs(plan, logn):
    """ntt_plan holds at most four passes"""
    return passes(plan, logn) <= 4


def emulator_seconds(plan, logn):
    """what one case costs the CPU tier, roughly: the emulator switches fibers once per lane and barrier (idle lanes of a
    64-lane tile over 16 elements included), every case builds its twiddle and power tables, and the first plan of a field also
    pays for the Python reference, which the later ones share.  The three constants were fitted by hand to timings of the
    emulator on Pallas Fp (a case at log n = 12: 0.05 s on the default plan, 0.15 s on radix3, 0.26 s on radix5_tile0; the
    reference 0.05 s) and are no better than that.  Nothing but the cut of the grid into pytest items depends on them: every
    case runs whatever they say, and a poor fit only makes items uneven."""
    ref = 1.1e-6 * logn * (1 << logn) if plan == next(iter(PLANS)) else 0.0
    return 0.001 + 6e-6 * (1 << logn) + ref + 0.9e-6 * sum(tiles * lanes * (r + 2) for r, _, tiles, lanes in plan_of(logn, **PLANS[plan]))


# ---------------------------------------------------------------- the grid
Case = namedtuple("Case", "logn log_in pre post scale r29 lp oop values seed")
BINARY = ("pre", "post", "scale", "r29", "oop")
FAMILIES = ("random", "edges")


def lp_values(logn):
    return sorted({0, min(1, logn), logn // 2, logn})


def lp_kind(logn, lp):
    """which of the four requested values lp is: several at once at small log n"""
    return {k for k, v in (("0", 0), ("1", min(1, logn)), ("half", logn // 2), ("full", logn)) if v == lp}


def log_ins(logn):
    return [None] + list(range(logn + 1))


def build_grid(seed=0x4E7707):
    """log n <= 4: the full product of the options at every (log n, log_in), the input family alternating; above: four cases
    per (log n, log_in) -- every lp value once, the two-valued options and the family in complementary pairs, so that every
    value of every option occurs in every cell"""
    rng = pyref.Rng(seed)
    out = []
    for logn in range(MAX_LOGN + 1):
        for log_in in log_ins(logn):
            if logn <= FULL_PRODUCT_MAX:
                for i, lp in enumerate(lp_values(logn)):
                    for bits in itertools.product((False, True), repeat=len(BINARY)):
                        # by half the number of options that are on, shifted by the lp index: both families meet both values
                        # of every option (asserted below)
                        family = FAMILIES[(sum(bits) // 2 + i) & 1]
                        out.append(Case(logn, log_in, *bits[:4], lp, bits[4], family, rng.u64() & 0xFFFFFFFF))
                continue
            lps = lp_values(logn)
            assert len(lps) == 4
            for i in range(len(lps) - 1, 0, -1):       # a seeded shuffle
                j = rng.u64() % (i + 1)
                lps[i], lps[j] = lps[j], lps[i]
            for i, lp in enumerate(lps):
                if i % 2 == 0:
                    bits = [bool((rng.u64() >> 17) & 1) for _ in range(len(BINARY) + 1)]
                else:
                    bits = [not b for b in bits]
                out.append(Case(logn, log_in, *bits[:4], lp, bits[4], FAMILIES[bits[5]], rng.u64() & 0xFFFFFFFF))
    return out


def option_values(c):
    """the (option, value) pairs a case covers"""
    out = {(k, getattr(c, k)) for k in BINARY} | {("values", c.values)}
    return out | {("lp", k) for k in lp_kind(c.logn, c.lp)}


def assert_coverage(grid):
    """what the issue asks of the sample, so that thinning it cannot silently drop a value"""
    cells = {}
    for c in grid:
        cells.setdefault((c.logn, c.log_in), []).append(c)
    assert set(cells) == {(logn, li) for logn in range(MAX_LOGN + 1) for li in log_ins(logn)}, "a (log n, log_in) cell is missing"
    every = {(k, v) for k in BINARY for v in (False, True)} | {("values", f) for f in FAMILIES} | {("lp", k) for k in ("0", "1", "half", "full")}
    for (logn, li), cs in cells.items():
        have = {(c.pre, c.post, c.scale, c.r29, c.lp, c.oop) for c in cs}
        if logn <= FULL_PRODUCT_MAX:
            want = {b[:4] + (lp, b[4]) for lp in lp_values(logn) for b in itertools.product((False, True), repeat=5)}
            assert have == want, (logn, li, "not the full product")
        seen = set().union(*(option_values(c) for c in cs))
        missing = every - seen
        assert not missing, (logn, li, "option values that never occur", sorted(map(str, missing)))
    # every pair of values of two different options within each of RANGES (so also within the log n <= 8 that the four-pass
    # plan runs); the ranges have nothing to do with how the grid is cut into pytest items
    for lo, hi in RANGES:
        seen = set()
        for c in grid:
            if lo <= c.logn <= hi:
                seen |= {frozenset(pr) for pr in itertools.combinations(sorted(option_values(c), key=str), 2)}
        want = {frozenset((x, y)) for x in every for y in every if x[0] != y[0]}
        missing = want - seen
        assert not missing, (lo, hi, "pairs of option values that never occur", [sorted(map(str, m)) for m in missing][:8])
    # every plan meets every pass count it can have
    for plan in PLANS:
        assert {passes(plan, c.logn) for c in grid if runs(plan, c.logn)} >= set(range(1, 1 + min(4, passes(plan, MAX_LOGN)))), plan


GRID = build_grid()
assert_coverage(GRID)
ITEM_SECONDS = 4.0


def cut_items(plan):
    """the plan's cases in grid order, cut between (log n, log_in) cells into pytest items of about ITEM_SECONDS on the CPU tier
    by the estimate of emulator_seconds (a cut by ranges of log n leaves log n = 12 alone at 8 - 14 s on the many-pass plans)"""
    items, cost = [[]], 0.0
    for _, cell in itertools.groupby((c for c in GRID if runs(plan, c.logn)), key=lambda c: (c.logn, c.log_in)):
        cell = list(cell)
        if items[-1] and cost + len(cell) * emulator_seconds(plan, cell[0].logn) > ITEM_SECONDS:
            items.append([])
            cost = 0.0
        items[-1] += cell
        cost += len(cell) * emulator_seconds(plan, cell[0].logn)
    return items


PARTS = {plan: cut_items(plan) for plan in PLANS}
assert all(sum(PARTS[plan], []) == [c for c in GRID if runs(plan, c.logn)] for plan in PLANS)
ITEMS = [(field, plan, part) for field in FIELDS for plan in PLANS for part in range(len(PARTS[plan]))]


# ---------------------------------------------------------------- one case
Ref = namedtuple("Ref", "a omega g_pre g_post flags exp")      # numpy Montgomery rows (g_*: a row or None), flags: the int
_refs = {}


def reference(field, logn, log_in, pre, post, scale, r29, lp, values, seed):
    """inputs and expected output of a case; computed once per process and shared by every plan, in place and out of place (the
    cache holds one field at a time)"""
    key = (field, logn, log_in, pre, post, scale, r29, lp, values, seed)
    if key in _refs:
        return _refs[key]
    if _refs and next(iter(_refs))[0] != field:
        _refs.clear()
    p = modulus(field)
    rng = pyref.Rng((seed << 8) ^ 0x5EED)
    n, m = 1 << logn, 1 << (logn if log_in is None else log_in)
    # any primitive 2^logn-th root: the inverse transforms use other roots than root_of_unity itself
    omega = pow(pyref.root_of_unity(field, logn), 2 * rng.below(1 << 20) + 1, p)
    assert logn == 0 or pow(omega, n // 2, p) == p - 1
    if values == "random":
        a = [rng.below(p) for _ in range(m)]
        g_pre, g_post = 1 + rng.below(p - 1), 1 + rng.below(p - 1)
    else:
        assert values == "edges"
        a = [(0, 1, p - 1)[rng.u64() % 3] for _ in range(m)]
        g_pre, g_post = (1, p - 1)[rng.u64() & 1], (1, p - 1)[rng.u64() & 1]
    g_pre, g_post = g_pre if pre else None, g_post if post else None
    flags = (1 if scale else 0) | (OUT_R29 if r29 else 0) | out_subcosets(lp)
    exp = expected(field, a, n, omega, g_pre, g_post, flags)
    row = lambda v: None if v is None else mont_rows(field, [v])[0]
    ref = Ref(mont_rows(field, a), row(omega), row(g_pre), row(g_post), flags, mont_rows(field, exp))
    _refs[key] = ref
    return ref


def run_case(zk, field, plan, logn, log_in, pre, post, scale, r29, lp, oop, values, seed):
    """one call of zk.ntt under one plan.  In place: the buffer's tail beyond 2^log_in is garbage.  Out of place: src holds
    exactly 2^log_in elements and must come back unchanged, dst starts as garbage."""
    args = "run_case(zk, %r, %r, logn=%r, log_in=%r, pre=%r, post=%r, scale=%r, r29=%r, lp=%r, oop=%r, values=%r, seed=%r)" % (
        field, plan, logn, log_in, pre, post, scale, r29, lp, oop, values, seed)
    ref = reference(field, logn, log_in, pre, post, scale, r29, lp, values, seed)
    n, m = 1 << logn, ref.a.shape[0]
    zk.ntt_configure(**PLANS[plan])
    try:
        if oop:
            src, dst = to_device(zk, ref.a), to_device(zk, garbage(n))
            zk.ntt(field, dst, ref.omega, scale_by_n_inv=ref.flags, coset_pre=ref.g_pre, coset_post=ref.g_post, device=True, in_log=log_in, src=src)
            got = to_host(zk, dst)
            assert (to_host(zk, src) == ref.a).all(), "src was written: " + args
        else:
            buf = to_device(zk, np.concatenate([ref.a, garbage(n - m)]))
            got = to_host(zk, zk.ntt(field, buf, ref.omega, scale_by_n_inv=ref.flags, coset_pre=ref.g_pre, coset_post=ref.g_post, device=True, in_log=log_in))
    except AssertionError:
        raise
    except Exception as e:          # a refusal of the library (ZkError) or of the wrapper: with the arguments, like a wrong result
        raise AssertionError("%s: %s: %s" % (type(e).__name__, e, args)) from e
    finally:
        zk.ntt_configure()
    bad = np.nonzero((got != ref.exp).any(axis=1))[0]
    assert not len(bad), "%d of %d outputs differ, the first at %s: %s" % (len(bad), n, bad[:8].tolist(), args)


def check_plan(zk, field, plan, part):
    for c in PARTS[plan][part]:
        run_case(zk, field, plan, *c)


def check_host(zk, field):
    """zk_ntt and zk_coset_mul on host memory (the numpy path of zk.ntt): log n = 0 .. 12 with pre, post and scale on and off"""
    rng = pyref.Rng(0x4057)
    for logn in range(MAX_LOGN + 1):
        for pre, post, scale in itertools.product((False, True), repeat=3):
            values, seed = FAMILIES[rng.u64() & 1], rng.u64() & 0xFFFFFFFF
            ref = reference(field, logn, None, pre, post, scale, False, 0, values, seed)
            got = zk.ntt(field, np.array(ref.a), ref.omega, scale_by_n_inv=scale, coset_pre=ref.g_pre, coset_post=ref.g_post)
            assert (got == ref.exp).all(), (field, logn, pre, post, scale, values, seed)


# ---------------------------------------------------------------- the default plan at large sizes (GPU tier only)
def default_plan(logn):
    """the radix split of the default plan, and the elements of one tile of its last pass"""
    pl = plan_of(logn)
    return tuple(r for r, _, _, _ in pl), 1 << (pl[-1][0] + pl[-1][1])


def sample_positions(n, lp, tile, rng, count=256):
    """output indices k: `count` seeded ones, both ends, every multiple of the last pass's tile and its neighbours within the
    first and the last 4096, and the results stored first and last in every sub-coset"""
    ks = {0, n - 1} | {rng.below(n) for _ in range(count)}
    for edge in (0, max(0, n - 4096)):
        for mult in range(edge - edge % tile, min(n, edge + 4096) + 1, tile):
            ks |= {k for k in (mult - 1, mult, mult + 1) if 0 <= k < n}
    if lp:
        parts, per = 1 << lp, n >> lp
        for j in range(parts):
            for at in (j * per, (j + 1) * per - 1):       # stored place -> result index
                ks.add((at % per) * parts + at // per)
    return sorted(ks)


def _rows_at(zk, buf, idx):
    """rows `idx` of a device buffer; only these are copied back"""
    if isinstance(buf, np.ndarray):
        return buf[np.asarray(idx, dtype=np.int64)]
    import torch
    sel = buf.index_select(0, torch.tensor(idx, dtype=torch.int64, device=buf.device))
    torch.cuda.synchronize()
    return sel.cpu().numpy().view(np.uint64)


def _device_garbage(zk, rows):
    if zk.backend_info().startswith("emu"):
        return garbage(rows)
    import torch
    return torch.full((rows, 4), -1, dtype=torch.int64, device="cuda")


def check_geometric(zk, field, logn, log_in, pre, post, scale, r29, lp, oop, seed):
    """a_j = c^j (j < m = 2^log_in), built on the device: with q = c g_pre omega^k the result is
    out[k] = s g_post^k sum_j q^j, checked as  out[k] (q - 1) == s g_post^k (q^m - 1)  at sampled k"""
    args = (field, logn, log_in, pre, post, scale, r29, lp, oop, seed)
    p = modulus(field)
    rng = pyref.Rng(seed)
    n, m = 1 << logn, 1 << log_in
    omega = pow(pyref.root_of_unity(field, logn), 2 * rng.below(1 << 20) + 1, p)
    g_pre = 1 + rng.below(p - 1) if pre else None
    g_post = 1 + rng.below(p - 1) if post else None
    rd, tile = default_plan(logn)
    ks = sample_positions(n, lp, tile, rng)
    while True:                                # c with q != 1 at every sampled k
        c = 2 + rng.below(p - 2)
        qs = [c * (g_pre or 1) % p * pow(omega, k, p) % p for k in ks]
        if 1 not in qs:
            break
    row = lambda v: None if v is None else mont_rows(field, [v])[0]
    src = _device_garbage(zk, m if oop else n)
    zk.halo2.vec_powers(field, src[:m], row(c))
    js = sorted({0, 1, m - 1} | {rng.below(m) for _ in range(64)})
    assert ints_of_rows(field, _rows_at(zk, src, js)) == [pow(c, j, p) for j in js], ("vec_powers", args)
    flags = (1 if scale else 0) | (OUT_R29 if r29 else 0) | out_subcosets(lp)
    if oop:
        dst = _device_garbage(zk, n)
        zk.ntt(field, dst, row(omega), scale_by_n_inv=flags, coset_pre=row(g_pre), coset_post=row(g_post), device=True, in_log=log_in, src=src)
        assert ints_of_rows(field, _rows_at(zk, src, js)) == [pow(c, j, p) for j in js], ("src was written", args)
    else:
        dst = zk.ntt(field, src, row(omega), scale_by_n_inv=flags, coset_pre=row(g_pre), coset_post=row(g_post), device=True, in_log=log_in)
    got = ints_of_rows(field, _rows_at(zk, dst, [out_index(n, lp, k) for k in ks]))
    s = (pow(n, -1, p) if scale else 1) * (R29_FACTOR if r29 else 1) % p
    bad = [k for k, q, v in zip(ks, qs, got) if v * (q - 1) % p != s * pow(g_post or 1, k, p) * (pow(q, m, p) - 1) % p]
    assert not bad, ("%d of %d sampled outputs differ" % (len(bad), len(ks)), bad[:8], rd, args)


def check_random_large(zk, field, logn, seed, samples=32):
    """random coefficients under g_pre: out[k] = A(g_pre omega^k) by Horner at sampled k"""
    p = modulus(field)
    rng = pyref.Rng(seed)
    n = 1 << logn
    omega = pyref.root_of_unity(field, logn)
    g_pre = 1 + rng.below(p - 1)
    a = [rng.below(p) for _ in range(n)]
    row = lambda v: mont_rows(field, [v])[0]
    buf = zk.ntt(field, to_device(zk, mont_rows(field, a)), row(omega), coset_pre=row(g_pre), device=True)
    ks = sorted({0, n - 1} | {rng.below(n) for _ in range(samples - 2)})
    got = ints_of_rows(field, _rows_at(zk, buf, ks))
    for k, v in zip(ks, got):
        x, acc = g_pre * pow(omega, k, p) % p, 0
        for coeff in reversed(a):
            acc = (acc * x + coeff) % p
        assert v == acc, (field, logn, seed, k)


LARGE_LOGNS = (12, 15, 17, 19, 21, 23, 24)
LARGE_SPLITS = {12: (6, 6), 15: (8, 7), 17: (9, 8), 19: (10, 9), 21: (7, 7, 7), 23: (8, 8, 7), 24: (8, 8, 8)}


def large_cases():
    """(field, logn, log_in, pre, post, scale, r29, lp, oop, seed): log_in = log n, log n - 1, log n - 3 at every size, the fields
    and the options rotating; every option is on and off at every size"""
    out = []
    for i, logn in enumerate(LARGE_LOGNS):
        assert default_plan(logn)[0] == LARGE_SPLITS[logn]
        field = FIELDS[i % len(FIELDS)]
        combos = [dict(pre=True, post=True, scale=True, r29=False, lp=0, oop=False),
                  dict(pre=True, post=False, scale=False, r29=True, lp=(1, 3, 4)[i % 3], oop=True),         # halo2's combination
                  dict(pre=False, post=True, scale=True, r29=True, lp=logn // 2 if i % 2 else 2, oop=True),
                  dict(pre=False, post=False, scale=False, r29=False, lp=1, oop=False)]
        mine = []
        for j, log_in in enumerate((logn, logn - 1, logn - 3)):
            o = combos[(i + j) % 4]
            mine.append((field, logn, log_in, o["pre"], o["post"], o["scale"], o["r29"], o["lp"], o["oop"], 0x1A46E + 16 * logn + j))
        assert all({bool(c[k]) for c in mine} == {False, True} for k in (3, 4, 5, 6, 8))
        out += mine
    return out
