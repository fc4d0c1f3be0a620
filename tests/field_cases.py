"""Case tables for the field and curve primitives, checked against Python integers.  One module for the CPU tier
(tests/test_f29.py, tests/test_field_ops.py: the g++ runner tests/emu/f29_check) and the GPU tier
(tests/test_field_probe_gpu.py: the gfx950 probe tests/emu/libzk_field_probe.so); both execute the op table of
tests/emu/field_ops.h.

A case is (target, op, a, b, check): the words of the two operand rows and a function that asserts on the result words.
Every check is exact: canonical outputs equal the Python integer word for word, lazy outputs satisfy the value congruence
and the limb / value bounds of the bound discipline (zk_field29.h).  tables(target) returns {family: [cases]} and asserts
that every op the dispatch header declares for the target is exercised."""
import functools
import os
import random
import subprocess

from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
EXE = os.path.join(EMU, "f29_check")
FIELDS = list(pyref.FIELD_IDS)
FQ2_FIELDS = ["Bn254Fq", "Bls381Fq"]
CURVES = list(pyref.CURVE_IDS)
CURVE_TARGETS = [c + s for c in CURVES for s in ("", "29")]
# W, L, 32-bit words: zk_params29.h (Bn254Fr and Bls381Fr are 254/255-bit fields in 9 x 29 bits like the Pasta fields)
SHAPE = {"PallasFp": (29, 9, 8), "PallasFq": (29, 9, 8), "Bn254Fr": (29, 9, 8), "Bls381Fr": (29, 9, 8),
         "Bn254Fq": (29, 9, 8), "Bls381Fq": (28, 14, 12)}
W = L = MASK = NW = None


def shape(field):
    global W, L, MASK, NW
    W, L, NW = SHAPE[field]
    MASK = (1 << W) - 1


def build():
    src = os.path.join(EMU, "f29_check.cc")
    csrc = os.path.join(ROOT, "contangle-zkcp_amd", "csrc")
    deps = [src, os.path.join(EMU, "field_ops.h")] + \
        [os.path.join(csrc, f) for f in ("zk_field29.h", "zk_curve29.h", "zk_curve.h", "zk_params29.h", "zk_params.h", "zk_field.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + csrc, "-I" + EMU, src, "-o", EXE])


def val(limbs):
    return sum(x << (W * i) for i, x in enumerate(limbs))


def limbs_of(x, strict_top=False):
    out = [(x >> (W * i)) & MASK for i in range(L - 1)]
    out.append(x >> (W * (L - 1)))
    return out


def spread_random(rng, x, lb):
    """random lazy representation of integer x with limbs below the top in [0, lb]"""
    out = limbs_of(x)
    for i in range(L - 1):
        # move a multiple of 2^W from limb i+1 into limb i when possible
        room = (lb - out[i]) >> W
        take = min(room, out[i + 1])
        if take > 0:
            t = rng.randint(0, take)
            out[i] += t << W
            out[i + 1] -= t
    assert val(out) == x and all(0 <= v < 1 << 32 for v in out)
    return out


def words_of(x, n):
    assert 0 <= x < 1 << (32 * n)
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def wval(ws):
    return sum(w << (32 * i) for i, w in enumerate(ws))


def run(lines):
    """(target, op, a, b[, check]) lines through the host runner; returns the result words of every line"""
    build()
    inp = "\n".join("%s %s %s %s" % (l[0], l[1], " ".join(map(str, l[2])), " ".join(map(str, l[3]))) for l in lines) + "\n"
    out = subprocess.run([EXE], input=inp, stdout=subprocess.PIPE, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(lines), out[-1]
    return [list(map(int, l.split())) for l in out]


def check(cases, results):
    assert len(cases) == len(results)
    for i, (c, r) in enumerate(zip(cases, results)):
        try:
            c[4](r)
        except AssertionError as e:
            raise AssertionError("%s %s case %d: a=%s b=%s got=%s %s" % (c[0], c[1], i, list(map(hex, c[2])), list(map(hex, c[3])),
                                                                          list(map(hex, r)), e)) from None


@functools.lru_cache(None)
def op_table():
    """{(target, op): (target id, op id, na, nb, no)} as the dispatch header declares it (f29_check --list)"""
    build()
    t = {}
    for l in subprocess.run([EXE, "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.strip().split("\n"):
        tn, ti, on, oi, na, nb, no = l.split()
        t[(tn, on)] = (int(ti), int(oi), int(na), int(nb), int(no))
    return t


def eq(exp):
    exp = list(exp)

    def chk(r):
        assert r == exp, "expected %s" % list(map(hex, exp))
    return chk


# ---------------------------------------------------------------------------------------------------------------------
# lazy-limb checks (the assertions of tests/test_f29.py)
# ---------------------------------------------------------------------------------------------------------------------
def mont29_exact(p, x, y=1, extra=0):
    """the integer fe29_mul / fe29_mulacc returns: (x y + extra + m p) / R' with m = -(x y + extra) / p mod R'"""
    Rp = 1 << (W * L)
    t = x * y + extra
    m = (-t * pow(p, -1, Rp)) % Rp
    assert (t + m * p) % Rp == 0
    return (t + m * p) // Rp


def check_mul(field, a, b):
    p = pyref.FIELDS[field][0]
    W_, L_ = SHAPE[field][:2]
    mask, Rp = (1 << W_) - 1, 1 << (W_ * L_)

    def v(l):
        return sum(x << (W_ * i) for i, x in enumerate(l))

    def chk(r):
        assert all(x <= mask for x in r[:L_ - 1])                              # strict limbs
        assert v(r) * Rp % p == v(a) * v(b) % p                                # Montgomery relation
        assert v(r) < v(a) * v(b) // Rp + p + 1                                # value bound
    return chk


def mul_extremes(field):
    shape(field)
    p = pyref.FIELDS[field][0]
    top = p >> (W * (L - 1))
    rng = random.Random(29)
    cases = []
    nplus = MASK + (1 << (32 - W)) - 1
    wide = MASK + 1 + 2 * (MASK + 1) + nplus                 # q - x3 + BIAS16K2: the widest form a product ever sees
    max_n = [nplus] * (L - 1)                # N+ limbs at their maximum
    max_s = [wide] * (L - 1)
    for k in range(200):
        if k == 0:
            a, b = max_n + [18 * top], max_s + [17 * top]
        elif k == 1:
            a, b = [2 * nplus] * (L - 1) + [16 * top], [2 * nplus] * (L - 1) + [16 * top]   # u = 2y squared in dbl
        elif k == 2:
            a, b = [0] * L, max_s + [1]
        elif k < 100:
            a = spread_random(rng, rng.randrange(18 * p), nplus)
            b = spread_random(rng, rng.randrange(17 * p), wide)
        else:
            a, b = limbs_of(rng.randrange(2 * p)), limbs_of(rng.randrange(2 * p))
        cases.append((field, "mul", a, b, check_mul(field, a, b)))
    # the NTT butterfly's product (zk_ntt29_kernels.h): t = mont29(w, tw) with the tile value w at LB(w) < 2^31.6,
    # VB(w) <= 128 after three stages of limb growth (2^29 + 3 * 2^29.72 per limb, 2 + 4 * 10 = 42 p deep in a tile, 128 p
    # allowed) against a strict twiddle < 2p -- the operands Bn254Fr / Bls381Fr (and the Pasta fields) meet in the transforms
    lb_ntt = (1 << 29) + 3 * int(2 ** 29.72)
    if W == 29:
        assert lb_ntt < 2 ** 31.6
        for k in range(60):
            if k == 0:
                a, b = [lb_ntt] * (L - 1) + [127 * top], [MASK] * (L - 1) + [2 * top - 1]
            else:
                a, b = spread_random(rng, rng.randrange(128 * p), lb_ntt), limbs_of(rng.randrange(2 * p))
            cases.append((field, "mul", a, b, check_mul(field, a, b)))
    return cases


def sub_cases(field):
    shape(field)
    p = pyref.FIELDS[field][0]
    rng = random.Random(7)
    nplus = MASK + (1 << (32 - W)) - 1
    cases = []

    def chk_val(e):
        W_ = W

        def chk(r):
            assert sum(x << (W_ * i) for i, x in enumerate(r)) == e and all(0 <= x < 1 << 32 for x in r)
        return chk
    for k in range(100):
        a = spread_random(rng, rng.randrange(2 * p), MASK)
        b12 = spread_random(rng, rng.randrange(12 * p), nplus)
        b2 = limbs_of(rng.randrange(2 * p))
        if k == 0:
            a, b12 = [0] * L, limbs_of(12 * p - 1)
        cases.append((field, "sub16k2", a, b12, chk_val(val(a) - val(b12) + 16 * p)))
        cases.append((field, "sub4k1", a, b2, chk_val(val(a) - val(b2) + 4 * p)))
        cases.append((field, "sub3", a, b2, chk_val(val(a) - 3 * val(b2) + 8 * p)))
        cases.append((field, "sub2x", a, b2, chk_val(val(a) - 2 * val(b2) + 4 * p)))
    return cases


def check_ncc(field, op, x):
    """norm / carry / canon of a lazy representation of the integer x"""
    p = pyref.FIELDS[field][0]
    W_, L_ = SHAPE[field][:2]
    mask = (1 << W_) - 1

    def chk(r):
        v = sum(t << (W_ * i) for i, t in enumerate(r))
        if op == "norm":
            assert v == x and all(t <= mask + (1 << (32 - W_)) - 1 for t in r[:L_ - 1])
        elif op == "carry":
            assert v == x and all(t <= mask for t in r[:L_ - 1])
        else:
            assert v == x % p and all(t <= mask for t in r[:L_ - 1])
    return chk


def carry_safe_lb():
    return (1 << 32) - 1 - (((1 << (32 - W)) - 1) << W)       # carry-in must not wrap a word


def norm_carry_canon_cases(field):
    shape(field)
    p = pyref.FIELDS[field][0]
    rng = random.Random(7 + 1000)
    cases = []
    for k in range(100):
        x = rng.randrange(19 * p)
        lazy = spread_random(rng, x, carry_safe_lb()) if k else [0xFFFFFFF0] * (L - 1) + [1]
        x = val(lazy)
        if x >= 20 * p:
            continue
        for op in ("norm", "carry", "canon"):
            cases.append((field, op, lazy, [0] * L, check_ncc(field, op, x)))
    return cases


def check_fromstd(field, x):
    """x: the value whose standard Montgomery form went in"""
    p = pyref.FIELDS[field][0]
    W_, L_ = SHAPE[field][:2]
    mask, Rp = (1 << W_) - 1, 1 << (W_ * L_)

    def chk(r):
        v = sum(t << (W_ * i) for i, t in enumerate(r))
        assert v % p == x * Rp % p and v < 2 * p and all(t <= mask for t in r[:L_ - 1])
        if x == 0:
            assert v == 0
    return chk


def conversion_cases(field):
    """fromstd of x R, then tostd of a lazy variant of x R' (+ k p) back to the canonical standard form"""
    shape(field)
    p = pyref.FIELDS[field][0]
    rng = random.Random(3)
    R, Rp = 1 << (32 * NW), 1 << (W * L)
    cases = []
    for k in range(50):
        x = [0, 1, p - 1][k] if k < 3 else rng.randrange(p)
        std = x * R % p
        cases.append((field, "fromstd", words_of(std, NW) + [0] * (L - NW), [0] * L, check_fromstd(field, x)))
        v29 = x * Rp % p + (p if k % 2 else 0)                # what fromstd may return: < 2p
        lazy = spread_random(rng, v29 + rng.randrange(10) * p, (1 << 31))
        cases.append((field, "tostd", lazy, [0] * L, eq(words_of(std, NW))))
    return cases


def check_filter(e):
    def chk(r):
        assert bool(r[2]) == e
    return chk


def zero_filter_cases(field):
    """multiples of p in range are accepted exactly, everything else rejected"""
    shape(field)
    p = pyref.FIELDS[field][0]
    rng = random.Random(3 + 1000)
    cases = []
    for k in range(3, 18):
        for delta in (0, 1, p // 3):
            lazy = spread_random(rng, k * p + delta, 1 << 31)
            cases.append((field, "filter", lazy, [3, 17] + [0] * (L - 2), check_filter(delta == 0)))
    for _ in range(200):
        x = rng.randrange(3 * p, 18 * p)
        cases.append((field, "filter", spread_random(rng, x, 1 << 31), [3, 17] + [0] * (L - 2), check_filter(x % p == 0)))
    return cases


def fq2_cases(field):
    """Fe29x2 (the G2 coordinates): product with a negated operand and one reduction per component, complex square,
    refresh, zero test -- at the limb / value bounds tools/check_f29_bounds.py allows at their call sites"""
    shape(field)
    p = pyref.FIELDS[field][0]
    W_, L_ = W, L
    Rp = 1 << (W * L)
    rng = random.Random(58)
    nplus = MASK + (1 << (32 - W)) - 1
    mask = MASK
    top = p >> (W * (L - 1))

    def v(l):
        return sum(x << (W_ * i) for i, x in enumerate(l))

    def lazy(vb, lb):
        return spread_random(rng, rng.randrange(int(vb * p)), lb)

    def chk_x2(kind, a0, a1, b0, b1, kb):
        def chk(r):
            c0, c1 = r[:L_], r[L_:]
            assert all(x <= mask for x in c0[:L_ - 1] + c1[:L_ - 1])            # strict limbs
            A0, A1 = v(a0), v(a1)
            if kind == "mul":
                B0, B1 = v(b0), v(b1)
                assert v(c0) * Rp % p == (A0 * B0 - A1 * B1) % p and v(c1) * Rp % p == (A0 * B1 + A1 * B0) % p
                assert v(c0) < (A0 * B0 + A1 * (kb * p - B1)) // Rp + p + 1 and v(c1) < (A0 * B1 + A1 * B0) // Rp + p + 1
            elif kind == "sqr":
                assert v(c0) * Rp % p == (A0 * A0 - A1 * A1) % p and v(c1) * Rp % p == 2 * A0 * A1 % p
                assert v(c0) < (A0 + A1) * (A0 - A1 + kb * p) // Rp + p + 1
            else:
                assert v(c0) % p == A0 % p and v(c1) % p == A1 % p and v(c0) < A0 // (1 << 6) + p + 1 and v(c0) < 2 * p
        return chk

    cases = []
    for op, bvb, blb, kmul in (("x2mul4k1", 2.9, MASK, 4), ("x2mul8k2", 6.9, nplus, 8), ("x2mul16k2", 14.9, nplus, 16)):
        for k in range(60):
            if k == 0:       # every limb at its maximum
                a0 = a1 = b0 = [nplus] * (L - 1) + [10 * top]
                b1 = [blb] * (L - 1) + [int((bvb - 1) * top)]
            else:
                a0, a1, b0, b1 = lazy(10, nplus), lazy(10, nplus), lazy(10, nplus), lazy(bvb, blb)
            cases.append((field, op, a0 + a1, b0 + b1, chk_x2("mul", a0, a1, b0, b1, kmul)))
    for op, avb, kb in (("x2sqr8k2", 6.9, 8), ("x2sqr16k2", 14.9, 16)):
        for k in range(60):
            a0, a1 = ([nplus] * (L - 1) + [int((avb - 1) * top)],) * 2 if k == 0 else (lazy(avb, nplus), lazy(avb, nplus))
            cases.append((field, op, a0 + a1, [0] * (2 * L), chk_x2("sqr", a0, a1, None, None, kb)))
    for k in range(40):
        a0, a1 = lazy(19, nplus), lazy(19, nplus)
        cases.append((field, "x2refresh", a0 + a1, [0] * (2 * L), chk_x2("refresh", a0, a1, None, None, 0)))
    # zero test: both components must be multiples of p inside [kmin p, kmax p]
    for k0 in (2, 5, 9):
        for k1 in (2, 9):
            for d0, d1 in ((0, 0), (1, 0), (0, 1), (p // 5, 0)):
                x0, x1 = spread_random(rng, k0 * p + d0, 1 << 31), spread_random(rng, k1 * p + d1, 1 << 31)
                cases.append((field, "x2iszero", x0 + x1, [2, 9] + [0] * (2 * L - 2), eq([int(d0 == 0 and d1 == 0)])))
    return cases


def sqr_mulacc_cases(field):
    """the square and the two-product multiply with one reduction, at the widest operands their call sites produce"""
    shape(field)
    p = pyref.FIELDS[field][0]
    W_, L_, mask = W, L, MASK
    Rp = 1 << (W * L)
    top = p >> (W * (L - 1))
    rng = random.Random(31)
    nplus = MASK + (1 << (32 - W)) - 1
    wide = MASK + 1 + 2 * (MASK + 1) + nplus

    def v(l):
        return sum(x << (W_ * i) for i, x in enumerate(l))

    def chk_sqr(a):
        def chk(r):
            assert all(x <= mask for x in r[:L_ - 1])
            assert v(r) * Rp % p == v(a) * v(a) % p and v(r) < v(a) * v(a) // Rp + p + 1
        return chk

    def chk_mulacc(a, b):
        def chk(r):
            c, d = [x >> 1 for x in b], [x >> 1 for x in a]
            tot = v(a) * v(b) + v(c) * v(d)
            assert all(x <= mask for x in r[:L_ - 1])
            assert v(r) * Rp % p == tot % p and v(r) < tot // Rp + p + 1
        return chk

    cases = []
    for k in range(120):
        if k == 0:
            a = [2 * nplus] * (L - 1) + [16 * top]           # u = 2y in dbl: the widest operand a square sees
        elif k == 1:
            a = [nplus] * (L - 1) + [18 * top]
        else:
            a = spread_random(rng, rng.randrange(16 * p), 2 * nplus)
        cases.append((field, "sqr", a, [0] * L, chk_sqr(a)))
    for k in range(120):
        if k == 0:
            a, b = [nplus] * (L - 1) + [18 * top], [wide] * (L - 1) + [17 * top]     # r and t = q - x3 + 16p
        else:
            a, b = spread_random(rng, rng.randrange(18 * p), nplus), spread_random(rng, rng.randrange(17 * p), wide)
        cases.append((field, "mulacc", a, b, chk_mulacc(a, b)))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# new tables: lazy ops at k p - 1, k p, k p + 1; conversions on the edge set; the two recorded miscompile shapes
# ---------------------------------------------------------------------------------------------------------------------
FILTER_RANGES = [(5, 17), (9, 17), (3, 5)]      # the call sites of fe29_zero_filter in zk_curve29.h
X2_RANGES = [(3, 5), (2, 9)]                    # ... and of fe29_is_zero_mod_p


def kp_cases(field):
    shape(field)
    p = pyref.FIELDS[field][0]
    rng = random.Random(1900)
    R, Rp = 1 << (32 * NW), 1 << (W * L)
    cases = []
    for k in range(20):
        for d in (-1, 0, 1):
            x = k * p + d
            if x < 0:
                continue
            assert x < 20 * p
            # strict, and two lazy representations (0xFFFFFFF0: the widest limb whose carry-in cannot wrap the word)
            for lazy in (limbs_of(x), spread_random(rng, x, 0xFFFFFFF0), spread_random(rng, x, 1 << 31)):
                for op in ("norm", "carry", "canon"):
                    cases.append((field, op, lazy, [0] * L, check_ncc(field, op, x)))
                cases.append((field, "tostd", lazy, [0] * L, eq(words_of(x * R * pow(Rp, -1, p) % p, NW))))
                for kmin, kmax in FILTER_RANGES:
                    hit = d == 0 and kmin <= k <= kmax

                    def chk(r, hit=hit, k=k):
                        assert bool(r[2]) == hit
                        if hit:
                            assert r[0] == 1 and r[1] == k
                    cases.append((field, "filter", lazy, [kmin, kmax] + [0] * (L - 2), chk))
                if field in FQ2_FIELDS:
                    for kmin, kmax in X2_RANGES:
                        hit = d == 0 and kmin <= k <= kmax
                        for k1 in (kmin, kmax):
                            other = spread_random(rng, k1 * p, 1 << 31)
                            cases.append((field, "x2iszero", lazy + other, [kmin, kmax] + [0] * (2 * L - 2), eq([int(hit)])))
                            cases.append((field, "x2iszero", other + lazy, [kmin, kmax] + [0] * (2 * L - 2), eq([int(hit)])))
    return cases


def edge_set(field):
    """the saturated edge operands E (values below p, as they sit in the words)"""
    p = pyref.FIELDS[field][0]
    n = SHAPE[field][2]
    R = 1 << (32 * n)
    E = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p, p - R % p]
    E += [1 << (32 * i) for i in range(n)]
    E += [(1 << (32 * i)) - 1 for i in range(1, n + 1) if (1 << (32 * i)) - 1 < p]
    assert len(E) == (33 if n == 12 else 25)
    E.append((((p >> (32 * (n - 1))) - 1) << (32 * (n - 1))) | ((1 << (32 * (n - 1))) - 1))
    out = []
    for e in E:
        assert 0 <= e < p
        if e not in out:
            out.append(e)
    return out


def edge_conversion_cases(field):
    """fromstd / tostd round trip and unpack / pack on the edge set"""
    shape(field)
    p = pyref.FIELDS[field][0]
    rng = random.Random(2900)
    R, Rp = 1 << (32 * NW), 1 << (W * L)
    to29 = Rp * Rp * pow(R, -1, p) % p
    cases = []
    for e in edge_set(field):
        x = e * pow(R, -1, p) % p
        v29 = mont29_exact(p, e, to29)                      # fe29_from_std is one exact Montgomery product with TO29
        assert v29 % p == x * Rp % p and v29 < 2 * p

        def chk(r, x=x, v29=v29, f=check_fromstd(field, x)):
            f(r)
            assert val_of(field, r) == v29
        cases.append((field, "fromstd", words_of(e, NW) + [0] * (L - NW), [0] * L, chk))
        for lazy in (limbs_of(v29), spread_random(rng, v29 + rng.randrange(18) * p, 1 << 31)):
            cases.append((field, "tostd", lazy, [0] * L, eq(words_of(e, NW))))
    # unpack: any 32 N-bit word pattern the NTT tiles read (< 2p and beyond); pack: strict limbs of a value < 2^(32 N)
    vals = edge_set(field) + [e + p for e in edge_set(field)] + [(1 << (32 * NW)) - 1] + [rng.randrange(1 << (32 * NW)) for _ in range(64)]
    for x in vals:
        if x >= 1 << (32 * NW):
            x -= p
        cases.append((field, "unpack", words_of(x, NW), [0], eq(limbs_of(x))))
        cases.append((field, "pack", limbs_of(x), [0], eq(words_of(x, NW))))
    return cases


def val_of(field, limbs):
    w = SHAPE[field][0]
    return sum(x << (w * i) for i, x in enumerate(limbs))


def canon_r03a_cases(field="Bn254Fq"):
    """profiles/r03_a: fe29_canon over [p, 2p) -- p, p + 1, 2p - 1 and 1000 uniform values in between"""
    shape(field)
    p = pyref.FIELDS[field][0]
    rng = random.Random(0x03A)
    xs = [p, p + 1, 2 * p - 1] + [rng.randrange(p, 2 * p) for _ in range(1000)]
    return [(field, "canon", limbs_of(x), [0] * L, check_ncc(field, "canon", x)) for x in xs]


SLOT_ORDERS = [(0, 1, 2, 3), (3, 2, 1, 0), (2, 3, 0, 1), (1, 0, 3, 2)]


def slots4_cases(field, order):
    """profiles/r03_b: four Fe29 slots selected by an if-chain on a (wave-uniform) slot number, each loaded from a different
    operand, then fe29_mul of the slots; slots 2 and 3 must stay distinct.  One slot order per table: the device reads the
    slot number of the first active lane."""
    shape(field)
    p = pyref.FIELDS[field][0]
    L_ = L
    rng = random.Random(0x03B0 + SLOT_ORDERS.index(order))
    cases = []
    for _ in range(96):
        vs = [rng.randrange(1, 2 * p) for _ in range(4)]
        assert len(set(vs)) == 4
        slot = [None] * 4
        for step, s in enumerate(order):
            slot[s] = vs[step]
        exp = limbs_of(mont29_exact(p, slot[0], slot[1])) + limbs_of(mont29_exact(p, slot[2], slot[3])) + limbs_of(slot[2]) + limbs_of(slot[3])

        def chk(r, exp=exp):
            assert r[2 * L_:3 * L_] != r[3 * L_:], "slots 2 and 3 hold the same value"
            assert r == exp, "expected %s" % list(map(hex, exp))
        cases.append((field, "slots4", sum((limbs_of(x) for x in vs), []), list(order), chk))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# saturated ops (zk_field.h; on the device fe_mul is the generated assembly of zk_mul_asm.h)
# ---------------------------------------------------------------------------------------------------------------------
SAT_BINARY = ["fe_add", "fe_sub", "fe_mul", "fe_mul_portable", "fe_mul_call"]
SAT_UNARY = ["fe_neg", "fe_dbl", "fe_sqr", "fe_to_mont", "fe_from_mont"]


def sat_expect(field, op, a, b):
    p = pyref.FIELDS[field][0]
    R = 1 << (32 * SHAPE[field][2])
    Ri = pow(R, -1, p)
    return {"fe_add": (a + b) % p, "fe_sub": (a - b) % p, "fe_neg": (-a) % p, "fe_dbl": 2 * a % p,
            "fe_mul": a * b * Ri % p, "fe_mul_portable": a * b * Ri % p, "fe_mul_call": a * b * Ri % p,
            "fe_sqr": a * a * Ri % p, "fe_to_mont": a * R % p, "fe_from_mont": a * Ri % p}[op]


def sat_case(field, op, a, b):
    n = SHAPE[field][2]
    return (field, op, words_of(a, n), words_of(b, n), eq(words_of(sat_expect(field, op, a, b), n)))


def needs_final_subtraction(field, a, b):
    """does the Montgomery product's t = (a b + m p) / R reach p (the conditional subtraction is taken)?"""
    p = pyref.FIELDS[field][0]
    R = 1 << (32 * SHAPE[field][2])
    m = (-a * b * pow(p, -1, R)) % R
    t = (a * b + m * p) // R
    assert (a * b + m * p) % R == 0 and t < 2 * p
    return t >= p


def sat_edge_cases(field):
    p = pyref.FIELDS[field][0]
    E = edge_set(field)
    rng = random.Random(0x5A7)
    cases = [sat_case(field, op, a, b) for op in SAT_BINARY for a in E for b in E]
    cases += [sat_case(field, op, a, 0) for op in SAT_UNARY for a in E]
    # directed: a + b in {p - 1, p, p + 1, 2p - 2};  a - b with a = b, a = b - 1, a = 0
    some = E + [rng.randrange(p) for _ in range(32)]
    for a in some:
        for s in (p - 1, p, p + 1, 2 * p - 2):
            b = s - a
            if 0 <= b < p:
                cases.append(sat_case(field, "fe_add", a, b))
        cases.append(sat_case(field, "fe_sub", a, a))
        if a + 1 < p:
            cases.append(sat_case(field, "fe_sub", a, a + 1))
        cases.append(sat_case(field, "fe_sub", 0, a))
    return cases


def sat_uniform_cases(field, count=4096, seed=1):
    p = pyref.FIELDS[field][0]
    rng = random.Random(seed)
    pairs = [(rng.randrange(p), rng.randrange(p)) for _ in range(count)]
    taken = sum(needs_final_subtraction(field, a, b) for a, b in pairs)
    assert taken >= 64 and count - taken >= 64, (field, taken)     # both Montgomery-reduction classes are present
    cases = [sat_case(field, op, a, b) for op in SAT_BINARY for a, b in pairs]
    cases += [sat_case(field, op, a, 0) for op in SAT_UNARY for a, _ in pairs[:512]]
    return cases


def fe2_cases(field):
    p = pyref.FIELDS[field][0]
    n = SHAPE[field][2]
    Ri = pow(1 << (32 * n), -1, p)
    E = edge_set(field)
    rng = random.Random(0xFE2)
    els = [(E[i], E[(7 * i + 3) % len(E)]) for i in range(len(E))]
    pairs = [(x, y) for x in els for y in els]
    pairs += [((rng.randrange(p), rng.randrange(p)), (rng.randrange(p), rng.randrange(p))) for _ in range(512)]
    cases = []
    for (a0, a1), (b0, b1) in pairs:
        aw, bw = words_of(a0, n) + words_of(a1, n), words_of(b0, n) + words_of(b1, n)
        cases.append((field, "fe2_mul", aw, bw, eq(words_of((a0 * b0 - a1 * b1) * Ri % p, n) + words_of((a0 * b1 + a1 * b0) * Ri % p, n))))
    for (a0, a1) in els + [b for _, b in pairs[-512:]]:
        aw = words_of(a0, n) + words_of(a1, n)
        cases.append((field, "fe2_sqr", aw, [0] * (2 * n), eq(words_of((a0 * a0 - a1 * a1) * Ri % p, n) + words_of(2 * a0 * a1 * Ri % p, n))))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# curve ops.  Operands and results cross the boundary in standard form (Montgomery words); results are normalised to
# affine here and compared with pyref.ec_add / ec_mul.
# ---------------------------------------------------------------------------------------------------------------------
class CurveCtx:
    def __init__(self, curve):
        self.curve = curve
        self.field = pyref.CURVES[curve][0]
        self.p = pyref.FIELDS[self.field][0]
        self.n = SHAPE[self.field][2]
        self.ext = 2 if pyref.is_g2(curve) else 1
        self.cw = self.ext * self.n
        self.k = pyref.K(curve)
        self.G = (pyref.CURVES[curve][3], pyref.CURVES[curve][4])
        self.Q = pyref.ec_mul(curve, 0x9E3779B97F4A7C15F39CC0605CEDC835, self.G)
        assert pyref.ec_on_curve(curve, self.G) and pyref.ec_on_curve(curve, self.Q) and self.Q[0] != self.G[0]

    def coord(self, c):
        """field element -> standard-form words"""
        if self.ext == 1:
            return words_of(pyref.mont(self.field, c), self.n)
        return words_of(pyref.mont(self.field, c[0]), self.n) + words_of(pyref.mont(self.field, c[1]), self.n)

    def uncoord(self, ws):
        if self.ext == 1:
            return pyref.unmont(self.field, wval(ws))
        return (pyref.unmont(self.field, wval(ws[:self.n])), pyref.unmont(self.field, wval(ws[self.n:])))

    def aff(self, P):
        return [0] * (2 * self.cw) if P is None else self.coord(P[0]) + self.coord(P[1])

    def zval(self, z):
        return z if self.ext == 1 else (z, (3 * z + 1) % self.p)

    def xyzz(self, P, z=1):
        """P as XYZZ with Z = z: (x z^2, y z^3, z^2, z^3); None -> the identity encoding (all zero)"""
        if P is None:
            return [0] * (4 * self.cw)
        k = self.k
        z = self.zval(z) if z != 1 else (1 if self.ext == 1 else (1, 0))
        zz = k.mul(z, z)
        zzz = k.mul(zz, z)
        return self.coord(k.mul(P[0], zz)) + self.coord(k.mul(P[1], zzz)) + self.coord(zz) + self.coord(zzz)

    def check_xyzz(self, exp, extra=None):
        cw, k, ctx = self.cw, self.k, self

        def chk(r):
            assert len(r) == 4 * cw + 1 + (0 if extra is None else 1)
            assert all(wval(r[i * ctx.n:(i + 1) * ctx.n]) < ctx.p for i in range(4 * ctx.ext)), "a coordinate is not canonical"
            x, y, zz, zzz = (ctx.uncoord(r[i * cw:(i + 1) * cw]) for i in range(4))
            if extra is not None:
                assert r[4 * cw + 1] == extra, "needs-doubling flag"
            if exp is None:
                assert r[4 * cw] == 1 and not any(r[2 * cw:3 * cw]), "not the literal infinity encoding"
                return
            assert r[4 * cw] == 0 and not k.zero(zz) and not k.zero(zzz)
            assert k.mul(k.mul(zz, zz), zz) == k.mul(zzz, zzz), "ZZ^3 != ZZZ^2"
            got = (k.mul(x, k.inv(zz)), k.mul(y, k.inv(zzz)))
            assert got == exp, "expected affine %s got %s" % (exp, got)
        return chk


def curve_cases(target):
    lazy = target.endswith("29")
    curve = target[:-2] if lazy else target
    c = CurveCtx(curve)
    add, mul, neg = (lambda P, Q: pyref.ec_add(curve, P, Q)), (lambda s, P: pyref.ec_mul(curve, s, P)), (lambda P: pyref.ec_neg(curve, P))
    G, Q = c.G, c.Q
    G2, G3 = mul(2, G), mul(3, G)
    cases = []
    # acc (XYZZ) + q (affine)
    for acc, z, q in ((None, 1, G), (G, 1, None), (None, 1, None), (G, 1, G), (G, 1, neg(G)), (G, 1, Q), (G2, 7, G2), (G2, 7, neg(G2)),
                      (G3, 0xABCDEF123, Q), (Q, 5, G), (Q, 5, Q), (Q, 5, neg(Q))):
        cases.append((target, "xyzz_add_mixed", c.xyzz(acc, z), c.aff(q), c.check_xyzz(add(acc, q))))
    # acc (XYZZ) + q (XYZZ), with and without the doubling branch
    for acc, z1, q, z2 in ((None, 1, G, 1), (G, 1, None, 1), (None, 1, None, 1), (G, 1, G, 1), (G, 3, G, 11), (G, 3, neg(G), 11), (G, 1, neg(G), 1),
                           (G, 3, Q, 11), (G2, 9, G3, 1), (Q, 2, Q, 13), (Q, 2, neg(Q), 13), (None, 1, G2, 6), (G2, 6, None, 1)):
        same = acc is not None and acc == q
        cases.append((target, "xyzz_add", c.xyzz(acc, z1), c.xyzz(q, z2), c.check_xyzz(add(acc, q))))
        # add_nodbl on equal operands leaves acc alone and asks for the doubling
        cases.append((target, "xyzz_add_nodbl", c.xyzz(acc, z1), c.xyzz(q, z2), c.check_xyzz(acc if same else add(acc, q), extra=int(same))))
    for P, z in ((None, 1), (G, 1), (G, 5), (Q, 0x1234567), (G2, 3)):
        cases.append((target, "xyzz_dbl", c.xyzz(P, z), [0], c.check_xyzz(add(P, P))))
    for P in (G, Q, G2, neg(G)):
        cases.append((target, "xyzz_dbl_affine", c.aff(P), [0], c.check_xyzz(add(P, P))))
    for P in (G, Q, None):
        for flag in (0, 1):
            e = neg(P) if flag else P
            cases.append((target, "aff_neg_if", c.aff(P), [flag], eq(c.aff(e) + [int(P is None)])))
    if lazy:
        cases += to_std_cases(target, c)
    return cases


def to_std_cases(target, c):
    """xyzz29_to_std on lazy limbs: strict and spread representations of x R' + k p inside the stored-point invariant
    (zk_curve29.h: G1 X < 12p, Y < 8p, N+ limbs; G2 X < 2p strict, Y < 6.9p N+; ZZ, ZZZ strict, < 2p)"""
    shape(c.field)
    p, k = c.p, c.k
    Rp = 1 << (W * L)
    nplus = MASK + (1 << (32 - W)) - 1
    rng = random.Random(0x570)
    cases = []
    pts = [(c.G, 1), (c.Q, 5), (pyref.ec_add(c.curve, c.G, c.Q), 0xFEDCBA987)]
    for P, z in pts:
        zv = c.zval(z) if z != 1 else (1 if c.ext == 1 else (1, 0))
        zz = k.mul(zv, zv)
        zzz = k.mul(zz, zv)
        coords = [k.mul(P[0], zz), k.mul(P[1], zzz), zz, zzz]
        for variant in range(4):
            limbs = []
            for ci, co in enumerate(coords):
                for comp in ((co,) if c.ext == 1 else co):
                    v = comp * Rp % p
                    if variant == 0 or ci >= 2 or (c.ext == 2 and ci == 0):
                        limbs += limbs_of(v + (variant & 1) * p)          # strict limbs, value < 2p
                    else:
                        kmax = (11 if ci == 0 else 7) if c.ext == 1 else 5
                        limbs += spread_random(rng, v + rng.randrange(kmax + 1) * p, nplus)
            cases.append((target, "xyzz29_to_std", limbs, [0], c.check_xyzz(P)))
    cl = (1 if c.ext == 1 else 2) * L
    junk = [rng.randrange(MASK) for _ in range(2 * cl)]
    cases.append((target, "xyzz29_to_std", junk + [0] * cl + junk[:cl], [0], c.check_xyzz(None)))    # identity: ZZ = literal 0
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# the tables of one target
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def tables(target):
    if target in FIELDS:
        t = {"lazy_extremes": mul_extremes(target) + sub_cases(target) + norm_carry_canon_cases(target) + sqr_mulacc_cases(target),
             "lazy_conversion": conversion_cases(target) + zero_filter_cases(target) + edge_conversion_cases(target),
             "lazy_kp": kp_cases(target),
             "sat_edge": sat_edge_cases(target),
             "sat_uniform": sat_uniform_cases(target)}
        for order in SLOT_ORDERS:
            t["slots4_" + "".join(map(str, order))] = slots4_cases(target, order)
        if target in FQ2_FIELDS:
            t["lazy_fq2"] = fq2_cases(target)
            t["sat_fe2"] = fe2_cases(target)
        if target == "Bn254Fq":
            t["canon_r03a"] = canon_r03a_cases()
    else:
        t = {"curve": curve_cases(target)}
    # coverage by construction: every op the dispatch header declares for this target is in at least one table
    declared = {op for (tn, op) in op_table() if tn == target}
    used = {c[1] for cases in t.values() for c in cases}
    assert declared and used == declared, (target, sorted(declared ^ used))
    for cases in t.values():
        for c in cases:
            _, _, na, nb, _ = op_table()[(c[0], c[1])]
            assert len(c[2]) == na and len(c[3]) == nb, (c[0], c[1], len(c[2]), na, len(c[3]), nb)
    return t
