"""TEST INFRASTRUCTURE shared by tests/test_ipa_verify_emu.py (CPU tier, emulator build) and tests/test_ipa_verify_gpu.py (-m gpu):
halo2 opening verification on the device (zk.halo2.compute_s / compute_b, MSM, commitment_verify_proof, Guard, verify_batch) against
a restatement of halo2_proofs 0.2 poly/commitment/{prover,verifier,msm}.rs on Python integers.

The restatement is an honest create_proof with blinding formed IN THE EXPONENT: the SRS is G_i = [gamma_i]G, U = [mu]G, W = [omega]G
with seeded logarithms, so a commitment is one integer, every L_j / R_j is one integer, and only the 2k + 2 points of a proof (and
the SRS itself) are ever materialised (points_of_logs).  Every comparison is exact."""
import ctypes
import random

import numpy as np

from oracle import pyref
from oracle import zk_oracle as orc
from halo2_keygen_cases import field_of, modulus, mont1, monts, py_point, unmonts
from parity_suite import to_device, to_host
from points_fft_cases import points_of_logs, seeded_scalars

CURVES = ["Pallas", "Vesta"]
SPLIT = 8                      # IPA_S_LOW_BITS: the low table has min(2^k, 256) entries, the high table 2^(k - 8) (one entry up to k = 8)
CAP = 8                        # IPA_S_MAX_COUNT: proofs per pass
# k of the compute_s checks: below a wave (1, 2, 5), one wave (6), just above (7: the low table still partial), the split itself
# (8: the high table has exactly one entry), both tables in use (9, 10), several workgroups and high entries (13)
S_KS = [1, 2, 5, 6, 7, 8, 9, 10, 13]
ACCEPT_KS = [1, 2, 4, 7, 10]


# ---------------------------------------------------------------- the restatement: compute_s, compute_b
def ref_compute_s(p, us, init):
    """verifier.rs compute_s as upstream builds it: the filled prefix times u_j copied behind itself, last challenge first"""
    s = [init % p]
    for u in reversed(us):
        s = s + [x * u % p for x in s]
    return s


def s_at(p, us, init, i):
    """the formula: init prod_j u_j^bit_(k-1-j)(i)"""
    k, x = len(us), init % p
    for j, u in enumerate(us):
        if (i >> (k - 1 - j)) & 1:
            x = x * u % p
    return x


def ref_compute_b(p, x, us):
    k, out = len(us), 1
    for j, u in enumerate(us):
        out = out * (1 + u * pow(x, 1 << (k - 1 - j), p)) % p
    return out


def special_draw(rnd, p, specials):
    """an element drawn from `specials` half of the time, uniformly otherwise"""
    return rnd.choice(specials) if rnd.randrange(2) else rnd.randrange(p)


def draw_batch(p, k, count, seed):
    rnd = random.Random(seed)
    us = [[special_draw(rnd, p, [1, p - 1]) for _ in range(k)] for _ in range(count)]
    inits = [special_draw(rnd, p, [1, p - 1, 0]) for _ in range(count)]
    if count >= 3:                 # every special value at least once
        inits[0], inits[1], us[1][0], us[2][k - 1] = 0, p - 1, p - 1, 1
    return us, inits


def ref_batch(p, us, inits):
    cols = [ref_compute_s(p, u, i) for u, i in zip(us, inits)]
    return [sum(c) % p for c in zip(*cols)]


def device_s(zk, field, us, inits, out=None, accumulate=False):
    u_arr = np.stack([monts(field, u) for u in us])
    return zk.halo2.compute_s(field, u_arr, monts(field, inits), out=out, accumulate=accumulate)


# ---------------------------------------------------------------- 1. compute_s
def check_compute_s(zk, curve, k, count, seed=41):
    """not accumulating (over a poisoned buffer), then accumulating over a seeded prior vector"""
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    us, inits = draw_batch(p, k, count, seed + 97 * k + count)
    exp = ref_batch(p, us, inits)
    rnd = random.Random(seed)
    for i in {0, n - 1, rnd.randrange(n), rnd.randrange(n)}:          # the reference against the formula
        assert exp[i] == sum(s_at(p, u, c, i) for u, c in zip(us, inits)) % p
    out = to_device(zk, np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
    got = to_host(zk, device_s(zk, field, us, inits, out=out))
    assert (got == monts(field, exp)).all(), (curve, k, count, "write")
    fresh = to_host(zk, device_s(zk, field, us, inits))               # the mirror allocates when no buffer is given
    assert (fresh == monts(field, exp)).all(), (curve, k, count, "fresh buffer")
    prior = [rnd.randrange(p) for _ in range(n)]
    out = to_device(zk, monts(field, prior))
    got = to_host(zk, device_s(zk, field, us, inits, out=out, accumulate=True))
    assert (got == monts(field, [(a + b) % p for a, b in zip(prior, exp)])).all(), (curve, k, count, "accumulate")


def check_chunking(zk, curve, k=6, seed=43):
    """count = cap + 1: two passes inside one call, the second accumulating whatever the caller asked for"""
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    us, inits = draw_batch(p, k, CAP + 1, seed)
    exp = ref_batch(p, us, inits)
    out = to_device(zk, np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
    assert (to_host(zk, device_s(zk, field, us, inits, out=out)) == monts(field, exp)).all()
    prior = [random.Random(seed).randrange(p) for _ in range(n)]
    out = to_device(zk, monts(field, prior))
    got = to_host(zk, device_s(zk, field, us, inits, out=out, accumulate=True))
    assert (got == monts(field, [(a + b) % p for a, b in zip(prior, exp)])).all()


def check_against_update_weights(zk, curve, k=9, seed=47):
    """compute_s(u, 1) is the final weight vector W of IpaProverVirtual: k calls of zk_ipa_update_weights_device on ones"""
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    rnd = random.Random(seed)
    us = [rnd.randrange(1, p) for _ in range(k)]
    w = to_device(zk, monts(field, [1] * n))
    lib = zk.halo2._plib()
    for j, u in enumerate(us):
        uu = mont1(field, u)
        assert lib.zk_ipa_update_weights_device(zk.field_id(field), dev_ptr(w), n, 1 << (k - 1 - j), uu.ctypes.data, None) == 0
    got = to_host(zk, device_s(zk, field, [us], [1]))
    assert (got == to_host(zk, w)).all()
    assert (got == monts(field, ref_compute_s(p, us, 1))).all()


def check_grid_stride(zk, curve, k=20, count=3, samples=4096, seed=53):
    """more rows than one sweep of the grid covers (2048 workgroups of 256): 4096 sampled indices by the direct product over bits"""
    field = field_of(curve)
    p = modulus(field)
    n = 1 << k
    assert n > 2048 * 256
    us, inits = draw_batch(p, k, count, seed)
    got = to_host(zk, device_s(zk, field, us, inits))
    rnd = random.Random(seed)
    idx = sorted({0, n - 1, 2048 * 256 - 1, 2048 * 256} | {rnd.randrange(n) for _ in range(samples)})
    exp = [sum(s_at(p, u, c, i) for u, c in zip(us, inits)) % p for i in idx]
    assert (got[idx] == monts(field, exp)).all()


# ---------------------------------------------------------------- 2. compute_b
def check_compute_b(zk, curve, seed=59):
    field = field_of(curve)
    p = modulus(field)
    rnd = random.Random(seed)
    for k in (1, 2, 3, 8, 13, 32):
        us = [special_draw(rnd, p, [1, p - 1, 0]) for _ in range(k)]
        s = unmonts(field, to_host(zk, device_s(zk, field, [us], [1]))) if k <= 8 else None
        for x in (0, 1, p - 1, rnd.randrange(p), rnd.randrange(p)):
            got = unmonts(field, zk.halo2.compute_b(field, mont1(field, x), monts(field, us)))[0]
            assert got == ref_compute_b(p, x, us), (curve, k, x)
            if s is not None:
                assert got == sum(si * pow(x, i, p) for i, si in enumerate(s)) % p, (curve, k, x, "sum s_i x^i")


# ---------------------------------------------------------------- the restatement: create_proof in the exponent
class Srs:
    """G_i = [gamma_i]G, U = [mu]G, W = [omega]G and the library's Params over them"""

    def __init__(self, zk, curve, k, seed=61):
        self.zk, self.curve, self.k, self.n = zk, curve, k, 1 << k
        self.field = field_of(curve)
        self.p = modulus(self.field)
        logs = seeded_scalars(curve, self.n + 2, seed + k)
        self.gamma, self.mu, self.omega = logs[:self.n], logs[self.n], logs[self.n + 1]
        pts = points_of_logs(curve, logs)
        self.u_point, self.w_point = pts[self.n].copy(), pts[self.n + 1].copy()
        self.params = zk.halo2.Params.from_g(curve, k, pts[:self.n].copy(), u=self.u_point, w=self.w_point)

    def free(self):
        self.params.free()


def dot(p, a, b):
    return sum(x * y for x, y in zip(a, b)) % p


def poly_eval(p, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


class Opening:
    """everything an honest prover knows, as integers (points as logarithms)"""


def opened_polynomial(srs, rnd):
    """-> (o with the committed polynomial, its blind, the point x and the value v, the blinding polynomial s with s(x) = 0, xi, z,
    p' = xi s + p with p'[0] -= v, blind' = xi s_blind + p_blind; P and S as logarithms)"""
    p, n = srs.p, srs.n
    o = Opening()
    o.coeffs = [rnd.randrange(p) for _ in range(n)]
    o.p_blind, o.x = rnd.randrange(p), rnd.randrange(p)
    o.v = poly_eval(p, o.coeffs, o.x)
    o.P = (dot(p, o.coeffs, srs.gamma) + o.p_blind * srs.omega) % p
    s = [rnd.randrange(p) for _ in range(n)]
    s[0] = (s[0] - poly_eval(p, s, o.x)) % p
    assert poly_eval(p, s, o.x) == 0
    s_blind = rnd.randrange(p)
    o.S = (dot(p, s, srs.gamma) + s_blind * srs.omega) % p
    o.xi, o.z = rnd.randrange(p), rnd.randrange(p)
    o.p1 = [(o.xi * a + b) % p for a, b in zip(s, o.coeffs)]
    o.p1[0] = (o.p1[0] - o.v) % p
    o.blind1 = (o.xi * s_blind + o.p_blind) % p
    return o


def honest_opening(srs, seed):
    """create_proof: k rounds of L_j = <p'_hi, G'_lo> + [value_l z]U + [l_blind]W (R likewise), the folds p'[i] += u^-1 p'[i + half],
    b[i] += u b[i + half], G'[i] += [u]G'[i + half], f = blind' + sum (l_blind u^-1 + r_blind u), c = p'[0] at the end"""
    p = srs.p
    rnd = random.Random(seed)
    o = opened_polynomial(srs, rnd)
    a, g = list(o.p1), list(srs.gamma)
    b = [pow(o.x, i, p) for i in range(srs.n)]
    o.rounds, o.f = [], o.blind1
    for j in range(srs.k):
        half = len(a) // 2
        l_blind, r_blind, u = rnd.randrange(p), rnd.randrange(p), rnd.randrange(1, p)
        L = (dot(p, a[half:], g[:half]) + dot(p, a[half:], b[:half]) * o.z * srs.mu + l_blind * srs.omega) % p
        R = (dot(p, a[:half], g[half:]) + dot(p, a[:half], b[half:]) * o.z * srs.mu + r_blind * srs.omega) % p
        ui = pow(u, -1, p)
        a = [(a[i] + ui * a[i + half]) % p for i in range(half)]
        b = [(b[i] + u * b[i + half]) % p for i in range(half)]
        g = [(g[i] + u * g[i + half]) % p for i in range(half)]
        o.f = (o.f + l_blind * ui + r_blind * u) % p
        o.rounds.append([L, R, u])
    o.c, o.g_final = a[0], g[0]
    us = [r[2] for r in o.rounds]
    assert b[0] == ref_compute_b(p, o.x, us) and g[0] == dot(p, ref_compute_s(p, us, 1), srs.gamma)       # the restatement's own identities
    return o


def materialise(srs, o, s_identity=False, l_points=None):
    """-> (P, IpaProof, x, v) as the library takes them: the 2k + 2 points from their logarithms in one fixed-base call.
    l_points: {round: affine point} replaces those L_j (points that have no known logarithm)"""
    zk, field = srs.zk, srs.field
    pts = points_of_logs(srs.curve, [o.P, o.S] + [r[0] for r in o.rounds] + [r[1] for r in o.rounds])
    k = srs.k
    rounds = [((l_points or {}).get(j, pts[2 + j]), pts[2 + k + j], mont1(field, o.rounds[j][2])) for j in range(len(o.rounds))]
    s_point = np.zeros_like(pts[1]) if s_identity else pts[1]
    proof = zk.halo2.IpaProof(s_point, mont1(field, o.xi), mont1(field, o.z), rounds, mont1(field, o.c), mont1(field, o.f))
    return pts[0], proof, mont1(field, o.x), mont1(field, o.v)


def guard_for(srs, o, **kw):
    zk = srs.zk
    P, proof, x, v = materialise(srs, o, **kw)
    m = zk.halo2.MSM(srs.params)
    m.append_term(mont1(srs.field, 1), P)
    return zk.halo2.commitment_verify_proof(srs.params, m, proof, x, v)


# ---------------------------------------------------------------- 3. accept
def check_accept(zk, curve, k, seed=67):
    srs = Srs(zk, curve, k)
    o = honest_opening(srs, seed + k)
    assert guard_for(srs, o).use_challenges().eval() is True, (curve, k, "use_challenges")
    g = guard_for(srs, o).compute_g()
    assert (g == points_of_logs(curve, [o.g_final])[0]).all(), (curve, k, "compute_g")
    m, acc = guard_for(srs, o).use_g(g)
    assert m.eval() is True and (acc.g == g).all(), (curve, k, "use_g")
    assert m.g_scalars is not None and int(m.g_scalars.shape[0]) == srs.n        # only the constant term went there
    srs.free()


# ---------------------------------------------------------------- 4. reject
def tampered(o, what, j=1):
    """one single change to an honest opening -> (opening, materialise keywords)"""
    import copy
    t = copy.deepcopy(o)
    kw = {}
    if what in ("c", "f", "v", "x", "xi", "z"):
        setattr(t, what, getattr(t, what) + 1)
    elif what == "L+G":
        t.rounds[j][0] += 1
    elif what == "swap":
        t.rounds[j][0], t.rounds[j][1] = t.rounds[j][1], t.rounds[j][0]
    elif what == "u":
        t.rounds[j][2] += 1
    elif what == "S=0":
        kw["s_identity"] = True
    else:
        raise KeyError(what)
    return t, kw


REJECTS = ["c", "f", "v", "L+G", "swap", "u", "x", "xi", "z", "S=0"]


def check_reject(zk, curve, k=4, seed=71):
    srs = Srs(zk, curve, k)
    o = honest_opening(srs, seed)
    assert guard_for(srs, o).use_challenges().eval() is True
    for what in REJECTS:
        t, kw = tampered(o, what)
        assert guard_for(srs, t, **kw).use_challenges().eval() is False, (curve, what)
    srs.free()


# ---------------------------------------------------------------- 5. round trip with the library's prover
def aff_limbs(curve, P):
    """affine Python integers (None = the identity) -> Montgomery limbs"""
    bf = pyref.CURVES[curve][0]
    if P is None:
        return np.zeros(8, dtype=np.uint64)
    return np.concatenate([orc.int_to_limbs(pyref.mont(bf, c), 4) for c in P])


def check_round_trip(zk, curve, k=8, seed=73):
    """IpaProver.round() / fold() on the device give L_j, R_j (before blinding) and the two inner products; the test adds
    [value z]U + [blind]W on Python integers and forms f; the device verifier accepts, and rejects an L without its U term"""
    srs = Srs(zk, curve, k)
    field, p = srs.field, srs.p
    rnd = random.Random(seed)
    o = opened_polynomial(srs, rnd)
    U, W = py_point(curve, srs.u_point), py_point(curve, srs.w_point)
    d_p = to_device(zk, monts(field, o.p1))
    d_b = to_device(zk, monts(field, [pow(o.x, i, p) for i in range(srs.n)]))
    d_g = to_device(zk, to_host(zk, srs.params.d_g).copy())
    prover = zk.halo2.IpaProver(curve, d_p, d_b, d_g)
    rounds, bare_l, f = [], {}, o.blind1
    for j in range(k):
        L, R, vl, vr = prover.round()
        l_blind, r_blind, u = rnd.randrange(p), rnd.randrange(p), rnd.randrange(1, p)
        pts = []
        for jac, val, blind in ((L, vl, l_blind), (R, vr, r_blind)):
            value = unmonts(field, val)[0]
            base = py_point(curve, zk.point_to_affine(curve, jac))
            with_w = pyref.ec_add(curve, base, pyref.ec_mul(curve, blind, W))
            pts.append((pyref.ec_add(curve, with_w, pyref.ec_mul(curve, value * o.z % p, U)), with_w))
        if j == 3:
            assert pts[0][0] != pts[0][1]
            bare_l[j] = aff_limbs(curve, pts[0][1])
        rounds.append((aff_limbs(curve, pts[0][0]), aff_limbs(curve, pts[1][0]), mont1(field, u)))
        f = (f + l_blind * pow(u, -1, p) + r_blind * u) % p
        prover.fold(mont1(field, u))
    c = to_host(zk, prover.p)[0].copy()
    prover.free()
    pts = points_of_logs(curve, [o.P, o.S])

    def verdict(replace):
        rs = [(replace.get(j, r[0]), r[1], r[2]) for j, r in enumerate(rounds)]
        proof = zk.halo2.IpaProof(pts[1], mont1(field, o.xi), mont1(field, o.z), rs, c, mont1(field, f))
        m = zk.halo2.MSM(srs.params)
        m.append_term(mont1(field, 1), pts[0])
        return zk.halo2.commitment_verify_proof(srs.params, m, proof, mont1(field, o.x), mont1(field, o.v)).use_challenges().eval()

    assert verdict({}) is True, (curve, "the library's prover against the library's verifier")
    assert verdict(bare_l) is False, (curve, "an L without its U term")
    srs.free()


# ---------------------------------------------------------------- 6. batch
def msm_state(zk, m):
    g = None if m.g_scalars is None else to_host(zk, m.g_scalars).copy()
    return g, list(m.other_scalars), [b.tolist() for b in m.other_bases], m.w_scalar, m.u_scalar


def check_batch(zk, curve, k=5, count=3, seed=79):
    srs = Srs(zk, curve, k)
    field, p = srs.field, srs.p
    rnd = random.Random(seed)
    honest = [honest_opening(srs, seed + 1 + i) for i in range(count)]
    assert len({tuple(o.coeffs) for o in honest}) == count
    weights = [mont1(field, rnd.randrange(1, p)) for _ in range(count)]

    def both(openings):
        items = [materialise(srs, o) for o in openings]
        seq = zk.halo2.MSM(srs.params)
        for (P, proof, x, v), r in zip(items, weights):
            seq.scale(r)
            seq.append_term(mont1(field, 1), P)
            seq = zk.halo2.commitment_verify_proof(srs.params, seq, proof, x, v).use_challenges()
        fused = zk.halo2.batch_msm(srs.params, items, weights)
        a, b = msm_state(zk, seq), msm_state(zk, fused)
        assert (a[0] == b[0]).all(), (curve, "g_scalars word for word")
        assert a[1:] == b[1:], (curve, "every other scalar and base")
        return seq.eval(), fused.eval(), zk.halo2.verify_batch(srs.params, items, weights)

    assert both(honest) == (True, True, True)
    for bad in range(count):
        openings = list(honest)
        openings[bad] = tampered(honest[bad], "c")[0]
        assert both(openings) == (False, False, False), (curve, bad)
    srs.free()


# ---------------------------------------------------------------- 7. the MSM's algebra
class ModelMSM:
    """msm.rs MSM on integers, every point by its logarithm"""

    def __init__(self, srs):
        self.srs, self.p = srs, srs.p
        self.g, self.w, self.u, self.terms = None, None, None, []

    def _g(self):
        if self.g is None:
            self.g = [0] * self.srs.n
        return self.g

    def append_term(self, s, log):
        self.terms.append([s % self.p, log])

    def add_constant_term(self, c):
        self._g()[0] = (self._g()[0] + c) % self.p

    def add_to_g_scalars(self, v):
        self.g = [(a + b) % self.p for a, b in zip(self._g(), v)]

    def add_to_w_scalar(self, s):
        self.w = ((self.w or 0) + s) % self.p

    def add_to_u_scalar(self, s):
        self.u = ((self.u or 0) + s) % self.p

    def scale(self, f):
        if self.g is not None:
            self.g = [a * f % self.p for a in self.g]
        self.terms = [[s * f % self.p, log] for s, log in self.terms]
        self.w = None if self.w is None else self.w * f % self.p
        self.u = None if self.u is None else self.u * f % self.p

    def add_msm(self, other):
        self.terms += [list(t) for t in other.terms]
        if other.g is not None:
            self.add_to_g_scalars(other.g)
        if other.w is not None:
            self.add_to_w_scalar(other.w)
        if other.u is not None:
            self.add_to_u_scalar(other.u)

    def total(self):
        t = sum(s * log for s, log in self.terms) + (self.w or 0) * self.srs.omega + (self.u or 0) * self.srs.mu
        return (t + (dot(self.p, self.g, self.srs.gamma) if self.g is not None else 0)) % self.p


def random_ops(srs, rnd, pair, steps, pool, allow_add_msm=True):
    """the same seeded operations on (library MSM, model)"""
    zk, field, p = srs.zk, srs.field, srs.p
    m, model = pair
    one = lambda x: mont1(field, x)
    for _ in range(steps):
        op = rnd.choice(["append_term", "add_constant_term", "add_to_g_scalars", "add_to_w_scalar", "add_to_u_scalar", "scale"] +
                        (["add_msm"] if allow_add_msm else []))
        x = rnd.randrange(p)
        if op == "append_term":
            log, point = rnd.choice(pool)
            m.append_term(one(x), point)
            model.append_term(x, log)
        elif op == "add_to_g_scalars":
            v = [rnd.randrange(p) for _ in range(srs.n)]
            m.add_to_g_scalars(to_device(zk, monts(field, v)))
            model.add_to_g_scalars(v)
        elif op == "add_msm":
            other = (zk.halo2.MSM(srs.params), ModelMSM(srs))
            random_ops(srs, rnd, other, rnd.randrange(5), pool, allow_add_msm=False)
            m.add_msm(other[0])
            model.add_msm(other[1])
        else:
            getattr(m, op)(one(x))
            getattr(model, op)(x)


def check_model_state(zk, srs, m, model):
    assert (m.g_scalars is None) == (model.g is None)
    if model.g is not None:
        assert (to_host(zk, m.g_scalars) == monts(srs.field, model.g)).all()
    assert m.other_scalars == [s for s, _ in model.terms] and m.w_scalar == model.w and m.u_scalar == model.u


def check_msm_algebra(zk, curve, k=4, seed=83):
    srs = Srs(zk, curve, k)
    field, p = srs.field, srs.p
    rnd = random.Random(seed)
    logs = [rnd.randrange(p) for _ in range(5)] + [0, 1]
    pool = list(zip(logs, points_of_logs(curve, logs)))           # the identity and the generator among them
    gen = pool[-1][1]
    one = lambda x: mont1(field, x)
    for trial in range(4):
        pair = (zk.halo2.MSM(srs.params), ModelMSM(srs))
        random_ops(srs, rnd, pair, 12, pool)
        m, model = pair
        check_model_state(zk, srs, m, model)
        assert model.total() != 0 and m.eval() is False, (curve, trial)
        m.append_term(one(-model.total() % p), gen)               # ... and cancelled exactly
        model.append_term(-model.total(), 1)
        assert model.total() == 0 and m.eval() is True, (curve, trial, "cancelled")
    # no g_scalars at all
    m = zk.halo2.MSM(srs.params)
    assert m.eval() is True                                       # the empty sum
    a = rnd.randrange(1, p)
    m.append_term(one(a), pool[0][1])
    assert m.g_scalars is None and m.eval() is False
    m.append_term(one(p - a), pool[0][1])
    m.add_to_w_scalar(one(5))
    m.add_to_w_scalar(one(p - 5))                                 # Some(0): W still goes into the small MSM
    assert m.g_scalars is None and m.w_scalar == 0 and m.eval() is True
    # the g part cancels the listed terms exactly
    v = [rnd.randrange(p) for _ in range(srs.n)]
    m = zk.halo2.MSM(srs.params)
    m.add_to_g_scalars(to_device(zk, monts(field, v)))
    assert m.eval() is False
    m.append_term(one(p - 1), points_of_logs(curve, [dot(p, v, srs.gamma)])[0])
    assert m.eval() is True
    # add_constant_term on a fresh MSM
    c = rnd.randrange(1, p)
    m = zk.halo2.MSM(srs.params)
    m.add_constant_term(one(c))
    assert (to_host(zk, m.g_scalars) == monts(field, [c] + [0] * (srs.n - 1))).all() and m.eval() is False
    m.append_term(one(p - c), to_host(zk, srs.params.d_g)[0])
    assert m.eval() is True
    # a scalar for U or W without the point
    bare = zk.halo2.Params(curve, k, srs.params.d_g, srs.params.d_g_lagrange)
    m = zk.halo2.MSM(bare)
    m.add_to_u_scalar(one(1))
    try:
        m.eval()
    except zk.ZkError as e:
        assert e.status == -1
    else:
        raise AssertionError("evaluated [u_scalar]U without a U")
    bare.free()
    srs.free()


# ---------------------------------------------------------------- 8. refusals
def dev_ptr(buf):
    return buf.ctypes.data if isinstance(buf, np.ndarray) else buf.data_ptr()


def check_refusals(zk, curve, seed=89):
    field = field_of(curve)
    fid = zk.field_id(field)
    p = modulus(field)
    lib = zk.halo2._plib()
    k, count = 5, 2
    n = 1 << k
    us, inits = draw_batch(p, k, count, seed)
    # 16-byte aligned host arrays with room to step 8 bytes off
    u_arr, i_arr = zk.halo2._aligned16(np.zeros((count * k + 1, 4), dtype=np.uint64)), zk.halo2._aligned16(np.zeros((count + 1, 4), dtype=np.uint64))
    u_arr[:count * k] = np.concatenate([monts(field, u) for u in us])
    i_arr[:count] = monts(field, inits)
    poison = np.full((n + 1, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    buf = to_device(zk, poison)
    base = dev_ptr(buf)
    assert base % 16 == 0 and u_arr.ctypes.data % 16 == 0 and i_arr.ctypes.data % 16 == 0
    call = lambda f=fid, kk=k, cnt=count, u=u_arr.ctypes.data, i=i_arr.ctypes.data, s=base, acc=0: lib.zk_halo2_ipa_s_device(f, kk, cnt, u, i, s, acc, None)
    assert call(u=None) == -1 and call(i=None) == -1 and call(s=None) == -1
    assert call(u=u_arr.ctypes.data + 8) == -1 and call(i=i_arr.ctypes.data + 8) == -1 and call(s=base + 8) == -1        # misaligned
    assert call(cnt=0) == -1
    assert call(kk=0) == -1 and call(kk=33) == -1                      # above the two-adicity (32 on both Pasta fields)
    assert call(f=9) == -1
    assert (to_host(zk, buf) == poison).all(), "refused calls write nothing"
    xb, out = mont1(field, 3), np.zeros(4, dtype=np.uint64)
    cb = lambda kk=k, x=xb.ctypes.data, u=u_arr.ctypes.data, o=out.ctypes.data: lib.zk_halo2_ipa_compute_b(fid, kk, x, u, o)
    assert cb(x=None) == -1 and cb(u=None) == -1 and cb(o=None) == -1 and cb(kk=0) == -1 and cb(kk=33) == -1
    assert not out.any()
    # ... and a good call through the same pointers is right
    assert call() == 0
    assert (to_host(zk, buf)[:n] == monts(field, ref_batch(p, us, inits))).all() and (to_host(zk, buf)[n] == poison[n]).all()
    # through the mirror
    for bad in (lambda: zk.halo2.compute_s(field, np.zeros((1, 0, 4), dtype=np.uint64), monts(field, [1])),                  # k = 0
                lambda: zk.halo2.compute_s(field, np.zeros((1, 33, 4), dtype=np.uint64), monts(field, [1])),                 # k = 33
                lambda: zk.halo2.compute_s(field, np.zeros((0, k, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64),   # count = 0
                                           out=to_device(zk, poison[:n])),
                lambda: zk.halo2.compute_s(field, monts(field, us[0]), monts(field, [1, 1])),                                # two inits, one proof
                lambda: zk.halo2.compute_b(field, xb, np.zeros((33, 4), dtype=np.uint64))):
        try:
            bad()
        except zk.ZkError as e:
            assert e.status == -1
        else:
            raise AssertionError("the mirror accepted a refused shape")
    try:
        zk.halo2.compute_s(field, monts(field, us[0]), monts(field, [1]), out=to_device(zk, poison[:n // 2]))
    except AssertionError as e:
        assert "s.len() == 1 << k" in str(e)
    else:
        raise AssertionError("accepted a vector of the wrong length")
    # verify_proof: the round count and a zero challenge, both before the msm is touched
    srs = Srs(zk, curve, 4)
    o = honest_opening(srs, seed)
    P, proof, x, v = materialise(srs, o)
    short = zk.halo2.IpaProof(proof.s_commitment, proof.xi, proof.z, proof.rounds[:-1], proof.c, proof.f)
    longer = zk.halo2.IpaProof(proof.s_commitment, proof.xi, proof.z, proof.rounds + proof.rounds[:1], proof.c, proof.f)
    zero_u = zk.halo2.IpaProof(proof.s_commitment, proof.xi, proof.z, proof.rounds[:2] + [(proof.rounds[2][0], proof.rounds[2][1], mont1(field, 0))] +
                               proof.rounds[3:], proof.c, proof.f)
    for bad in (short, longer, zero_u):
        m = zk.halo2.MSM(srs.params)
        try:
            zk.halo2.commitment_verify_proof(srs.params, m, bad, x, v)
        except zk.ZkError as e:
            assert e.status == -1
        else:
            raise AssertionError("accepted a malformed proof")
        assert m.g_scalars is None and not m.other_scalars and m.w_scalar is None and m.u_scalar is None
        try:
            zk.halo2.verify_batch(srs.params, [(P, bad, x, v)], [mont1(field, 1)])
        except zk.ZkError as e:
            assert e.status == -1
        else:
            raise AssertionError("the batch accepted a malformed proof")
    for items, weights in (([], []), ([(P, proof, x, v)], [])):
        try:
            zk.halo2.verify_batch(srs.params, items, weights)
        except zk.ZkError as e:
            assert e.status == -1
        else:
            raise AssertionError("accepted an empty batch or a missing weight")
    # ... and the library is still usable: an accept case
    assert guard_for(srs, o).use_challenges().eval() is True
    assert zk.halo2.verify_batch(srs.params, [(P, proof, x, v)], [mont1(field, 7)]) is True
    srs.free()
