"""TEST INFRASTRUCTURE: an independent reference for the optimal ate pairing on BLS12-381 and BN254, on Python integers.

Nothing here follows the library's tower code.  Fq12 is ONE polynomial ring, Fq[w] / (w^12 - A w^6 - B) (w^12 - 2 w^6 + 2 on
BLS12-381, w^12 - 18 w^6 + 82 on BN254: w^6 = xi = k + u with u^2 = -1 gives (w^6 - k)^2 + 1 = 0), an element a list of 12
integers.  The twist point is lifted to E(Fq12) -- (x w^2, y w^3) for the D-type twist of BN254, (x / w^2, y / w^3) for the M-type
twist of BLS12-381 -- and checked against y^2 = x^3 + b there; the Miller loop is the textbook affine one with the slope
computed by an Fq12 inversion (extended Euclid on polynomials); the Frobenius of BN254's last two lines is a literal p-th power;
and the final exponentiation is pow(f, (p^12 - 1) / r).  Vertical lines are left out: they lie in Fq6.  For the negative x of
BLS12-381 the Miller value is inverted (equal to conjugating it once the final exponentiation is applied).

One pairing costs about a second: the CPU tier keeps to about ten per curve."""

BLS_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
BLS_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BN_P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
BN_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BN_X = 4965661367192848881

# p, r, b of E, k of xi = k + u, (A, B) of w^12 = A w^6 + B, the loop scalar, M-type twist?, negative loop scalar?, BN?
PARAMS = {
    "Bls381": dict(p=BLS_P, r=BLS_R, b=4, k=1, red=(2, -2), loop=0xd201000000010000, m_twist=True, negative=True, bn=False),
    "Bn254": dict(p=BN_P, r=BN_R, b=3, k=9, red=(18, -82), loop=6 * BN_X + 2, m_twist=False, negative=False, bn=True),
}


class Fq12:
    def __init__(self, pairing):
        c = PARAMS[pairing]
        self.p, self.red, self.k = c["p"], c["red"], c["k"]
        self.one = [1] + [0] * 11
        self.modulus = [-c["red"][1] % self.p, 0, 0, 0, 0, 0, -c["red"][0] % self.p, 0, 0, 0, 0, 0, 1]

    def const(self, a):
        return [a % self.p] + [0] * 11

    def w_pow(self, e):
        out = [0] * 12
        out[e] = 1
        return out

    def add(self, a, b):
        return [(x + y) % self.p for x, y in zip(a, b)]

    def sub(self, a, b):
        return [(x - y) % self.p for x, y in zip(a, b)]

    def mul(self, a, b):
        t = [0] * 23
        for i, x in enumerate(a):
            if x:
                for j, y in enumerate(b):
                    t[i + j] += x * y
        A, B = self.red
        for i in range(22, 11, -1):
            c = t[i]
            t[i - 6] += A * c
            t[i - 12] += B * c
        return [v % self.p for v in t[:12]]

    def pow(self, a, e):
        out = self.one
        for bit in bin(e)[2:]:
            out = self.mul(out, out)
            if bit == "1":
                out = self.mul(out, a)
        return out

    # ---- inversion: extended Euclid in Fq[w]
    def _trim(self, a):
        a = list(a)
        while a and a[-1] == 0:
            a.pop()
        return a

    def _divmod(self, a, b):
        p = self.p
        a, q = list(a), [0] * max(len(a) - len(b) + 1, 1)
        inv = pow(b[-1], -1, p)
        while len(a) >= len(b):
            c = a[-1] * inv % p
            s = len(a) - len(b)
            q[s] = c
            for i, y in enumerate(b):
                a[s + i] = (a[s + i] - c * y) % p
            a = self._trim(a)
            if not a:
                break
        return q, a

    def _pmul(self, a, b):
        if not a or not b:
            return []
        t = [0] * (len(a) + len(b) - 1)
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                t[i + j] += x * y
        return self._trim([v % self.p for v in t])

    def _psub(self, a, b):
        n = max(len(a), len(b))
        a, b = a + [0] * (n - len(a)), b + [0] * (n - len(b))
        return self._trim([(x - y) % self.p for x, y in zip(a, b)])

    def inv(self, a):
        r0, r1 = list(self.modulus), self._trim(a)
        assert r1, "inverse of zero"
        s0, s1 = [], [1]
        while r1:
            q, rem = self._divmod(r0, r1)
            r0, r1 = r1, rem
            s0, s1 = s1, self._psub(s0, self._pmul(q, s1))
        assert len(r0) == 1               # the modulus is irreducible: the gcd is a constant
        c = pow(r0[0], -1, self.p)
        out = [v * c % self.p for v in s0]
        return out + [0] * (12 - len(out))

    def from_fq2(self, a):
        """a0 + a1 u with u = w^6 - k"""
        out = [0] * 12
        out[0], out[6] = (a[0] - self.k * a[1]) % self.p, a[1] % self.p
        return out

    def from_tower(self, coeffs):
        """the 12 integers of an Fq12 element in ark's Fp12 order (c_i over w, then c_j over v = w^2, then c_k over u) -> the polynomial"""
        out = [0] * 12
        for i in range(2):
            for j in range(3):
                e = i + 2 * j
                a0, a1 = coeffs[6 * i + 2 * j], coeffs[6 * i + 2 * j + 1]
                out[e] = (out[e] + a0 - self.k * a1) % self.p
                out[e + 6] = (out[e + 6] + a1) % self.p
        return out


def lift_g2(pairing, Q):
    """a point of the twist, ((x0, x1), (y0, y1)), as a point of E(Fq12)"""
    c, F = PARAMS[pairing], Fq12(pairing)
    x, y = F.from_fq2(Q[0]), F.from_fq2(Q[1])
    if c["m_twist"]:
        x, y = F.mul(x, F.inv(F.w_pow(2))), F.mul(y, F.inv(F.w_pow(3)))
    else:
        x, y = F.mul(x, F.w_pow(2)), F.mul(y, F.w_pow(3))
    assert F.mul(y, y) == F.add(F.mul(F.mul(x, x), x), F.const(c["b"])), "the lifted point is on E"
    return x, y


def _line_and_sum(F, T, Q, P):
    """the line through T and Q (the tangent when T == Q) at P = (xP, yP) in Fq, and T + Q"""
    (x1, y1), (x2, y2) = T, Q
    if T == Q:
        lam = F.mul(F.mul(F.const(3), F.mul(x1, x1)), F.inv(F.add(y1, y1)))
    else:
        assert x1 != x2
        lam = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
    line = F.sub(F.sub(F.const(P[1]), y1), F.mul(lam, F.sub(F.const(P[0]), x1)))
    x3 = F.sub(F.sub(F.mul(lam, lam), x1), x2)
    y3 = F.sub(F.mul(lam, F.sub(x1, x3)), y1)
    return line, (x3, y3)


def miller(pairing, P, Q):
    """P = (x, y) integers on E(Fq), Q a twist point; neither the identity"""
    c, F = PARAMS[pairing], Fq12(pairing)
    Ql = lift_g2(pairing, Q)
    T, f = Ql, F.one
    for bit in bin(c["loop"])[3:]:
        line, T2 = _line_and_sum(F, T, T, P)
        f = F.mul(F.mul(f, f), line)
        T = T2
        if bit == "1":
            line, T = _line_and_sum(F, T, Ql, P)
            f = F.mul(f, line)
    if c["bn"]:
        p = c["p"]
        Q1 = (F.pow(Ql[0], p), F.pow(Ql[1], p))
        Q2 = (F.pow(Q1[0], p), F.sub(F.const(0), F.pow(Q1[1], p)))
        line, T = _line_and_sum(F, T, Q1, P)
        f = F.mul(f, line)
        line, _ = _line_and_sum(F, T, Q2, P)
        f = F.mul(f, line)
    if c["negative"]:
        f = F.inv(f)
    return f


def final_exponentiation(pairing, f):
    c = PARAMS[pairing]
    return Fq12(pairing).pow(f, (c["p"] ** 12 - 1) // c["r"])


def pairing(name, P, Q):
    """e(P, Q) as a polynomial; None in either slot is the identity"""
    if P is None or Q is None:
        return list(Fq12(name).one)
    return final_exponentiation(name, miller(name, P, Q))
