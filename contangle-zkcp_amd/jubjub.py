"""JubJub on the host: ark-ed-on-bls12-381 0.3's twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over BLS12-381 Fr, a = -1,
d = -10240/10241, on Python integers.  No device and no library call: the two scalar multiplications of EncryptCircuit::encrypt
(c1 = [r]G, the shared point [r]pk), keygen, and the compressed point codec of ark-serialize 0.3.

d is a non-square, so the affine addition law is complete: one formula, no exceptional cases, the identity (0, 1) included.

GENERATOR is the prime-subgroup generator as the project's issue tracker states upstream's; the crate source is not at hand, so its
parity with `EdwardsProjective::prime_subgroup_generator()` is unpinned.  Nothing but `keygen` and the default
argument of encryption.EncryptCircuit depends on the constant."""

P = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001        # BLS12-381 Fr, the curve's base field
A = P - 1
D = (-10240 * pow(10241, -1, P)) % P
ORDER = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7    # the prime-order subgroup; the curve has 8 * ORDER points
COFACTOR = 8
IDENTITY = (0, 1)
GENERATOR = (8076246640662884909881801758704306714034609987455869804520522091855516602923,
             13262374693698910701929044844600465831413122818447359594527400194675274060458)


class PointDecodeError(ValueError):
    pass


def is_on_curve(pt):
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (A * x * x + y * y - 1 - D * x * x % P * y * y) % P == 0


def add(p1, p2):
    """the complete affine addition: (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2)"""
    (x1, y1), (x2, y2) = p1, p2
    t = D * x1 % P * x2 % P * y1 % P * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + t, -1, P) % P, (y1 * y2 - A * x1 * x2) * pow(1 - t, -1, P) % P)


def neg(pt):
    return ((P - pt[0]) % P, pt[1])


def mul(k, pt):
    """[k] pt, k a non-negative integer (not reduced: the circuit multiplies by the bits it is given)"""
    k = int(k)
    if k < 0:
        raise ValueError("negative scalar")
    acc = IDENTITY
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt, k = add(pt, pt), k >> 1
    return acc


def in_prime_subgroup(pt):
    return is_on_curve(pt) and mul(ORDER, pt) == IDENTITY


def keygen(sk, base=None):
    """EncryptCircuit::keygen with the secret key given: (sk, [sk] G)"""
    sk = int(sk) % ORDER
    return sk, mul(sk, GENERATOR if base is None else base)


def _sqrt(v):
    """Tonelli-Shanks in Fr (P - 1 = 2^32 t); None for a non-residue"""
    v %= P
    if v == 0:
        return 0
    if pow(v, (P - 1) // 2, P) != 1:
        return None
    s, t = 0, P - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (P - 1) // 2, P) == 1:
        z += 1
    m, c, x, b = s, pow(z, t, P), pow(v, (t + 1) // 2, P), pow(v, t, P)
    while b != 1:
        i, b2 = 0, b
        while b2 != 1:
            b2, i = b2 * b2 % P, i + 1
        cc = pow(c, 1 << (m - i - 1), P)
        m, c, x, b = i, cc * cc % P, x * cc % P, b * cc * cc % P
    return x


def to_bytes(pt):
    """ark-serialize 0.3, compressed: x little-endian, bit 7 of the last byte set when y > -y"""
    x, y = pt
    out = bytearray(x.to_bytes(32, "little"))
    if y > P - y:
        out[31] |= 0x80
    return bytes(out)


def from_bytes(buf, check_subgroup=True):
    """the checked decode: x canonical (255 bits: only bit 7 of the last byte is a flag), y the root of (1 - a x^2) / (1 - d x^2) that the flag names, and (by default) the
    point in the prime-order subgroup.  Raises PointDecodeError."""
    buf = bytes(buf)
    if len(buf) != 32:
        raise PointDecodeError("a compressed point is 32 bytes")
    greater = bool(buf[31] & 0x80)
    x = int.from_bytes(buf, "little") & ((1 << 255) - 1)
    if x >= P:
        raise PointDecodeError("x is not canonical")
    y = _sqrt((1 - A * x * x) * pow(1 - D * x * x, -1, P))
    if y is None:
        raise PointDecodeError("not on the curve")
    if (y > P - y) != greater:
        y = (P - y) % P
    if (y > P - y) != greater:
        raise PointDecodeError("the sign flag names no root")           # y = 0
    pt = (x, y)
    if check_subgroup and mul(ORDER, pt) != IDENTITY:
        raise PointDecodeError("not in the prime-order subgroup")
    return pt
