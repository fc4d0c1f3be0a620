"""A small R1CS builder on the host and the gadgets EncryptCircuit's fixed section needs (circuits-ark/src/encryption.rs:219-251):
booleans, the complete twisted-Edwards addition, conditional select, scalar multiplication over little-endian bits, and the
Poseidon permutation / sponge hash of a poseidon.PoseidonParameters.  Python integers; no device.

  variable             an int: 0 is the constant one, i > 0 the i-th public input, -1 - j the j-th witness
  linear combination   a {variable: coefficient} dict, coefficients reduced mod p, no zero entries
  enforce(a, b, c)     appends the row <a, z> * <b, z> = <c, z>

`new_input` / `new_witness` carry a value when one is known, so one pass both lays the rows out and computes the assignment.  The rows
depend on the order of the calls alone, never on a value: no gadget looks at a value to decide what to allocate or enforce.

The layout is this module's own, not ark-r1cs-std's: proving keys made by the reference's `compile` are not interchangeable with keys
made over these matrices.  What the gadgets enforce is stated next to each."""

ONE = 0


def lc(*terms):
    """lc((var, coeff), ...) -> linear combination (coefficients not yet reduced: pass it through ConstraintSystem.norm)"""
    out = {}
    for v, c in terms:
        out[v] = out.get(v, 0) + c
    return out


class ConstraintSystem:
    def __init__(self, p):
        self.p = p
        self.input_values = [1]          # variable 0: the constant one
        self.witness_values = []
        self.rows = []                   # (a, b, c) linear combinations

    # ---- variables and linear combinations
    def new_input(self, value=None):
        self.input_values.append(None if value is None else int(value) % self.p)
        return len(self.input_values) - 1

    def new_witness(self, value=None):
        self.witness_values.append(None if value is None else int(value) % self.p)
        return -len(self.witness_values)

    @property
    def num_inputs(self):
        return len(self.input_values)

    @property
    def num_witnesses(self):
        return len(self.witness_values)

    def value_of(self, var):
        return self.input_values[var] if var >= 0 else self.witness_values[-1 - var]

    def norm(self, a):
        return {v: c % self.p for v, c in a.items() if c % self.p}

    def const(self, c):
        return self.norm({ONE: c})

    def add(self, a, b):
        out = dict(a)
        for v, c in b.items():
            out[v] = out.get(v, 0) + c
        return self.norm(out)

    def scale(self, a, k):
        return self.norm({v: c * k for v, c in a.items()})

    def sub(self, a, b):
        return self.add(a, self.scale(b, -1))

    @staticmethod
    def is_const(a):
        return all(v == ONE for v in a)

    def eval(self, a):
        """the value of a linear combination, None while a variable of it has none"""
        acc = 0
        for v, c in a.items():
            x = self.value_of(v)
            if x is None:
                return None
            acc += c * x
        return acc % self.p

    def enforce(self, a, b, c):
        self.rows.append((self.norm(a), self.norm(b), self.norm(c)))

    def is_satisfied(self):
        """the first row that does not hold, None when all do (needs every value)"""
        for i, (a, b, c) in enumerate(self.rows):
            if self.eval(a) * self.eval(b) % self.p != self.eval(c):
                return i
        return None

    # ---- products and quotients as fresh variables; constants fold, so a constant operand costs no row
    def mul(self, a, b):
        """-> a linear combination equal to <a, z> <b, z>: a fresh witness w with the row a * b = w, unless an operand is constant"""
        if self.is_const(a):
            return self.scale(b, a.get(ONE, 0))
        if self.is_const(b):
            return self.scale(a, b.get(ONE, 0))
        va, vb = self.eval(a), self.eval(b)
        w = self.new_witness(None if va is None or vb is None else va * vb)
        self.enforce(a, b, {w: 1})
        return {w: 1}

    def div(self, num, den):
        """-> num / den: a fresh witness q with the row q * den = num.  The caller guarantees den != 0 for every valid witness."""
        if self.is_const(num) and self.is_const(den):
            return self.const(num.get(ONE, 0) * pow(den[ONE], -1, self.p))
        vn, vd = self.eval(num), self.eval(den)
        q = self.new_witness(None if vn is None or vd is None else vn * pow(vd, -1, self.p))
        self.enforce({q: 1}, den, num)
        return {q: 1}

    # ---- CSR
    def csr(self, column_of, mont):
        """the three matrices as (row_ptr, cols, coefficient words) lists; column_of: variable -> column, mont: integer -> 4 u64 words"""
        out = []
        for side in range(3):
            row_ptr, cols, vals = [0], [], []
            for row in self.rows:
                for v, c in row[side].items():
                    cols.append(column_of(v))
                    vals.append(mont(c))
                row_ptr.append(len(cols))
            out.append((row_ptr, cols, vals))
        return out


# ---------------------------------------------------------------- gadgets
def boolean(cs, value=None):
    """a witness b with b (1 - b) = 0"""
    b = cs.new_witness(value)
    cs.enforce({b: 1}, {ONE: 1, b: -1}, {})
    return b


def te_add(cs, d, p1, p2):
    """The complete addition on a twisted Edwards curve with a = -1; points are pairs of linear combinations.
        U = (x1 + y1)(x2 + y2)   A = y2 x1   B = x2 y1   C = d A B   x3 (1 + C) = A + B   y3 (1 - C) = U - A - B
    (y1 y2 + x1 x2 = U - A - B).  6 rows for two variable points, 3 when one of them is constant, none for two constants.  With a
    non-square d the denominators never vanish on curve points."""
    (x1, y1), (x2, y2) = p1, p2
    u = cs.mul(cs.add(x1, y1), cs.add(x2, y2))
    a = cs.mul(y2, x1)
    b = cs.mul(x2, y1)
    c = cs.mul(cs.scale(a, d), b)
    one = cs.const(1)
    x3 = cs.div(cs.add(a, b), cs.add(one, c))
    y3 = cs.div(cs.sub(cs.sub(u, a), b), cs.sub(one, c))
    return x3, y3


def on_curve(cs, d, pt):
    """x^2 = xx, y^2 = yy, (d xx) yy = yy - xx - 1   (a = -1)"""
    x, y = pt
    xx, yy = cs.mul(x, x), cs.mul(y, y)
    cs.enforce(cs.scale(xx, d), yy, cs.sub(cs.sub(yy, xx), cs.const(1)))


def select(cs, bit, if_true, if_false):
    """-> bit ? if_true : if_false on one linear combination, as a fresh variable `out` with the row bit (t - f) = out - f (so that what
    is selected over and over, like a running sum, stays one term); linear, without a row, when t - f is constant"""
    diff = cs.sub(if_true, if_false)
    if cs.is_const(diff):
        return cs.add(if_false, cs.scale({bit: 1}, diff.get(ONE, 0)))
    vb, vt, vf = cs.value_of(bit), cs.eval(if_true), cs.eval(if_false)
    out = cs.new_witness(None if None in (vb, vt, vf) else (vt if vb else vf))
    cs.enforce({bit: 1}, diff, cs.sub({out: 1}, if_false))
    return {out: 1}


def select_point(cs, bit, p_true, p_false):
    return select(cs, bit, p_true[0], p_false[0]), select(cs, bit, p_true[1], p_false[1])


def scalar_mul_le(cs, d, bits, base):
    """[sum bits_i 2^i] base, bits a list of boolean variables, lowest first.  base: a pair of linear combinations (a witness point:
    double, add, select per bit) or a pair of integers (a constant point: its 2^i multiples are constants, so add and select per bit)."""
    constant = isinstance(base[0], int)
    cur = (cs.const(base[0]), cs.const(base[1])) if constant else base
    identity = (cs.const(0), cs.const(1))
    acc = None
    for i, bit in enumerate(bits):
        total = cur if acc is None else te_add(cs, d, acc, cur)
        acc = select_point(cs, bit, total, identity if acc is None else acc)
        if i + 1 < len(bits):
            cur = te_add(cs, d, cur, cur)
    return acc if acc is not None else identity


def poseidon_sbox(cs, x, alpha):
    """x^alpha by the kernel's chain: square-and-multiply from the top bit down, one row per product"""
    r = x
    for b in range(alpha.bit_length() - 2, -1, -1):
        r = cs.mul(r, r)
        if (alpha >> b) & 1:
            r = cs.mul(r, x)
    return r


def poseidon_permute(cs, prm, state):
    """state: `width` linear combinations -> the permuted state.  Every S-box output is a fresh variable; the untouched elements of a
    partial round stay linear combinations (they gain one term a round)."""
    t, half = prm.width, prm.full_rounds // 2
    s = list(state)
    for i in range(prm.full_rounds + prm.partial_rounds):
        s = [cs.add(s[j], cs.const(prm.ark[i][j])) for j in range(t)]
        full = i < half or i >= half + prm.partial_rounds
        s = [poseidon_sbox(cs, s[j], prm.alpha) if (full or j == 0) else s[j] for j in range(t)]
        nxt = []
        for j in range(t):
            acc = {}
            for k in range(t):
                acc = cs.add(acc, cs.scale(s[k], prm.mds[j][k]))
            nxt.append(acc)
        s = nxt
    return s


def poseidon_hash(cs, prm, elems):
    """the library's sponge hash (poseidon.PoseidonParameters.hash) over linear combinations -> one fresh variable"""
    s = [cs.const(x) for x in prm.init]
    off = prm.rate_offset
    for blk in range(0, len(elems), prm.rate):
        for q, x in enumerate(elems[blk:blk + prm.rate]):
            s[off + q] = cs.add(s[off + q], x)
        s = poseidon_permute(cs, prm, s)
    v = cs.eval(s[off])
    out = cs.new_witness(v)
    cs.enforce(s[off], {ONE: 1}, {out: 1})
    return out
