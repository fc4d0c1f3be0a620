"""Seeded synthetic inputs of the benchmarks and tests: uniform field elements / scalars from a vectorised
splitmix64 stream with rejection sampling, and the 0/1-heavy "realistic witness" mix.  Product-side code: bench.py and the
tools use it directly, tests import it from here."""
import numpy as np

from . import FIELD_NAMES, field_modulus

# scalar field of each curve (zk_curve_scalar_field)
CURVE_SCALAR_FIELD = {"Pallas": "PallasFq", "Vesta": "PallasFp", "Bn254G1": "Bn254Fr", "Bn254G2": "Bn254Fr",
                      "Bls381G1": "Bls381Fr", "Bls381G2": "Bls381Fr"}
_moduli = {}


def modulus(field):
    if field not in _moduli:
        assert field in FIELD_NAMES, field
        _moduli[field] = field_modulus(field)
    return _moduli[field]


def rand_field(name, n, seed):
    """n uniform elements of the field (as stored words: read them as Montgomery residues or as canonical integers),
    uint64 [n, 4]"""
    p = modulus(name)
    out = np.zeros((n, 4), dtype=np.uint64)
    todo = np.arange(n)
    top_mask = np.uint64((1 << (p.bit_length() - 192)) - 1)
    pl = [np.uint64((p >> (64 * i)) & 0xFFFFFFFFFFFFFFFF) for i in range(4)]
    rnd = 0
    while todo.size:
        m = todo.size
        with np.errstate(over="ignore"):
            idx = (np.arange(m * 4, dtype=np.uint64) + np.uint64(rnd * 0x1000003) * np.uint64(n * 4 + 1)
                   + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15))
            z = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        c = z.reshape(m, 4).copy()
        c[:, 3] &= top_mask
        lt = np.zeros(m, dtype=bool)
        eq = np.ones(m, dtype=bool)
        for i in (3, 2, 1, 0):
            lt |= eq & (c[:, i] < pl[i])
            eq &= c[:, i] == pl[i]
        out[todo[lt]] = c[lt]
        todo = todo[~lt]
        rnd += 1
    return out


def scalars_for(curve, n, seed, realistic=False):
    """canonical scalars [n,4] in [0, r); `realistic` = 40% zeros, 25% ones, 10% < 2^8."""
    sf = CURVE_SCALAR_FIELD[curve]
    s = rand_field(sf, n, seed)   # uniform in [0, r): read as canonical integers
    if realistic:
        u = rand_field(sf, n, seed + 1)[:, 0] % np.uint64(100)
        z, o, sm = u < 40, (u >= 40) & (u < 65), (u >= 65) & (u < 75)
        s[z] = 0
        s[o] = 0
        s[o, 0] = 1
        s[sm, 1:] = 0
        s[sm, 0] &= np.uint64(0xFF)
    return s


def quotient_program(n_adv, n_fix, n_inst=0):
    """A gate set in the style of the reference's circuit (circuits-halo2/src/encryption.rs:83-161: ECC-style multiplication
    gates, a Pow5 S-box with a rotation, boolean / range checks behind fixed selectors, the lookup and permutation argument
    constraints), folded with y: columns [0, n_adv) advice, [n_adv, n_adv + n_fix) fixed, then A', S', Z_lookup, Z_perm x3, then
    the n_inst instance columns (equality-enabled in the reference's circuit: they enter through the last permutation chunk).
    consts: [y, 5, 1, beta, gamma]"""
    A = lambda i, r=0: ("col", i % n_adv, r)
    Fx = lambda i, r=0: ("col", n_adv + i % n_fix, r)
    X = n_adv + n_fix
    I = lambda i: ("col", X + 6 + i % n_inst, 0)
    ap, sp, zl = ("col", X, 0), ("col", X + 1, 0), ("col", X + 2, 0)
    zp = [("col", X + 3 + c, 0) for c in range(3)]
    prog = []
    # every term after the first is folded in as  acc = acc * y + term
    # multiplication gates  q (a b - c), eight of them
    first = True
    for g in range(8):
        term = [Fx(g), A(g), A(g + 1), ("mul",), A(g + 2), ("sub",), ("mul",)]
        prog.extend(term if first else [("scale", 0)] + term + [("add",)])
        first = False
    # Pow5 with a rotation  q (a^5 + 5 - b(omega X)), three of them
    for g in range(3):
        a = A(3 * g + 1)
        prog.extend([("scale", 0), Fx(g + 3), a, a, ("mul",), a, ("mul",), a, ("mul",), a, ("mul",), ("const", 1), ("add",),
                     ("col", (3 * g + 2) % n_adv, 1), ("sub",), ("mul",), ("add",)])
    # boolean checks  q a (a - 1), four of them
    for g in range(4):
        a = A(g + 9)
        prog.extend([("scale", 0), Fx(g + 4), a, a, ("const", 2), ("sub",), ("mul",), ("mul",), ("add",)])
    # lookup: Z(omega X)(A' + beta)(S' + gamma) - Z(X)(A + beta)(S + gamma), and (A' - S')(A' - A'(omega^-1 X))
    prog.extend([("scale", 0), ("col", X + 2, 1), ap, ("const", 3), ("add",), ("mul",), sp, ("const", 4), ("add",), ("mul",),
                 zl, A(0), ("const", 3), ("add",), ("mul",), Fx(7), ("const", 4), ("add",), ("mul",), ("sub",), ("add",)])
    prog.extend([("scale", 0), ap, sp, ("sub",), ap, ("col", X, -1), ("sub",), ("mul",), ("add",)])
    # permutation, per chunk: Z(omega X) prod (v + beta s + gamma) - Z(X) prod (v + delta-term + gamma), two columns of each chunk written out
    for c in range(3):
        v0, v1 = (I(0), I(1)) if (n_inst and c == 2) else (A(2 * c), A(2 * c + 1))
        prog.extend([("scale", 0), ("col", X + 3 + c, 1), v0, Fx(c), ("scale", 3), ("add",), ("const", 4), ("add",), ("mul",),
                     v1, Fx(c + 1), ("scale", 3), ("add",), ("const", 4), ("add",), ("mul",),
                     zp[c], v0, ("const", 4), ("add",), ("mul",), v1, ("const", 3), ("add",), ("mul",), ("sub",), ("add",)])
    return prog


def rotated_advice(n_adv):
    """the advice columns quotient_program reads at the next row (the Pow5 gates): they are opened at x AND omega x"""
    return sorted({(3 * g + 2) % n_adv for g in range(3)})


def _limbs_to_ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).astype(object)
    return a[:, 0] + (a[:, 1] << 64) + (a[:, 2] << 128) + (a[:, 3] << 192)


def _ints_to_limbs(v):
    return np.stack([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], axis=1).astype(np.uint64)


def satisfied_circuit(field, k, n_adv=13, n_fix=8, n_inst=3, blinding_factors=5, seed=1):
    """A synthetic circuit WITH a witness that satisfies it, for halo2.MockProver: the gate families of quotient_program as
    separate programs -- q (a b - c), q (a^5 + 5 - b(omega X)), q a (a - 1) -- one lookup shaped like the reference's
    LookupRangeCheckConfig (one selector-gated advice expression into one table column), and copy constraints between two advice
    columns and the instance columns.  Rows go in fours: a multiplication row, a Pow5 row, the row after it (no gate: the cell the
    Pow5 gate determines stays free; the lookup is switched on here), a boolean row; every family's selectors take turns.  No
    selector is set in the blinding rows, and none on a Pow5 row whose next row is not usable.  All arithmetic is on the stored
    (Montgomery) words -- a stored product is a b / R -- so only the computed cells pass through Python integers: k = 20 takes
    seconds.  Fixed columns: [0, n_mul) multiplication selectors, then the Pow5 selectors, the boolean selector, the lookup
    selector (n_fix - 2) and the table (n_fix - 1).

    Returns a dict: field, k, blinding_factors, usable, advice [n_adv, n, 4] / fixed [n_fix, n, 4] (host, Montgomery), instance (a
    list of [m, 4] Montgomery arrays), consts, gates [(name, [program]), ...], lookups [([input], [table])], permutation_columns
    (flat indices), copies [count, 4] (columns as positions in permutation_columns), assembly (halo2.Assembly with the copies
    applied) and rows: the rows of each family {"mul", "pow5", "bool", "lookup"} with the family member enabled there."""
    assert n_adv >= 12 and n_fix >= 6 and n_inst >= 0
    n = 1 << k
    if n < blinding_factors + 3:
        raise ValueError("NotEnoughRowsAvailable: n = %d < blinding_factors + 3 = %d" % (n, blinding_factors + 3))
    usable = n - (blinding_factors + 1)
    p = modulus(field)
    R = (1 << 256) % p
    r_inv = pow(R, -1, p)
    n_pow = 2 if n_fix >= 8 else 1
    n_mul = n_fix - 3 - n_pow
    f_pow, f_bool, f_lk, f_tab = n_mul, n_mul + n_pow, n_fix - 2, n_fix - 1
    advice = np.zeros((n_adv, n, 4), dtype=np.uint64)
    fixed = np.zeros((n_fix, n, 4), dtype=np.uint64)
    one = _ints_to_limbs(np.array([R], dtype=object))[0]
    for c in range(n_adv):                       # blinding rows: random, like a prover's
        advice[c, usable:] = rand_field(field, n - usable, seed * 1000 + c)
    rows = np.arange(usable)
    quad = rows // 4
    mul_rows, pow_rows, free_rows, bool_rows = rows[rows % 4 == 0], rows[rows % 4 == 1], rows[rows % 4 == 2], rows[rows % 4 == 3]
    pow_rows = pow_rows[pow_rows + 1 < usable]
    free_rows = free_rows[:len(pow_rows)] if len(free_rows) > len(pow_rows) else free_rows
    # multiplication gates: c = a b
    g_mul = quad[mul_rows] % n_mul
    a_st, b_st = rand_field(field, len(mul_rows), seed * 1000 + 101), rand_field(field, len(mul_rows), seed * 1000 + 102)
    c_st = _ints_to_limbs(_limbs_to_ints(a_st) * _limbs_to_ints(b_st) * r_inv % p) if len(mul_rows) else a_st
    for g in range(n_mul):
        m = g_mul == g
        advice[g, mul_rows[m]], advice[g + 1, mul_rows[m]], advice[g + 2, mul_rows[m]] = a_st[m], b_st[m], c_st[m]
        fixed[g, mul_rows[m]] = one
    # Pow5: b(next row) = a^5 + 5
    g_pow = quad[pow_rows] % n_pow
    x_st = rand_field(field, len(pow_rows), seed * 1000 + 103)
    if len(pow_rows):
        xi = _limbs_to_ints(x_st)
        y_st = _ints_to_limbs((xi ** 5 * pow(r_inv, 4, p) + 5 * R) % p)
    for g in range(n_pow):
        m = g_pow == g
        advice[3 * g + 1, pow_rows[m]] = x_st[m]
        advice[3 * g + 2, pow_rows[m] + 1] = y_st[m] if len(pow_rows) else 0
        fixed[f_pow + g, pow_rows[m]] = one
    # boolean checks: a in {0, 1}
    bits = rand_field(field, len(bool_rows), seed * 1000 + 104)[:, 0] & np.uint64(1)
    advice[9, bool_rows[bits == 1]] = one
    fixed[f_bool, bool_rows] = one
    # the range-check lookup: q a into the table 0 .. T - 1, on the free rows
    T = min(usable, 1 << 10)
    fixed[f_tab, :T] = _ints_to_limbs(np.arange(T).astype(object) * R % p)
    small = rand_field(field, len(free_rows), seed * 1000 + 105)[:, 0] % np.uint64(T)
    advice[0, free_rows] = fixed[f_tab][small.astype(np.int64)]
    fixed[f_lk, free_rows] = one
    # copies: (x, 2 t) = (y, 2 t + 1) between the two last advice columns; the first cells of every instance column into x
    cx, cy = n_adv - 2, n_adv - 1
    t = np.arange(usable // 2)
    v = rand_field(field, len(t), seed * 1000 + 106)
    advice[cx, 2 * t], advice[cy, 2 * t + 1] = v, v
    copies = [np.stack([np.zeros_like(t), 2 * t, np.ones_like(t), 2 * t + 1], axis=1)]
    m_inst = min(usable // 2, 4)
    instance = []
    for i in range(n_inst):
        r_i = 2 * np.arange(m_inst) + 1            # odd rows of x are otherwise unconstrained
        vals = rand_field(field, m_inst, seed * 1000 + 110 + i)
        if i == 0:
            advice[cx, r_i] = vals
            copies.append(np.stack([np.full(m_inst, 2), np.arange(m_inst), np.zeros(m_inst, dtype=np.int64), r_i], axis=1))
        else:                                       # further instance columns repeat the first one's cells: longer cycles
            vals = instance[0]
            copies.append(np.stack([np.full(m_inst, 2 + i), np.arange(m_inst), np.full(m_inst, 2), np.arange(m_inst)], axis=1))
        instance.append(vals)
    copies = np.concatenate(copies).astype(np.uint32)
    A = lambda i, r=0: ("col", i, r)
    Fx = lambda i: ("col", n_adv + i, 0)
    gates = []
    for g in range(n_mul):
        gates.append(("mul %d" % g, [[Fx(g), A(g), A(g + 1), ("mul",), A(g + 2), ("sub",), ("mul",)]]))
    for g in range(n_pow):
        a = A(3 * g + 1)
        gates.append(("pow5 %d" % g, [[Fx(f_pow + g), a, a, ("mul",), a, ("mul",), a, ("mul",), a, ("mul",), ("const", 0), ("add",),
                                       A(3 * g + 2, 1), ("sub",), ("mul",)]]))
    gates.append(("bool", [[Fx(f_bool), A(9), A(9), ("const", 1), ("sub",), ("mul",), ("mul",)]]))
    lookups = [([[Fx(f_lk), A(0), ("mul",)]], [[Fx(f_tab)]])]
    consts = _ints_to_limbs(np.array([5 * R % p, R], dtype=object))
    from . import halo2
    perm_cols = [cx, cy] + [n_adv + n_fix + i for i in range(n_inst)]
    asm = halo2.Assembly(n, len(perm_cols))
    asm.copy_many(copies)
    return {"field": field, "k": k, "blinding_factors": blinding_factors, "usable": usable, "advice": advice, "fixed": fixed, "instance": instance,
            "consts": consts, "gates": gates, "lookups": lookups, "permutation_columns": perm_cols, "copies": copies, "assembly": asm,
            "rows": {"mul": (mul_rows, g_mul), "pow5": (pow_rows, g_pow), "bool": (bool_rows, None), "lookup": (free_rows, None)}}


def mock_prover(circuit, stream=0):
    """halo2.MockProver over a satisfied_circuit (or an edited copy of one): uploads the columns"""
    from . import halo2
    from .groth16 import _upload
    return halo2.MockProver(circuit["field"], circuit["k"], circuit["blinding_factors"], _upload(circuit["advice"]), _upload(circuit["fixed"]),
                            instance=circuit["instance"], gates=circuit["gates"], lookups=circuit["lookups"],
                            permutation=(circuit["permutation_columns"], circuit["assembly"]), consts=circuit["consts"], stream=stream)
