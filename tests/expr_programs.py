"""TEST INFRASTRUCTURE: a seeded corpus of quotient-evaluator programs (zk_expr_eval_device, zk_expr_eval_lazy_device and the kernel
generated per program) and their inputs, with the expected outputs from oracle/pyref_halo2.eval_program on Python integers.

Programs are in the Python mirror's tuple form: ("col", column, rotation) ("const", i) ("add",) ("sub",) ("mul",) ("neg",)
("scale", i).  Every family is built on purpose to reach one part of the host code that depends on the program's shape
(contangle-zkcp_amd/csrc/zk_poly.inl: expr_compile29, expr_jit_source):
  gate      selector x polynomial gates with rotations, folded with ("scale", 0) by y (the shape of synth.quotient_program)
  bound     long addition chains (carry steps: NORM; values past 256 p: REFRESH), subtractions / negations of sums of growing size
            (every bias table), products and scalings of values that were never normalised, neg of neg
  slot      more (column, rotation) pairs than slots, reuse distances on both sides of the 12-op load hoisting window, one column
            at several rotations, a slot reloaded right after its last use
  limit     stack depth exactly EXPR_STACK, EXPR_MAX_OPS ops, all 64 columns and 32 constants, one-op programs, no column at all
  rot       rotations 0, +-1, +-(n - 1), +-32767; a rot_scale whose products wrap the domain several times; sub-coset scales

Inputs are STORED WORDS (canonical, < p): random words, the extremes p - 1, 0, 1, words just below p (p - 2, and the densest one:
every limb below the top one 2^29 - 1), rows alternating between extremes.  A stored word w stands for x = w / R mod p with
R = 2^261 on the lazy-limb paths and R = 2^256 on the saturated one: the words are written directly, not through a conversion,
so that the extremes reach the kernels."""
import random

import numpy as np

from oracle import pyref
from oracle import pyref_halo2 as h2

EXPR_STACK, EXPR_MAX_OPS, EXPR_MAX_COLS, EXPR_MAX_CONSTS = 8, 512, 64, 32      # zk_poly_kernels.h
FIELDS = ["PallasFp", "PallasFq", "Bn254Fr", "Bls381Fr"]
R_LAZY, R_MONT = 1 << 261, 1 << 256


class Program:
    def __init__(self, name, family, ops, n_cols, n_consts, rot_scale=1):
        self.name, self.family, self.ops, self.n_cols, self.n_consts, self.rot_scale = name, family, ops, n_cols, n_consts, rot_scale

    def __repr__(self):
        return "Program(%s, %d ops)" % (self.name, len(self.ops))


def depth(ops):
    """the largest stack the program builds; None if it is not a valid program (underflow, or not exactly one value left)"""
    d = best = 0
    for o in ops:
        if o[0] in ("col", "const"):
            d += 1
        elif o[0] in ("neg", "scale"):
            if d < 1:
                return None
        else:
            if d < 2:
                return None
            d -= 1
        best = max(best, d)
    return best if d == 1 else None


def _fold(terms):
    """acc = term_0; acc = acc * y + term_k  (y = constant 0)"""
    out = list(terms[0])
    for t in terms[1:]:
        out += [("scale", 0)] + list(t) + [("add",)]
    return out


# ------------------------------------------------------------------------------------------------------------ families
def _gate(rng, n_cols, n_consts, n_gates, rots=(0, 0, 0, 1, -1, 2, -3)):
    C = lambda: ("col", rng.randrange(n_cols), rng.choice(rots))
    K = lambda: ("const", rng.randrange(1, n_consts))
    terms = []
    for _ in range(n_gates):
        kind = rng.randrange(5)
        q = ("col", rng.randrange(n_cols), 0)
        if kind == 0:                                   # q (a b - c)
            terms.append([q, C(), C(), ("mul",), C(), ("sub",), ("mul",)])
        elif kind == 1:                                 # q (a^5 + k - b(omega X))
            a = C()
            terms.append([q, a, a, ("mul",), a, ("mul",), a, ("mul",), a, ("mul",), K(), ("add",), ("col", rng.randrange(n_cols), 1), ("sub",), ("mul",)])
        elif kind == 2:                                 # q a (a - 1)
            a = C()
            terms.append([q, a, a, K(), ("sub",), ("mul",), ("mul",)])
        elif kind == 3:                                 # Z(omega X)(a + beta)(s + gamma) - Z(X)(b + beta)(t + gamma)
            z = rng.randrange(n_cols)
            terms.append([("col", z, 1), C(), K(), ("add",), ("mul",), C(), K(), ("add",), ("mul",),
                          ("col", z, 0), C(), K(), ("add",), ("mul",), C(), ("scale", rng.randrange(n_consts)), K(), ("add",), ("mul",), ("sub",)])
        else:                                           # -q (a - b(omega^-1 X)) + c
            terms.append([q, C(), ("col", rng.randrange(n_cols), -1), ("sub",), ("mul",), ("neg",), C(), ("add",)])
    return _fold(terms)


def _add_chain(n_loads, n_cols, rot=0):
    ops = [("col", 0, rot)]
    for k in range(1, n_loads):
        ops += [("col", k % n_cols, rot if k % 3 else -rot), ("add",)]
    return ops


def _sum(cols):
    ops = [cols[0]]
    for c in cols[1:]:
        ops += [c, ("add",)]
    return ops


def _bias_ladder(rng, n_cols):
    """a - (sum of s loads) and -(sum of s loads) for s = 1 .. 9, and products / scalings of the unnormalised sums: the operand
    bounds walk through every bias table (and past them: a carry step or a contraction first)"""
    C = lambda: ("col", rng.randrange(n_cols), rng.choice((0, 1, -1)))
    terms = []
    for s in range(1, 10):
        terms.append([C()] + _sum([C() for _ in range(s)]) + [("sub",)])
        terms.append(_sum([C() for _ in range(s)]) + [("neg",)])
    prog = []
    for t in terms:
        prog = t if not prog else prog + t + [("add",)]
    return prog


def _unnormalised_products(rng, n_cols):
    C = lambda: ("col", rng.randrange(n_cols), 0)
    prog = _sum([C() for _ in range(7)]) + _sum([C() for _ in range(7)]) + [("mul",)]          # both factors carry 7 loads
    prog += _sum([C() for _ in range(12)]) + [("scale", 1), ("mul",)]                           # scale of an unnormalised sum
    prog += [C(), ("neg",), ("neg",), ("neg",), ("neg",), ("neg",), ("add",)]                  # neg of neg ...
    prog += _sum([C() for _ in range(5)]) + [("neg",), ("neg",), ("mul",)]
    prog += [C(), C(), ("sub",), C(), ("sub",), C(), ("sub",), ("neg",), ("scale", 2), ("sub",)]
    return prog


def _carry_before_bias():
    """a difference whose subtrahend is zero keeps the bias in its limbs (a + BIAS4K1, limbs up to 3 2^29): negating it needs a
    carry step first.  Columns 3 and 4 are, in the "mixed" inputs, rows alternating dense / 1 and the constant 0"""
    a, z = ("col", 3, 0), ("col", 4, 0)
    return [a, z, ("sub",), ("neg",), ("col", 3, 1), z, ("sub",), ("col", 2, 0), ("sub",), ("neg",), ("mul",),
            a, z, ("sub",), ("col", 3, -1), ("sub",), ("neg",), ("add",)]


def _slot_pool(rng, n_ops_target, pairs):
    """a random walk over a pool of (column, rotation) pairs: with more pairs than slots every slot is evicted; pushes interleave
    with products / sums so that reuse distances straddle the 12-op hoisting window"""
    prog = [("col",) + rng.choice(pairs)]
    d = 1
    while len(prog) < n_ops_target or d > 1:
        if d < 2 or (d < EXPR_STACK and rng.random() < 0.45 and len(prog) < n_ops_target):
            prog.append(("col",) + rng.choice(pairs))
            d += 1
        else:
            prog.append((rng.choice(("add", "sub", "mul", "mul")),))
            d -= 1
    return prog


def _reuse_distances(n_cols):
    """the pair (0, 0) read again after gaps of g other ops, g = 2 .. 20 (the hoisting window is 12 words)"""
    prog = [("col", 0, 0)]
    other = 1
    for g in range(2, 21):
        for k in range(g // 2):
            prog += [("col", other % n_cols, (k % 3) - 1), ("mul",) if k % 2 else ("add",)]
            other += 1
        prog += [("col", 0, 0), ("sub",)]
    return prog


def _rotations_of_one_column(n):
    rots = [0, 1, -1, 2, -2, 3, n - 1, -(n - 1), 32767, -32767, -32768]
    prog = [("col", 1, rots[0])]
    for r in rots[1:]:
        prog += [("col", 1, r), ("mul",), ("col", 0, r), ("add",)]
    return prog


def _reload_right_after(n_cols):
    """alternating pairs so that the farthest-next-use victim is the slot just used (1 .. 4 slots all thrash)"""
    seq = [(c % n_cols, r) for c, r in ((0, 0), (1, 0), (2, 1), (0, 0), (3, 0), (4, -1), (1, 0), (2, 1), (5, 0), (0, 0), (6, 0), (3, 0))]
    prog = [("col",) + seq[0]]
    for k, pr in enumerate(seq[1:] * 3):
        prog += [("col",) + pr, ("add",) if k % 3 else ("mul",)]
    return prog


def _depth8(rng, n_cols):
    a = [("col", rng.randrange(n_cols), rng.choice((0, 1, -1))) for _ in range(8)]
    # 8 values on the stack at once, then folded back with every binary op
    return a + [("mul",), ("sub",), ("add",), ("mul",), ("neg",), ("sub",), ("mul",), ("add",)]


def _max_ops(rng, n_cols):
    """exactly EXPR_MAX_OPS ops (its annotated form stays within 2 * EXPR_MAX_OPS words)"""
    pairs = [(c, r) for c in range(min(n_cols, 6)) for r in (0, 1)]
    prog = [("col",) + pairs[0]]
    k = 0
    while len(prog) < EXPR_MAX_OPS - 1:
        prog += [("col",) + rng.choice(pairs), (("add",), ("mul",), ("sub",), ("mul",))[k % 4]]
        k += 1
    prog += [("neg",)] * (EXPR_MAX_OPS - len(prog))
    assert len(prog) == EXPR_MAX_OPS
    return prog


def _all_columns_and_constants():
    prog = [("col", 0, 0)]
    for c in range(1, EXPR_MAX_COLS):
        prog += [("col", c, (c % 5) - 2), ("mul",) if c % 2 else ("add",)]
        if c % 2 == 0:
            prog += [("scale", (c // 2) % EXPR_MAX_CONSTS)]
    for j in range(EXPR_MAX_CONSTS):
        prog += [("const", j), ("sub",) if j % 2 else ("mul",)]
    return prog


def corpus(log_n, seed=0xC0DE):
    """the programs for an extended domain of 2^log_n rows (the rotations +-(n - 1) depend on it); deterministic from the seed"""
    n = 1 << log_n
    rng = random.Random(seed * 1009 + log_n)
    P = []
    for g in range(3):
        nc = (6, 12, 24)[g]
        P.append(Program("gate%d" % g, "gate", _gate(rng, nc, 5, (4, 9, 16)[g]), nc, 5, rot_scale=(1, 2, 4)[g]))
    P.append(Program("add_chain_140", "bound", _add_chain(140, 7), 7, 1))
    P.append(Program("add_chain_40_rot", "bound", _add_chain(40, 5, rot=1) + [("col", 5, 0), ("mul",)], 6, 1, rot_scale=8))
    P.append(Program("bias_ladder", "bound", _bias_ladder(rng, 10), 10, 1))
    P.append(Program("unnormalised", "bound", _unnormalised_products(rng, 9), 9, 3))
    P.append(Program("carry_before_bias", "bound", _carry_before_bias(), 5, 1))
    P.append(Program("slot_pool_5", "slot", _slot_pool(rng, 120, [(c, r) for c in range(3) for r in (0, 1)][:5]), 3, 1))
    P.append(Program("slot_pool_12", "slot", _slot_pool(rng, 200, [(c, r) for c in range(6) for r in (0, -1)]), 6, 1, rot_scale=2))
    P.append(Program("reuse_distances", "slot", _reuse_distances(9), 9, 1))
    P.append(Program("one_column_rotations", "rot", _rotations_of_one_column(n), 2, 1))
    P.append(Program("reload_right_after", "slot", _reload_right_after(7), 7, 1))
    P.append(Program("depth8", "limit", _depth8(rng, 8), 8, 1))
    P.append(Program("max_ops", "limit", _max_ops(rng, 6), 6, 1))
    P.append(Program("all_cols_consts", "limit", _all_columns_and_constants(), EXPR_MAX_COLS, EXPR_MAX_CONSTS))
    P.append(Program("one_col", "limit", [("col", 0, -1)], 1, 1))
    P.append(Program("one_const", "limit", [("const", 0)], 1, 1))
    P.append(Program("no_column", "limit", [("const", 0), ("const", 1), ("mul",), ("const", 2), ("sub",), ("scale", 0), ("neg",)], 0, 3))
    P.append(Program("rot_wrap", "rot", [("col", 0, 1), ("col", 1, -5), ("mul",), ("col", 0, 32767), ("sub",), ("col", 1, -32767), ("add",)], 2, 1,
                     rot_scale=3 * n + 1))
    for s in (1, 2, 4, 8):                               # one sub-coset of a 1 / 2 / 4 / 8-way sharded quotient
        P.append(Program("subcoset_%d" % s, "rot", _gate(rng, 5, 3, 3, rots=(0, 1, -1, n - 1, -(n - 1))), 5, 3, rot_scale=s))
    for p in P:
        assert depth(p.ops) is not None and depth(p.ops) <= EXPR_STACK and len(p.ops) <= EXPR_MAX_OPS, p
    assert len({tuple(p.ops) for p in P}) == len(P)
    return P


# ------------------------------------------------------------------------------------------------------------ inputs
def extremes(field):
    """stored words at the edges: 0, 1, p - 1, p - 2, and the densest word below p (every limb under the top one 2^29 - 1)"""
    p = pyref.FIELDS[field][0]
    dense = ((p >> 232) << 232) - 1
    assert dense < p and all((dense >> (29 * i)) & (2 ** 29 - 1) == 2 ** 29 - 1 for i in range(8))
    return [0, 1, p - 1, p - 2, dense]


def input_words(field, prog, n, kind, seed=1):
    """(columns, constants) as stored words.  kind "mixed": per column one of -- a per-row pick among random words and the
    extremes, random words, rows alternating p - 1 / 0 or dense / 1, one extreme in every row; kind "dense": every column
    the densest word below p, alternating with p - 1 every third row (the largest limbs the lazy paths can be given)"""
    p = pyref.FIELDS[field][0]
    ex = extremes(field)
    rng = random.Random(seed * 7919 + n + len(prog.ops))
    cols = []
    for c in range(prog.n_cols):
        if kind == "dense":
            cols.append([ex[2] if i % 3 == 2 else ex[4] for i in range(n)])
            continue
        m = c % 5
        if m == 0:
            cols.append([rng.choice(ex) if rng.random() < 0.5 else rng.randrange(p) for _ in range(n)])
        elif m == 1:
            cols.append([rng.randrange(p) for _ in range(n)])
        elif m == 2:
            cols.append([(ex[2], ex[0]) [i % 2] for i in range(n)])
        elif m == 3:
            cols.append([(ex[4], ex[1]) [i % 2] for i in range(n)])
        else:
            cols.append([ex[(c // 5) % len(ex)]] * n)
    consts = [(ex[4], ex[2], rng.randrange(p), ex[1], ex[3], ex[0])[j % 6] if kind == "dense" or j % 2 else rng.randrange(p)
              for j in range(prog.n_consts)]
    return cols, consts


def expected(field, prog, cols, consts, n, radix, rows=None):
    """eval_program on the values behind the stored words (x = w / radix), as the canonical Montgomery words x 2^256 mod p the
    evaluators return: uint64 [len(rows), 4]"""
    p = pyref.FIELDS[field][0]
    inv = pow(radix, -1, p)
    xc = [[w * inv % p for w in col] for col in cols]
    xk = [w * inv % p for w in consts]
    rows = range(n) if rows is None else rows
    vals = [h2.eval_program(field, prog.ops, xc, xk, n, prog.rot_scale, i) * R_MONT % p for i in rows]
    return words_array(vals)


def words_array(ints):
    m = (1 << 64) - 1
    return np.array([[(v >> (64 * k)) & m for k in range(4)] for v in ints], dtype=np.uint64).reshape(-1, 4)


def mont_words_for_lazy_consts(field, consts):
    """zk_expr_eval_lazy_device takes its constants in the usual Montgomery form and doubles them 5 times (x R -> x R'): the
    words that become the given stored words there"""
    p = pyref.FIELDS[field][0]
    return words_array([w * pow(32, -1, p) % p for w in consts])
