"""TEST INFRASTRUCTURE shared by tests/test_poseidon_emu.py (CPU tier: emulator build, and the host twin without any device) and
tests/test_poseidon_gpu.py (-m gpu): the Poseidon permutation and sponge, the Merkle tree over it, its paths, and the ElGamal c2
stream -- the nine entries through the C ABI and the zk.poseidon mirror -- against RefPoseidon / ref_tree, a restatement of
DESIGN.md section 5 "Poseidon" on Python integers that shares no code with the library.  Every comparison is exact, word for word."""
import ctypes
import functools
import itertools
import json
import os
import random

import numpy as np

from halo2_mock_cases import FIELD_IDS, dev, host, limbs_of, modulus, mont, on_emulator, ptr, unmont, unmont_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NOT_INITIALIZED, BAD_HANDLE = -1, -2, -7
FIELDS = ["PallasFp", "PallasFq", "Bn254Fr", "Bls381Fr"]
WG, GRID, TAIL_LOG, PATHS_PER_LAUNCH = 256, 1024, 8, 256      # csrc/zk_poseidon_kernels.h
TRIP = WG * GRID                                              # lanes of one trip of the grid-stride loop
COUNTS = [1, 63, 64, 65, 255, 256, 257]

# computed with a separate prototype from the reference's constants reduced mod r (BLS12-381 Fr); canonical hex
PIN_PERMUTE_012 = ["70d4d604ff545c4f10d6eadaf0b5c244ac623db27297a49c05a4d2d7ede6b80a",
                   "17b550b5ea92e95d8d7ff4a8c9b270f67f759cd8d26467a31a9475df6d7034b5",
                   "07a396c1fd912582fdc6cb8320caaa5562520db5ef99d980af04965df267a0fb"]
PIN_HASH_0 = "259a29adaf36d7d9a5e23ea964c3900afe4d78e7934379a2323e67c3a20450dd"
PIN_HASH_567 = "4dfb6e6a62d61b3cf059936676651ed0baebcb7ff6ec16e4d5b3b8b248ff9942"
PIN_ROOT_4 = "201c1b33f2bcaa43bbfcdb994ec4dcc3832a4b8ca4822e056d2e9559470203d9"
PIN_ROOT_1024 = "030fe89d9db5f171ac92a7277cf130d7a7f47b5b0c56cfafc57c784eb0cae468"


# ---------------------------------------------------------------- the restatement
class RefPoseidon:
    """The permutation and the sponge hash as the issue text states them, on Python integers."""

    def __init__(self, p, rate, rate_offset, full_rounds, partial_rounds, alpha, ark, mds, init=None):
        self.p, self.t, self.rate, self.rate_offset = p, len(mds), rate, rate_offset
        self.rf, self.rp, self.alpha = full_rounds, partial_rounds, alpha
        self.ark = [[int(x) % p for x in row] for row in ark]
        self.mds = [[int(x) % p for x in row] for row in mds]
        self.init = [int(x) % p for x in init] if init is not None else [0] * self.t
        assert rate >= 1 and rate_offset + rate <= self.t and full_rounds % 2 == 0 and len(self.ark) == full_rounds + partial_rounds
        self._memo = {}

    def permute(self, state):
        p, t = self.p, self.t
        s = [int(x) % p for x in state]
        assert len(s) == t
        for i in range(self.rf + self.rp):
            s = [(s[j] + self.ark[i][j]) % p for j in range(t)]
            if i < self.rf // 2 or i >= self.rf // 2 + self.rp:
                s = [pow(x, self.alpha, p) for x in s]
            else:
                s[0] = pow(s[0], self.alpha, p)
            s = [sum(self.mds[j][k] * s[k] for k in range(t)) % p for j in range(t)]
        return s

    def hash(self, elems):
        key = tuple(int(x) % self.p for x in elems)
        if key not in self._memo:
            assert len(key) >= 1
            s, r, off = list(self.init), self.rate, self.rate_offset
            for b in range(0, len(key), r):
                for q, x in enumerate(key[b:b + r]):
                    s[off + q] = (s[off + q] + x) % self.p
                s = self.permute(s)
            self._memo[key] = s[off]
        return self._memo[key]


def ref_tree(ref, leaves):
    """leaves: n = 2^log_n lists of elements -> the 2n - 1 nodes in the library's layout: level 0 (the leaf digests), then every
    level behind the one below, the root last"""
    level = [ref.hash(x) for x in leaves]
    assert len(level) >= 2 and len(level) & (len(level) - 1) == 0
    nodes = list(level)
    while len(level) > 1:
        level = [ref.hash([level[2 * i], level[2 * i + 1]]) for i in range(len(level) // 2)]
        nodes += level
    return nodes


def level_offset(log_n, j):
    return (2 << log_n) - (2 << (log_n - j))


# ---------------------------------------------------------------- parameter sets
def reference_constants():
    with open(os.path.join(ROOT, "tests", "golden", "poseidon_bls12_377_rate2.json")) as f:
        d = json.load(f)
    assert d["width"] == 3 and d["rate"] == 2 and len(d["ark"]) == d["full_rounds"] + d["partial_rounds"] == 39 and len(d["mds"]) == 3
    p = modulus("Bls381Fr")
    # the decimal strings are 377-bit: ark-ff 0.3 from_str accumulates the digits in the field, i.e. takes them mod r
    return d, [[int(x) % p for x in row] for row in d["ark"]], [[int(x) % p for x in row] for row in d["mds"]]


# name: (field, width, rate, capacity_first, full_rounds, partial_rounds, alpha, how the constants are drawn, init)
#   capacity_first with no init is ark-sponge 0.3's layout; rate first with init[2] = 2 * 2^64 is halo2_gadgets' ConstantLength<2>
PSETS = {
    "reference": ("Bls381Fr", 3, 2, True, 8, 31, 17, "reference", None),
    "pallas_fp_a5": ("PallasFp", 3, 2, False, 8, 56, 5, "uniform", [0, 0, 2 << 64]),      # the shape of P128Pow5T3, seeded constants
    "pallas_fq_a3": ("PallasFq", 3, 2, True, 8, 1, 3, "uniform", None),
    "bn254_a7": ("Bn254Fr", 3, 2, True, 2, 31, 7, "uniform", None),
    "bls381_a17_rp0": ("Bls381Fr", 3, 2, False, 8, 0, 17, "uniform", [0, 0, 2 << 64]),
    "t2_a2": ("PallasFp", 2, 1, True, 2, 1, 2, "uniform", None),
    "t4_a65537": ("Bn254Fr", 4, 3, True, 2, 0, (1 << 16) + 1, "uniform", None),
    "t5_amax": ("Bls381Fr", 5, 2, True, 2, 1, (1 << 64) - 1, "uniform", None),
    "t5_rate_first": ("PallasFq", 5, 2, False, 2, 31, 5, "uniform", [1, 2, 3, 4, 5]),
    "edge_consts": ("PallasFq", 3, 2, True, 8, 56, 5, "edge", [0, 1, -1]),
    "zero_consts": ("Bn254Fr", 3, 2, True, 2, 1, 3, "zero", None),
}
TREE_PSETS = {1: "reference", 3: "pallas_fq_a3"}      # leaf_arity -> parameter set (the second one keeps the Python side cheap)


class PSet:
    def __init__(self, name):
        self.name = name
        self.field, self.t, self.rate, self.capacity_first, self.rf, self.rp, self.alpha, kind, init = PSETS[name]
        self.p = modulus(self.field)
        self.rate_offset = self.t - self.rate if self.capacity_first else 0
        rng = random.Random("poseidon " + name)
        draw = {"uniform": lambda: rng.randrange(self.p), "edge": lambda: rng.choice([0, 1, self.p - 1]), "zero": lambda: 0}
        if kind == "reference":
            _, self.ark, self.mds = reference_constants()
        else:
            self.ark = [[draw[kind]() for _ in range(self.t)] for _ in range(self.rf + self.rp)]
            self.mds = [[draw[kind]() for _ in range(self.t)] for _ in range(self.t)]
        self.init = [x % self.p for x in init] if init is not None else None
        self.ref = RefPoseidon(self.p, self.rate, self.rate_offset, self.rf, self.rp, self.alpha, self.ark, self.mds, self.init)

    def params(self, zk):
        """zk.poseidon.PoseidonParameters of this set on the library that is loaded now"""
        return zk.poseidon.PoseidonParameters(self.field, self.rf, self.rp, self.alpha, self.mds, self.ark, rate=self.rate,
                                              capacity_first=self.capacity_first, init=self.init)

    def elements(self, count, seed):
        """canonical integers: 0, 1, p - 1 in all orders first (the all-zero state among them), then edge-heavy, then uniform"""
        rng = random.Random("%s elements %s" % (self.name, seed))
        edge = [0, 1, self.p - 1]
        out = [0] * self.t + [e for combo in itertools.product(edge, repeat=self.t) for e in combo][:81]
        while len(out) < count:
            out.append(rng.choice(edge) if rng.random() < 0.1 else rng.randrange(self.p))
        return out[:count]


@functools.lru_cache(maxsize=None)
def pset(name):
    return PSet(name)


def hexes(values):
    return ["%064x" % v for v in values]


def plib(zk):
    return zk.poseidon._plib()


def filled(count):
    """`count` elements of 0xFF bytes: what an output buffer holds before the call"""
    return np.full((count, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


# ---------------------------------------------------------------- 1. pins
def check_ref_pins():
    """RefPoseidon reproduces the values a separate prototype gave: it is trusted only after this"""
    ref = pset("reference").ref
    assert hexes(ref.permute([0, 1, 2])) == PIN_PERMUTE_012
    assert hexes([ref.hash([0])]) == [PIN_HASH_0]
    assert hexes([ref.hash([1, 2])]) == [PIN_PERMUTE_012[1]]
    assert hexes([ref.hash([5, 6, 7])]) == [PIN_HASH_567]
    assert hexes([ref_tree(ref, [[i] for i in range(1, 5)])[-1]]) == [PIN_ROOT_4]
    assert hexes([ref_tree(ref, [[i] for i in range(1, 1025)])[-1]]) == [PIN_ROOT_1024]


def check_host_pins(zk):
    """the library's host twin and the Python mirror over it reproduce the pins (no device is used)"""
    po = zk.poseidon
    prm = pset("reference").params(zk)
    assert hexes(prm.permute([0, 1, 2])) == PIN_PERMUTE_012
    assert hexes([po.CRH.evaluate(prm, [0])]) == [PIN_HASH_0]
    assert hexes([po.TwoToOneCRH.evaluate(prm, 1, 2), po.TwoToOneCRH.compress(prm, 1, 2)]) == [PIN_PERMUTE_012[1]] * 2
    assert hexes([po.CRH.evaluate(prm, [5, 6, 7])]) == [PIN_HASH_567]
    sp = po.PoseidonSponge(prm)
    sp.absorb([5])
    sp.absorb([6, 7])
    assert hexes(sp.squeeze_field_elements(1)) == [PIN_HASH_567]
    # the duplex beyond one hash: squeezing on, then absorbing again, against the same bookkeeping on RefPoseidon's permutation
    ref = pset("reference").ref
    s = ref.permute(ref.permute([0, 5, 6])[:1] + [(ref.permute([0, 5, 6])[1] + 7) % ref.p] + ref.permute([0, 5, 6])[2:])
    more = sp.squeeze_field_elements(3)          # the second rate element, then a permutation and two more
    s2 = ref.permute(s)
    assert more == [s[2], s2[1], s2[2]]
    sp.absorb(9)                                 # squeezing -> absorbing: a permutation first
    s3 = ref.permute(s2)
    s3[1] = (s3[1] + 9) % ref.p
    assert sp.squeeze_field_elements(1) == [ref.permute(s3)[1]]
    prm.free()


# ---------------------------------------------------------------- 2. permutation and hash
def check_permute(zk, name, device):
    """count states in place, every count of COUNTS as a prefix of one reference run; host twin or device entry"""
    ps, lib = pset(name), plib(zk)
    prm = ps.params(zk)
    states = ps.elements(max(COUNTS) * ps.t, "states")
    exp = mont(ps.field, [y for i in range(max(COUNTS)) for y in ps.ref.permute(states[i * ps.t:(i + 1) * ps.t])])
    words = mont(ps.field, states)
    for count in COUNTS:
        buf = words.copy()                      # the states past `count` must stay as they are
        if device:
            d = dev(zk, buf)
            assert lib.zk_poseidon_permute_device(prm.handle, ptr(d), count, None) == 0
            got = host(d)
        else:
            assert lib.zk_poseidon_permute_host(prm.handle, ptr(buf), count) == 0
            got = buf
        assert (got[:count * ps.t] == exp[:count * ps.t]).all(), (name, count)
        assert (got[count * ps.t:] == words[count * ps.t:]).all(), (name, count)
    prm.free()


def _hash_call(zk, lib, prm, words, arity, count, device):
    out = filled(count + 1)                     # one element more than is written
    if device:
        d_in, d_out = dev(zk, words), dev(zk, out)
        assert lib.zk_poseidon_hash_device(prm.handle, ptr(d_in), arity, count, ptr(d_out), None) == 0
        got, back = host(d_out), host(d_in)
    else:
        w = words.copy()
        assert lib.zk_poseidon_hash_host(prm.handle, ptr(w), arity, count, ptr(out)) == 0
        got, back = out, w
    assert (back == words).all(), "the input changed"
    assert (got[count] == 0xFFFFFFFFFFFFFFFF).all(), "written past the end"
    return got[:count]


def check_hash(zk, name, device):
    """arity 1 .. 2 rate + 1 and 64 at three hashes each; COUNTS at arity 2 as prefixes of one reference run"""
    ps, lib = pset(name), plib(zk)
    prm = ps.params(zk)
    for arity in list(range(1, 2 * ps.rate + 2)) + [64]:
        count = 3
        elems = ps.elements(arity * count, "hash %d" % arity)
        exp = mont(ps.field, [ps.ref.hash(elems[i * arity:(i + 1) * arity]) for i in range(count)])
        assert (_hash_call(zk, lib, prm, mont(ps.field, elems), arity, count, device) == exp).all(), (name, arity)
    elems = ps.elements(2 * max(COUNTS), "hash counts")
    exp = mont(ps.field, [ps.ref.hash(elems[2 * i:2 * i + 2]) for i in range(max(COUNTS))])
    words = mont(ps.field, elems)
    for count in COUNTS:
        assert (_hash_call(zk, lib, prm, words[:2 * count], 2, count, device) == exp[:count]).all(), (name, count)
    prm.free()


def check_grid_stride(zk, name="reference"):
    """GPU only: TRIP + 257 hashes and as many permutations, so the grid-stride loops take a second trip that ends inside a
    workgroup.  The inputs repeat with period 251 (no multiple of it is a workgroup or grid boundary), which gives every output
    from 251 reference values: the whole arrays are compared, not samples."""
    ps, lib = pset(name), plib(zk)
    prm = ps.params(zk)
    count, period = TRIP + 257, 251
    reps = -(-count // period)
    elems = ps.elements(period, "stride")
    exp = np.tile(mont(ps.field, [ps.ref.hash([x]) for x in elems]), (reps, 1))[:count]
    words = np.tile(mont(ps.field, elems), (reps, 1))[:count]
    d_in, d_out = dev(zk, words), dev(zk, filled(count + 1))
    assert lib.zk_poseidon_hash_device(prm.handle, ptr(d_in), 1, count, ptr(d_out), None) == 0
    got = host(d_out)
    assert (got[:count] == exp).all() and (got[count] == 0xFFFFFFFFFFFFFFFF).all() and (host(d_in) == words).all()
    states = ps.elements(period * ps.t, "stride states")
    exp = np.tile(mont(ps.field, [y for i in range(period) for y in ps.ref.permute(states[i * ps.t:(i + 1) * ps.t])]), (reps, 1))[:count * ps.t]
    tail = filled(ps.t)
    d = dev(zk, np.concatenate([np.tile(mont(ps.field, states), (reps, 1))[:count * ps.t], tail]))
    assert lib.zk_poseidon_permute_device(prm.handle, ptr(d), count, None) == 0
    got = host(d)
    assert (got[:count * ps.t] == exp).all() and (got[count * ps.t:] == tail).all()
    prm.free()


# ---------------------------------------------------------------- 3. tree and paths
def tree_leaves(ps, log_n, leaf_arity):
    """leaf i = (i + 1, ...): the trees of all sizes share their left part, so RefPoseidon's memo makes them cost the largest one"""
    return [[(i + 1) * (q + 1) % ps.p for q in range(leaf_arity)] for i in range(1 << log_n)]


def check_tree(zk, log_n, leaf_arity):
    """all 2n - 1 nodes; then paths: every index up to log_n = 4, seeded ones plus 0 and n - 1 above; Path.verify and its negatives"""
    ps = pset(TREE_PSETS[leaf_arity])
    po, prm, n = zk.poseidon, ps.params(zk), 1 << log_n
    leaves = tree_leaves(ps, log_n, leaf_arity)
    nodes = ref_tree(ps.ref, leaves)
    words = mont(ps.field, [x for leaf in leaves for x in leaf])
    d_leaves = dev(zk, words)
    tree = po.MerkleTree.new(prm, d_leaves, leaf_arity)
    assert (host(tree.nodes) == mont(ps.field, nodes)).all(), (log_n, leaf_arity)
    assert (host(d_leaves) == words).all(), "the leaves changed"
    assert tree.root() == nodes[-1] and tree.log_n == log_n
    rng = random.Random(log_n * 8 + leaf_arity)
    indices = list(range(n)) if log_n <= 4 else [0, n - 1] + [rng.randrange(n) for _ in range(6)]
    paths = tree.generate_proofs(indices)
    for i, path in zip(indices, paths):
        sib = [nodes[level_offset(log_n, j) + ((i >> j) ^ 1)] for j in range(log_n)]
        assert (path.leaf_index, path.leaf_sibling_hash, path.auth_path) == (i, sib[0], sib[1:][::-1]), (log_n, i)
    single = tree.generate_proof(indices[-1])
    assert (single.leaf_index, single.leaf_sibling_hash, single.auth_path) == (paths[-1].leaf_index, paths[-1].leaf_sibling_hash, paths[-1].auth_path)
    leaf_of = (lambda i: leaves[i][0]) if leaf_arity == 1 else (lambda i: leaves[i])
    for i, path in list(zip(indices, paths))[:4]:
        root = nodes[-1]
        assert path.verify(prm, root, leaf_of(i))
        wrong_leaf = [(leaves[i][0] + 1) % ps.p] + leaves[i][1:]
        assert not path.verify(prm, root, wrong_leaf[0] if leaf_arity == 1 else wrong_leaf)
        assert not path.verify(prm, (root + 1) % ps.p, leaf_of(i))
        assert not po.Path((path.leaf_sibling_hash + 1) % ps.p, path.auth_path, i).verify(prm, root, leaf_of(i))
        for q in range(len(path.auth_path)):
            changed = path.auth_path[:q] + [(path.auth_path[q] + 1) % ps.p] + path.auth_path[q + 1:]
            assert not po.Path(path.leaf_sibling_hash, changed, i).verify(prm, root, leaf_of(i))
        assert not po.Path(path.leaf_sibling_hash, path.auth_path, i ^ 1).verify(prm, root, leaf_of(i))
    tree.free()
    prm.free()


def check_many_paths(zk, log_n=6):
    """the index list is cut into launches of PATHS_PER_LAUNCH: counts on both sides of the cut, indices repeating"""
    ps = pset(TREE_PSETS[3])
    prm, n = ps.params(zk), 1 << log_n
    leaves = tree_leaves(ps, log_n, 3)
    nodes = ref_tree(ps.ref, leaves)
    tree = zk.poseidon.MerkleTree.new(prm, dev(zk, mont(ps.field, [x for leaf in leaves for x in leaf])), 3)
    for count in (1, PATHS_PER_LAUNCH, PATHS_PER_LAUNCH + 1, 2 * PATHS_PER_LAUNCH + 3):
        rng = random.Random(count)
        draws = [rng.randrange(n) for _ in range(count)]
        idx = np.array(draws, dtype=np.uint64)
        out = dev(zk, filled(count * log_n + 1))
        assert plib(zk).zk_merkle_paths_device(FIELD_IDS[ps.field], ptr(tree.nodes), log_n, ptr(idx), count, ptr(out), None) == 0
        idx[:] = 0                               # the list was read before the entry returned
        got = host(out)
        exp = mont(ps.field, [nodes[level_offset(log_n, j) + ((i >> j) ^ 1)] for i in draws for j in range(log_n)])
        assert (got[:count * log_n] == exp).all() and (got[count * log_n] == 0xFFFFFFFFFFFFFFFF).all(), count
    prm.free()


def check_large_tree(zk, log_n):
    """GPU only.  Leaves periodic with period 2^10 except a few replaced ones, so every node is known: the 2^10-leaf subtree tiled,
    the chain h(x, x) above it, and the replaced leaves' paths recomputed (log_n hashes each).  The whole nodes array is compared."""
    ps = pset("reference")
    prm, n, sub_log = ps.params(zk), 1 << log_n, 10
    sub = 1 << sub_log
    base = [[i + 1] for i in range(sub)]
    sub_nodes = ref_tree(ps.ref, base)
    exp = np.zeros((2 * n - 1, 4), dtype=np.uint64)
    for j in range(sub_log + 1):                 # the levels inside the subtree: tiled
        lv = mont(ps.field, sub_nodes[level_offset(sub_log, j):level_offset(sub_log, j) + (sub >> j)])
        exp[level_offset(log_n, j):level_offset(log_n, j) + (n >> j)] = np.tile(lv, (n // sub, 1))
    x = sub_nodes[-1]
    for j in range(sub_log + 1, log_n + 1):      # above it every node of a level is the same: h(x, x)
        x = ps.ref.hash([x, x])
        exp[level_offset(log_n, j):level_offset(log_n, j) + (n >> j)] = mont(ps.field, [x])[0]
    leaves = np.tile(mont(ps.field, [b[0] for b in base]), (n // sub, 1))
    replaced = sorted({0, n - 1, WG - 1, WG, 2 * WG * 3 + 1, min(TRIP, n) - 1, TRIP % n, (n // 2 + 12345) % n})
    rng = random.Random(log_n)
    for i in replaced:                           # in order: a later path sees the earlier replacements
        v = rng.randrange(ps.p)
        leaves[i] = mont(ps.field, [v])[0]
        cur = ps.ref.hash([v])
        exp[i] = mont(ps.field, [cur])[0]
        for j in range(log_n):
            pos = i >> j
            sib = unmont(ps.field, exp[level_offset(log_n, j) + (pos ^ 1)])[0]
            cur = ps.ref.hash([sib, cur] if pos & 1 else [cur, sib])
            exp[level_offset(log_n, j + 1) + (pos >> 1)] = mont(ps.field, [cur])[0]
    d_leaves = dev(zk, leaves)
    tree = zk.poseidon.MerkleTree.new(prm, d_leaves)
    got = host(tree.nodes)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (log_n, bad[:8].tolist(), bad.size)
    assert (host(d_leaves) == leaves).all()
    path = tree.generate_proof(replaced[-1])
    assert path.verify(prm, tree.root(), unmont(ps.field, leaves[replaced[-1]])[0])
    tree.free()
    prm.free()


# ---------------------------------------------------------------- 4. the ElGamal stream
ELGAMAL_NS = [1, 255, 256, 257, (1 << 16) + 1]


def check_elgamal(zk, field, n):
    po, p = zk.poseidon, modulus(field)
    rng = random.Random("elgamal %s %d" % (field, n))
    m = [p - 1, 0, 1][:n] + [rng.randrange(p) for _ in range(max(n - 3, 0))]
    m[-1] = p - 1
    words = mont(field, m)
    marr = np.array(m, dtype=object)
    for dh in (0, 1, p - 1, rng.randrange(p)):
        d_m = dev(zk, words)
        c2 = po.elgamal_mask(field, d_m, dh)
        assert (unmont_array(field, host(c2)) == (marr + dh) % p).all(), (field, n, dh)
        assert (host(c2) == mont(field, (marr + dh) % p)).all()          # canonical words, not only the right residues
        assert (host(d_m) == words).all(), "the plaintext changed"
        back = po.elgamal_unmask(field, c2, dh)
        assert (host(back) == words).all(), (field, n, dh)
        assert po.elgamal_mask(field, d_m, dh, out=d_m) is d_m and (host(d_m) == host(c2)).all()      # in place


# ---------------------------------------------------------------- 5. refusals
def check_refusals(zk):
    """every refusal of the header's list, each followed by a good call that succeeds"""
    ps, lib = pset("pallas_fq_a3"), plib(zk)
    f, p = FIELD_IDS[ps.field], ps.p
    ark, mds, init = mont(ps.field, [x for r in ps.ark for x in r]), mont(ps.field, [x for r in ps.mds for x in r]), mont(ps.field, [0, 0, 0])
    h = ctypes.c_uint64(0)

    def create(width=3, rate=2, off=1, rf=ps.rf, rp=ps.rp, alpha=3, a=ark, m=mds, i=None, out=h):
        return lib.zk_poseidon_create(f, width, rate, off, rf, rp, alpha, ptr(a) if a is not None else None, ptr(m) if m is not None else None,
                                      ptr(i) if i is not None else None, ctypes.byref(out) if out is not None else None)

    prm = ps.params(zk)
    elems = ps.elements(8, "refusals")
    words, want = mont(ps.field, elems), mont(ps.field, [ps.ref.hash(elems[2 * i:2 * i + 2]) for i in range(4)])

    def good():
        out = filled(4)
        assert lib.zk_poseidon_hash_host(prm.handle, ptr(words), 2, 4, ptr(out)) == 0 and (out == want).all()
        d_out = dev(zk, filled(4))
        assert lib.zk_poseidon_hash_device(prm.handle, ptr(dev(zk, words)), 2, 4, ptr(d_out), None) == 0 and (host(d_out) == want).all()

    def refused(status, expect=INVALID_ARG, which=None):
        assert status == expect, (status, which)
        good()

    good()
    noncanon = lambda arr, v: np.concatenate([arr[:1], limbs_of([v]), arr[2:]])      # noqa: E731
    big = np.zeros((300 * 3, 4), dtype=np.uint64)
    for st in (lambda: create(a=None),
               lambda: create(m=None),
               lambda: create(out=None),
               lambda: create(width=1, rate=1, off=0),
               lambda: create(width=6),
               lambda: create(rate=0),
               lambda: create(rate=3, off=1),
               lambda: create(rate=2, off=2),
               lambda: create(off=0xFFFFFFFF),
               lambda: create(rf=ps.rf + 1),
               lambda: create(rf=0, rp=0),
               lambda: create(rf=2, rp=255, a=big),
               lambda: create(rf=258, rp=0, a=big),
               lambda: create(alpha=0),
               lambda: create(a=noncanon(ark, p)),
               lambda: create(m=noncanon(mds, p)),
               lambda: create(m=noncanon(mds, (1 << 256) - 1)),
               lambda: create(i=noncanon(init, p + 1))):
        refused(st())
    assert lib.zk_poseidon_create(7, 3, 2, 1, ps.rf, ps.rp, 3, ptr(ark), ptr(mds), None, ctypes.byref(h)) == INVALID_ARG     # no such field
    assert create(i=init) == 0 and lib.zk_poseidon_free(h.value) == 0           # a good create, with an explicit zero init
    assert create(rf=2, rp=254, a=big) == 0 and lib.zk_poseidon_free(h.value) == 0     # 256 rounds are allowed
    dead = h.value

    d_in, d_out = dev(zk, np.concatenate([words, words])), dev(zk, filled(16))
    d_nodes, idx = dev(zk, filled(15)), np.array([0, 7], dtype=np.uint64)
    one = mont(ps.field, [1])
    at = lambda buf, elems_: ctypes.c_void_p(ptr(buf).value + 32 * elems_)      # noqa: E731
    hd, which = prm.handle, 0
    for st in (lambda: lib.zk_poseidon_permute_host(hd, None, 1),
               lambda: lib.zk_poseidon_hash_host(hd, None, 2, 1, ptr(filled(1))),
               lambda: lib.zk_poseidon_hash_host(hd, ptr(words), 2, 1, None),
               lambda: lib.zk_poseidon_hash_host(hd, ptr(words), 0, 1, ptr(filled(1))),
               lambda: lib.zk_poseidon_hash_host(hd, ptr(words), 65, 1, ptr(filled(1))),
               lambda: lib.zk_poseidon_permute_device(hd, None, 1, None),
               lambda: lib.zk_poseidon_hash_device(hd, None, 2, 1, ptr(d_out), None),
               lambda: lib.zk_poseidon_hash_device(hd, ptr(d_in), 2, 1, None, None),
               lambda: lib.zk_poseidon_hash_device(hd, ptr(d_in), 0, 1, ptr(d_out), None),
               lambda: lib.zk_poseidon_hash_device(hd, ptr(d_in), 65, 1, ptr(d_out), None),
               lambda: lib.zk_poseidon_hash_device(hd, ptr(d_in), 2, 4, at(d_in, 7), None),            # out = the last input element
               lambda: lib.zk_poseidon_hash_device(hd, at(d_in, 3), 2, 4, ptr(d_in), None),            # in begins inside out
               lambda: lib.zk_poseidon_merkle_tree_device(hd, None, 1, 3, ptr(d_nodes), None),
               lambda: lib.zk_poseidon_merkle_tree_device(hd, ptr(d_in), 1, 3, None, None),
               lambda: lib.zk_poseidon_merkle_tree_device(hd, ptr(d_in), 0, 3, ptr(d_nodes), None),
               lambda: lib.zk_poseidon_merkle_tree_device(hd, ptr(d_in), 65, 3, ptr(d_nodes), None),
               lambda: lib.zk_poseidon_merkle_tree_device(hd, ptr(d_in), 1, 0, ptr(d_nodes), None),
               lambda: lib.zk_poseidon_merkle_tree_device(hd, ptr(d_in), 1, 31, ptr(d_nodes), None),
               lambda: lib.zk_poseidon_merkle_tree_device(hd, ptr(d_in), 1, 3, at(d_in, 7), None),     # nodes begin at the last leaf
               lambda: lib.zk_poseidon_merkle_tree_device(hd, at(d_out, 2), 1, 1, ptr(d_out), None),   # the leaves begin inside nodes
               lambda: lib.zk_merkle_paths_device(f, None, 3, ptr(idx), 2, ptr(d_out), None),
               lambda: lib.zk_merkle_paths_device(f, ptr(d_nodes), 3, None, 2, ptr(d_out), None),
               lambda: lib.zk_merkle_paths_device(f, ptr(d_nodes), 3, ptr(idx), 2, None, None),
               lambda: lib.zk_merkle_paths_device(f, ptr(d_nodes), 0, ptr(idx), 2, ptr(d_out), None),
               lambda: lib.zk_merkle_paths_device(f, ptr(d_nodes), 31, ptr(idx), 2, ptr(d_out), None),
               lambda: lib.zk_merkle_paths_device(f, ptr(d_nodes), 3, ptr(np.array([0, 8], dtype=np.uint64)), 2, ptr(d_out), None),       # index = n
               lambda: lib.zk_merkle_paths_device(f, ptr(d_nodes), 3, ptr(np.array([1 << 40, 0], dtype=np.uint64)), 2, ptr(d_out), None),
               lambda: lib.zk_merkle_paths_device(f, ptr(d_nodes), 3, ptr(idx), 2, at(d_nodes, 14), None),                                 # out = the root
               lambda: lib.zk_merkle_paths_device(9, ptr(d_nodes), 3, ptr(idx), 2, ptr(d_out), None),
               lambda: lib.zk_vec_add_scalar_device(f, None, ptr(d_in), 4, ptr(one), None),
               lambda: lib.zk_vec_add_scalar_device(f, ptr(d_out), None, 4, ptr(one), None),
               lambda: lib.zk_vec_add_scalar_device(f, ptr(d_out), ptr(d_in), 4, None, None),
               lambda: lib.zk_vec_add_scalar_device(f, ptr(d_out), ptr(d_in), 4, ptr(limbs_of([p])), None),
               lambda: lib.zk_vec_add_scalar_device(f, at(d_in, 1), ptr(d_in), 4, ptr(one), None),     # shifted by one element
               lambda: lib.zk_vec_add_scalar_device(9, ptr(d_out), ptr(d_in), 4, ptr(one), None)):
        refused(st(), which=which)
        which += 1
    for st in (lambda: lib.zk_poseidon_free(dead),
               lambda: lib.zk_poseidon_free(1 << 40),
               lambda: lib.zk_poseidon_permute_host(dead, ptr(words.copy()), 1),
               lambda: lib.zk_poseidon_hash_host(dead, ptr(words), 2, 1, ptr(filled(1))),
               lambda: lib.zk_poseidon_permute_device(dead, ptr(d_in), 1, None),
               lambda: lib.zk_poseidon_hash_device(dead, ptr(d_in), 2, 1, ptr(d_out), None),
               lambda: lib.zk_poseidon_merkle_tree_device(dead, ptr(d_in), 1, 3, ptr(d_nodes), None)):
        refused(st(), BAD_HANDLE)
    # nothing was written by a refused call
    assert (host(d_in) == np.concatenate([words, words])).all() and (host(d_out) == filled(16)).all() and (host(d_nodes) == filled(15)).all()
    # the good forms of the device entries that good() does not make
    assert lib.zk_poseidon_merkle_tree_device(hd, ptr(d_in), 1, 3, ptr(d_nodes), None) == 0
    assert (host(d_nodes) == mont(ps.field, ref_tree(ps.ref, [[x] for x in elems]))).all()
    assert lib.zk_merkle_paths_device(f, ptr(d_nodes), 3, ptr(idx), 2, ptr(d_out), None) == 0
    assert lib.zk_vec_add_scalar_device(f, ptr(d_out), ptr(d_in), 4, ptr(one), None) == 0
    assert (host(d_out)[:4] == mont(ps.field, [(x + 1) % p for x in elems[:4]])).all()
    prm.free()


def check_lifecycle(zk, device_id=0):
    """without a device the *_device entries return ZK_ERR_NOT_INITIALIZED; the host twin and the handle do not care; after the next
    zk_init the handle's table is uploaded again"""
    ps, lib = pset("bn254_a7"), plib(zk)
    prm = ps.params(zk)
    elems = ps.elements(6, "lifecycle")
    words, want = mont(ps.field, elems), mont(ps.field, [ps.ref.hash(elems[3 * i:3 * i + 3]) for i in range(2)])
    d_in, d_out = dev(zk, words), dev(zk, filled(2))
    assert lib.zk_poseidon_hash_device(prm.handle, ptr(d_in), 3, 2, ptr(d_out), None) == 0 and (host(d_out) == want).all()
    emu = on_emulator(zk)
    zk.shutdown()
    try:
        buf = np.zeros((16, 4), dtype=np.uint64)       # (never touched: every call below is refused first)
        one = mont(ps.field, [1])
        idx = np.zeros(1, dtype=np.uint64)
        for st in (lib.zk_poseidon_permute_device(prm.handle, ptr(buf), 1, None), lib.zk_poseidon_hash_device(prm.handle, ptr(buf), 1, 1, ptr(buf[8:]), None),
                   lib.zk_poseidon_merkle_tree_device(prm.handle, ptr(buf), 1, 1, ptr(buf[8:]), None),
                   lib.zk_merkle_paths_device(FIELD_IDS[ps.field], ptr(buf), 1, ptr(idx), 1, ptr(buf[8:]), None),
                   lib.zk_vec_add_scalar_device(FIELD_IDS[ps.field], ptr(buf[8:]), ptr(buf), 1, ptr(one), None)):
            assert st == NOT_INITIALIZED, st
        assert not buf.any()
        out = filled(2)
        assert lib.zk_poseidon_hash_host(prm.handle, ptr(words), 3, 2, ptr(out)) == 0 and (out == want).all()
    finally:
        zk.init(device_id)
    assert on_emulator(zk) == emu
    d_in, d_out = dev(zk, words), dev(zk, filled(2))
    assert lib.zk_poseidon_hash_device(prm.handle, ptr(d_in), 3, 2, ptr(d_out), None) == 0 and (host(d_out) == want).all()
    prm.free()
