"""CPU tier: the quotient evaluators on the generated program corpus (tests/expr_programs.py) against
oracle/pyref_halo2.eval_program on Python integers, every row, no GPU.

  * the kernel generated per program (zk_expr_specialised_source, from the HIP build of the library: it needs no device) is
    compiled with g++ against tests/emu (one translation unit and kernel symbol per source, in parallel) and launched over a
    grid through emu::launch: all four scalar fields at the default slot count, PallasFp at 1 / 2 / 3 / 4 / 5 / 8 slots;
  * the emulated interpreters that exist in the emulator build: zk_expr_eval_device (saturated limbs) and
    zk_expr_eval_lazy_device (lazy limbs, two slots);
  * coverage of the generated sources is asserted (every bias table that the bound walk can pick, carry steps, contractions,
    slot evictions), and text mutations of a generated source (a smaller bias table, a dropped carry step, a load into the
    wrong slot) are shown to fail the comparison;
  * refusals: malformed or oversized programs raise ZkError on every path, a rotation outside int16 is refused by the mirror."""
import concurrent.futures
import ctypes
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import expr_programs as xp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "contangle-zkcp_amd", "csrc")
LOG_N = 8                                         # 256 extended rows; the emulated grid below is smaller, so rows are strided
GRID = 3
SWEEP = [1, 2, 3, 4, 5, 8]                        # PallasFp slot counts (ZK_EXPR_JIT_SLOTS)
# BIAS4K2 (limb bound above strict, value bound <= 2 p) is never the walk's pick: see DESIGN.md section 5 and
# test_bias4k2_is_unreachable_by_the_walk
REACHABLE_BIASES = ["BIAS4K1", "BIAS8K2", "BIAS8K3", "BIAS16K2"]

# the child loads the HIP build of the library (no device needed for the source) and writes every source as JSON
SOURCES_SCRIPT = r"""
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import contangle_zkcp_amd as zk
import expr_programs as xp
zk.load()
out = {}
for field, slots in %(jobs)r:
    if slots is None:
        os.environ.pop("ZK_EXPR_JIT_SLOTS", None)
    else:
        os.environ["ZK_EXPR_JIT_SLOTS"] = str(slots)
    for p in xp.corpus(%(log_n)d):
        key = "%%s/%%s/%%s" %% (field, slots, p.name)
        try:
            out[key] = zk.halo2.expr_specialised_source(field, p.ops, p.n_cols, p.n_consts)
        except zk.ZkError as e:
            out[key] = {"refused": e.status}
json.dump(out, open(sys.argv[1], "w"))
"""


def _child(script, timeout=600, env=None):
    r = subprocess.run([sys.executable, "-c", script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("expr_sources") / "sources.json")
    jobs = [(f, None) for f in xp.FIELDS] + [("PallasFp", s) for s in SWEEP]
    r = subprocess.run([sys.executable, "-c", SOURCES_SCRIPT % {"root": ROOT, "jobs": jobs, "log_n": LOG_N}, path],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return json.load(open(path))


class JitLib:
    """g++ builds of generated sources under the emulator: one translation unit and kernel symbol per source, one shared object"""

    def __init__(self, srcs, workdir):
        self.entries = {}
        units = []
        for k, (key, src) in enumerate(srcs.items()):
            sym = "zk_expr_jit_u%d" % k
            tu = os.path.join(workdir, "u%d.cc" % k)
            with open(tu, "w") as f:
                f.write('#include "emu_hip.h"\n#define zk_expr_jit %s\n%s\n#undef zk_expr_jit\n'
                        '#define ZK_EXPR_JIT_KERNEL %s\n#define ZK_EXPR_JIT_ENTRY %s_run\n#include "expr_jit_harness.h"\n' % (sym, src, sym, sym))
            units.append((tu, tu[:-3] + ".o"))
            self.entries[key] = sym + "_run"
        base = ["g++", "-O1", "-std=c++17", "-fPIC", "-DZK_EMU", "-fvisibility=hidden", "-w", "-I" + EMU, "-I" + CSRC]

        def cc(u):
            r = subprocess.run(base + ["-c", u[0], "-o", u[1]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            return u[0], r.returncode, r.stdout

        with concurrent.futures.ThreadPoolExecutor(max_workers=os.cpu_count() or 4) as ex:
            for tu, rc, log in ex.map(cc, units):
                assert rc == 0, (tu, log[-3000:])
        so = os.path.join(workdir, "libexprjit.so")
        subprocess.check_call(["g++", "-shared", "-fPIC", "-O2", "-std=c++17", "-fvisibility=hidden", "-I" + EMU, os.path.join(EMU, "emu_hip.cpp")]
                              + [o for _, o in units] + ["-o", so])
        self.lib = ctypes.CDLL(so)

    def run(self, key, cols, consts, log_n, rot_scale, grid=GRID):
        """cols / consts: lists of stored words (ints); returns uint64 [n, 4]"""
        n = 1 << log_n
        arrs = [xp.words_array(c) for c in cols]
        ptrs = (ctypes.c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
        ks = xp.words_array(consts) if consts else np.zeros((1, 4), dtype=np.uint64)
        out = np.zeros((n, 4), dtype=np.uint64)
        fn = getattr(self.lib, self.entries[key])
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint]
        fn(ctypes.cast(ptrs, ctypes.c_void_p), ks.ctypes.data, log_n, rot_scale, out.ctypes.data, grid)
        return out


# ------------------------------------------------------------------------------------------------------------ mutations
def _mut_bias(src):
    """every subtraction / negation whose table has a smaller one, swapped for it (one mutant each, at most 6)"""
    smaller = {"BIAS16K2": "BIAS8K2", "BIAS8K3": "BIAS8K2", "BIAS8K2": "BIAS4K1", "BIAS4K2": "BIAS4K1"}
    out = []
    for m in re.finditer(r"K::(BIAS16K2|BIAS8K3|BIAS8K2|BIAS4K2)\b", src):
        out.append(src[:m.start(1)] + smaller[m.group(1)] + src[m.end(1):])
    return out[:6]


def _mut_norm(src):
    out = []
    for m in re.finditer(r"    fe29_norm\(t\d+, t\d+\);\n", src):
        out.append(src[:m.start()] + src[m.end():])
    return out[:8]


def _mut_slot(src, nslots):
    """a load that (re)fills slot a written into slot b instead -- both slots already loaded before it, so nothing reads an
    unwritten slot"""
    out = []
    loaded = set()
    for m in re.finditer(r"    s(\d+) = cols\[", src):
        a = int(m.group(1))
        if a in loaded:
            for b in sorted(loaded - {a}):
                out.append(src[:m.start(1)] + str(b) + src[m.end(1):])
                break
        loaded.add(a)
    return out[:6]


MUTATION_PROGRAMS = {"bias": ["bias_ladder", "unnormalised"], "norm": ["add_chain_140", "unnormalised", "carry_before_bias"],
                     "slot": ["slot_pool_12", "reuse_distances", "gate2"]}


@pytest.fixture(scope="module")
def jit(sources, tmp_path_factory):
    srcs = {k: v for k, v in sources.items() if isinstance(v, str)}
    for kind, progs in MUTATION_PROGRAMS.items():
        for name in progs:
            src = sources["PallasFp/None/" + name]
            muts = _mut_bias(src) if kind == "bias" else _mut_norm(src) if kind == "norm" else _mut_slot(src, 4)
            for j, m in enumerate(muts):
                srcs["mutant/%s/%s/%d" % (kind, name, j)] = m
    d = str(tmp_path_factory.mktemp("expr_jit_emu"))
    lib = JitLib(srcs, d)
    yield lib
    shutil.rmtree(d, ignore_errors=True)


def _corpus():
    return xp.corpus(LOG_N)


_EXPECTED = {}


def _case(field, prog, kind, radix):
    """(columns, constants, expected words) of one input set, cached: the sweep and the interpreters reuse them"""
    key = (field, prog.name, kind, radix)
    if key not in _EXPECTED:
        cols, consts = xp.input_words(field, prog, 1 << LOG_N, kind)
        _EXPECTED[key] = (cols, consts, xp.expected(field, prog, cols, consts, 1 << LOG_N, radix))
    return _EXPECTED[key]


def _check_jit(jit, field, slots, prog):
    for kind in ("mixed", "dense"):
        cols, consts, exp = _case(field, prog, kind, xp.R_LAZY)
        got = jit.run("%s/%s/%s" % (field, slots, prog.name), cols, consts, LOG_N, prog.rot_scale)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert len(bad) == 0, (field, slots, prog.name, kind, "rows", bad[:8].tolist())


@pytest.mark.parametrize("field", xp.FIELDS)
def test_generated_kernel_matches_python_integers(jit, sources, field):
    for p in _corpus():
        assert isinstance(sources["%s/None/%s" % (field, p.name)], str), (field, p.name, sources["%s/None/%s" % (field, p.name)])
        _check_jit(jit, field, None, p)


@pytest.mark.parametrize("slots", SWEEP)
def test_generated_kernel_slot_sweep(jit, sources, slots):
    for p in _corpus():
        src = sources["PallasFp/%d/%s" % (slots, p.name)]
        # the source function honours ZK_EXPR_JIT_SLOTS: exactly s0 .. s(slots - 1) are declared
        assert "    Fe<F> %s;\n" % ", ".join("s%d" % q for q in range(slots)) in src, (slots, p.name)
        _check_jit(jit, "PallasFp", slots, p)
    if slots == 4:    # the default
        assert all(sources["PallasFp/4/" + p.name] == sources["PallasFp/None/" + p.name] for p in _corpus())


@pytest.mark.parametrize("field", xp.FIELDS)
def test_generated_sources_cover_the_bound_walk_and_the_slots(sources, field):
    srcs = [sources["%s/None/%s" % (field, p.name)] for p in _corpus()]
    text = "".join(srcs)
    for b in REACHABLE_BIASES:
        assert "K::%s)" % b in text, (field, b)
    assert "fe29_norm(" in text and "fe29_one(o)" in text, field
    # loads outnumber the distinct (column, rotation) pairs: slots are evicted and refilled
    evicted = 0
    for p, src in zip(_corpus(), srcs):
        pairs = {(o[1], o[2]) for o in p.ops if o[0] == "col"}
        loads = len(re.findall(r" = cols\[", src))
        assert loads >= len(pairs), (field, p.name)
        evicted += loads > len(pairs)
    assert evicted >= 5, (field, evicted)
    # hoisting: in some source a load sits more than one statement ahead of its first use
    assert any(re.search(r"    s(\d+) = cols\[[^\n]*\n(?:(?!    s\1 = )[^\n]*\n){2,}[^\n]*fe29_unpack\(t\d+, s\1\)", s) for s in srcs)


def test_bias4k2_is_unreachable_by_the_walk(sources):
    """BIAS4K2 needs an operand whose limb bound is above strict (a sum, a carry step's output, a difference) and whose value bound
    is at most 2 p; every such value has a value bound above 2 p (a product's is above p, a load's is 2 p, a sum adds them), so
    expr_compile29 never picks it -- the table stays for the curve formulas (fe29_sub2x).  Nothing in the corpus reaches it."""
    assert not any(isinstance(v, str) and "K::BIAS4K2)" in v for v in sources.values())


@pytest.mark.parametrize("kind", ["bias", "norm", "slot"])
def test_mutated_kernel_source_fails_the_comparison(jit, kind):
    """every mutation kind is detected by the corpus inputs for at least one mutant; the mutants that no input tells apart are
    the bound slack recorded in DESIGN.md section 5"""
    progs = {p.name: p for p in _corpus()}
    detected, missed = [], []
    for key in sorted(k for k in jit.entries if k.startswith("mutant/%s/" % kind)):
        name = key.split("/")[2]
        p = progs[name]
        caught = False
        for ik in ("mixed", "dense"):
            cols, consts, exp = _case("PallasFp", p, ik, xp.R_LAZY)
            if (jit.run(key, cols, consts, LOG_N, p.rot_scale) != exp).any():
                caught = True
        (detected if caught else missed).append(key)
    print(kind, "detected", detected, "missed", missed)
    assert detected, (kind, missed)


# ------------------------------------------------------------------------------------------------------------ emulated interpreters
@pytest.fixture(scope="module")
def zk_emu():
    spec = importlib.util.spec_from_file_location("zk_build", os.path.join(ROOT, "contangle-zkcp_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    emu = b.build_emu()
    import contangle_zkcp_amd as zk
    zk.load(path=emu)
    zk.init(0)
    assert zk.backend_info().startswith("emu")
    yield zk
    zk.shutdown()
    zk._lib = None


@pytest.mark.parametrize("field", xp.FIELDS)
def test_emulated_interpreters_match_python_integers(zk_emu, field):
    zk = zk_emu
    n = 1 << LOG_N
    for p in _corpus():
        for kind in ("mixed", "dense"):
            # saturated limbs: the stored words are Montgomery words (x = w / 2^256)
            cols, consts, exp = _case(field, p, kind, xp.R_MONT)
            out = np.zeros((n, 4), dtype=np.uint64)
            zk.halo2.evaluate_expression(field, p.ops, [xp.words_array(c) for c in cols], xp.words_array(consts), LOG_N, p.rot_scale, out)
            assert (out == exp).all(), (field, p.name, kind, "saturated")
            # lazy limbs, two slots: the stored words are x 2^261; the constants go in as Montgomery words and are scaled by 2^5
            cols, consts, exp = _case(field, p, kind, xp.R_LAZY)
            out = np.zeros((n, 4), dtype=np.uint64)
            zk.halo2.evaluate_expression(field, p.ops, [xp.words_array(c) for c in cols], xp.mont_words_for_lazy_consts(field, consts),
                                         LOG_N, p.rot_scale, out, lazy=True)
            assert (out == exp).all(), (field, p.name, kind, "lazy")


# ------------------------------------------------------------------------------------------------------------ refusals
def refused_programs():
    """(label, ops, n_cols, n_consts, paths that must refuse): every one is refused on the host, before any kernel runs"""
    a, b = ("col", 0, 0), ("col", 1, 0)
    deep = [("col", k % 2, 0) for k in range(9)] + [("add",)] * 8
    long_ = [a] + [b, ("add",)] * 256                                       # 513 ops
    # 512 ops whose annotated form exceeds 2 * EXPR_MAX_OPS words: a chain of subtractions over 64 (column, rotation) pairs, so
    # that every push is a slot miss (a load and a push) and the chain needs a carry step and a contraction now and then
    pairs = [(c, r) for c in range(16) for r in (-2, -1, 1, 2)]
    over = [("col",) + pairs[0]]
    for k in range(1, 256):
        over += [("col",) + pairs[k % len(pairs)], ("sub",)]
    over += [("neg",)]
    every = ("saturated", "lazy", "source")
    return [
        ("depth 9", deep, 2, 1, every),
        ("513 ops", long_, 2, 1, every),
        ("65 columns", [a], 65, 1, every),
        ("33 constants", [a], 1, 33, every),
        ("column index out of range", [("col", 2, 0)], 2, 1, every),
        ("scale index out of range", [a, ("scale", 1)], 1, 1, every),
        ("constant index out of range", [("const", 3)], 1, 3, every),
        ("stack underflow", [a, ("add",)], 1, 1, every),
        ("neg of nothing", [("neg",)], 1, 1, every),
        ("two values left", [a, b], 2, 1, every),
        ("annotated form over 2 * EXPR_MAX_OPS words", over, 16, 1, ("lazy", "source")),
    ], over


REFUSAL_SCRIPT = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import contangle_zkcp_amd as zk
import test_expr_corpus as t
zk.load()
for label, ops, nc, nk, paths in t.refused_programs()[0]:
    if "source" not in paths:
        continue
    try:
        zk.halo2.expr_specialised_source("PallasFp", ops, nc, nk)
        print("ACCEPTED", label)
    except zk.ZkError as e:
        print("REFUSED", label, e.status)
"""


def test_refusals_of_the_source_function():
    out = _child(REFUSAL_SCRIPT % {"root": ROOT})
    labels = [r[0] for r in refused_programs()[0]]
    for lab in labels:
        assert ("REFUSED " + lab) in out, (lab, out[-2000:])
    assert "ACCEPTED" not in out, out


def test_refusals_of_the_emulated_evaluators(zk_emu):
    zk = zk_emu
    n = 1 << 4
    progs, over = refused_programs()
    for label, ops, nc, nk, paths in progs:
        cols = [np.zeros((n, 4), dtype=np.uint64) for _ in range(nc)]
        ks = np.zeros((nk, 4), dtype=np.uint64)
        for lazy in (False, True):
            if ("lazy" if lazy else "saturated") not in paths:
                continue
            with pytest.raises(zk.ZkError):
                zk.halo2.evaluate_expression("PallasFp", ops, cols, ks, 4, 1, np.zeros((n, 4), dtype=np.uint64), lazy=lazy)
    # the over-long annotated form is the lazy walk's limit only: the saturated interpreter evaluates that program
    assert len(over) == xp.EXPR_MAX_OPS and xp.depth(over) is not None
    ex = xp.Program("over", "limit", over, 16, 1)
    cols, consts = xp.input_words("PallasFp", ex, n, "mixed")
    out = np.zeros((n, 4), dtype=np.uint64)
    zk.halo2.evaluate_expression("PallasFp", over, [xp.words_array(c) for c in cols], xp.words_array(consts), 4, 1, out)
    assert (out == xp.expected("PallasFp", ex, cols, consts, n, xp.R_MONT)).all()


@pytest.mark.parametrize("op", [("col", 0, 40000), ("col", 0, -40000), ("col", 0, 32768), ("col", 0, -32769), ("col", -1, 0),
                                ("const", -1), ("scale", -2), ("col", 1 << 32, 0), ("col", 0), ("mul", 1), ("pow",)])
def test_mirror_refuses_ops_it_cannot_represent(zk_emu, op):
    """ctypes would write a rotation of 40000 as -25536 and an index of -1 as 2^32 - 1: the mirror refuses them instead"""
    zk = zk_emu
    n = 1 << 4
    prog = [("col", 0, 0), ("const", 0), ("add",)] + ([op] if op[0] in ("scale", "neg") else [op, ("mul",)])
    cols = [np.zeros((n, 4), dtype=np.uint64)]
    ks = np.zeros((1, 4), dtype=np.uint64)
    for lazy in (False, True):
        with pytest.raises(zk.ZkError):
            zk.halo2.evaluate_expression("PallasFp", prog, cols, ks, 4, 1, np.zeros((n, 4), dtype=np.uint64), lazy=lazy)
    with pytest.raises(zk.ZkError):
        zk.halo2.expr_specialised_source("PallasFp", prog, 1, 1)      # (refused before the library is asked: the emulator has no source)


def test_mirror_keeps_the_int16_extremes(zk_emu):
    """-32768 and 32767 are representable and evaluated as stated (not refused, not wrapped)"""
    zk = zk_emu
    n, scale = 1 << 5, 3
    p = xp.Program("int16_edges", "rot", [("col", 0, 32767), ("col", 0, -32768), ("sub",)], 1, 1, rot_scale=scale)
    cols, consts = xp.input_words("PallasFp", p, n, "mixed")
    out = np.zeros((n, 4), dtype=np.uint64)
    zk.halo2.evaluate_expression("PallasFp", p.ops, [xp.words_array(c) for c in cols], xp.words_array(consts), 5, scale, out)
    assert (out == xp.expected("PallasFp", p, cols, consts, n, xp.R_MONT)).all()
