"""GPU tier (-m gpu): the generated program corpus (tests/expr_programs.py) through every quotient evaluator on the MI355X,
bit-exact against oracle/pyref_halo2.eval_program on Python integers:
  * zk_expr_eval_device (saturated limbs, Montgomery columns), the lazy-limb interpreter (expr_configure("never")) and the kernel
    compiled for the program by hiprtc (expr_configure("always"), 4 slots) on every row, at 2^8 .. 2^12 extended rows, all four
    scalar fields;
  * PallasFp: the compiled kernel at 1 / 2 / 3 / 4 / 5 / 8 slots (ZK_EXPR_JIT_SLOTS) and at 1 / 2 / 4 waves (ZK_EXPR_JIT_WAVES, its
    __launch_bounds__ and with it the register allocation);
  * one program at 2^21 rows in "auto" mode (the compiled kernel) and "never" mode: past both kernels' grid caps, so their
    grid-stride loops run; checked on sampled rows including every row whose rotations wrap.
Every case that claims the compiled kernel proves it ran: with ZK_EXPR_STATS=1 the library writes "expr jit: ... bytes of code
object" on the first call for a source and "expr jit: compilation failed" when hiprtc fails (after which the interpreter would
quietly run instead)."""
import re
import time

import numpy as np
import pytest

import expr_programs as xp
import parity_suite as ps

pytestmark = pytest.mark.gpu

BUILT_RE = re.compile(r"expr jit: (\d+) bytes of source -> (\d+) bytes of code object")
FAILED = "expr jit: compilation failed"
SLOT_SWEEP = [1, 2, 3, 4, 5, 8]
WAVES = [1, 2, 4]
SWEEP_PROGRAMS = ["slot_pool_12", "reuse_distances", "gate2", "bias_ladder", "one_column_rotations"]
WAVE_PROGRAMS = ["gate1", "unnormalised", "slot_pool_5"]
_BUILT = set()          # (field, source) built in this process: the library caches the code object per (device, source)
_TIMES = []             # (field, program, slots, waves, seconds of the first call, bytes of source, bytes of code object)


@pytest.fixture(scope="module")
def zk():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    import contangle_zkcp_amd as zk
    zk._lib = None
    zk.load()
    zk.init(0)
    assert zk.backend_info().startswith("hip gfx950"), zk.backend_info()
    yield zk
    zk.halo2.expr_configure("auto")
    zk.shutdown()
    if _TIMES:
        tot = sum(t[4] for t in _TIMES)
        print("\nexpr jit builds: %d, %.1f s in first calls (hiprtc + one launch)" % (len(_TIMES), tot))
        for t in _TIMES:
            print("  %-9s %-22s slots %-4s waves %-4s %6.2f s  %6d B source -> %7d B code object" % t)


@pytest.fixture
def stats(monkeypatch):
    monkeypatch.setenv("ZK_EXPR_STATS", "1")
    yield monkeypatch


def _lazy(zk, field, prog, d_cols, consts, log_n, out, mode, capfd, label=("", None, None)):
    """zk_expr_eval_lazy_device in `mode`; for the compiled kernel, proof from the library's stderr that it was built (first call
    for its source) and never failed to build"""
    import torch
    zk.halo2.expr_configure(mode)
    src = zk.halo2.expr_specialised_source(field, prog.ops, prog.n_cols, prog.n_consts) if mode != "never" else None
    capfd.readouterr()
    t0 = time.time()
    try:
        zk.halo2.evaluate_expression(field, prog.ops, d_cols, consts, log_n, prog.rot_scale, out, lazy=True)
        torch.cuda.synchronize()
    finally:
        zk.halo2.expr_configure("auto")
    dt = time.time() - t0
    err = capfd.readouterr().err
    assert FAILED not in err, err[-2000:]
    if src is not None and (field, src) not in _BUILT:
        m = BUILT_RE.search(err)
        assert m, ("the compiled kernel was not built", field, prog.name, err[-2000:])
        assert int(m.group(1)) == len(src)
        _BUILT.add((field, src))
        _TIMES.append((field, prog.name, label[1], label[2], dt, len(src), int(m.group(2))))
    return ps.to_host(zk, out)


def _programs():
    """(log_n, program): the corpus at 2^8 .. 2^12 rows -- long programs at the small sizes (the reference is Python)"""
    out = []
    for i, p in enumerate(xp.corpus(8)):
        log_n = 8 + i % 5 if len(p.ops) <= 120 else 8 + i % 2
        out.append((log_n, next(q for q in xp.corpus(log_n) if q.name == p.name)))
    return out


def _run_all_paths(zk, field, log_n, p, kind, capfd, jit_only=False, label=None):
    n = 1 << log_n
    cols, consts, exp_lazy = _case(field, p, log_n, kind, xp.R_LAZY)
    d_cols = [ps.to_device(zk, xp.words_array(c)) for c in cols]
    out = ps.to_device(zk, np.zeros((n, 4), dtype=np.uint64))
    kc = xp.mont_words_for_lazy_consts(field, consts)
    modes = ["always"] if jit_only else ["never", "always"]
    for mode in modes:
        got = _lazy(zk, field, p, d_cols, kc, log_n, out, mode, capfd, label or (field, 4, 2))
        bad = np.nonzero((got != exp_lazy).any(axis=1))[0]
        assert len(bad) == 0, (field, p.name, log_n, kind, mode, label, bad[:8].tolist())
    if jit_only:
        return
    # saturated limbs: the same words read as Montgomery words
    _, _, exp_mont = _case(field, p, log_n, kind, xp.R_MONT)
    zk.halo2.evaluate_expression(field, p.ops, d_cols, xp.words_array(consts), log_n, p.rot_scale, out)
    got = ps.to_host(zk, out)
    bad = np.nonzero((got != exp_mont).any(axis=1))[0]
    assert len(bad) == 0, (field, p.name, log_n, kind, "saturated", bad[:8].tolist())


_CASES = {}


def _case(field, p, log_n, kind, radix):
    key = (field, p.name, log_n, kind, radix)
    if key not in _CASES:
        cols, consts = xp.input_words(field, p, 1 << log_n, kind)
        _CASES[key] = (cols, consts, xp.expected(field, p, cols, consts, 1 << log_n, radix))
    return _CASES[key]


def test_hiprtc_builds_the_quotient_kernel(zk, stats, capfd):
    """guard for the whole suite: the "always" checks elsewhere also pass when hiprtc fails and the interpreter runs instead"""
    p = xp.Program("hiprtc_guard", "limit", [("col", 0, 3), ("const", 1), ("mul",), ("col", 0, -3), ("scale", 0), ("sub",)], 1, 2)
    _run_all_paths(zk, "PallasFp", 6, p, "mixed", capfd)
    assert any(f == "PallasFp" and "hiprtc_guard" == t for f, t, *_ in _TIMES)


@pytest.mark.parametrize("field", xp.FIELDS)
def test_corpus_every_path_every_row(zk, stats, capfd, field):
    for log_n, p in _programs():
        for kind in ("mixed", "dense"):
            _run_all_paths(zk, field, log_n, p, kind, capfd)


@pytest.mark.parametrize("slots", SLOT_SWEEP)
def test_compiled_kernel_slot_sweep(zk, stats, capfd, slots):
    stats.setenv("ZK_EXPR_JIT_SLOTS", str(slots))
    for log_n, p in _programs():
        if p.name in SWEEP_PROGRAMS:
            src = zk.halo2.expr_specialised_source("PallasFp", p.ops, p.n_cols, p.n_consts)
            assert "    Fe<F> %s;\n" % ", ".join("s%d" % q for q in range(slots)) in src
            for kind in ("mixed", "dense"):
                _run_all_paths(zk, "PallasFp", log_n, p, kind, capfd, jit_only=True, label=("PallasFp", slots, 2))


@pytest.mark.parametrize("waves", WAVES)
def test_compiled_kernel_waves(zk, stats, capfd, waves):
    stats.setenv("ZK_EXPR_JIT_WAVES", str(waves))
    for log_n, p in _programs():
        if p.name in WAVE_PROGRAMS:
            src = zk.halo2.expr_specialised_source("PallasFp", p.ops, p.n_cols, p.n_consts)
            assert "__launch_bounds__(64, %d)" % waves in src
            for kind in ("mixed", "dense"):
                _run_all_paths(zk, "PallasFp", log_n, p, kind, capfd, jit_only=True, label=("PallasFp", 4, waves))


class _WordColumn:
    """a stored-word column seen as the Python integers behind the words (x = w / R'), converted on access"""

    def __init__(self, arr, inv, p):
        self.arr, self.inv, self.p = arr, inv, p

    def __getitem__(self, i):
        w = self.arr[i]
        return (int(w[0]) | int(w[1]) << 64 | int(w[2]) << 128 | int(w[3]) << 192) * self.inv % self.p


def test_corpus_program_at_2p21_rows(zk, stats, capfd):
    """2^21 rows: the compiled kernel's grid is capped at CUs x 4 x waves x 4 blocks of 64 lanes (2^19 rows on 256 CUs), the
    interpreter's at 16384 blocks of 64 lanes (2^20 rows), so both run their grid-stride loops"""
    from oracle import pyref
    field, log_n = "PallasFp", 21
    n = 1 << log_n
    p = next(q for q in xp.corpus(log_n) if q.name == "gate2")
    prime = pyref.FIELDS[field][0]
    ex = xp.extremes(field)
    cols = []
    for c in range(p.n_cols):
        a = ps.rand_field(field, n, 0x2100 + c).copy()            # uniform canonical words
        a[c::p.n_cols] = xp.words_array([ex[c % len(ex)]])          # every n_cols-th row an extreme
        a[:4] = xp.words_array(ex[:4])
        a[-4:] = xp.words_array(ex[-4:])
        cols.append(a)
    consts = [ex[4], ex[2], ex[1], ex[3], 12345][:p.n_consts]
    d_cols = [ps.to_device(zk, a) for a in cols]
    out = ps.to_device(zk, np.zeros((n, 4), dtype=np.uint64))
    kc = xp.mont_words_for_lazy_consts(field, consts)
    got = {}
    for mode in ("auto", "never"):
        got[mode] = _lazy(zk, field, p, d_cols, kc, log_n, out, mode, capfd, (field, 4, 2)).copy()
    assert (field, zk.halo2.expr_specialised_source(field, p.ops, p.n_cols, p.n_consts)) in _BUILT
    assert (got["auto"] == got["never"]).all()
    span = max(abs(o[2]) for o in p.ops if o[0] == "col") * p.rot_scale
    rng = pyref.Rng(21)
    rows = set(range(span + 1)) | set(range(n - span - 1, n))                   # every row whose rotations wrap
    for cap in (1 << 19, 1 << 20):                                              # the first rows of each kernel's second stride
        rows |= {cap - 1, cap, cap + 1, 2 * cap - 1, 2 * cap}
    rows |= {rng.below(n) for _ in range(64)}
    rows = sorted(r for r in rows if 0 <= r < n)
    inv = pow(xp.R_LAZY, -1, prime)
    icols = [_WordColumn(a, inv, prime) for a in cols]
    ik = [w * inv % prime for w in consts]
    from oracle import pyref_halo2 as h2
    exp = xp.words_array([h2.eval_program(field, p.ops, icols, ik, n, p.rot_scale, i) * xp.R_MONT % prime for i in rows])
    for mode in ("auto", "never"):
        bad = [r for r, g, e in zip(rows, got[mode][rows], exp) if (g != e).any()]
        assert not bad, (mode, bad[:8])
