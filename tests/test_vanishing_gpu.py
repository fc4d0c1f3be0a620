"""GPU tier (-m gpu): the halo2 quotient against the vanishing identity (tests/vanishing_cases.py) on the MI355X.
  * k = 10 and 14, the bench's program in all four scalar fields, every route: (a) saturated, (b) the lazy interpreter, (c) the
    kernel compiled for the program by hiprtc, (d) QP = 2, 4, 8 sub-cosets from both coset sources;
  * the corpus programs of degree <= 15 at k = 10 (extended ratios 1 .. 16), every route;
  * the bench's own shape: k = 20 in PallasFp, 31 columns of 2^23 extended rows, QP = 1 in "auto" mode and QP = 8;
  * a genuine lookup (no aux column) at 2^16 and 2^20 rows.
Every route that claims the compiled kernel proves it ran: with ZK_EXPR_STATS=1 the library writes "expr jit: ... bytes of code
object" on the first call for a source and "expr jit: compilation failed" when hiprtc fails (tests/test_expr_corpus_gpu.py)."""
import re
import time

import pytest

import vanishing_cases as vc

pytestmark = pytest.mark.gpu

BUILT_RE = re.compile(r"expr jit: (\d+) bytes of source -> (\d+) bytes of code object")
FAILED = "expr jit: compilation failed"
_BUILT = set()          # (field, source) built in this process
_TIMES = []


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
        print("\nvanishing cases:")
        for t in _TIMES:
            print("  %-40s %7.2f s" % t)


@pytest.fixture
def stats(monkeypatch):
    monkeypatch.setenv("ZK_EXPR_STATS", "1")
    yield monkeypatch


def _caller(zk, case, capfd, jit_modes=("always",)):
    """case.route, and for the compiled kernel the proof from the library's stderr that it was built (on the first call for its
    source) and never failed to build"""
    src = zk.halo2.expr_specialised_source(case.field, case.prog, case.ncols, len(case.consts))

    def call(spec):
        mode = spec[3] if isinstance(spec, tuple) else spec
        capfd.readouterr()
        out = case.route(spec)
        vc._sync(zk)
        err = capfd.readouterr().err
        assert FAILED not in err, err[-2000:]
        if mode in jit_modes and (case.field, src) not in _BUILT:
            m = BUILT_RE.search(err)
            assert m, ("the compiled kernel was not built", case.field, spec, err[-2000:])
            assert int(m.group(1)) == len(src)
            _BUILT.add((case.field, src))
        return out
    return call


def _routes(ratio):
    return ["saturated", "never", "always"] + vc.part_routes(ratio, modes=("never", "always"))


def _timed(label, fn):
    t0 = time.time()
    fn()
    _TIMES.append((label, time.time() - t0))


@pytest.mark.parametrize("k", [10, 14])
@pytest.mark.parametrize("field", vc.FIELDS)
def test_bench_program(zk, stats, capfd, field, k):
    prog, nc, nk = vc.bench_program()

    def run():
        case = vc.aux_case(zk, field, prog, nc, nk, k, seed=3)
        assert case.ratio == 8
        vc.check_routes(case, _routes(case.ratio), call=_caller(zk, case, capfd))
    _timed("bench program %s k=%d" % (field, k), run)


@pytest.mark.parametrize("name", [q[0] for q in vc.corpus_programs(10)])
def test_corpus_program(zk, stats, capfd, name):
    i = [q[0] for q in vc.corpus_programs(10)].index(name)
    field = vc.FIELDS[i % 4]
    _, ops, nc, nk = next(q for q in vc.corpus_programs(10) if q[0] == name)
    case = vc.aux_case(zk, field, ops, nc, nk, 10, seed=11 + i)
    vc.check_routes(case, _routes(case.ratio), call=_caller(zk, case, capfd))


def test_bench_shape(zk, stats, capfd):
    """k = 20, PallasFp: the bench's 30 columns plus aux on 2^23 extended rows (about 8 GB of cosets per route); QP = 1 in "auto"
    mode (the compiled kernel from 2^16 rows on) and QP = 8 from both coset sources; pieces 5, 6 and 7 of h are all zero"""
    prog, nc, nk = vc.bench_program()

    def run():
        case = vc.aux_case(zk, "PallasFp", prog, nc, nk, 20, seed=20)
        assert case.ratio == 8 and case.ncols == 31
        vc.check_routes(case, ["auto", ("part", 8, "whole", "auto"), ("part", 8, "part", "never")],
                        call=_caller(zk, case, capfd, jit_modes=("auto",)))
        h, _ = case.route(("part", 8, "part", "auto"))
        assert bool((h[5 * case.n:] == 0).all()) and bool((h[:5 * case.n] != 0).any())
    _timed("bench shape PallasFp k=20", run)


@pytest.mark.parametrize("dist", ["range_check", "random_dups", "extremes", "low_byte"])
def test_lookup_2_16(zk, stats, capfd, dist):
    field = vc.FIELDS[["range_check", "random_dups", "extremes", "low_byte"].index(dist)]

    def run():
        case = vc.lookup_case(zk, field, dist, 16, seed=5)
        vc.check_routes(case, _routes(case.ratio), call=_caller(zk, case, capfd))
    _timed("lookup %s %s 2^16" % (field, dist), run)


@pytest.mark.parametrize("dist", ["range_check", "random_dups"])
def test_lookup_2_20(zk, stats, capfd, dist):
    def run():
        case = vc.lookup_case(zk, "PallasFp", dist, 20, seed=6)
        vc.check_routes(case, ["auto", ("part", 4, "part", "never"), ("part", 2, "whole", "auto")],
                        call=_caller(zk, case, capfd, jit_modes=("auto",)))
    _timed("lookup PallasFp %s 2^20" % dist, run)


def test_lookup_detects_swapped_rows(zk):
    case = vc.lookup_case(zk, "PallasFp", "random_dups", 16, seed=9, swap_rows=True)
    vc.assert_detected(case, "always")
    vc.assert_detected(case, ("part", 4, "part", "never"))
