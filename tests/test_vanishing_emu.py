"""CPU tier: the halo2 quotient against the vanishing identity (tests/vanishing_cases.py) in the emulator build of the HIP sources
(tests/emu), k = 4 .. 6: the bench's program in all four scalar fields, the corpus programs of degree <= 15 (extended ratios 1, 2,
4, 8 and 16), a genuine lookup with no aux column, and the negative controls that show the checker detects each fault.  Routes
(a), (b) and (d); the hiprtc kernel (c) and the large shapes are in tests/test_vanishing_gpu.py (-m gpu)."""
import importlib.util
import os

import pytest

import vanishing_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOKUP_DISTS = ["range_check", "random_dups", "extremes", "low_byte"]


@pytest.fixture(scope="module")
def zk():
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


def _routes(ratio):
    return ["saturated", "never"] + vc.part_routes(ratio, modes=("never", "saturated"))


def test_degree():
    assert vc.degree([("col", 0, 1)]) == 1 and vc.degree([("const", 0)]) == 0
    assert vc.degree([("col", 0, 0), ("col", 1, 0), ("mul",), ("const", 0), ("add",), ("neg",), ("scale", 0)]) == 2
    assert vc.degree([("col", 0, 0), ("col", 0, 0), ("col", 0, 0), ("mul",), ("mul",), ("col", 1, 0), ("sub",)]) == 3
    prog, _, _ = vc.bench_program()
    assert vc.degree(prog) == 6 and vc.degree(vc.LOOKUP_PROGRAM) == 3
    ratios = {vc.extended_ratio(vc.degree(ops + [("col", nc, 0), ("sub",)])) for _, ops, nc, _ in vc.corpus_programs(5)}
    assert ratios == {1, 2, 4, 8, 16}


def test_barycentric_against_eval_program(zk):
    """the right-hand side's two tools on their own: a column's polynomial at omega^r from the barycentric formula is the
    Lagrange value r rows on; the point evaluator agrees with eval_program there"""
    from oracle import pyref
    from oracle import pyref_halo2 as h2
    p = pyref.FIELDS["PallasFp"][0]
    n = 8
    w = vc._int("PallasFp", zk.root_of_unity("PallasFp", 3))
    assert pow(w, n, p) == 1 and pow(w, n // 2, p) != 1
    wpow = [pow(w, i, p) for i in range(n)]
    rng = pyref.Rng(5)
    vals = [rng.below(p) for _ in range(n)]
    # at a point outside H: against the coefficients by an O(n^2) inverse DFT
    coef = [sum(vals[i] * pow(w, (-i * t) % n, p) for i in range(n)) * pow(n, -1, p) % p for t in range(n)]
    z = rng.below(p)
    assert vc.barycentric(p, vals, wpow, z) == vc.horner(p, coef, z)
    prog = [("col", 0, 1), ("col", 1, -1), ("mul",), ("const", 0), ("sub",), ("col", 0, 0), ("neg",), ("scale", 0), ("add",)]
    cols = [vals, vals[::-1]]
    for i in range(n):
        v = vc.eval_at("PallasFp", prog, lambda c, r: cols[c][(i + r) % n], [7])
        assert v == h2.eval_program("PallasFp", prog, cols, [7], n, 1, i)


@pytest.mark.parametrize("field", vc.FIELDS)
def test_bench_program(zk, field):
    prog, nc, nk = vc.bench_program()
    case = vc.aux_case(zk, field, prog, nc, nk, 5, seed=3)
    assert case.ratio == 8 and case.d == 6 and case.dom.extended_k == 8
    vc.check_routes(case, _routes(case.ratio))
    # (i) at the bench's own shape: the quotient's pieces 5, 6 and 7 (of 8) are all zero
    h, _ = case.route("never")
    assert (h[5 * case.n:] == 0).all() and (h[:5 * case.n] != 0).any()


@pytest.mark.parametrize("k", [4, 6])
def test_bench_program_other_sizes(zk, k):
    prog, nc, nk = vc.bench_program()
    case = vc.aux_case(zk, "PallasFp", prog, nc, nk, k, seed=k)
    vc.check_routes(case, _routes(case.ratio))


@pytest.mark.parametrize("name", [q[0] for q in vc.corpus_programs(5)])
def test_corpus_program(zk, name):
    i = [q[0] for q in vc.corpus_programs(5)].index(name)
    k = 4 + i % 3
    field = vc.FIELDS[i % 4]
    _, ops, nc, nk = next(q for q in vc.corpus_programs(k) if q[0] == name)
    case = vc.aux_case(zk, field, ops, nc, nk, k, seed=11 + i)
    vc.check_routes(case, _routes(case.ratio))


@pytest.mark.parametrize("dist", LOOKUP_DISTS)
def test_lookup(zk, dist):
    for j, field in enumerate(vc.FIELDS):
        case = vc.lookup_case(zk, field, dist, 4 + j % 3, seed=2 + j)
        assert case.ratio == 4
        vc.check_routes(case, _routes(case.ratio))


# ------------------------------------------------------------------------------------------------------------ negative controls
@pytest.mark.parametrize("spec", ["saturated", "never", ("part", 4, "part", "never"), ("part", 8, "whole", "saturated")])
def test_detects_changed_lagrange_value(zk, spec):
    prog, nc, nk = vc.bench_program()
    case = vc.aux_case(zk, "PallasFp", prog, nc, nk, 5, seed=3, corrupt=(0, 9))
    vc.assert_detected(case, spec)


def test_detects_changed_aux_value(zk):
    _, ops, nc, nk = next(q for q in vc.corpus_programs(4) if q[0] == "gate1")
    case = vc.aux_case(zk, "Bn254Fr", ops, nc, nk, 4, seed=5, corrupt=(nc, 0))
    vc.assert_detected(case, "saturated")
    vc.assert_detected(case, ("part", 2, "whole", "never"))


@pytest.mark.parametrize("fault", ["rot_scale_x2", "rot_neg"])
@pytest.mark.parametrize("spec", ["saturated", "never", ("part", 2, "part", "never"), ("part", 8, "whole", "saturated")])
def test_detects_wrong_rotation(zk, fault, spec):
    prog, nc, nk = vc.bench_program()
    case = vc.aux_case(zk, "PallasFq", prog, nc, nk, 5, seed=4)
    vc.assert_detected(case, spec, fault)


@pytest.mark.parametrize("fault", ["rot_scale_x2", "rot_neg"])
def test_detects_wrong_rotation_corpus(zk, fault):
    """rotations that wrap H many times over (+-32767 with n = 32)"""
    _, ops, nc, nk = next(q for q in vc.corpus_programs(5) if q[0] == "rot_wrap")
    case = vc.aux_case(zk, "Bls381Fr", ops, nc, nk, 5, seed=6)
    assert case.ratio == 2
    vc.assert_detected(case, "never", fault)
    vc.assert_detected(case, ("part", 2, "part", "never"), fault)


@pytest.mark.parametrize("spec", [("part", 2, "part", "never"), ("part", 8, "whole", "never"), ("part", 8, "part", "saturated")])
def test_detects_swapped_subcosets(zk, spec):
    prog, nc, nk = vc.bench_program()
    case = vc.aux_case(zk, "PallasFp", prog, nc, nk, 5, seed=7)
    vc.assert_detected(case, spec, "swap_parts")


@pytest.mark.parametrize("field", ["PallasFp", "Bn254Fr"])
def test_lookup_detects_swapped_rows(zk, field):
    case = vc.lookup_case(zk, field, "random_dups", 5, seed=9, swap_rows=True)
    vc.assert_detected(case, "saturated")
    vc.assert_detected(case, ("part", 4, "part", "never"))
