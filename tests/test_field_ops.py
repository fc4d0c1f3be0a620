"""CPU: the saturated field ops (zk_field.h), the lazy ops at k p - 1, k p, k p + 1, the conversions on the edge set and
the curve formulas' exceptional branches one call at a time (zk_curve.h, zk_curve29.h), through the g++ runner
tests/emu/f29_check, against Python integers -- for all six fields and all six curves in both limb forms.  The tables are
tests/field_cases.py; tests/test_field_probe_gpu.py sends the same tables to a gfx950 build of the same op table."""
import pytest

import field_cases as fc
from oracle import pyref


def run_and_check(cases):
    assert cases
    fc.check(cases, fc.run(cases))


def test_op_table_lists_every_field_and_curve():
    targets = {t for t, _ in fc.op_table()}
    assert targets == set(fc.FIELDS) | set(fc.CURVE_TARGETS)
    # ids follow oracle/pyref.py's order: the probe is addressed by them
    for i, f in enumerate(pyref.FIELD_IDS):
        assert fc.op_table()[(f, "fe_mul")][0] == i
    for i, c in enumerate(pyref.CURVE_IDS):
        assert fc.op_table()[(c, "xyzz_add")][0] == 100 + 2 * i and fc.op_table()[(c + "29", "xyzz_add")][0] == 101 + 2 * i


@pytest.mark.parametrize("field", fc.FIELDS)
def test_edge_set(field):
    E = fc.edge_set(field)
    p = pyref.FIELDS[field][0]
    n = fc.SHAPE[field][2]
    assert len(E) == len(set(E)) == (33 if n == 12 else 25) and all(0 <= e < p for e in E)     # 1 = 2^0 dropped, last member added
    assert {0, 1, p - 1, (1 << (32 * (n - 1)))} <= set(E)


@pytest.mark.parametrize("field", fc.FIELDS)
def test_saturated_edges(field):
    """all pairs of the edge set for add / sub / mul, the edge set for the unary ops, the directed sums and differences"""
    run_and_check(fc.tables(field)["sat_edge"])


@pytest.mark.parametrize("field", fc.FIELDS)
def test_saturated_uniform(field):
    """4096 uniform pairs, both classes of the Montgomery product's final subtraction present (asserted by the generator)"""
    run_and_check(fc.tables(field)["sat_uniform"])


@pytest.mark.parametrize("field", fc.FQ2_FIELDS)
def test_saturated_fe2(field):
    run_and_check(fc.tables(field)["sat_fe2"])


@pytest.mark.parametrize("field", fc.FIELDS)
def test_lazy_kp(field):
    """canon / carry / norm / tostd / filter / x2iszero at k p - 1, k p, k p + 1 for 0 <= k <= 19, strict and lazy limbs"""
    run_and_check(fc.tables(field)["lazy_kp"])


@pytest.mark.parametrize("field", fc.FIELDS)
def test_lazy_edge_conversions(field):
    """fromstd / tostd round trip, unpack / pack on the saturated edge set"""
    run_and_check(fc.edge_conversion_cases(field))


@pytest.mark.parametrize("field", fc.FIELDS)
def test_slots4_shape(field):
    for order in fc.SLOT_ORDERS:
        run_and_check(fc.slots4_cases(field, order))


def test_canon_r03a_shape():
    run_and_check(fc.canon_r03a_cases())


@pytest.mark.parametrize("target", fc.CURVE_TARGETS)
def test_curve_ops(target):
    """inf + G, G + inf, inf + inf, G + G, G + (-G), G + Q, (2G, ZZ != 1) + 2G, add_nodbl on equal / opposite operands with
    different Z, dbl of inf and G, aff_neg_if -- normalised to affine and compared with pyref"""
    run_and_check(fc.tables(target)["curve"])


@pytest.mark.parametrize("target", fc.FIELDS + fc.CURVE_TARGETS)
def test_every_declared_op_is_exercised(target):
    fc.tables(target)        # asserts the coverage and the operand row lengths
