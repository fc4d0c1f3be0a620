"""CPU: the F29 field primitives (9 x 29-bit lazy limbs, zk_field29.h) against Python integers, at random AND at the
extreme limb values the bound discipline permits (where a wrong bound would overflow a column or a word), plus the
machine check of the bounds of every curve formula (tools/check_f29_bounds.py).  The generators and their assertions
live in tests/field_cases.py, where the device probe (tests/test_field_probe_gpu.py) shares them; all six F29<>
instantiations of zk_params29.h run the single-field tests."""
import os
import subprocess
import sys

import pytest

import field_cases as fc

ROOT = fc.ROOT
FIELDS = fc.FIELDS
assert FIELDS == ["PallasFp", "PallasFq", "Bn254Fr", "Bls381Fr", "Bn254Fq", "Bls381Fq"]


def run_and_check(cases):
    assert cases
    fc.check(cases, fc.run(cases))


def test_bound_checker():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_f29_bounds.py")], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "all F29 bounds hold" in r.stdout, r.stdout


@pytest.mark.parametrize("field", FIELDS)
def test_f29_mul_extremes(field):
    run_and_check(fc.mul_extremes(field))


@pytest.mark.parametrize("field", FIELDS)
def test_f29_sub_norm_canon(field):
    run_and_check(fc.sub_cases(field))
    cases = fc.norm_carry_canon_cases(field)
    assert {c[1] for c in cases} == {"norm", "carry", "canon"}
    run_and_check(cases)


@pytest.mark.parametrize("field", FIELDS)
def test_f29_conversion_and_zero_filter(field):
    run_and_check(fc.conversion_cases(field))
    run_and_check(fc.zero_filter_cases(field))


@pytest.mark.parametrize("field", fc.FQ2_FIELDS)
def test_f29_fq2_mul_sqr_extremes(field):
    """Fe29x2 (the G2 coordinates): product with a negated operand and one reduction per component, complex square,
    refresh, zero test -- at the limb / value bounds tools/check_f29_bounds.py allows at their call sites"""
    run_and_check(fc.fq2_cases(field))


@pytest.mark.parametrize("field", FIELDS)
def test_f29_sqr_and_mulacc(field):
    """the dedicated square (doubled operand, symmetric half of the products) and the two-product multiply with one
    reduction, at the widest operands their call sites produce"""
    run_and_check(fc.sqr_mulacc_cases(field))
