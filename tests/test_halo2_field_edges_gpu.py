"""GPU tier (-m gpu): the field-side kernels of the halo2 prover at launch and operand edges on a real MI355X -- the checks of
tests/halo2_field_edge_cases.py against the Python-integer reference written there, exact on Montgomery limbs.

What the shapes are for (he.TILE = 4096 elements per scan workgroup, he.G / he.G_WIDE / he.G_IP = one grid of a capped kernel):
  test_scan_*            scan_totals_kernel owning more than one tile total per lane: 257 tiles (per = 2, lanes 129 .. 255 empty), 511
                         (per = 2, the last lane owns one tile), 513 (per = 3, lanes from 171 on empty), in place and out of place
  test_second_trip       every grid-capped kernel at one grid + 257 elements with 0 first and p - 1 last; permutation_product at k = 21
                         through the local relation z[i + 1] den_i = z[i] num_i on a fixed row set
  test_batch_invert_*    zeros through the inversion 16 elements share; a zero denominator through both grand products
  test_*_small           lengths 0, 1, 2 and around one workgroup; vectors of 0, 1, p - 1
  test_eval_batch_stride zk_poly_eval_batch_device with polynomials further apart than they are long
  test_alias_*           out == b, out == a source, in == out as the headers document them; a partial overlap refused"""
import pytest

import halo2_field_edge_cases as he

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    import contangle_zkcp_amd as zk
    zk._lib = None
    zk.load()
    zk.init(0)
    info = zk.backend_info()
    assert info.startswith("hip gfx950"), info
    yield zk
    zk.shutdown()


# ---- A
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("n", he.SCAN_NS)
def test_scan_depth(zk, n, in_place):
    he.check_scan(zk, "PallasFp", n, in_place)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_scan_depth_bls381(zk, in_place):
    he.check_scan(zk, "Bls381Fr", he.SCAN_ALIAS_N, in_place)


def test_scan_zero_in_last_tile(zk):
    he.check_scan_zero_in_last_tile(zk, "PallasFp")


# ---- B
@pytest.mark.parametrize("case", sorted(he.SECOND_TRIP))
def test_second_trip(zk, case):
    he.run_second_trip(zk, case)


# ---- C
@pytest.mark.parametrize("n", he.INVERT_NS)
@pytest.mark.parametrize("field", he.INVERT_FIELDS)
def test_batch_invert_zeros(zk, field, n):
    he.check_batch_invert_zeros(zk, field, n)


@pytest.mark.parametrize("field", he.INVERT_FIELDS)
def test_lookup_product_zero_denominator(zk, field):
    he.check_lookup_zero_denominator(zk, field)


@pytest.mark.parametrize("field", he.INVERT_FIELDS)
def test_permutation_product_zero_denominator(zk, field):
    he.check_permutation_zero_denominator(zk, field)


# ---- D
@pytest.mark.parametrize("n", he.SMALL_NS)
@pytest.mark.parametrize("field", he.SMALL_FIELDS + ("Bls381Fr",))
def test_inner_product_small(zk, field, n):
    he.check_inner_product_small(zk, field, n)


@pytest.mark.parametrize("field", he.SMALL_FIELDS + ("Bls381Fr",))
def test_inner_product_of_minus_ones(zk, field):
    he.check_inner_product_minus_ones(zk, field)


@pytest.mark.parametrize("half", he.SMALL_NS)
@pytest.mark.parametrize("field", he.SMALL_FIELDS)
def test_vec_fold_small(zk, field, half):
    he.check_vec_fold_small(zk, field, half)


@pytest.mark.parametrize("half", he.SMALL_NS)
@pytest.mark.parametrize("field", he.SMALL_FIELDS)
def test_ipa_fold_round_small(zk, field, half):
    he.check_ipa_fold_round_small(zk, field, half)


@pytest.mark.parametrize("field", he.SMALL_FIELDS)
def test_ipa_fold_round_weights_small(zk, field):
    he.check_ipa_fold_round_weights_small(zk, field)


@pytest.mark.parametrize("field", he.SMALL_FIELDS)
def test_ipa_fold_round_refuses_zero_challenge(zk, field):
    he.check_ipa_fold_round_refuses_zero(zk, field)


@pytest.mark.parametrize("field", he.SMALL_FIELDS)
def test_ipa_scalar_helpers_small(zk, field):
    he.check_ipa_scalar_helpers_small(zk, field)


# ---- E
@pytest.mark.parametrize("n", he.EVAL_NS)
def test_eval_batch_stride(zk, n):
    he.check_eval_batch_stride(zk, "PallasFp", n)


# ---- F
@pytest.mark.parametrize("field", he.SMALL_FIELDS)
def test_alias_muladd_into_b(zk, field):
    he.check_muladd_into_b(zk, field)


@pytest.mark.parametrize("field", he.SMALL_FIELDS)
def test_alias_fold_many_into_a_source(zk, field):
    he.check_fold_many_into_source(zk, field)


def test_alias_prefix_product_in_place(zk):
    he.check_scan(zk, "PallasFp", he.SCAN_ALIAS_N, True)


@pytest.mark.parametrize("field", he.SMALL_FIELDS)
def test_alias_fold_many_refuses_partial_overlap(zk, field):
    he.check_fold_many_refuses_partial_overlap(zk, field)
