"""CPU tier: the field-side kernels of the halo2 prover at launch and operand edges, in the emulator build of the HIP sources
(tests/emu) against the Python-integer reference of tests/halo2_field_edge_cases.py.  Zeros in the batch inversion, small lengths,
the evaluation stride and the documented aliasing run in full; the scan runs up to 257 tiles (per = 2 in scan_totals_kernel, lanes past
the end empty); the cases past one grid are he.SECOND_TRIP_EMU, at present all of them (1 - 12 s each, most of it the Python
reference).  511 and 513 tiles and the real gate are tests/test_halo2_field_edges_gpu.py (-m gpu).  (The emulator launches zk_poly_eval_batch_device's polynomials one by
one, so there the stride is checked in the host's pointer arithmetic only.)"""
import importlib.util
import os

import pytest

import halo2_field_edge_cases as he

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    spec = importlib.util.spec_from_file_location("zk_build", os.path.join(ROOT, "contangle-zkcp_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


@pytest.fixture(scope="module")
def zk():
    emu = _build().build_emu()
    import contangle_zkcp_amd as zk
    zk.load(path=emu)
    zk.init(0)
    assert zk.backend_info().startswith("emu")
    yield zk
    zk.shutdown()
    zk._lib = None


# ---- A
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("n", he.SCAN_NS_EMU)
def test_scan_depth(zk, n, in_place):
    he.check_scan(zk, "PallasFp", n, in_place)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_scan_depth_bls381(zk, in_place):
    he.check_scan(zk, "Bls381Fr", he.SCAN_ALIAS_N, in_place)


def test_scan_zero_in_last_tile(zk):
    he.check_scan_zero_in_last_tile(zk, "PallasFp", he.SCAN_ALIAS_N + 2000)      # 257 tiles, the zero in the last one


# ---- B
@pytest.mark.parametrize("case", he.SECOND_TRIP_EMU)
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
