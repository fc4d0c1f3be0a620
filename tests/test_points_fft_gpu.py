"""GPU tier (-m gpu): the DFT of a vector of curve points on a real MI355X (tests/points_fft_cases.py).  Which k crosses which
path of the schedule (stage s of log n runs with one twiddle per wave while n / 2^(s+1) >= 64, per lane afterwards):
  k = 0            no stage: load, normalise
  k = 1            one stage, the twiddle 1 only, a single partial wave
  k = 2, 3, 5      every stage per lane; one partial wave (n / 2 < 64)
  k = 7            the first stage uniform (exactly 64 blocks), six per lane; the twiddle table is first read here
  k = 10, 13, 14   4 / 7 / 8 uniform stages ahead of the six per-lane ones; several waves per twiddle and several twiddles per
                   launch; the twiddle kernel's grid exceeds one workgroup (k >= 10)
  k = 18, 20       at size (Pallas, Vesta): Params.from_g, sampled against the oracle, a linear combination over all n"""
import pytest

import points_fft_cases as pc

pytestmark = pytest.mark.gpu
KS = [0, 1, 2, 3, 5, 7, 10, 13, 14]


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


@pytest.mark.parametrize("curve", pc.CURVES)
@pytest.mark.parametrize("k", KS)
def test_forward_inverse_round_trip(zk, curve, k):
    pc.check_transform(zk, curve, k)


@pytest.mark.parametrize("curve", pc.CURVES)
@pytest.mark.parametrize("k", [0, 1, 2, 3, 5])
def test_against_the_definition(zk, curve, k):
    pc.check_direct(zk, curve, k)


@pytest.mark.parametrize("curve", pc.CURVES)
@pytest.mark.parametrize("k", KS)
def test_degenerate_inputs(zk, curve, k):
    pc.check_degenerate(zk, curve, k)


@pytest.mark.parametrize("curve", pc.CURVES)
@pytest.mark.parametrize("k", KS)
def test_commit_lagrange_equals_commit(zk, curve, k):
    pc.check_commit_property(zk, curve, k)


@pytest.mark.parametrize("curve", pc.CURVES)
@pytest.mark.parametrize("k", KS)
def test_host_jacobian_entry_point(zk, curve, k):
    pc.check_host_jacobian(zk, curve, k)


@pytest.mark.parametrize("curve", pc.CURVES)
def test_refusals(zk, curve):
    pc.check_refusals(zk, curve)


def test_at_size_vesta_2_20(zk):
    pc.check_at_size(zk, "Vesta", 20)


def test_at_size_pallas_2_18(zk):
    pc.check_at_size(zk, "Pallas", 18)
