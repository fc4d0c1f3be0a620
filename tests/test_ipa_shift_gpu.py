"""GPU tier (-m gpu): the generator collapse over shift tables (zk_bases_precompute_shifts) on the device, at 2^10 points, and the
automatic build at 2^16 -- the checks are tests/ipa_shift_suite.py."""
import pytest

import ipa_shift_suite as suite

pytestmark = pytest.mark.gpu
CURVES = ["Vesta", "Pallas", "Bn254G1"]


@pytest.fixture(scope="module")
def zk():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    import contangle_zkcp_amd as zk
    zk._lib = None
    zk.load()                       # the in-tree HIP library; raises if missing
    zk.init(0)
    info = zk.backend_info()
    assert info.startswith("hip gfx950"), info
    yield zk
    zk.shutdown()


@pytest.mark.parametrize("cname", CURVES)
def test_collapse_three_way(zk, cname):
    suite.check_three_way(zk, cname, 10)


@pytest.mark.parametrize("cname", CURVES)
def test_collapse_crafted_weights(zk, cname):
    suite.check_crafted_weights(zk, cname)


@pytest.mark.parametrize("cname", CURVES)
def test_collapse_wider_handle(zk, cname):
    suite.check_wider_handle(zk, cname, 10)


@pytest.mark.parametrize("cname", CURVES)
def test_collapse_after_refresh(zk, cname):
    suite.check_refresh(zk, cname, 10)


def test_collapse_builds_tables_on_second_use(zk):
    suite.check_automatic(zk, "Vesta")
