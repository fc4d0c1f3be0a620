"""GPU tier (-m gpu): the option space of the NTT launch sequence at log n = 0 .. 12 on a real MI355X -- the same seeded sample
as tests/test_ntt_options_emu.py, exact against a Python-integer DFT (tests/ntt_option_cases.py) -- and the default plan at
log n = 12, 15, 17, 19, 21, 23, 24 (two passes at four radix splits, three passes at (7,7,7), (8,8,7), (8,8,8)) on a geometric
input built on the device, checked in closed form at sampled outputs."""
import pytest

import ntt_option_cases as nc

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


def test_reference_is_pinned():
    nc.check_reference()


@pytest.mark.parametrize("field,plan,part", nc.ITEMS)
def test_ntt_options(zk, field, plan, part):
    nc.check_plan(zk, field, plan, part)


@pytest.mark.parametrize("field", nc.FIELDS)
def test_host_entry_points(zk, field):
    nc.check_host(zk, field)


@pytest.mark.parametrize("field,logn,log_in,pre,post,scale,r29,lp,oop,seed", nc.large_cases())
def test_default_plan_geometric_input(zk, field, logn, log_in, pre, post, scale, r29, lp, oop, seed):
    nc.check_geometric(zk, field, logn, log_in, pre, post, scale, r29, lp, oop, seed)


@pytest.mark.parametrize("field,logn", [(nc.FIELDS[i % 4], logn) for i, logn in enumerate(nc.LARGE_LOGNS) if logn <= 16])
def test_default_plan_random_input(zk, field, logn):
    nc.check_random_large(zk, field, logn, seed=0xA11CE + logn)
