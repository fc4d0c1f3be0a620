"""CPU tier: the option space of the NTT launch sequence (pass plan, lazy / saturated limbs, g_pre / g_post, zero extension,
n^-1, ZK_NTT_OUT_R29, ZK_NTT_OUT_SUBCOSETS, in place / out of place) at log n = 0 .. 12 in the emulator build of the HIP
sources (tests/emu), exact against a Python-integer DFT (tests/ntt_option_cases.py).  One item is one plan of one field over
a run of (log n, log_in) cells cut to a few seconds (ntt_option_cases.cut_items); tests/test_ntt_options_gpu.py (-m gpu) runs the same sample on the MI355X and adds the large sizes."""
import importlib.util
import os

import pytest

import ntt_option_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_reference_is_pinned():
    nc.check_reference()


@pytest.mark.parametrize("field,plan,part", nc.ITEMS)
def test_ntt_options(zk, field, plan, part):
    nc.check_plan(zk, field, plan, part)


@pytest.mark.parametrize("field", nc.FIELDS)
def test_host_entry_points(zk, field):
    nc.check_host(zk, field)
