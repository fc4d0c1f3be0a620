"""CPU tier: zk_halo2_permute_expression_pair_device (the lookup argument's permute_expression_pair on the device) in the
emulator build of the HIP sources (tests/emu), against oracle.pyref_halo2 and the host mirror halo2.permute_expression_pair.
The real gate is tests/test_lookup_permute_gpu.py (-m gpu)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lookup_permute_cases as lc
from parity_suite import _monts, to_device, to_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# usable_rows and the paths they reach (2u merged keys):
#   1, 2        a single run / the smallest multi-run case; 2u < one wave
#   63, 64, 65  2u around two waves: a tile of 256 keys with a partial last wave, and 2u = 128 / 130 around 2 x 64
#   1000        2u = 2000: the key kernel's grid-stride loop over several workgroups, one LSD chunk (4096 keys), many runs
#   2100        2u = 4200 > 4096: two LSD workgroup chunks -- the cross-workgroup count / offset / scatter path and the
#               run scan's block sums (offsets by the one-workgroup scan, up to 8 chunks)
#   16400       2u = 32800: 9 chunks, the offsets by one workgroup per bucket (its loop over > 256 chunks is crossed at the
#               GPU tier's 2^20 rows)
SIZES = [1, 2, 63, 64, 65, 1000]
BIG = 2100
HUGE = 16400


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


@pytest.mark.parametrize("name", lc.FIELDS)
@pytest.mark.parametrize("dist", lc.DISTRIBUTIONS)
def test_permute_small_sizes(zk, name, dist):
    for u in SIZES:
        lc.check_dist(zk, name, dist, u, host_mirror=True, close=(u == 1000))


@pytest.mark.parametrize("name", lc.FIELDS)
@pytest.mark.parametrize("dist", ["range_check", "random_dups"])
def test_permute_multi_workgroup(zk, name, dist):
    lc.check_dist(zk, name, dist, BIG, host_mirror=True)


@pytest.mark.parametrize("dist", ["all_equal", "no_repeats", "extremes", "top_limb", "low_byte"])
def test_permute_multi_workgroup_shapes(zk, dist):
    lc.check_dist(zk, "PallasFp", dist, BIG)


@pytest.mark.parametrize("dist", ["range_check", "low_byte"])
def test_permute_per_bucket_offsets(zk, dist):
    lc.check_dist(zk, "Bn254Fr", dist, HUGE, close=False)


@pytest.mark.parametrize("where", ["below", "above", "between"])
def test_input_not_in_table(zk, where):
    lc.check_missing(zk, "PallasFp", where, 200)


def test_missing_value_repeated(zk):
    lc.check_missing(zk, "Bls381Fr", "between", 500, repeats=120)
    lc.check_missing(zk, "Bn254Fr", "above", 3000, repeats=900)


def test_zk_err_lookup_status(zk):
    lib = zk.load()
    assert lib.zk_strerror(-9).decode() == "a lookup input value is not in the table"
    inputs, table = lc.missing_case("PallasFq", "below", 64)
    d_in, d_tab = to_device(zk, _monts("PallasFq", inputs)), to_device(zk, _monts("PallasFq", table))
    a, s = np.zeros((64, 4), dtype=np.uint64), np.zeros((64, 4), dtype=np.uint64)
    zk.halo2._plib()
    st = lib.zk_halo2_permute_expression_pair_device(1, d_in.ctypes.data, d_tab.ctypes.data, 64, a.ctypes.data, s.ctypes.data, None)
    assert st == -9


def test_invalid_arguments(zk):
    lib = zk.halo2._plib()
    f = 0
    u = 16
    inputs, table = lc.make_case("PallasFp", "random_dups", u)
    buf = np.zeros((8 * u + 8, 4), dtype=np.uint64)           # one allocation, carved into 16-B aligned columns
    base = buf.ctypes.data
    assert base % 16 == 0
    col = lambda k: base + k * u * 32
    buf[0:u] = _monts("PallasFp", inputs)
    buf[u:2 * u] = _monts("PallasFp", table)
    before = buf.copy()
    call = lambda i, t, a, s, n=u: lib.zk_halo2_permute_expression_pair_device(f, i, t, n, a, s, None)
    good = (col(0), col(1), col(2), col(3))
    for args in [(None, col(1), col(2), col(3)), (col(0), None, col(2), col(3)), (col(0), col(1), None, col(3)), (col(0), col(1), col(2), None),
                 (col(0) + 8, col(1), col(2), col(3)), (col(0), col(1), col(2) + 8, col(3)), (col(0), col(1), col(2), col(3) + 8)]:
        assert call(*args) == -1, args
    # overlapping ranges: the outputs with each other, with either input, partially
    for args in [(col(0), col(1), col(2), col(2)), (col(0), col(1), col(2), col(2) + 32 * (u - 1)), (col(0), col(1), col(0), col(3)),
                 (col(0), col(1), col(2), col(1)), (col(0), col(1), col(1) + 32 * 3, col(3)), (col(0), col(1), col(2), col(0) + 32 * (u - 1))]:
        assert call(*args) == -1, args
    assert call(*good, n=1 << 31) == -1
    assert lib.zk_halo2_permute_expression_pair_device(7, *good, u, None) == -1      # unknown field
    assert (buf == before).all(), "refused calls write nothing"
    # usable_rows = 0: a no-op that returns 0, even with null buffers
    assert call(*good, n=0) == 0 and call(None, None, None, None, n=0) == 0
    assert (buf == before).all()
    # inputs may share one buffer (A and S read only); the adjacent, non-overlapping outputs are fine
    assert call(*good) == 0
    a_exp, s_exp = lc.h2.permute_expression_pair("PallasFp", inputs, table, u)
    assert (buf[2 * u:3 * u] == _monts("PallasFp", a_exp)).all() and (buf[3 * u:4 * u] == _monts("PallasFp", s_exp)).all()
    assert call(col(1), col(1), col(4), col(5)) == 0


def test_allocates_outputs(zk):
    inputs, table = lc.make_case("Bn254Fr", "range_check", 300)
    a, s = zk.halo2.permute_expression_pair_device("Bn254Fr", to_device(zk, _monts("Bn254Fr", inputs)), to_device(zk, _monts("Bn254Fr", table)), 300)
    a_exp, s_exp = lc.h2.permute_expression_pair("Bn254Fr", inputs, table, 300)
    assert a.shape == (300, 4) and (to_host(zk, a) == _monts("Bn254Fr", a_exp)).all() and (to_host(zk, s) == _monts("Bn254Fr", s_exp)).all()
