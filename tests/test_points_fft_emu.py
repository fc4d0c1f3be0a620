"""CPU tier: the DFT of a vector of curve points (zk_ntt_points_device / zk_ntt_points, halo2.best_fft_points, halo2.Params) in
the emulator build of the HIP sources (tests/emu), against the O(n^2) definition on the oracle's point arithmetic and against
the transform in the exponent (tests/points_fft_cases.py).  k = 0 has no stage, k = 1 one stage with the twiddle 1 only;
k = 2, 3, 5 run every stage with per-lane twiddles (fewer than 64 blocks); k = 7 runs its first stage with one twiddle per
wave (64 blocks) and the other six per lane.  The real gate is tests/test_points_fft_gpu.py (-m gpu)."""
import importlib.util
import os

import pytest

import points_fft_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [0, 1, 2, 3, 5, 7]


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


def test_not_initialized():
    """before zk_init both entry points answer ZK_ERR_NOT_INITIALIZED (a fresh process: this one has the library initialised)"""
    import subprocess
    import sys
    spec = importlib.util.spec_from_file_location("zk_build", os.path.join(ROOT, "contangle-zkcp_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    code = ("import ctypes, numpy as np\n"
            "lib = ctypes.CDLL(%r)\n"
            "buf = np.zeros((2, 12), dtype=np.uint64); om = np.zeros(4, dtype=np.uint64)\n"
            "vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)\n"
            "lib.zk_ntt_points.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]\n"
            "lib.zk_ntt_points_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]\n"
            "print(lib.zk_ntt_points(0, vp(buf), 1, vp(om), 0), lib.zk_ntt_points_device(0, vp(buf), vp(buf), 1, vp(om), 0, None))\n") % b.build_emu()
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert out == ["-2", "-2"], out
