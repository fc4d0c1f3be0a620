"""CPU tier: MSMs over colliding inputs (equal, opposite and identity points) and halo2's generator fold in the emulator build of
the HIP sources (tests/emu), against [sum k_i s_i] G formed in Python integers (tests/msm_collision_cases.py).  Vesta,
BLS12-381 G1 and BN254 G2 (a 9-limb, a 14-limb and a twist point type), n <= 600.

What runs here.  The emulator pays per launched lane and window: about a second per MSM call whatever n is, three at c = 2.
The rule, stated once:
  * Vesta runs the grid of window widths, slice lengths and piece counts in full, except family 5 at c = 2 (128 windows of
    two buckets: the dearest calls for the least reduction), which the GPU tier runs;
  * the other two point types run every family on every path, at one or two widths per path, without what only repeats work
    already done on them (LEAN): the two extra top-bucket cases of family 5, the default form over a handle that holds a
    table, the second width of the device partials, the middle piece count;
  * the saturated limbs are one template over the field (zk_curve.h): Vesta runs its three paths, BN254 G2 (Fq2) the default
    path and family 5, BLS12-381 G1 is left to the GPU tier; family 5 there at slice lengths 1 and 3 (a power of two, and not);
  * every edge scalar as an MSM of its own at one width (Vesta, c = 7).
tests/test_msm_collisions_gpu.py (-m gpu) is the real gate: the whole grid on every curve, c = 16 and n = 5200."""
import importlib.util
import os

import pytest

import msm_collision_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["Vesta", "Bls381G1", "Bn254G2"]
FULL = dict(tops=True, also_default=True, widths=(4, 7), splits=(1, 2, 4))
LEAN = dict(tops=False, also_default=False, widths=(4,), splits=(1, 4))


def grid(curve):
    return FULL if curve == "Vesta" else LEAN


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


@pytest.mark.parametrize("curve,c", [("Vesta", 2), ("Vesta", 4), ("Vesta", 7), ("Bls381G1", 4), ("Bls381G1", 7), ("Bn254G2", 4), ("Bn254G2", 7)])
def test_default_path(zk, curve, c):
    mc.check_default_path(zk, curve, c)


@pytest.mark.parametrize("curve,c", [("Vesta", 2), ("Vesta", 4), ("Vesta", 7), ("Vesta", 13), ("Bls381G1", 4), ("Bls381G1", 13),
                                     ("Bn254G2", 7), ("Bn254G2", 13)])
def test_digit_edges(zk, curve, c):
    mc.check_digit_edges(zk, curve, c, singles=(curve, c) == ("Vesta", 7))


@pytest.mark.parametrize("curve,c", [("Vesta", 4), ("Vesta", 7), ("Bls381G1", 4), ("Bn254G2", 4)])
def test_reduce_collisions(zk, curve, c):
    mc.check_reduce_collisions(zk, curve, c, tops=grid(curve)["tops"])        # every slice length


@pytest.mark.parametrize("curve", CURVES)
def test_oversized_buckets(zk, curve):
    mc.check_oversized_buckets(zk, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_bucket_splitting(zk, curve):
    mc.check_bucket_splitting(zk, curve, splits=grid(curve)["splits"])


@pytest.mark.parametrize("curve,paths", [("Vesta", 3), ("Bn254G2", 1)])
def test_saturated_limbs(zk, curve, paths):
    mc.check_saturated_limbs(zk, curve, slices=(1, 3), tops=grid(curve)["tops"], paths=paths)


@pytest.mark.parametrize("curve", CURVES)
def test_precomputed_table(zk, curve):
    mc.check_precomputed_table(zk, curve, also_default=grid(curve)["also_default"])


@pytest.mark.parametrize("curve", CURVES)
def test_batch(zk, curve):
    mc.check_batch(zk, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_window_shares(zk, curve):
    mc.check_window_shares(zk, curve)


@pytest.mark.parametrize("curve", CURVES)
def test_device_partials(zk, curve):
    mc.check_device_partials(zk, curve, widths=grid(curve)["widths"])


@pytest.mark.parametrize("curve", CURVES)
def test_deferred_results(zk, curve):
    mc.check_deferred(zk, curve)


@pytest.mark.parametrize("curve", ["Vesta", "Pallas"])
@pytest.mark.parametrize("half", [1, 5, 64, 200])
def test_ipa_fold_bases(zk, curve, half):
    mc.check_ipa_fold(zk, curve, half)
