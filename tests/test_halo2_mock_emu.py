"""CPU tier: MockProver::verify on the device (the four zk_halo2_mock_* entries and zk.halo2.MockProver) in the emulator build of
the HIP sources (tests/emu), against RefMockProver, the restatement on Python integers in tests/halo2_mock_cases.py.  The real
gate is tests/test_halo2_mock_gpu.py (-m gpu)."""
import importlib.util
import os

import pytest

import halo2_mock_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_FIELDS = ["PallasFp", "PallasFq"]


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


@pytest.mark.parametrize("field", FULL_FIELDS)
@pytest.mark.parametrize("k", mc.EVAL_KS)
def test_eval(zk, field, k):
    mc.check_eval(zk, field, k)


@pytest.mark.parametrize("field,k", [("Bn254Fr", 7), ("Bls381Fr", 7)])
def test_eval_other_fields(zk, field, k):
    mc.check_eval(zk, field, k)


@pytest.mark.parametrize("field", FULL_FIELDS)
def test_eval_256_programs(zk, field):
    mc.check_eval_many_programs(zk, field)


@pytest.mark.parametrize("field", FULL_FIELDS)
def test_eval_refusals(zk, field):
    mc.check_eval_refusals(zk, field)


@pytest.mark.parametrize("pattern", mc.COMPACT_PATTERNS)
@pytest.mark.parametrize("n", mc.COMPACT_NS)
def test_compaction(zk, n, pattern):
    mc.check_compaction(zk, n, pattern)


@pytest.mark.parametrize("kind", mc.LOOKUP_TABLES)
@pytest.mark.parametrize("u", mc.LOOKUP_US)
def test_lookup(zk, u, kind):
    mc.check_lookup(zk, "PallasFp" if u % 2 else "PallasFq", u, kind)


def test_lookup_refusals(zk):
    mc.check_lookup_refusals(zk, "PallasFp")


@pytest.mark.parametrize("field", FULL_FIELDS)
@pytest.mark.parametrize("shape", mc.PERM_SHAPES)
def test_permutation(zk, field, shape):
    mc.check_permutation(zk, field, *shape)


@pytest.mark.parametrize("case", ["satisfied"] + mc.MUTATIONS)
@pytest.mark.parametrize("field", FULL_FIELDS)
@pytest.mark.parametrize("k", [3, 6, 10])
def test_mock_prover(zk, field, k, case):
    mc.check_mock(zk, field, k, case)


@pytest.mark.parametrize("field", FULL_FIELDS)
def test_mock_prover_truncation(zk, field):
    mc.check_truncation(zk, field)


@pytest.mark.parametrize("field", FULL_FIELDS)
def test_mock_prover_wide_lookup(zk, field):
    mc.check_wide_lookup(zk, field)


@pytest.mark.parametrize("field", FULL_FIELDS)
def test_mock_prover_refusals(zk, field):
    mc.check_mock_refusals(zk, field)
