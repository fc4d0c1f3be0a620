"""GPU tier (-m gpu): MockProver::verify on a real MI355X -- the four zk_halo2_mock_* entries and zk.halo2.MockProver -- the checks of
tests/halo2_mock_cases.py against RefMockProver.

mock_eval_kernel: workgroups of 128 rows, at most MOCK_GRID_X = 512 of them per program (2^16 rows a trip of the grid-stride
loop), the grid program-major.  Which k of test_eval crosses what:
  1, 3      2 and 8 rows: one partial wave; at k = 1 column 0 is Poison everywhere (poison_from = max(n - 6, 0) = 0)
  6         64 rows, exactly one wave
  7, 8      128 and 256 rows: exactly one workgroup, and two
  13        64 workgroups per program, 37 programs
  17        test_eval_grid_stride: 2^17 rows > 512 x 128, the smallest k that takes the second trip of the loop
test_eval_256_programs: 256 programs of 8 rows in one launch (256 workgroups, one per program).

flags_count / flags_scan / flags_emit: one 16-byte load per lane, 4096 bytes per workgroup.  N of test_compaction: 1, 63 .. 65 and
255 .. 257 end inside the first lane groups (the bytewise tail of flags_load), 4097 opens a second workgroup with one byte,
2^16 + 1 is 17 workgroups with a one-byte tail; `boundaries` puts a flag either side of every 256-byte edge.

Lookup: the sort's tile is 256 keys and its chunk 4096 (zk_lookup_kernels.h); usable_rows 63 .. 65, 255 .. 257, 4095 .. 4097 sit on
those edges, 2^13 + 3 is three chunks, 2^16 + 1 (GPU only) seventeen and more than LK_SMALL_SCAN = 8, so lk_offsets_kernel runs
instead of the small scan.  `equal` makes every digit dead, `range` leaves two live.

mock_permutation_kernel: 256 cells per workgroup, at most MOCK_PERM_GRID = 1024 workgroups (2^18 cells a trip).  (1, 1) is two
cells, (6, 1) one wave, (6, 17) 4.25 workgroups, (13, 5) 160; test_permutation_grid_stride: 17 x 2^14 = 278528 cells > 2^18.

test_mock_prover: n = blinding_factors + 3 exactly (k = 3), 6, 10, and 16 (satisfied, plus three mutations)."""
import pytest

import halo2_mock_cases as mc

pytestmark = pytest.mark.gpu
FULL_FIELDS = ["PallasFp", "PallasFq"]


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


@pytest.mark.parametrize("field", FULL_FIELDS)
@pytest.mark.parametrize("k", mc.EVAL_KS)
def test_eval(zk, field, k):
    mc.check_eval(zk, field, k)


@pytest.mark.parametrize("field,k", [("Bn254Fr", 7), ("Bls381Fr", 7)])
def test_eval_other_fields(zk, field, k):
    mc.check_eval(zk, field, k)


def test_eval_grid_stride(zk):
    mc.check_eval_grid_stride(zk, "PallasFp", 17)


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
@pytest.mark.parametrize("u", mc.LOOKUP_US + [(1 << 16) + 1])
def test_lookup(zk, u, kind):
    mc.check_lookup(zk, "PallasFp" if u % 2 else "PallasFq", u, kind)


def test_lookup_refusals(zk):
    mc.check_lookup_refusals(zk, "PallasFp")


@pytest.mark.parametrize("field", FULL_FIELDS)
@pytest.mark.parametrize("shape", mc.PERM_SHAPES)
def test_permutation(zk, field, shape):
    mc.check_permutation(zk, field, *shape)


def test_permutation_grid_stride(zk):
    mc.check_permutation_large(zk, "PallasFq", 14, 17)


@pytest.mark.parametrize("case", ["satisfied"] + mc.MUTATIONS)
@pytest.mark.parametrize("field", FULL_FIELDS)
@pytest.mark.parametrize("k", [3, 6, 10])
def test_mock_prover(zk, field, k, case):
    mc.check_mock(zk, field, k, case)


@pytest.mark.parametrize("case", ["satisfied", "mul", "lookup", "copy"])
def test_mock_prover_k16(zk, case):
    mc.check_mock(zk, "PallasFp", 16, case)


@pytest.mark.parametrize("field", FULL_FIELDS)
def test_mock_prover_truncation(zk, field):
    mc.check_truncation(zk, field)


@pytest.mark.parametrize("field", FULL_FIELDS)
def test_mock_prover_wide_lookup(zk, field):
    mc.check_wide_lookup(zk, field)


@pytest.mark.parametrize("field", FULL_FIELDS)
def test_mock_prover_refusals(zk, field):
    mc.check_mock_refusals(zk, field)
