"""GPU tier (-m gpu): Poseidon, the Merkle tree over it, its paths and the ElGamal stream on a real MI355X -- the checks of
tests/poseidon_cases.py against RefPoseidon / ref_tree, exact.

poseidon_permute_kernel / poseidon_hash_kernel: one lane per permutation / hash, workgroups of 256, at most 1024 of them (2^18
lanes a trip of the grid-stride loop).  COUNTS = 1, 63 .. 65, 255 .. 257 end inside the first wave, on its edge, and on the edge of
the first workgroup; test_grid_stride runs 2^18 + 257 of each, the second trip ending inside a workgroup.  The parameter sets of
PSETS cross: the four fields at width 3, widths 2, 4, 5, alpha 3, 5, 7, 17 (the short chains) and 2, 2^16 + 1, 2^64 - 1 (the same
loop, longer), full rounds 2 and 8, partial rounds 0, 1, 31, 56, both sponge layouts, constants all zero and drawn from {0, 1, p - 1}.

Tree: one launch for the leaves, one per level of more than 2^8 nodes, one workgroup for all the levels above.  log_n 1 .. 8 is the
tail kernel alone (from 1 hash to 256 in its first level), 9 is the first tree with a level kernel launch, 10 and 11 have two and
three; 17 and 20 (reference parameters) check every node of a large tree, 20 taking the second trip in the leaves and in level 1.
merkle_paths_kernel: 256 indices a launch; test_many_paths asks for 1, 256, 257 and 515."""
import pytest

import poseidon_cases as pc

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


def test_host_pins(zk):
    pc.check_ref_pins()
    pc.check_host_pins(zk)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(pc.PSETS))
def test_permute(zk, name, device):
    pc.check_permute(zk, name, device)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(pc.PSETS))
def test_hash(zk, name, device):
    pc.check_hash(zk, name, device)


def test_grid_stride(zk):
    pc.check_grid_stride(zk)


@pytest.mark.parametrize("leaf_arity", [1, 3])
@pytest.mark.parametrize("log_n", range(1, 12))
def test_tree(zk, log_n, leaf_arity):
    pc.check_tree(zk, log_n, leaf_arity)


@pytest.mark.parametrize("log_n", [17, 20])
def test_large_tree(zk, log_n):
    pc.check_large_tree(zk, log_n)


def test_many_paths(zk):
    pc.check_many_paths(zk)


@pytest.mark.parametrize("n", pc.ELGAMAL_NS)
@pytest.mark.parametrize("field", pc.FIELDS)
def test_elgamal(zk, field, n):
    pc.check_elgamal(zk, field, n)


def test_refusals(zk):
    pc.check_refusals(zk)


def test_lifecycle(zk):
    pc.check_lifecycle(zk)
