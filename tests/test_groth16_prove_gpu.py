"""GPU tier (-m gpu): the Groth16 prove path on a real MI355X at its edges (tests/groth16_prove_cases.py) -- every row length
around the 64/65-term switch between the two mat-vec kernels and around the 256-lane stride of the long one, every layout of
the long-row list, the operand values next to the +-1 shortcut, the zero-fill past the last row, the witness map at domains of
2^k - 1, 2^k and 2^k + 1 rows (k = 5, 10), and whole proofs over all-zero, 0/1-heavy and p - 1 assignments, verified by
groth16.verify.  References: Python integers; every comparison is exact."""
import pytest

import groth16_prove_cases as pc

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


@pytest.fixture(scope="module")
def row_lengths(zk):
    return {field: pc.run_row_lengths(zk, field) for field in pc.FIELDS}


# ---- 1. the row-major mat-vec
@pytest.mark.parametrize("length", pc.ROW_LENGTHS)
@pytest.mark.parametrize("field", pc.FIELDS)
def test_row_length(row_lengths, field, length):
    pc.check_row_length(row_lengths[field], length)


@pytest.mark.parametrize("layout", list(pc.LAYOUTS))
@pytest.mark.parametrize("field", pc.FIELDS)
def test_long_row_list(zk, field, layout):
    pc.check_layout(zk, field, layout)


@pytest.mark.parametrize("kind", list(pc.EDGE_ROW))
@pytest.mark.parametrize("edge", pc.EDGES)
@pytest.mark.parametrize("field", pc.FIELDS)
def test_operand_edge(zk, field, edge, kind):
    pc.check_edge(zk, field, edge, kind)


@pytest.mark.parametrize("fill", ["exact", "plus_one", "double"])
@pytest.mark.parametrize("field", pc.FIELDS)
def test_zero_fill(zk, field, fill):
    pc.check_zero_fill(zk, field, fill)


def test_matvec_refusals(zk):
    pc.check_matvec_refusals(zk)


# ---- 2. the witness map
@pytest.mark.parametrize("edge", list(pc.DOMAIN_EDGES))
@pytest.mark.parametrize("field", pc.FIELDS)
def test_witness_map_domain_edge(zk, field, edge):
    pc.check_domain_edge(zk, field, edge)


@pytest.mark.parametrize("field", pc.FIELDS)
def test_witness_map_zero_quotient(zk, field):
    pc.check_zero_quotient(zk, field)


# ---- 3. whole proofs
@pytest.mark.parametrize("blinding", pc.BLINDINGS)
@pytest.mark.parametrize("assignment", pc.ASSIGNMENTS)
@pytest.mark.parametrize("pairing", pc.PAIRINGS)
def test_proof(zk, pairing, assignment, blinding):
    pc.check_proof(zk, pairing, assignment, [blinding])


@pytest.mark.parametrize("pairing", pc.PAIRINGS)
def test_proof_with_a_row_of_300_terms(zk, pairing):
    """the long kernel's second stride iteration inside a whole proof"""
    pc.check_proof(zk, pairing, "boolean", ["random"], long_row=True)
