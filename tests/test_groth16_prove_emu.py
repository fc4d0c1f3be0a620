"""CPU tier: the Groth16 prove path at its edges (tests/groth16_prove_cases.py) in the emulator build of the HIP sources
(tests/emu).  Part 1 -- the row-major mat-vec at every row length, long-row-list layout, operand edge and zero-fill length -- runs
in full: it has no curve arithmetic.  The witness map runs at the k = 5 domain edges and the small systems, and one whole proof
per pairing; the k = 10 domains and every assignment x blinding pair run in tests/test_groth16_prove_gpu.py (-m gpu), the real gate."""
import importlib.util
import os

import pytest

import groth16_prove_cases as pc
from oracle import pyref_groth16 as g16

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
@pytest.mark.parametrize("edge", pc.SMALL_DOMAIN_EDGES)
@pytest.mark.parametrize("field", pc.FIELDS)
def test_witness_map_domain_edge(zk, field, edge):
    pc.check_domain_edge(zk, field, edge)


@pytest.mark.parametrize("field", pc.FIELDS)
def test_witness_map_zero_quotient(zk, field):
    pc.check_zero_quotient(zk, field)


def test_sampled_tau_identity_rejects_a_corrupted_h():
    """the independent check of part 2 on the reference's own h, without a device: right h accepted, any single coefficient off refused"""
    field = "Bn254Fr"
    p = pc.modulus(field)
    r1cs, z = pc.domain_edge_system(field, "k5_one_over")
    evals, h = g16.evaluations(r1cs, z), g16.h_coefficients(r1cs, z)
    assert len(h) == 64 and h == pc.h_coefficients_fft(r1cs, z)
    tau = 0x1234567 % p
    assert pc.quotient_identity(field, evals, h, tau)
    for i in range(len(h)):
        bad = list(h)
        bad[i] = (bad[i] + 1) % p
        assert not pc.quotient_identity(field, evals, bad, tau), i


@pytest.mark.parametrize("assignment", pc.ASSIGNMENTS)
@pytest.mark.parametrize("field", pc.FIELDS)
def test_edge_systems_are_satisfied(field, assignment):
    r1cs, z = pc.edge_system(field, assignment)
    g16.h_coefficients(r1cs, z)                       # asserts that the quotient divides
    p = pc.modulus(field)
    ni = r1cs["num_inputs"]
    if assignment == "zero_witness":
        assert not any(z[ni:]) and z[0] == 1
    elif assignment == "boolean":
        assert sum(1 for v in z if v in (0, 1)) >= 0.8 * len(z) and any(not row for row in r1cs["C"])
    else:
        assert z.count(p - 1) >= 3 and z[1] == p - 1


# ---- 3. whole proofs: one per pairing here
def test_proof_bls381(zk):
    pc.check_proof(zk, "Bls381", "boolean", ["one_minus_one"])


def test_proof_bn254(zk):
    pc.check_proof(zk, "Bn254", "zero_witness", ["zero"])
