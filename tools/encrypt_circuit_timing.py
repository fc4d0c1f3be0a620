#!/usr/bin/env python3
"""Times the path plaintext -> EncryptCircuit assignment -> Groth16 proof -> verify (zk.encryption, zk.groth16) on one GPU at the
reference's own test size: n = 196608, scalar_bits = 256, BLS12-381, the reference's Poseidon set.  Every repeated row: 2 warm-up runs,
then the median [min, max] of 7 runs, wall-clock milliseconds around a device synchronisation.  Rows:
  csr_upload        EncryptCircuit.csr() and the upload of the three matrices: once per circuit (one run)
  keygen            groth16.generate_random_parameters over them: once per circuit (one run; not part of a proof)
  fixed_section     the host's share of assign: two 256-bit JubJub multiplications, one Poseidon permutation, ~5.4 k rows on Python integers
  witness_kernel    zk_encrypt_witness_device alone, with `floor_ms`: its products (one Fermat inversion per 16 elements plus three per
                    element) at the measured Bls381Fr product rate of profiles/r03_k_microbench.txt (90.0 Gmul/s) -- a floor with every
                    SIMD busy, which 192 waves on 1024 SIMDs cannot reach; not a target
  assign            EncryptCircuit.assign as a whole (fixed section, one upload, the kernel)
  first_unsatisfied groth16.first_unsatisfied over the honest assignment
  prove_device      Prover.prove_device from the resident assignment
  verify            groth16.verify with a prepared key and the public inputs on the device: its n + 2 point MSM is the O(n) part of `buy`
That results are right is what tests/test_encrypt_circuit_gpu.py checks.  Writes one JSON line per row.
usage: encrypt_circuit_timing.py [out.jsonl]   (default profiles/encrypt_circuit_timing.jsonl)"""
import json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import contangle_zkcp_amd as zk

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "encrypt_circuit_timing.jsonl")
WARM, RUNS = 2, 7
N, BITS, FIELD = 196608, 256, "Bls381Fr"
MUL_RATE = 90.0e9          # profiles/r03_k_microbench.txt: Bls381Fr fe_mul, 1024 blocks of one wave
assert torch.cuda.is_available(), "this is a measurement on the GPU"
zk.load(); zk.init(0)
backend = zk.backend_info()
print("backend:", backend, flush=True)
enc, g16, jj, po = zk.encryption, zk.groth16, zk.jubjub, zk.poseidon
with open(os.path.join(ROOT, "tests", "golden", "poseidon_bls12_377_rate2.json")) as fh:
    d = json.load(fh)
prm = po.PoseidonParameters(FIELD, d["full_rounds"], d["partial_rounds"], d["alpha"], [[int(x) for x in r] for r in d["mds"]],
                            [[int(x) for x in r] for r in d["ark"]], rate=d["rate"])
rows = []
def sync(): torch.cuda.synchronize()
def record(row, what, ts, warm, **extra):
    r = dict(row=row, what=what, n=N, scalar_bits=BITS, ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
             runs=len(ts), warmup=warm, clock="host wall clock around a device synchronisation", backend=backend, **extra)
    rows.append(r); print(json.dumps(r), flush=True)
def timed(row, what, fn, runs=RUNS, warm=WARM, **extra):
    for _ in range(warm): fn()
    ts = []
    for _ in range(runs):
        sync(); t = time.perf_counter(); fn(); sync(); ts.append((time.perf_counter() - t) * 1e3)
    record(row, what, ts, warm, **extra)

rng = random.Random(196608)
params = enc.Parameters(N, prm)
t = time.perf_counter()
circ = enc.EncryptCircuit(params, scalar_bits=BITS)
circ.csr()
A, B, C = circ.matrices()
sync()
record("csr_upload", "EncryptCircuit(...), csr(), matrices(): once per circuit", [(time.perf_counter() - t) * 1e3], 0, rows_total=circ.num_constraints(),
       fixed_rows=circ.num_fixed_rows, fixed_witnesses=circ.num_fixed, n_vars=circ.n_vars)
t = time.perf_counter()
key = g16.generate_random_parameters("Bls381", A, B, C, circ.num_inputs, circ.n_vars)
sync()
record("keygen", "groth16.generate_random_parameters: once per circuit", [(time.perf_counter() - t) * 1e3], 0)
prover = g16.Prover("Bls381", key, A, B, C, circ.num_inputs, lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda())
pvk = g16.prepare_verifying_key(g16.VerifyingKey.from_parameters(key))

sk, pk = jj.keygen(rng.randrange(1, jj.ORDER))
r = rng.randrange(jj.ORDER)
d_msg = enc.bytes_to_plaintext_chunks_direct(bytes(rng.randrange(256) for _ in range(N)), N)
timed("fixed_section", "EncryptCircuit.fixed_assignment (host, Python integers)", lambda: circ.fixed_assignment(pk, r))
_, dh, _, _ = circ.fixed_assignment(pk, r)
d_z = circ.assign(pk, r, d_msg)
seg = (d_z[3:3 + N], d_z[circ.m0:circ.b0], d_z[circ.b0:circ.k0], d_z[circ.k0:])
inv_products = 256 + bin(jj.P - 2).count("1")            # fe_inv: a squaring per bit, a product per set bit of p - 2
products = (N + 15) // 16 * inv_products + 3 * N
timed("witness_kernel", "zk_encrypt_witness_device", lambda: enc.encrypt_witness(d_msg, N, N, dh, *seg), products=products,
      floor_ms=round(products / MUL_RATE * 1e3, 4), floor_note="products / 90.0 Gmul/s (every SIMD busy); the launch has 192 waves")
timed("assign", "EncryptCircuit.assign (fixed section + upload + kernel)", lambda: circ.assign(pk, r, d_msg))
assert g16.first_unsatisfied(A, B, C, d_z) is None
timed("first_unsatisfied", "groth16.first_unsatisfied, honest assignment", lambda: g16.first_unsatisfied(A, B, C, d_z))
blinds = po.to_mont(jj.P, [rng.randrange(jj.P), rng.randrange(jj.P)])
proof = prover.prove_device(d_z, blinds[0], blinds[1])[1]
timed("prove_device", "Prover.prove_device from the resident assignment", lambda: prover.prove_device(d_z, blinds[0], blinds[1]))
public = enc.get_public_inputs(enc.encrypt(pk, d_msg, r, params), params)
assert g16.verify(pvk, public, proof) is True
timed("verify", "groth16.verify, prepared key, %d public inputs on the device" % (N + 2), lambda: g16.verify(pvk, public, proof))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    for r_ in rows:
        fh.write(json.dumps(r_) + "\n")
