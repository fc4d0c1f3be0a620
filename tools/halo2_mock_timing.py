#!/usr/bin/env python3
"""Times zk.halo2.MockProver.verify (MockProver::verify on the device) on synth.satisfied_circuit's default shape -- 13 advice, 8 fixed,
3 instance columns, 6 gates, one range-check lookup, copies over five columns, PallasFp -- at k = 12 (the reference's
MockProver::run(12, ..)) and k = 20: verify() on the satisfied witness and with 1000 seeded faults (a multiplication operand
changed at 1000 rows), and the split by the four entry points (the gates' evaluation, the lookup's evaluation + membership test,
the copy-constraint check, one compaction of the gates' status array).  Wall-clock seconds around a device synchronisation, one
run each after one warm-up verify().  Appends one JSON line per size to the path given (default: stdout only).
usage: halo2_mock_timing.py [out.jsonl] [k ...]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import contangle_zkcp_amd as zk
from contangle_zkcp_amd import synth

OUT = sys.argv[1] if len(sys.argv) > 1 else None
KS = [int(a) for a in sys.argv[2:]] or [12, 20]
FIELD = "PallasFp"
zk.load(); zk.init(0)
print("backend:", zk.backend_info(), flush=True)
def sync(): torch.cuda.synchronize()
for K in KS:
    res = {"k": K, "field": FIELD}
    def timed(name, fn):
        sync(); t = time.perf_counter(); r = fn(); sync(); res[name] = round(time.perf_counter() - t, 5); print(K, name, res[name], flush=True); return r
    circuit = timed("build_circuit_host_s", lambda: synth.satisfied_circuit(FIELD, K))
    prover = timed("upload_s", lambda: synth.mock_prover(circuit))
    n = 1 << K
    res.update(advice=len(circuit["advice"]), fixed=len(circuit["fixed"]), instance=len(circuit["instance"]),
               gate_programs=sum(len(p) for _, p in circuit["gates"]), copies=int(len(circuit["copies"])))
    assert prover.verify() == []                       # warm-up: scratch, and the claim itself
    assert timed("verify_satisfied_s", lambda: prover.verify()) == []
    programs = [p for _, polys in prover.gates for p in polys]
    status, _ = timed("entry_eval_gates_s", lambda: zk.halo2.mock_eval(prover.field, K, programs, prover.columns, prover.poison_from, prover.consts))
    timed("entry_failures_gates_s", lambda: zk.halo2.mock_failures(status, len(programs) * n, 65536))
    timed("lookups_eval_and_membership_s", lambda: prover._verify_lookups(65536))
    timed("entry_permutation_and_failures_s", lambda: prover._verify_permutation(65536))
    # 1000 seeded faults: one operand of a multiplication gate changed
    rows, members = circuit["rows"]["mul"]
    pick = np.random.default_rng(7).choice(len(rows), size=min(1000, len(rows)), replace=False)
    for r, g in zip(rows[pick].tolist(), members[pick].tolist()):
        circuit["advice"][g + 1, r, 0] ^= np.uint64(1)
    faulty = synth.mock_prover(circuit)
    faulty.verify()
    got = timed("verify_1000_faults_s", lambda: faulty.verify())
    res["faults_seeded"], res["failures_reported"] = int(len(pick)), len(got)
    assert len(got) == len(pick) and all(type(f).__name__ == "ConstraintNotSatisfied" for f in got)
    print(json.dumps(res), flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(json.dumps(res) + "\n")
    del prover, faulty, status
    circuit["assembly"].free()
