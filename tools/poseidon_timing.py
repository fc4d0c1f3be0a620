#!/usr/bin/env python3
"""Times Poseidon on the device (zk.poseidon; csrc/zk_poseidon_kernels.h) on one GPU, Bls381Fr, the reference's parameter set
(width 3, 8 full and 31 partial rounds, alpha 17; tests/golden/poseidon_bls12_377_rate2.json).  Every row: 2 warm-up runs, then the
median [min, max] of 7 runs, wall-clock milliseconds around a device synchronisation.  Rows:
  hash      zk_poseidon_hash_device over 2^20 single-element leaves
  tree_K    zk_poseidon_merkle_tree_device at log_n = 12, 18, 20 (`launches` = kernel launches of one tree, `permutations` = 2n - 1)
  paths     zk_merkle_paths_device, 64 paths of the 2^20 tree (the launch alone, and generate_proofs with its download)
  mask      zk_vec_add_scalar_device over 2^20 elements
  host      the host twin, one thread, 2^12 permutations: nanoseconds per permutation as measured, not extrapolated
Inputs are seeded random elements: the time does not depend on them; that results are right is what tests/test_poseidon_gpu.py checks.
Writes one JSON line per row.  usage: poseidon_timing.py [out.jsonl]   (default profiles/poseidon_timing.jsonl)"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import contangle_zkcp_amd as zk
from contangle_zkcp_amd import synth

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "poseidon_timing.jsonl")
WARM, RUNS = 2, 7
FIELD = "Bls381Fr"
assert torch.cuda.is_available(), "this is a measurement on the GPU"
zk.load(); zk.init(0)
backend = zk.backend_info()
print("backend:", backend, flush=True)
po = zk.poseidon
with open(os.path.join(ROOT, "tests", "golden", "poseidon_bls12_377_rate2.json")) as fh:
    d = json.load(fh)
prm = po.PoseidonParameters(FIELD, d["full_rounds"], d["partial_rounds"], d["alpha"], [[int(x) for x in r] for r in d["mds"]],
                            [[int(x) for x in r] for r in d["ark"]], rate=d["rate"])
lib = po._plib()
rows = []
def sync(): torch.cuda.synchronize()
def timed(row, what, fn, runs=RUNS, warm=WARM, **extra):
    for _ in range(warm): fn()
    ts = []
    for _ in range(runs):
        sync(); t = time.perf_counter(); fn(); sync(); ts.append((time.perf_counter() - t) * 1e3)
    r = dict(row=row, what=what, field=FIELD, ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
             runs=runs, warmup=warm, clock="host wall clock around a device synchronisation", backend=backend, **extra)
    rows.append(r); print(json.dumps(r), flush=True)
    return r

n = 1 << 20
leaves = torch.from_numpy(synth.rand_field(FIELD, n, 1).view(np.int64)).cuda()
digests = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
timed("hash", "zk_poseidon_hash_device, 2^20 hashes of one element", lambda: prm.hash_batch(leaves, 1, out=digests), permutations=n)
tree = None
for log_n in (12, 18, 20):
    m = 1 << log_n
    nodes = torch.zeros((2 * m - 1, 4), dtype=torch.int64, device="cuda")
    def build(m=m, log_n=log_n, nodes=nodes):
        st = lib.zk_poseidon_merkle_tree_device(prm.handle, leaves.data_ptr(), 1, log_n, nodes.data_ptr(), None)
        assert st == 0, st
    timed("tree_%d" % log_n, "zk_poseidon_merkle_tree_device, log_n = %d, leaf_arity 1" % log_n, build, permutations=2 * m - 1,
          launches=2 + max(log_n - 9, 0))
    if log_n == 20:
        tree = po.MerkleTree(prm, nodes, log_n)
idx = np.random.default_rng(2).integers(0, n, 64).astype(np.uint64)
out = torch.zeros((64 * 20, 4), dtype=torch.int64, device="cuda")
def paths():
    st = lib.zk_merkle_paths_device(prm.field, tree.nodes.data_ptr(), 20, idx.ctypes.data, 64, out.data_ptr(), None)
    assert st == 0, st
timed("paths", "zk_merkle_paths_device, 64 paths of the 2^20 tree", paths)
timed("proofs", "MerkleTree.generate_proofs(64 indices): the launch, the download, 64 Path objects", lambda: tree.generate_proofs(idx))
c2 = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
timed("mask", "zk_vec_add_scalar_device (elgamal_mask), 2^20 elements", lambda: po.elgamal_mask(FIELD, leaves, 12345, out=c2), bytes_moved=64 * n)
# the host twin: one thread, as measured
count = 1 << 12
states = synth.rand_field(FIELD, 3 * count, 3)
ts = []
for _ in range(WARM + RUNS):
    buf = states.copy()
    t = time.perf_counter()
    st = lib.zk_poseidon_permute_host(prm.handle, buf.ctypes.data, count)
    ts.append((time.perf_counter() - t) * 1e3)
    assert st == 0, st
ts = ts[WARM:]
rows.append(dict(row="host", what="zk_poseidon_permute_host, one thread, 2^12 permutations", field=FIELD, ms_median=round(statistics.median(ts), 3),
                 ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), ns_per_permutation=round(statistics.median(ts) * 1e6 / count, 1), runs=RUNS,
                 warmup=WARM, clock="host wall clock"))
print(json.dumps(rows[-1]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    for r in rows:
        fh.write(json.dumps(r) + "\n")
