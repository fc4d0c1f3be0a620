#!/usr/bin/env python3
"""Times halo2 opening verification on the device (zk.halo2.compute_s, MSM.eval, commitment_verify_proof, verify_batch; halo2_proofs
0.2 poly/commitment/verifier.rs, msm.rs) on one GPU, Vesta, 2^k points (default k = 20).  Every row: 2 warm-up runs, then the median
[min, max] of 7 runs, wall-clock milliseconds around a device synchronisation (the calls end in host work, so device events would
miss part of them).  Rows:
  a  zk_halo2_ipa_s_device, count = 1
  b  the same vector by k calls of zk_ipa_update_weights_device (the only way before this kernel); the two results are compared
  c  count = 8 in one call, against 8 calls of count = 1 with accumulate
  d  MSM.eval() whole: the n-point MSM over the resident g_scalars, the small MSM over 2k + 4 terms, the host sum
  e  one commitment_verify_proof + use_challenges + eval, end to end
  f  verify_batch of 8
  g  for context: the oracle's CPU best_multiexp (a restatement, not upstream) at 2^k on this machine's CPU threads, one run
Proof points and scalars are seeded random values: the time of a verification does not depend on its verdict, which is False here;
that verdicts are right is what tests/test_ipa_verify_gpu.py checks.
Writes one JSON line per row.  usage: halo2_verify_timing.py [k] [out.jsonl]   (default profiles/halo2_verify_timing.jsonl)"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import contangle_zkcp_amd as zk
from contangle_zkcp_amd import synth

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "halo2_verify_timing.jsonl")
WARM, RUNS, BATCH = 2, 7, 8
curve = "Vesta"
assert torch.cuda.is_available(), "this is a measurement on the GPU"
zk.load(); zk.init(0)
backend = zk.backend_info()
print("backend:", backend, flush=True)
field = synth.CURVE_SCALAR_FIELD[curve]
fid = zk.field_id(field)
n = 1 << K
H = zk.halo2
lib = H._plib()
rows = []
def sync(): torch.cuda.synchronize()
def timed(row, what, fn, runs=RUNS, warm=WARM, **extra):
    for _ in range(warm): fn()
    ts = []
    for _ in range(runs):
        sync(); t = time.perf_counter(); fn(); sync(); ts.append((time.perf_counter() - t) * 1e3)
    r = dict(row=row, what=what, k=K, curve=curve, ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
             runs=runs, warmup=warm, clock="host wall clock around a device synchronisation", backend=backend, **extra)
    rows.append(r); print(json.dumps(r), flush=True)
    return r

# SRS, U, W
ks = synth.scalars_for(curve, n + 2, 1)
d_pts = torch.empty((n + 2, 8), dtype=torch.int64, device="cuda")
zk.fixed_base_mul_device(curve, torch.from_numpy(ks.view(np.int64)).cuda(), d_pts, n + 2)
sync()
tail = d_pts[n:].cpu().numpy().view(np.uint64)
params = H.Params.from_g(curve, K, d_pts[:n].clone(), u=tail[0], w=tail[1])
some_points = d_pts[:2 * K + 2].cpu().numpy().view(np.uint64)
mont = lambda count, seed: synth.rand_field(field, count, seed)
one = H._mont_limbs(1, zk.field_modulus(field))

# a, b
u1 = mont(K, 2)
s_a = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
a = timed("a", "zk_halo2_ipa_s_device count=1", lambda: H.compute_s(field, u1, one, out=s_a), bytes_written=32 * n)
w = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
def by_weights():
    H.vec_powers(field, w, one)
    for j in range(K):
        lib.zk_ipa_update_weights_device(fid, w.data_ptr(), n, 1 << (K - 1 - j), u1[j].ctypes.data, None)
fill = timed("b0", "vec_powers(1): the fill of ones that row b includes", lambda: H.vec_powers(field, w, one))
b = timed("b", "k x zk_ipa_update_weights_device on ones (fill included)", by_weights, bytes_moved=K * 32 * n)
same = bool((s_a == w).all().item())
rows.append(dict(row="a==b", same_vector=same)); print(rows[-1], flush=True)
# c
u8, i8 = mont(BATCH * K, 3).reshape(BATCH, K, 4), mont(BATCH, 4)
s_c = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
timed("c1", "count=8 in one call", lambda: H.compute_s(field, u8, i8, out=s_c))
ref_c = s_c.clone()
def eight_calls():
    for p in range(BATCH):
        H.compute_s(field, u8[p], i8[p], out=s_c, accumulate=p > 0)
timed("c8", "8 calls of count=1 with accumulate", eight_calls)
rows.append(dict(row="c1==c8", same_vector=bool((ref_c == s_c).all().item()))); print(rows[-1], flush=True)
# d, e, f
def proof(seed):
    sc = mont(K + 4, seed)
    rounds = [(some_points[2 + 2 * j], some_points[3 + 2 * j], sc[4 + j]) for j in range(K)]
    return some_points[0], H.IpaProof(some_points[1], sc[0], sc[1], rounds, sc[2], sc[3]), mont(1, seed + 100)[0], mont(1, seed + 200)[0]
def one_guard(seed=5):
    P, pr, x, v = proof(seed)
    m = H.MSM(params)
    m.append_term(one, P)
    return H.commitment_verify_proof(params, m, pr, x, v)
ready = one_guard().use_challenges()
timed("d", "MSM.eval() whole (n-point MSM + %d-term MSM + host sum)" % (2 * K + 4), lambda: ready.eval())
timed("e", "commitment_verify_proof + use_challenges + eval", lambda: one_guard().use_challenges().eval())
items = [proof(10 + i) for i in range(BATCH)]
weights = list(mont(BATCH, 6))
timed("f", "verify_batch of 8", lambda: H.verify_batch(params, items, weights))
# g
from oracle import zk_oracle as orc
orc.build()
threads = min(16, os.cpu_count() or 1)
bases_host = d_pts[:n].cpu().numpy().view(np.uint64)
sc_host = mont(n, 7)
t = time.perf_counter(); orc.msm_halo2(curve, bases_host, sc_host, threads=threads); dt = (time.perf_counter() - t) * 1e3
rows.append(dict(row="g", what="oracle CPU best_multiexp restatement, %d threads, one run" % threads, k=K, ms=round(dt, 1))); print(rows[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    for r in rows:
        fh.write(json.dumps(r) + "\n")
assert same and rows[6]["same_vector"]
