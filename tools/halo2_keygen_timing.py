#!/usr/bin/env python3
"""Times halo2 key generation on the device (zk.halo2.keygen_vk + keygen_pk; halo2_proofs 0.2 plonk/keygen.rs) once for the
bench's shape -- 2^k rows (default k = 20), 8 fixed and 16 permutation columns, degree 9 (extended_k = k + 3), Vesta -- and the
split by step: the Assembly on the host (2^(k + 2) random copies through copy_many), the mapping's read-back and upload, the
sigma call, the 16 permutation commitments, one transform of each kind, then keygen_vk, keygen_pk(cosets="lazy") and
keygen_pk(cosets=None) as wholes.  Wall-clock seconds around a device synchronisation, one run each after one warm-up call of
the sigma entry.  Beside them the time the tests' Python restatement takes for ONE sigma column, which is also compared with
the device's column 0.  Prints one JSON line and writes it to the path given as the second argument, if any.
usage: halo2_keygen_timing.py [k] [out.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import contangle_zkcp_amd as zk
import halo2_keygen_cases as kc

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
NF, NP, DEG, BF = 8, 16, 9, 5
curve = "Vesta"
zk.load(); zk.init(0)
print("backend:", zk.backend_info(), flush=True)
field = kc.field_of(curve)
n = 1 << K
res = {"k": K, "fixed": NF, "perm": NP, "degree": DEG, "curve": curve}
def sync(): torch.cuda.synchronize()
def timed(name, fn):
    sync(); t = time.perf_counter(); r = fn(); sync(); res[name] = round(time.perf_counter() - t, 4); print(name, res[name], flush=True); return r

# SRS
rng = np.random.default_rng(1)
ks = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64); ks[:, 3] &= np.uint64((1 << 58) - 1)
d_g = torch.empty((n, 8), dtype=torch.int64, device="cuda")
zk.fixed_base_mul_device(curve, torch.from_numpy(ks.view(np.int64)).cuda(), d_g, n)
params = timed("params_from_g_s", lambda: zk.halo2.Params.from_g(curve, K, d_g))
fixed = [torch.from_numpy(rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64).view(np.int64)).cuda() for _ in range(NF)]
# copies: 2^22 random pairs
nc = 1 << (K + 2)
quads = np.stack([rng.integers(0, NP, nc), rng.integers(0, n, nc), rng.integers(0, NP, nc), rng.integers(0, n, nc)], axis=1).astype(np.uint32)
res["copies"] = nc
asm = timed("assembly_new_s", lambda: zk.halo2.Assembly(n, NP))
timed("assembly_copy_many_s", lambda: asm.copy_many(quads))
mapping = timed("assembly_mapping_readback_s", lambda: asm.mapping())
d_map = timed("mapping_upload_s", lambda: torch.from_numpy(mapping.view(np.int64)).cuda())
sig = zk.halo2.permutation_sigmas(field, K, d_map)      # warm: power tables, scratch
sig = timed("sigma_kernel_call_s", lambda: zk.halo2.permutation_sigmas(field, K, d_map, sigmas=sig))
timed("commit_16_perm_s", lambda: params.commit_lagrange_batch(sig))
dom = zk.halo2.EvaluationDomain(field, DEG, K)
res["extended_k"] = dom.extended_k
poly = torch.zeros((n, 4), dtype=torch.int64, device="cuda"); ext = torch.zeros((dom.extended_len(), 4), dtype=torch.int64, device="cuda")
dom.lagrange_to_coeff(sig[0], out=poly); dom.coeff_to_extended(ext, coeffs=poly, lazy_out=True)
timed("one_lagrange_to_coeff_s", lambda: dom.lagrange_to_coeff(sig[0], out=poly))
timed("one_coeff_to_extended_lazy_s", lambda: dom.coeff_to_extended(ext, coeffs=poly, lazy_out=True))
del poly, ext, sig
# the whole thing, warm
vk = timed("keygen_vk_s", lambda: zk.halo2.keygen_vk(params, DEG, fixed, asm, BF))
pk = timed("keygen_pk_lazy_s", lambda: zk.halo2.keygen_pk(params, vk, fixed, asm, cosets="lazy"))
res["pk_resident_gb"] = round(torch.cuda.memory_allocated() / 2**30, 2)
pk.free(); del pk
pk = timed("keygen_pk_no_cosets_s", lambda: zk.halo2.keygen_pk(params, vk, fixed, asm, cosets=None))
# sampled check of sigma against Python, and the CPU restatement's time for ONE sigma column
def python_column(col):
    p_ = kc.modulus(field); w = kc.pyref.root_of_unity(field, K); dl = kc.delta_int(field)
    wp = [1]
    for _ in range(n - 1): wp.append(wp[-1] * w % p_)
    dp = [pow(dl, c, p_) for c in range(NP)]
    return kc.monts(field, [dp[m >> 32] * wp[m & 0xFFFFFFFF] % p_ for m in mapping[col].tolist()])
t = time.perf_counter(); exp0 = [python_column(0)]; res["python_one_sigma_column_s"] = round(time.perf_counter() - t, 3)
got0 = pk.permutation.permutations[0].cpu().numpy().view(np.uint64)
res["sigma_column0_matches_python"] = bool((got0 == exp0[0]).all())
print(json.dumps(res), flush=True)
if len(sys.argv) > 2:
    json.dump(res, open(sys.argv[2], "w"), indent=1)
assert res["sigma_column0_matches_python"]
