#!/usr/bin/env python3
"""Times the stages of Groth16 verification at the reference's key shape: gamma_abc_g1 of 196 611 compressed BLS12-381 G1 points
(2 + n public inputs with n = 196 608, circuits-ark/src/encryption.rs:139-152).  The points are generated on the device
(zk_fixed_base_msm_device over random scalars) and encoded by the host encoder; then
  decode_device    zk_ark_points_decode_checked_device: the copy of the bytes to the device, the kernel, the status word
  decode_host      zk_ark_points_decode_checked on the host threads this process may use (at most 16 are taken)
  prepare_inputs   zk_groth16_prepare_inputs over the resident gamma_abc_g1[1..] at 196 610 inputs (scalars already on the device)
  verify_tail      zk_groth16_verify on the host: three Miller loops and one final exponentiation, the right-hand side cached
Wall-clock milliseconds around calls that synchronise; `warmup` unrecorded runs, then `repeat` recorded ones: median, minimum and
maximum.  Appends one JSON line to --out.
usage: groth16_verify_timing.py [--n 196611] [--pairing Bls381] [--repeat 7] [--host-repeat 3] [--out profiles/groth16_verify_timing.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import contangle_zkcp_amd as zk


def timed(fn, warmup, repeat):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": repeat}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=196611)
    ap.add_argument("--pairing", default="Bls381")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--host-repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify_timing.jsonl"))
    args = ap.parse_args()
    cpus = sorted(os.sched_getaffinity(0))
    if len(cpus) > 16:
        os.sched_setaffinity(0, cpus[:16])
    az, g16 = zk.ark_serialize, zk.groth16
    zk.init(0)
    pairing = az.pairing_id(args.pairing)
    g1, g2 = az.PAIRING_CURVES[pairing]
    field = "Bls381Fr" if pairing == az.BLS12_381 else "Bn254Fr"
    n, limbs = args.n, 2 * zk.base_limbs(g1)
    rng = np.random.default_rng(0x5EED)

    def random_scalars(count):
        a = rng.integers(0, 1 << 63, (count, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 58) - 1)                      # any limbs below the modulus are a valid (Montgomery) element
        return torch.from_numpy(a.view(np.int64)).cuda()

    d_pts = torch.zeros((n, limbs), dtype=torch.int64, device="cuda")
    zk.fixed_base_msm_device(g1, random_scalars(n), d_pts, n, montgomery=True)
    torch.cuda.synchronize()
    pts = d_pts.cpu().numpy().view(np.uint64)
    buf = az.points_to_bytes(g1, pts, True)
    d_out = torch.zeros((n, limbs), dtype=torch.int64, device="cuda")
    rec = {"pairing": args.pairing, "n_points": n, "encoded_bytes": len(buf), "backend": zk.backend_info(),
           "host_threads": len(os.sched_getaffinity(0))}
    rec["decode_device"] = timed(lambda: az.points_from_bytes_checked_device(g1, buf, n, d_out), args.warmup, args.repeat)
    assert (d_out.cpu().numpy().view(np.uint64) == pts).all()
    host = [None]

    def host_decode():
        host[0] = az.points_from_bytes_checked(g1, buf, n, True)

    rec["decode_host"] = timed(host_decode, 1, args.host_repeat)
    assert (host[0] == pts).all()
    # prepare_inputs over the decoded, resident points
    d_g2 = torch.zeros((3, 2 * zk.base_limbs(g2)), dtype=torch.int64, device="cuda")
    zk.fixed_base_msm_device(g2, random_scalars(3), d_g2, 3, montgomery=True)
    torch.cuda.synchronize()
    g2s = d_g2.cpu().numpy().view(np.uint64)
    vk = g16.VerifyingKey(pairing, pts[0], g2s[0], g2s[1], g2s[2], d_out)
    pvk = g16.prepare_verifying_key(vk)
    d_x = random_scalars(n - 1)
    g_ic = [None]

    def prep():
        g_ic[0] = g16.prepare_inputs(pvk, d_x)

    rec["prepare_inputs"] = timed(prep, args.warmup, args.repeat)
    proof = (pts[1], g2s[0], pts[2])                             # points of the right subgroups: the verdict is False, the work is the same
    rec["verify_tail"] = timed(lambda: g16.verify_proof_with_prepared_inputs(pvk, proof, g_ic[0]), 1, args.repeat)
    rec["decode_speedup_device_over_host"] = round(rec["decode_host"]["median_ms"] / rec["decode_device"]["median_ms"], 2)
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    zk.shutdown()


if __name__ == "__main__":
    main()
