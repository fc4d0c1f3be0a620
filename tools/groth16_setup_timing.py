#!/usr/bin/env python3
"""Times Groth16 key generation on the device (zk.groth16.generate_parameters, ark-groth16 0.3 generate_parameters) stage by
stage, for a synthetic R1CS whose evaluation domain has 2^log_m points (2^log_m - 3 constraints + 3 inputs; 1-3 terms per A
row, 1-2 per B row, one per C row; variable 0 in every fourth A row and one A row over every variable, like the reference's
public-input packing; three quarters of the coefficients +-1):
  lagrange                    zk_lagrange_coefficients_device
  transposed_matvecs_first    the three zk_r1cs_matvec_transposed_device calls on fresh handles: includes building the
                              column-major companions (histogram, scan, scatter)
  transposed_matvecs_cached   the same three calls again
  key_scalars                 zk_groth16_key_scalars_device
  fixed_base_*                each zk_fixed_base_msm_device call (a_query, b_g1_query, b_g2_query, h_query, gamma_abc_g1 + l_query)
  d2h_encode                  copying the point vectors to the host and encoding them to the key file bytes (host encoder)
  setup_first / setup_warm    generate_parameters(...).serialize_unchecked() as a whole, on fresh handles and again
Wall-clock milliseconds around a device synchronisation, one run each (nothing here is fast enough to need repetition).  Beside
them the only CPU figure available: the oracle's fixed-base multiplication (255-bit double-and-add per point) on one thread
and on all threads, in microseconds per point, as bench.py measures it.  One JSON line per (pairing, log_m).
usage: groth16_setup_timing.py [--cases Bls381:20,Bn254:20] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import contangle_zkcp_amd as zk

NUM_INPUTS = 3


def synthetic_r1cs(field, log_m, rng):
    """CSR arrays (row_ptr, col, val in Montgomery form) of A, B, C; key generation does not need a satisfying assignment"""
    az = zk.ark_serialize
    p = zk.field_modulus(field)
    nc = (1 << log_m) - NUM_INPUTS
    n_vars = NUM_INPUTS + 4 + nc
    one, minus_one = az.scalars_from_bytes(field, (1).to_bytes(32, "little") + (p - 1).to_bytes(32, "little"), 2)
    pack = nc - 3

    def matrix(lo, hi, with_one, packing):
        cnt = rng.integers(lo, hi + 1, nc).astype(np.int64)
        defined = NUM_INPUTS + 4 + np.arange(nc, dtype=np.int64)            # variables that exist when constraint i is written
        if packing:
            cnt[pack] = defined[pack]
        row_ptr = np.zeros(nc + 1, dtype=np.uint64)
        row_ptr[1:] = np.cumsum(cnt)
        nnz = int(row_ptr[-1])
        row_of = np.repeat(np.arange(nc, dtype=np.int64), cnt)
        col = (rng.integers(0, 1 << 62, nnz) % defined[row_of]).astype(np.uint32)
        if with_one:
            col[row_ptr[:-1][::4].astype(np.int64)] = 0
        if packing:
            s = int(row_ptr[pack])
            col[s:s + int(cnt[pack])] = np.arange(int(cnt[pack]), dtype=np.uint32)
        val = rng.integers(0, 1 << 63, (nnz, 4), dtype=np.uint64)
        val[:, 3] &= np.uint64((1 << 58) - 1)                                # any limbs below the modulus are a valid element
        kind = rng.integers(0, 8, nnz)
        val[kind < 4] = one
        val[(kind >= 4) & (kind < 6)] = minus_one
        return row_ptr, col, val

    a, b = matrix(1, 3, True, True), matrix(1, 2, False, False)
    c_ptr = np.arange(nc + 1, dtype=np.uint64)
    c = (c_ptr, (NUM_INPUTS + 4 + np.arange(nc)).astype(np.uint32), np.tile(one, (nc, 1)))
    return (a, b, c), nc, n_vars


def upload(field, csr, n_vars):
    return [zk.groth16.R1csMatrix(field, n_cols=n_vars, csr=m) for m in csr]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round((time.perf_counter() - t0) * 1e3, 3)


def cpu_rates(curve):
    from contangle_zkcp_amd import synth
    from oracle import zk_oracle as orc
    threads = min(256, int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count() or 1)
    k1, k = synth.scalars_for(curve, 1 << 9, 78), synth.scalars_for(curve, 1 << 15, 77)
    t0 = time.perf_counter()
    orc.fixed_base_mul(curve, k1, threads=1)
    one = (time.perf_counter() - t0) / (1 << 9)
    t0 = time.perf_counter()
    orc.fixed_base_mul(curve, k, threads=threads)
    return {"threads": threads, "one_thread_us_per_point": round(one * 1e6, 2), "all_threads_us_per_point": round((time.perf_counter() - t0) / (1 << 15) * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="Bls381:20,Bn254:20")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    zk.load()
    zk.init(0)
    torch.cuda.set_device(0)
    g16, az = zk.groth16, zk.ark_serialize
    for case in args.cases.split(","):
        pairing, log_m = case.split(":")
        log_m = int(log_m)
        field = "Bls381Fr" if pairing == "Bls381" else "Bn254Fr"
        c1, c2 = az.PAIRING_CURVES[az.pairing_id(pairing)]
        rng = np.random.default_rng(log_m)
        csr, nc, n_vars = synthetic_r1cs(field, log_m, rng)
        m = 1 << log_m
        p = zk.field_modulus(field)
        trap = az.scalars_from_bytes(field, b"".join(int(1 + int(rng.integers(0, 1 << 62)) * 0x9E3779B97F4A7C15F39CC0605CEDC835 % (p - 1)).to_bytes(32, "little")
                                                     for _ in range(5)), 5)
        alpha, beta, gamma, delta, tau = trap
        rec = {"pairing": pairing, "log_m": log_m, "num_constraints": nc, "num_inputs": NUM_INPUTS, "n_vars": n_vars,
               "nnz": [int(mm[0][-1]) for mm in csr], "backend": zk.backend_info()}
        # the whole setup, cold (fresh handles: includes the transpositions) and warm
        mats = upload(field, csr, n_vars)
        whole = lambda: g16.generate_parameters(pairing, mats[0], mats[1], mats[2], NUM_INPUTS, n_vars, alpha, beta, gamma, delta, tau).serialize_unchecked()
        blob, rec["setup_first_ms"] = timed(whole)
        blob2, rec["setup_warm_ms"] = timed(whole)
        assert blob == blob2
        rec["key_bytes"] = len(blob)
        del blob, blob2
        for mtx in mats:
            mtx.free()
        # stage by stage, on fresh handles
        mats = upload(field, csr, n_vars)
        new = lambda n, w=4: torch.zeros((n, w), dtype=torch.int64, device="cuda")
        d_L, d_u, d_v, d_w, d_h = new(m), new(n_vars), new(n_vars), new(n_vars), new(m - 1)
        zt, rec["lagrange_ms"] = timed(lambda: g16.lagrange_coefficients(field, log_m, tau, d_L))
        three = lambda: [mtx.matvec_transposed(d_L, out) for mtx, out in zip(mats, (d_u, d_v, d_w))]
        _, rec["transposed_matvecs_first_ms"] = timed(three)
        _, rec["transposed_matvecs_cached_ms"] = timed(three)
        _, rec["key_scalars_ms"] = timed(lambda: g16.key_scalars(field, d_u, d_v, d_w, NUM_INPUTS, log_m, alpha, beta, gamma, delta, tau, zt, d_w, d_h))
        l1, l2 = 2 * zk.base_limbs(c1), 2 * zk.base_limbs(c2)
        pts = {}
        for name, curve, d_s, limbs in (("a_query", c1, d_u, l1), ("b_g1_query", c1, d_v, l1), ("b_g2_query", c2, d_v, l2), ("h_query", c1, d_h, l1),
                                        ("abc", c1, d_w, l1)):
            out = new(int(d_s.shape[0]), limbs)
            _, rec["fixed_base_%s_ms" % name] = timed(lambda: zk.fixed_base_msm_device(curve, d_s, out, int(d_s.shape[0]), montgomery=True))
            pts[name] = out

        def encode():
            total = 0
            for name, curve in (("a_query", c1), ("b_g1_query", c1), ("b_g2_query", c2), ("h_query", c1), ("abc", c1)):
                total += len(az.vec_to_bytes(curve, pts[name].cpu().numpy().view(np.uint64), False))
            return total
        _, rec["d2h_encode_ms"] = timed(encode)
        stages = {k: v for k, v in rec.items() if k.endswith("_ms") and not k.startswith("setup_") and k != "transposed_matvecs_cached_ms"}
        rec["dominant_stage"] = max(stages, key=stages.get)
        if not args.no_cpu:
            rec["cpu_oracle_fixed_base"] = {c1: cpu_rates(c1), c2: cpu_rates(c2)}
        print(json.dumps(rec), flush=True)
        for mtx in mats:
            mtx.free()
        del pts, d_L, d_u, d_v, d_w, d_h
    zk.shutdown()


if __name__ == "__main__":
    main()
