#!/usr/bin/env python3
"""Times zk_halo2_permute_expression_pair_device (the lookup argument's permute_expression_pair on the device) on PallasFp at
2^20 and 2^22 rows (usable = n - 6: the bench's 5 blinding rows + 1), for two input shapes:
  range_check   the reference's 10-bit range check: table 0..1023 then zeros, ~70 % of the inputs 0
  random_dups   theta-compressed full-width values: 3000 distinct values, repeated
3 warm-up calls, then 20 calls timed with device events on one stream (each call synchronises its stream once, at the end,
so an event pair brackets exactly one call).  Also printed: the live 8-bit digits of the merged keys, the bytes the LSD
passes move (3 x 2u keys x 32 B per live digit: count read, scatter read + write) and, at 2^20, the host mirror
halo2.permute_expression_pair (numpy + Python integers, CPU).  One JSON line per case.
usage: lookup_permute_timing.py [--sizes 20,22] [--no-host]"""
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

FIELD = "PallasFp"


def canonical_case(dist, u, rng):
    """(inputs, table) canonical limbs [u, 4] (values below 2^254 < p)"""
    if dist == "range_check":
        m = min(1024, u)
        tv = np.zeros(u, dtype=np.uint64)
        tv[:m] = np.arange(m, dtype=np.uint64)
        iv = np.where(rng.random(u) < 0.7, 0, rng.integers(0, m, u)).astype(np.uint64)
        pad = lambda v: np.stack([v, np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)], axis=1)
        return pad(iv), pad(tv)
    vals = rng.integers(0, 1 << 63, (3000, 4), dtype=np.uint64, endpoint=False) * 2 + rng.integers(0, 2, (3000, 4), dtype=np.uint64)
    vals[:, 3] &= np.uint64((1 << 62) - 1)
    table = np.concatenate([vals, vals[rng.integers(0, len(vals), u - len(vals))]])
    return vals[rng.integers(0, len(vals), u)], table


def live_digits(inputs, table):
    """8-bit digits of the merged keys (value << 1 | tag) in which more than one bucket is used"""
    c = np.concatenate([inputs, table])
    tag = np.concatenate([np.zeros(len(inputs), np.uint64), np.ones(len(table), np.uint64)])
    k = np.empty_like(c)
    k[:, 0] = (c[:, 0] << np.uint64(1)) | tag
    for w in range(1, 4):
        k[:, w] = (c[:, w] << np.uint64(1)) | (c[:, w - 1] >> np.uint64(63))
    live = 0
    for d in range(32):
        b = (k[:, d // 8] >> np.uint64(8 * (d % 8))) & np.uint64(255)
        live += int((b != b[0]).any())
    return live


def to_mont_device(canon):
    d = torch.from_numpy(np.ascontiguousarray(canon).view(np.int64)).cuda()
    zk.vec_op(FIELD, "from_repr", d)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,22")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    zk.load()
    zk.init(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(20)
    for logn in [int(s) for s in args.sizes.split(",")]:
        n = 1 << logn
        u = n - 6
        for dist in ("range_check", "random_dups"):
            ci, ct = canonical_case(dist, u, rng)
            d_in, d_tab = to_mont_device(np.concatenate([ci, np.zeros((6, 4), np.uint64)])), to_mont_device(np.concatenate([ct, np.zeros((6, 4), np.uint64)]))
            a_out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            s_out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            call = lambda: zk.halo2.permute_expression_pair_device(FIELD, d_in, d_tab, u, a_out, s_out, stream=stream.cuda_stream)
            for _ in range(3):
                call()
            ms = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            live = live_digits(ci, ct)
            rec = {"field": FIELD, "log_n": logn, "usable_rows": u, "dist": dist, "gpu_ms_median": round(float(np.median(ms)), 4),
                   "gpu_ms_min": round(min(ms), 4), "gpu_ms_max": round(max(ms), 4), "calls": len(ms), "live_digits": live,
                   "lsd_bytes": live * 3 * 2 * u * 32}
            if not args.no_host and logn <= 20:
                host_in, host_tab = d_in.cpu().numpy().view(np.uint64), d_tab.cpu().numpy().view(np.uint64)
                t0 = time.perf_counter()
                ha, hs = zk.halo2.permute_expression_pair(FIELD, host_in, host_tab, u)
                rec["cpu_host_mirror_s"] = round(time.perf_counter() - t0, 3)
                torch.cuda.synchronize()
                rec["matches_host_mirror"] = bool((a_out[:u].cpu().numpy().view(np.uint64) == ha).all() and
                                                  (s_out[:u].cpu().numpy().view(np.uint64) == hs).all())
            print(json.dumps(rec), flush=True)
            del d_in, d_tab, a_out, s_out
    zk.shutdown()


if __name__ == "__main__":
    main()
