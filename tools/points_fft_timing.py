"""Wall time of halo2.Params.from_g (g -> g_lagrange: one zk_ntt_points_device with omega^-1 and the 1/n scaling) on one GPU.
Events on the stream around the transform alone, one warm-up, median of --reps; one JSON line per size.
    python tools/points_fft_timing.py [--curve Vesta] [--k 16 18 20] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", default="Vesta")
    ap.add_argument("--k", type=int, nargs="+", default=[16, 18, 20])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import contangle_zkcp_amd as zk
    from contangle_zkcp_amd import synth
    zk.load()
    zk.init(0)
    field = zk.scalar_field(a.curve)
    for k in a.k:
        n = 1 << k
        d_s = torch.from_numpy(synth.scalars_for(a.curve, n, 7).view("int64")).cuda()
        d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        d_out = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        zk.fixed_base_mul_device(a.curve, d_s, d_g, n)
        omega_inv = zk.field_inverse(field, zk.root_of_unity(field, k))
        times = []
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            zk.ntt_points_device(a.curve, d_g, d_out, k, omega_inv, True)
            e1.record()
            e1.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1))
        print(json.dumps({"curve": a.curve, "k": k, "reps": a.reps, "median_ms": round(statistics.median(times), 3),
                          "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}), flush=True)
    zk.shutdown()


if __name__ == "__main__":
    main()
