"""CPU: the MSM launch plan (contangle-zkcp_amd/csrc/zk_msm_plan.h) through the g++ runner tests/emu/msm_plan_check, which includes
nothing but that header.  The plan is not restated here: it is held against what the project states elsewhere, in Python integers --
the workspace sizes of DESIGN.md section 4, the bounds the kernels index by, the refusal boundaries, and the window groups of the
small shapes the emulator tests use.  The runner is built a second time with -fsanitize=undefined,address (a stand-alone program)
and must print the same lines."""
import functools
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "contangle-zkcp_amd", "csrc")
OK, UNSUPPORTED = 0, -6

# the kernel views: sizeof(XYZZ<CK>), sizeof(XYZZ<C>), tree lanes, resident accumulate waves, diagnostic words per partial, lazy.
# An XYZZ point is 4 base-field coordinates (8 on G2) of 9 x 29-bit limbs (14 x 28 for BLS12-381) or 8 (12) 32-bit words; 256 of
# them must fit 48 KiB of LDS or the tree kernels run 128 lanes (zk_msm_kernels.h)
VIEWS = {
    "pasta29": (144, 128, 256, 4, 4 * (27 + 8), 1),
    "pasta32": (128, 128, 256, 4, 0, 0),
    "bls381g1_29": (224, 192, 128, 2, 4 * (42 + 12), 1),
    "bn254g2_29": (288, 256, 128, 2, 8 * (27 + 8), 1),
    "bls381g2_29": (448, 384, 128, 1, 8 * (42 + 12), 1),
}
FR_BITS = {"pasta": 255, "bn254": 254, "bls381": 255}      # the six curves' scalar fields


def windows(c, bits=255):
    return (bits + 1 + c - 1) // c


def shape(n, c, nwin=None, w0=0, w1=None, batch=1, pre=0, slices=0, devp=0, group=0, cus=256, view="pasta29"):
    nwin = windows(c) if nwin is None else nwin
    return (n, c, nwin, w0, nwin if w1 is None else w1, batch, pre, slices, devp, group, cus) + VIEWS[view]


def build(sanitize=False):
    src = os.path.join(EMU, "msm_plan_check.cc")
    exe = os.path.join(EMU, "msm_plan_check" + ("_san" if sanitize else ""))
    deps = [src, os.path.join(CSRC, "zk_msm_plan.h"), os.path.join(ROOT, "include", "zkcp_amd.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        flags = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-O1", "-std=c++17"] + flags +
                              ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    return exe


def run_text(shapes, sanitize=False):
    text = "".join(" ".join(map(str, s)) + "\n" for s in shapes)
    # (the runner allocates nothing: the leak check at exit, which needs ptrace rights some containers withhold, is left out)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0") if sanitize else None
    return subprocess.run([build(sanitize)], input=text, stdout=subprocess.PIPE, text=True, check=True, env=env).stdout


def parse(line):
    d = {}
    for kv in line.split():
        k, v = kv.split("=")
        if k == "groups":                                  # (status, windows) per group
            d[k] = [tuple(map(int, g.split(":"))) for g in v.split(",")]
        else:
            d[k] = tuple(map(int, v.split(","))) if "," in v else int(v)
    return d


def run(shapes):
    lines = run_text(shapes).strip().split("\n")
    assert len(lines) == len(shapes)
    return [parse(l) for l in lines]


# ---- the sweep: every window width, sizes around the powers of two and the thresholds of the plan, both forms; and the other
# options (a window sub-range, batches, the slice reduction, the diagnostic partials, the other views) at a few widths
SIZES = sorted({1, 60, 300} | {(1 << k) + d for k in (8, 12, 13, 14, 15, 16, 20, 24, 26, 27, 28, 30) for d in (-1, 0, 1)} | {(1 << 31) - 1, 1 << 31})


@functools.lru_cache(None)
def sweep():
    shapes = []
    for n, c, pre in itertools.product(SIZES, range(2, 21), (0, 1)):
        shapes.append(shape(n, c, pre=pre))
    for n, c in itertools.product(SIZES, (4, 8, 15, 16, 20)):
        nwin = windows(c)
        shapes.append(shape(n, c, w0=nwin // 2))
        shapes.append(shape(n, c, w1=nwin // 2, batch=3))
        shapes.append(shape(n, c, nwin=windows(c, FR_BITS["bn254"]), batch=4))
        shapes.append(shape(n, c, batch=4, pre=1))
        shapes.append(shape(n, c, slices=1, view="pasta32"))
        shapes.append(shape(n, c, slices=1, batch=2, view="bls381g2_29", cus=64))
        shapes.append(shape(n, c, devp=1, view="bls381g1_29"))
        shapes.append(shape(n, c, devp=1, pre=1, view="bn254g2_29", cus=1))
    return shapes, run(shapes)


def pow2(x):
    return x > 0 and x & (x - 1) == 0


def test_sweep_sizes_and_bounds():
    shapes, plans = sweep()
    accepted = 0
    for s, p in zip(shapes, plans):
        n, c, nwin, w0, w1, batch, pre, slices, devp = s[:9]
        xyzz_ck, xyzz_c, tl, waves, dbg_words, lazy = s[11:]
        assert p["status"] in (OK, UNSUPPORTED), s
        if p["status"] != OK:
            continue
        accepted += 1
        W = p["nw"]                                        # windows of the job
        N = p["n"]                                         # entries per window
        assert (W, N) == ((batch, n * nwin) if pre else (batch * (w1 - w0), n)), s
        # DESIGN section 4, as requested bytes
        assert p["digits_bytes"] == W * N * (4 if pre else 2), s
        assert p["stage_idx_bytes"] + p["stage_low_bytes"] == W * N * (4 + 2), s
        assert p["sorted_bytes"] == W * N * 4, s
        assert p["buckets_bytes"] == W * 2 ** (c - 1) * xyzz_ck, s
        assert p["subacc_bytes"] == (p["buckets_bytes"] << p["split_log"] if p["split_log"] else 0), s
        # what the kernels index by
        assert n < 2 ** 31 and W * N < 2 ** 32, s
        assert p["nranges"] * p["rb"] == p["nbk"] == 2 ** (c - 1), s
        assert p["nreg"] == W * p["nranges"] <= 4096, s
        assert p["nranges"] <= (1024 if pre else 64), s
        assert pow2(p["sblk"]) and 256 <= p["sblk"] <= 4096, s
        assert p["nblocks_real"] == -(-n // p["sblk"]), s
        assert p["nblocks_real"] >= 64 or n < 64 * 256, s
        assert not pre or n % p["sblk"] == 0, s
        assert p["cap"] % 2 == 0 and p["cap"] <= 24576, s
        assert pow2(p["seg"]) and 128 <= p["seg"] <= 2048, s
        assert 0 <= p["split_log"] <= 4, s
        assert 1 <= p["accumulate"][0] <= p["ntasks"], s
        assert p["accumulate"][0] <= s[10] * 4 * waves, s
        assert 1 <= p["hot_slices"] <= 32 and (not p["hot_help"] or p["nreg"] <= 1024), s
        for k, v in p.items():                             # every launch: a non-empty grid, <= 1024 lanes, <= 64 KiB of LDS
            if isinstance(v, tuple) and len(v) == 3:
                assert v[0] >= 1 and 64 <= v[1] <= 1024 and v[2] <= 65536, (s, k, v)
        # the sub-arrays lie inside their workspaces, one behind the other
        assert p["offs_at"] == p["nbuckets"] * 4 and p["order_at"] == p["nbuckets"] * 8 and p["wg_total_at"] == p["nbuckets"] * 12, s
        assert p["region_base_at"] == p["wg_total_at"] + p["nreg"] * 4 and p["counts_bytes"] == p["region_base_at"] + p["nreg"] * 4, s
        assert p["seg_list_at"] == 16 and p["big_list_at"] == 16 + p["max_seg"] * 16, s
        assert p["queue_bytes"] >= p["big_list_at"] + p["max_big"] * 4 and p["seg_out_bytes"] == p["max_seg"] * xyzz_ck, s
        # no list can overflow: more than big_thresh entries make a bucket oversized, and it yields ceil(entries / seg) segments
        assert p["max_big"] * p["big_thresh"] > W * N, s
        assert p["max_seg"] * p["seg"] * p["big_thresh"] >= W * N * (p["big_thresh"] + p["seg"]), s
        assert p["blockcnt_bytes"] == p["nreg"] * p["nblocks"] * 4, s
        if p["hot_help"]:
            assert p["hot_list_at"] == p["nreg"] * 4 and p["gcur_at"] == p["hot_list_at"] + 9 * 4 and p["hot_bytes"] == p["gcur_at"] + p["nbuckets"] * 4, s
        else:
            assert p["hot_bytes"] == 0, s
        # the partial sums that go to the host
        assert bool(p["axes"]) == (not slices) and bool(p["dev_std"]) == bool(devp and lazy and not slices), s
        assert p["pbytes1"] == xyzz_ck + ((xyzz_c + 4 * dbg_words) if p["dev_std"] else 0) and p["hbytes"] == W * p["per"] * p["pbytes1"], s
        if p["axes"]:
            assert p["rows"] * p["cols"] == p["nbk"] and p["cols"] == 2 ** p["log_cols"] and p["rows"] <= p["cols"], s
            assert p["per"] == 2 * (p["row_blocks"] + p["col_blocks"]) and 2 ** p["log_tl"] == tl, s
            assert p["row_blocks"] * tl >= p["rows"] and p["col_blocks"] * tl >= p["cols"], s
            assert p["part_a_bytes"] == (p["row_lanes"] + p["col_lanes"]) * xyzz_ck, s
            assert p["part_b_out_at"] == W * (p["rows"] + p["cols"]) * xyzz_ck and p["part_b_bytes"] == p["part_b_out_at"] + W * p["per"] * xyzz_ck, s
            if p["dev_std"]:
                np_ = W * p["per"]
                assert p["std_at"] == np_ * xyzz_ck and p["dbg_at"] == p["std_at"] + np_ * xyzz_c, s
                assert p["part_std_bytes"] == p["dbg_at"] + np_ * 4 * dbg_words == p["hbytes"], s
            else:
                assert p["part_std_bytes"] == 0, s
        else:
            assert p["per"] <= 8 and p["spw"] * p["L"] >= p["nbk"] and p["nslices"] == W * p["spw"], s
            assert p["part_a_bytes"] == p["nslices"] * xyzz_ck, s
            per = p["spw"]
            for k in range(p["nsum"]):                     # the tree: every step fits the buffer it writes, the last leaves `per`
                pin, pout, e, grid, block = p["sum%d" % k]
                assert pin == per and pout * block * e >= pin and grid == W * pout and block == tl, s
                assert pout * W * xyzz_ck <= (p["part_b_bytes"] if k % 2 == 0 else p["part_a_bytes"]), s
                per = pout
            assert per == p["per"], s
    assert accepted > len(shapes) // 3


def test_refusal_boundaries():
    cases = [
        (shape(1 << 27, 16, nwin=16), OK),                 # Vesta-sized windows: n W = 2^31 entry positions
        (shape(1 << 28, 16, nwin=16), UNSUPPORTED),        # 2^32 of them
        (shape(1 << 31, 16, nwin=16), UNSUPPORTED),
        (shape(1 << 31, 8), UNSUPPORTED),
        (shape(1 << 20, 16, nwin=16, batch=4), OK),        # 4 x 16 windows x 64 ranges = 4096 regions
        (shape(1 << 20, 16, nwin=16, batch=5), UNSUPPORTED),
        (shape(1 << 20, 20, pre=1), OK),
        (shape((1 << 20) + 1, 20, pre=1), UNSUPPORTED),    # the table must tile into scalar blocks
        (shape(1 << 20, 20, pre=1, w0=1), UNSUPPORTED),    # the precomputed form takes the whole scalar
        (shape(1 << 20, 20, pre=1, w1=12), UNSUPPORTED),
    ]
    plans = run([c[0] for c in cases])
    for (s, want), p in zip(cases, plans):
        assert p["status"] == want, s
    assert plans[0]["n"] * plans[0]["nw"] == 2 ** 31
    assert plans[4]["nreg"] == 4096 and plans[4]["per_job"] == 4
    assert (plans[6]["pre_w"], plans[6]["nranges"], plans[6]["nw"], plans[6]["n"]) == (13, 1024, 1, 13 << 20)
    # zk_msm_batch_device: four vectors where they fit, one where four would pass the u32 entry positions
    assert [p["per_job"] for p in run([shape(1 << 25, 16, nwin=16), shape(1 << 26, 16, nwin=16), shape(1 << 20, 20, pre=1)])] == [4, 1, 4]


@pytest.mark.parametrize("group", [1, 3, 5, 100])
def test_window_groups_of_the_small_shapes(group):
    shapes = [shape(300, 8, group=group), shape(60, 5, group=group), shape(300, 4, group=group), shape(300, 8, w0=3, w1=20, group=group),
              shape(60, 5, slices=1, view="pasta32", group=group)]
    for s, p in zip(shapes, run(shapes)):
        nwj = s[4] - s[3]
        assert p["status"] == OK and all(st == OK for st, _ in p["groups"]), s
        sizes = [w for _, w in p["groups"]]
        assert sum(sizes) == nwj and len(sizes) == p["ng"] == -(-nwj // min(group, nwj)), s
        assert max(sizes) == p["gw"] <= min(group, nwj) and min(sizes) >= 1, s
    assert run([shape(300, 4)])[0]["nranges"] == 1


def test_sanitized_runner_prints_the_same():
    """the plan's arithmetic under -fsanitize=undefined,address (-fno-sanitize-recover): same lines, clean exit"""
    shapes, _ = sweep()
    assert run_text(shapes, sanitize=True) == run_text(shapes)
