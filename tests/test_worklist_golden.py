"""The bench's halo2 work-list, every proof element it dumps, against an independent restatement (oracle/pyref_halo2_worklist.py ->
tests/golden/halo2_worklist_*.json).

CPU: the goldens regenerate byte for byte; the generator's circuit constants are bench.py's (read with ast); the generator loads no
product module but synth.py; the comparator decodes bench.py's dump encoding and names the array and row of a one-bit change; the
one undocumented deviation of the bench from upstream (BENCH_SHORTCUTS perm_chunk_link) changes exactly the arrays it lists.
GPU: `bench.py --dump-outputs` in every mode of the work-list, each dump compared word for word with its golden."""
import ast
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import pyref_halo2_worklist as W
from test_bench_consistency import _limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _golden(cfg):
    return json.load(open(W.golden_path(cfg)))


def _want(gold, name):
    return np.array([[int(w, 16) for w in row] for row in gold["arrays"][name]], dtype=np.uint64)


def compare(arrays, gold):
    """arrays: {name: uint64 limbs as dumped} -> one line per array that differs from the golden (shape, or the count and first
    mismatching row), [] when every word is equal"""
    problems = []
    for name in W.OUTPUT_NAMES:
        want = _want(gold, name)
        shape = (want.shape[1],) if name in W.SINGLE_OUTPUTS else want.shape
        if name not in arrays:
            problems.append("%s: missing" % name)
            continue
        got = np.asarray(arrays[name])
        if got.shape != shape:
            problems.append("%s: shape %s, want %s" % (name, got.shape, shape))
            continue
        got = got.reshape(want.shape)
        bad = np.flatnonzero((got != want).any(axis=1))
        if bad.size:
            i = int(bad[0])
            problems.append("%s: %d of %d rows differ, first row %d%s: got %s want %s" % (
                name, bad.size, want.shape[0], i, " (%s)" % gold["eval_rows"][name][i] if name in gold["eval_rows"] else "",
                [hex(int(w)) for w in got[i]], [hex(int(w)) for w in want[i]]))
    for name in sorted(set(arrays) - set(W.OUTPUT_NAMES)):
        problems.append("%s: not in the golden" % name)
    return problems


def load_dump(d):
    return {f[:-4]: _limbs(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def _bench_source():
    return ast.parse(open(BENCH).read(), BENCH)


def _bench_dump_outputs():
    """bench.py's dump_outputs (and the budget it reads), taken from its source without importing bench.py"""
    ns = {"os": os}
    for node in _bench_source().body:
        if (isinstance(node, ast.FunctionDef) and node.name == "dump_outputs") or (
                isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "DUMP_MAX_BYTES" for t in node.targets)):
            exec(compile(ast.Module(body=[node], type_ignores=[]), BENCH, "exec"), ns)
    return ns["dump_outputs"]


def _write_dump(gold, d):
    """the golden's arrays through bench.py's own dump encoder (single elements 1-D, as the bench holds them)"""
    class E:
        pass
    e = E()
    e.np, e.args = np, E()
    e.args.dump_outputs = str(d)
    arrs = {}
    for name in W.OUTPUT_NAMES:
        a = _want(gold, name)
        arrs[name] = a[0] if name in W.SINGLE_OUTPUTS else a
    _bench_dump_outputs()(e, arrs)


# ------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("cfg", sorted(W.CONFIGS))
def test_goldens_regenerate_exactly(cfg):
    doc = W.golden_document(cfg)
    assert doc["generator_sha256"] == W.source_sha256()
    assert json.loads(json.dumps(doc)) == _golden(cfg), "python -m oracle.pyref_halo2_worklist --write"


def test_constants_are_the_bench_constants():
    consts = {}
    for node in _bench_source().body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Tuple):
            consts.update(zip([t.id for t in node.targets[0].elts], ast.literal_eval(node.value)))
        elif isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "NCOL":
            consts["NCOL"] = ast.literal_eval(node.value)
    for name in ("N_INST", "N_FIXED", "N_PERM_COLS", "PERM_CHUNK", "N_H_PIECES", "NCOL"):
        assert consts[name] == getattr(W, name), name


def test_domain_constants_are_pastas():
    from parity_suite import PASTA_ZETA
    for curve, k in (("Vesta", 8), ("Pallas", 12)):
        dom = W.Domain(W.Field(W.SCALAR_FIELD[curve]), W.GATE_DEGREE, k)
        p = dom.F.p
        assert dom.zeta == PASTA_ZETA[dom.F.name] and pow(dom.zeta, 3, p) == 1 != dom.zeta
        assert dom.extended_k == k + 3 and pow(dom.extended_omega, 8, p) == dom.omega and pow(dom.omega, 1 << (k - 1), p) == p - 1


def test_generator_loads_no_product_module():
    code = ("import sys; from oracle import pyref_halo2_worklist as w; w.generate('Vesta', 4); "
            "bad = [m for m in sys.modules if m.startswith('contangle') or m in ('bench', 'halo2')]; assert not bad, bad")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    src = ast.parse(open(W.__file__.replace(".pyc", ".py")).read())
    imported = {a.name for n in ast.walk(src) if isinstance(n, ast.Import) for a in n.names}
    imported |= {n.module or "" for n in ast.walk(src) if isinstance(n, ast.ImportFrom)}
    assert not [m for m in imported if "contangle" in m or m in ("bench", "halo2")], imported


def test_golden_shapes_and_rows():
    for cfg, (curve, k) in W.CONFIGS.items():
        g = _golden(cfg)
        assert g["curve"] == curve and g["logn"] == k
        a = g["arrays"]
        assert len(a["instance_advice_commitments"]) == 16 and len(a["h_commitments"]) == 8 and len(a["ipa_L"]) == k
        assert len(a["evals_at_x"]) == len(g["eval_rows"]["evals_at_x"]) and "h0" in g["eval_rows"]["evals_at_x"]
        assert g["eval_rows"]["evals_at_omega_last_x"] == ["zp0", "zp1"] and g["eval_rows"]["evals_at_omega_inv_x"] == ["lkA'"]
        for name in W.OUTPUT_NAMES:
            width = 8 if name in W.POINT_OUTPUTS else 4
            assert all(len(r) == width for r in a[name]), name
            if name in W.POINT_OUTPUTS:
                assert all(any(int(w, 16) for w in r) for r in a[name]), name


def test_comparator_decodes_the_bench_encoding(tmp_path):
    gold = _golden("vesta_k8")
    _write_dump(gold, tmp_path)
    dumped = load_dump(tmp_path)
    assert sorted(dumped) == sorted(W.OUTPUT_NAMES)
    assert compare(dumped, gold) == []
    raw = np.load(tmp_path / "ipa_a.npy")
    w = int(gold["arrays"]["ipa_a"][0][0], 16)
    assert raw.dtype == np.float32 and [int(v) for v in raw[0, :4]] == [(w >> (16 * i)) & 0xFFFF for i in range(4)]   # least significant first


@pytest.mark.parametrize("name,row,word,piece,bit", [("h_commitments", 5, 6, 3, 15), ("instance_advice_commitments", 0, 0, 0, 0),
                                                     ("evals_at_x", 17, 2, 1, 7), ("v", 0, 3, 3, 13), ("ipa_L", 7, 1, 2, 4),
                                                     ("ipa_vr", 3, 0, 0, 9), ("ipa_a", 0, 3, 1, 0), ("q_commitment", 0, 4, 0, 1)])
def test_comparator_names_a_one_bit_change(tmp_path, name, row, word, piece, bit):
    gold = _golden("vesta_k8")
    _write_dump(gold, tmp_path)
    f = tmp_path / (name + ".npy")
    a = np.load(f)
    flat = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(1, -1)
    flat[row, 4 * word + piece] = float(int(flat[row, 4 * word + piece]) ^ (1 << bit))
    np.save(f, flat.reshape(a.shape))
    problems = compare(load_dump(tmp_path), gold)
    assert len(problems) == 1 and problems[0].startswith(name + ": 1 of ") and ("first row %d" % row) in problems[0], problems


def test_comparator_rejects_a_congruent_non_canonical_word():
    gold = _golden("vesta_k8")
    arrs = {n: (_want(gold, n)[0] if n in W.SINGLE_OUTPUTS else _want(gold, n)) for n in W.OUTPUT_NAMES}
    p = W.Field(W.SCALAR_FIELD["Vesta"]).p
    v = W._words_to_int(arrs["evals_at_x"][2].tolist()) + p
    assert v < 1 << 256
    arrs["evals_at_x"][2] = [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    assert [s.split(":")[0] for s in compare(arrs, gold)] == ["evals_at_x"]


def test_bench_deviation_from_upstream_is_visible():
    """BENCH_SHORTCUTS entries with an upstream switch: the as-built and the upstream work-list differ in exactly the listed arrays"""
    built, _ = W.generate("Vesta", 6)
    for s in W.BENCH_SHORTCUTS:
        if s.get("upstream_switch"):
            up, _ = W.generate("Vesta", 6, upstream=(s["name"],))
            assert sorted(n for n in W.OUTPUT_NAMES if up[n] != built[n]) == sorted(s["changes"]), s["name"]


# ------------------------------------------------------------------ GPU tier
MODES = [("vesta_k8", "default", ()), ("vesta_k8", "qp2", ("--quotient-parts", "2")), ("vesta_k8", "qp4", ("--quotient-parts", "4")),
         ("vesta_k8", "qp8", ("--quotient-parts", "8")), ("vesta_k8", "expr_never", ("--expr-kernel", "never")),
         ("vesta_k8", "expr_always", ("--expr-kernel", "always")), ("vesta_k8", "expr_limbs32", ("--expr-limbs", "32")),
         ("vesta_k8", "ntt_limbs32", ("--ntt-limbs", "32")), ("vesta_k8", "serial", ("--serial",)), ("vesta_k8", "ipa_fold", ("--ipa", "fold")),
         ("vesta_k8", "ipa_virtual", ("--ipa", "virtual")), ("vesta_k8", "collapse_2_5", ("--ipa-collapse-after", "2,5")),
         ("vesta_k8", "precomputed", ("--precomputed",)), ("vesta_k8", "window_bits4", ("--window-bits", "4")),
         ("vesta_k8", "window_bits13", ("--window-bits", "13")),
         ("pallas_k8", "default", ()), ("pallas_k8", "qp8", ("--quotient-parts", "8")),
         ("vesta_k12", "default", ()), ("vesta_k12", "qp8_expr_always", ("--quotient-parts", "8", "--expr-kernel", "always"))]


@pytest.mark.gpu
def test_work_list_outputs_match_the_reference_in_every_mode(tmp_path):
    """one bench run per mode, in sequence; every dumped array against the golden.  A run that fails ends the test there (no
    further GPU run); mismatches of every mode are reported together"""
    report, walls = {}, []
    for cfg, mode, flags in MODES:
        curve, k = W.CONFIGS[cfg]
        d = tmp_path / ("%s_%s" % (cfg, mode))
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, BENCH, "--logn", str(k), "--curve", curve, "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
                            "--dump-outputs", str(d), *flags], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        walls.append("%s %s: %.1f s" % (cfg, mode, time.perf_counter() - t0))
        assert r.returncode == 0, (cfg, mode, r.stderr[-2000:])
        problems = compare(load_dump(d), _golden(cfg))
        if problems:
            report["%s %s" % (cfg, mode)] = problems
    print("\n".join(walls))
    assert not report, json.dumps(report, indent=1)
