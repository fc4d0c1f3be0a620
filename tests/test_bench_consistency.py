"""GPU: the bench's work-list at 2^12 rows produces the same proof elements (the `digest` of the quotient's piece commitments and of the
evaluations at x) whatever the order of work: upstream's quotient order / 8 sub-cosets, interpreter / compiled evaluator, one stream.
--dump-outputs writes those proof elements, the same from run to run."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--logn", "12", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", *flags],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "constraints/sec" and line["config"]["rows_per_step"] == 1 << 12
    return line["digest"]


@pytest.mark.gpu
def test_work_list_digest_is_independent_of_the_order_of_work():
    base = _run()
    assert len(base["h_commitments"]) == 16 and len(base["evals_at_x"]) == 16
    for flags in (("--quotient-parts", "8"), ("--quotient-parts", "2"), ("--expr-kernel", "never"), ("--expr-kernel", "always"), ("--serial",),
                  ("--expr-limbs", "32"), ("--ipa", "virtual")):
        assert _run(*flags) == base, flags


def _limbs(path):
    """a dumped array back to its uint64 limbs (bench.py dump_outputs: four 16-bit pieces per limb, least significant first)"""
    a = np.load(path)
    assert a.dtype == np.float32 and (a == np.floor(a)).all() and a.min() >= 0 and a.max() < 1 << 16
    return np.ascontiguousarray(a.astype(np.uint16)).view(np.uint64)


@pytest.mark.gpu
def test_dumped_outputs_are_the_proof_elements_and_repeat(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    digest = _run("--dump-outputs", str(a))
    assert _run("--steps", "2", "--dump-outputs", str(b)) == digest       # (the later --steps wins: two timed steps, the same inputs)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "h_commitments.npy" in names and "ipa_L.npy" in names
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    for n in names:
        assert (np.load(a / n) == np.load(b / n)).all(), n
    h = _limbs(a / "h_commitments.npy")
    assert h.shape == (8, 8) and hashlib.sha256(h.tobytes()).hexdigest()[:16] == digest["h_commitments"]
    assert hashlib.sha256(_limbs(a / "evals_at_x.npy").tobytes()).hexdigest()[:16] == digest["evals_at_x"]
    assert _limbs(a / "ipa_L.npy").shape == (12, 8) and _limbs(a / "ipa_a.npy").shape == (1, 4)
