"""GPU: the tables of tests/field_cases.py through the device probe (tests/emu/libzk_field_probe.so: the op table of
tests/emu/field_ops.h compiled for gfx950 with the product's flags), one case per lane, in three lane modes.  Every result
is checked against Python integers and then, limb for limb, against the host runner's output for the same line; rows of
inactive lanes must come back untouched.  The probe is self-contained (no zk.init()); a missing library is a failure.
One process: after a failing HIP call nothing more is launched."""
import ctypes
import os

import numpy as np
import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu

LIB = os.path.join(fc.EMU, "libzk_field_probe.so")
BLOCK = 64
SENTINEL = 0xA5A5A5A5
MODES = {"all_lanes": 0, "odd_lanes": 1, "one_lane_per_workgroup": 2}
_state = {"lib": None, "hip_error": None, "host": {}}

FIELD_FAMILIES = ["lazy_extremes", "lazy_conversion", "lazy_kp", "sat_edge", "sat_uniform"] + ["slots4_" + "".join(map(str, o)) for o in fc.SLOT_ORDERS]
PARAMS = [(f, fam) for f in fc.FIELDS for fam in FIELD_FAMILIES] + \
         [(f, fam) for f in fc.FQ2_FIELDS for fam in ("lazy_fq2", "sat_fe2")] + \
         [("Bn254Fq", "canon_r03a")] + [(t, "curve") for t in fc.CURVE_TARGETS]


def probe():
    if _state["lib"] is None:
        assert os.path.exists(LIB), "the device probe is not built: build() / contangle-zkcp_amd/build.py probe"
        lib = ctypes.CDLL(LIB)
        lib.zk_probe_run.restype = ctypes.c_int
        lib.zk_probe_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        lib.zk_probe_shape.restype = ctypes.c_int
        lib.zk_probe_shape.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 3
        _state["lib"] = lib
    return _state["lib"]


def active_rows(n, mode):
    i = np.arange(n, dtype=np.int64)
    if mode == 0:
        return n, i
    if mode == 1:
        return 2 * n, 2 * i + 1
    return BLOCK * n, BLOCK * i + (5 * i + 1) % BLOCK


def run_device(target, op, cases, mode):
    """one launch: the cases of one op on the active lanes of `mode`; returns the result words per case"""
    assert _state["hip_error"] is None, "an earlier HIP call failed (%s): nothing more is launched in this process" % (_state["hip_error"],)
    lib = probe()
    tid, oid, na, nb, no = fc.op_table()[(target, op)]
    sa, sb, so = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.zk_probe_shape(tid, oid, sa, sb, so) == 0 and (sa.value, sb.value, so.value) == (na, nb, no), "host and device op tables differ"
    n = len(cases)
    nl, rows = active_rows(n, mode)
    a = np.zeros((nl, na), dtype=np.uint32)
    b = np.zeros((nl, nb), dtype=np.uint32)
    a[:] = np.array(cases[0][2], dtype=np.uint32)          # inactive lanes hold valid operands, and must not run
    b[:] = np.array(cases[0][3], dtype=np.uint32)
    a[rows] = np.array([c[2] for c in cases], dtype=np.uint32)
    b[rows] = np.array([c[3] for c in cases], dtype=np.uint32)
    out = np.full((nl, no), SENTINEL, dtype=np.uint32)
    rc = lib.zk_probe_run(tid, oid, a.ctypes.data, b.ctypes.data, out.ctypes.data, nl, mode)
    if rc != 0:
        _state["hip_error"] = (target, op, rc)
    assert rc == 0, "zk_probe_run(%s, %s) returned %d" % (target, op, rc)
    idle = np.ones(nl, dtype=bool)
    idle[rows] = False
    assert (out[idle] == SENTINEL).all(), "%s %s: an inactive lane wrote its output row" % (target, op)
    return out[rows].tolist()


def host_results(target, family):
    key = (target, family)
    if key not in _state["host"]:
        _state["host"][key] = fc.run(fc.tables(target)[family])
    return _state["host"][key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("target,family", PARAMS)
def test_probe(target, family, mode):
    cases = fc.tables(target)[family]
    host = host_results(target, family)
    ops = sorted({c[1] for c in cases})
    for op in ops:
        idx = [i for i, c in enumerate(cases) if c[1] == op]
        sub = [cases[i] for i in idx]
        dev = run_device(target, op, sub, MODES[mode])
        fc.check(sub, dev)                                                   # against Python integers
        for i, r in zip(idx, dev):                                           # and the host runner, limb for limb
            assert r == host[i], "%s %s case %d (%s): device %s host %s" % (target, op, i, mode, list(map(hex, r)), list(map(hex, host[i])))


def test_probe_op_table_matches_host():
    """every (target, op) of the host runner's table has the same shape in the probe; an undeclared op is refused"""
    lib = probe()
    sa, sb, so = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for (target, op), (tid, oid, na, nb, no) in fc.op_table().items():
        assert lib.zk_probe_shape(tid, oid, sa, sb, so) == 0 and (sa.value, sb.value, so.value) == (na, nb, no), (target, op)
    assert lib.zk_probe_shape(0, 10 ** 6, sa, sb, so) == -2 and lib.zk_probe_shape(99, 0, sa, sb, so) == -1
