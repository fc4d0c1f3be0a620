"""CPU tier: the buffer-overlap refusals of the entry points whose overlap tests go through the one spans_overlap helper and had no
case of their own -- zk_ntt_oop_device, zk_kate_division_device, zk_vec_fold_many_device, zk_halo2_permutation_sigmas_device and
zk_halo2_mock_eval / _lookup / _permutation_device -- at the smallest size, 4 elements: buffers that share one element (one byte,
where the pointer need not be aligned) are refused, adjacent ones and, where the entry point allows it, equal ones are accepted
and give what disjoint buffers give.  The buffers are carved out of one numpy allocation, which is 'device memory' only in the
emulator build (tests/emu), so there is no GPU twin of this file."""
import ctypes
import importlib.util
import os
import random

import numpy as np
import pytest

import halo2_keygen_cases as kc
import halo2_mock_cases as mc
import parity_suite as ps
from oracle import pyref
from oracle import zk_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zk():
    spec = importlib.util.spec_from_file_location("zk_build", os.path.join(ROOT, "contangle-zkcp_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    emu = b.build_emu()
    import contangle_zkcp_amd as zk
    zk.load(path=emu)
    zk.init(0)
    assert zk.backend_info().startswith("emu")
    yield zk
    zk.shutdown()
    zk._lib = None


def check_field_overlap_refusals(zk, name, seed=89):
    """The buffer-overlap refusals of zk_ntt_oop_device, zk_kate_division_device and zk_vec_fold_many_device at 4 elements: buffers
    that share one element are refused (ZK_ERR_INVALID_ARG, before anything is launched), adjacent ones and -- where the entry
    point allows it -- the same buffer twice are accepted and give what disjoint buffers give.  CPU tier: the buffers are carved
    out of one numpy allocation, which is 'device memory' only under the emulator."""
    assert zk.backend_info().startswith("emu")
    lib, fid, E, n = zk.halo2._plib(), zk.field_id(name), 32, 4
    p = pyref.FIELDS[name][0]
    rng = pyref.Rng(seed)
    buf = np.zeros((24, 4), dtype=np.uint64)
    base = buf.ctypes.data
    assert base % 16 == 0
    at = lambda elem: ctypes.c_void_p(base + E * elem)
    vals = lambda: ps._monts(name, [rng.below(p) for _ in range(n)])
    x = ps._monts(name, [rng.below(p)])[0]
    xp = ctypes.c_void_p(x.ctypes.data)

    # zk_kate_division_device(a, q): in place or disjoint
    a = vals()
    exp = ps.to_host(zk, zk.halo2.kate_division(name, a.copy(), x))
    kate = lambda ea, eq: lib.zk_kate_division_device(fid, at(ea), at(eq), n, xp, None)
    for ea, eq, want in ((8, 11, -1), (8, 5, -1), (8, 9, -1), (8, 12, 0), (8, 4, 0), (8, 8, 0)):
        buf[:] = 0
        buf[ea:ea + n] = a
        assert kate(ea, eq) == want, ("kate_division", ea, eq)
        assert (buf[eq:eq + n] == exp).all() if want == 0 else (buf[ea:ea + n] == a).all() and not np.delete(buf, range(ea, ea + n), 0).any()

    # zk_vec_fold_many_device(out, first, stride, count = 2): out is one of the sources or disjoint from both
    s0, s1 = vals(), vals()
    for stride, e0, e1 in ((n, 8, 12), (-n, 12, 8)):           # source i at element e_i; the pair covers elements [8, 16)
        srcs = np.stack([s0, s1])
        exp = ps.to_host(zk, zk.halo2.vec_fold_many(name, np.zeros((n, 4), dtype=np.uint64), srcs, x))
        for eo, want in ((5, -1), (15, -1), (9, -1), (13, -1), (4, 0), (16, 0), (8, 0), (12, 0)):
            buf[:] = 0
            buf[e0:e0 + n], buf[e1:e1 + n] = s0, s1
            assert lib.zk_vec_fold_many_device(fid, at(eo), at(e0), stride, 2, n, xp, None) == want, ("vec_fold_many", stride, eo)
            if want == 0:
                assert (buf[eo:eo + n] == exp).all(), ("vec_fold_many", stride, eo)

    # zk_ntt_oop_device(src, dst): 2^log_in elements in, 2^log_n out; the same buffer (in place) or disjoint
    w = orc.root_of_unity(name, 2)
    wp = ctypes.c_void_p(w.ctypes.data)
    a = vals()
    for log_in in (2, 1):
        n_in = 1 << log_in
        padded = np.zeros((n, 4), dtype=np.uint64)
        padded[:n_in] = a[:n_in]
        exp = orc.halo2_best_fft(name, padded, w, 2, threads=1)
        oop = lambda es, ed: zk.load().zk_ntt_oop_device(fid, at(es), at(ed), 2, log_in, wp, 0, None, None, None)
        cases = ((8, 8 + n_in - 1, -1), (8, 8 - n + 1, -1), (8, 8 + n_in, 0), (8, 8 - n, 0), (8, 8, 0))
        for es, ed, want in cases:
            buf[:] = 0
            buf[es:es + n_in] = a[:n_in]
            assert oop(es, ed) == want, ("ntt_oop", log_in, es, ed)
            if want == 0:
                assert (buf[ed:ed + n] == exp).all(), ("ntt_oop", log_in, es, ed)


def check_mock_overlap_refusals(zk, field):
    """The output-over-input refusals of zk_halo2_mock_eval_device, _lookup_device and _permutation_device at 4 rows: an output that
    shares one element (one byte, where the pointer need not be aligned) with an input or with the other output is refused
    (ZK_ERR_INVALID_ARG, nothing written), an adjacent one is accepted and holds what disjoint buffers give.  CPU tier: the buffers
    are carved out of one numpy allocation, which is 'device memory' only under the emulator."""
    assert mc.on_emulator(zk)
    k, n = 2, 4
    p, lib, fid = mc.modulus(field), mc.plib(zk), mc.FIELD_IDS[field]
    rnd = random.Random(17)
    buf = np.zeros(512, dtype=np.uint8)
    base = buf.ctypes.data
    assert base % 16 == 0
    at = lambda off: ctypes.c_void_p(base + off)

    def put(off, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf[off:off + raw.size] = raw

    col = [rnd.randrange(p) for _ in range(n)]
    d_col = mc.dev(zk, mc.limbs_of(col))
    table = (ctypes.c_void_p * 1)(mc.ptr(d_col).value)
    pf = np.array([n], dtype=np.uint64)

    # eval: 32 bytes per entry in values_out [256, 384), 1 in status_out (both 16-byte aligned)
    prog = [("col", 0, 0), ("scale", 0)]
    exp_st, exp_val = mc.call_eval(zk, field, k, [prog], [col], [n], [7])
    ops, offs, cs = zk.halo2._expr_ops(prog), np.array([0, len(prog)], dtype=np.uint32), mc.mont(field, [7])
    for s_off, want in ((256, mc.INVALID_ARG), (368, mc.INVALID_ARG), (384, 0), (240, 0)):
        buf[:] = 0xEE
        st = lib.zk_halo2_mock_eval_device(fid, k, ops, mc.ptr(offs), 1, table, mc.ptr(pf), 1, mc.ptr(cs), 1, at(256), at(s_off), None)
        assert st == want, ("eval", s_off, st)
        if want == 0:
            assert (buf[s_off:s_off + n] == exp_st[0]).all() and (buf[256:384].view(np.uint64).reshape(n, 4) == exp_val[0]).all(), ("eval", s_off)
        else:
            assert (buf == 0xEE).all(), ("eval", s_off)

    # lookup: inputs [256, 384), their status bytes [64, 68), the table elsewhere; status_out needs no alignment
    inputs, in_st = [col[0], 5, col[2], col[3]], [mc.ZERO, mc.NONZERO, mc.NONZERO, mc.POISON]
    exp = mc.call_lookup(zk, field, k, inputs, in_st, col, None, n)
    d_tab = mc.dev(zk, mc.mont(field, col))
    for o_off, want in ((383, mc.INVALID_ARG), (253, mc.INVALID_ARG), (384, 0), (252, 0), (67, mc.INVALID_ARG), (61, mc.INVALID_ARG), (68, 0), (60, 0)):
        buf[:] = 0xEE
        put(256, mc.mont(field, inputs))
        put(64, np.array(in_st, dtype=np.uint8))
        before = buf.copy()
        st = lib.zk_halo2_mock_lookup_device(fid, k, at(256), at(64), mc.ptr(d_tab), None, n, at(o_off), None)
        assert st == want, ("lookup", o_off, st)
        if want == 0:
            assert (buf[o_off:o_off + n] == exp).all(), ("lookup", o_off)
        else:
            assert (buf == before).all(), ("lookup", o_off)

    # permutation: 8 bytes per cell in the mapping [256, 288), 1 in status_out (no alignment)
    mapping = np.array([[1, 0, 2, 3]], dtype=np.uint64)          # column 0: rows 0 and 1 exchanged, their values differ
    exp = mc.call_permutation(zk, field, k, [col], [n], mapping)
    for o_off, want in ((287, mc.INVALID_ARG), (253, mc.INVALID_ARG), (288, 0), (252, 0)):
        buf[:] = 0xEE
        put(256, mapping)
        before = buf.copy()
        st = lib.zk_halo2_mock_permutation_device(fid, k, 1, table, mc.ptr(pf), at(256), at(o_off), None)
        assert st == want, ("permutation", o_off, st)
        if want == 0:
            assert (buf[o_off:o_off + n] == exp[0]).all(), ("permutation", o_off)
        else:
            assert (buf == before).all(), ("permutation", o_off)


# ---------------------------------------------------------------- permutation
PERM_SHAPES = [(1, 1), (3, 16), (6, 1), (6, 17), (7, 3), (13, 5)]


def check_sigmas_overlap(zk, field="PallasFp"):
    """zk_halo2_permutation_sigmas_device at 4 cells (k = 2, one column): the mapping is 8 bytes a cell, the output 32, both 16-byte
    aligned.  An output that covers the mapping's last (or first) 16 bytes is refused and writes nothing; one that ends where the
    mapping begins, or begins where it ends, is accepted and right.  CPU tier: the buffers are carved out of one numpy allocation,
    which is 'device memory' only under the emulator."""
    assert zk.backend_info().startswith("emu")
    k, n = 2, 4
    lib, fid = zk.halo2._plib(), zk.field_id(field)
    mapping = np.array([[2, 1, 0, 3]], dtype=np.uint64)          # rows 0 and 2 exchanged
    exp = kc.sigma_expected(field, k, mapping)[0]
    dl = zk.halo2.delta(field)
    buf = np.zeros(64, dtype=np.uint64)                          # the mapping in words [32, 36) = bytes [256, 288)
    base = buf.ctypes.data
    assert base % 16 == 0
    for o_off, want in ((272, -1), (144, -1), (288, 0), (128, 0)):
        buf[:] = 0xA5
        buf[32:36] = mapping[0]
        before = buf.copy()
        st = lib.zk_halo2_permutation_sigmas_device(fid, k, 1, ctypes.c_void_p(base + 256), ctypes.c_void_p(dl.ctypes.data), ctypes.c_void_p(base + o_off), None)
        assert st == want, (o_off, st)
        if want == 0:
            assert (buf[o_off // 8:o_off // 8 + 4 * n].reshape(n, 4) == exp).all(), o_off
        else:
            assert (buf == before).all(), o_off


def test_field_overlap_refusals(zk):
    check_field_overlap_refusals(zk, "PallasFp")


def test_mock_overlap_refusals(zk):
    check_mock_overlap_refusals(zk, "PallasFp")


def test_sigmas_overlap(zk):
    check_sigmas_overlap(zk)
