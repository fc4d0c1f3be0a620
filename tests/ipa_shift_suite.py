"""The generator collapse over a handle's shift tables ([2^64] G_i, [2^128] G_i, [2^192] G_i: zk_bases_precompute_shifts), shared by
the emulator tier and the GPU tier like parity_suite.py.  The collapse returns canonical affine points, so every comparison is
bit-exact: tables built explicitly == no tables == the literal folds of IpaProver == the oracle's MSM."""
import ctypes

import numpy as np

import parity_suite as ps
from oracle import pyref
from oracle import zk_oracle as orc


def _sf(cname):
    return pyref.CURVES[cname][1]


def _collapse(zk, cname, bases, W, m0, cur, first=0, count=None):
    """zk_ipa_collapse_range_device over `bases` -> host array [count, 2 L]"""
    count = cur - first if count is None else count
    L = orc.coord_limbs(cname)
    out = ps.to_device(zk, np.zeros((count, 2 * L), dtype=np.uint64))
    st = zk.halo2._plib().zk_ipa_collapse_range_device(zk.curve_id(cname), bases.handle, zk._ptr(W), m0, cur, first, count, zk._ptr(out), ctypes.c_void_p(0))
    assert st == 0, (cname, m0, cur, first, count, st)
    return ps.to_host(zk, out).reshape(count, 2 * L).copy()


def _with_tables(zk, cname, pts):
    b = zk.Bases(cname, pts)
    assert not b.has_shift_tables()
    b.precompute_shifts()
    assert b.has_shift_tables()
    return b


def _folded(zk, cname, gens, us):
    """the generators after 0, 1, ... len(us) literal folds (IpaProver) and the weight vector W after as many fold-free rounds"""
    sf = _sf(cname)
    n = gens.shape[0]
    ipa = zk.halo2.IpaProver(cname, ps.to_device(zk, ps.rand_field(sf, n, 1)), ps.to_device(zk, ps.rand_field(sf, n, 2)), ps.to_device(zk, gens.copy()))
    g_after = {0: gens.copy()}
    for j, u in enumerate(us):
        ipa.fold(ps._monts(sf, [u])[0])
        g_after[j + 1] = ps.to_host(zk, ipa.g)[:n >> (j + 1)].copy()
    ipa.free()
    return g_after


def _weights(zk, cname, n, us, rounds):
    """W after `rounds` fold-free rounds with the challenges us (device buffer [n, 4]); the prover object keeps it alive"""
    sf = _sf(cname)
    new_buffer = lambda shape: ps.to_device(zk, np.zeros(shape, dtype=np.uint64))
    dummy = zk.Bases(cname, np.zeros((n, 2 * orc.coord_limbs(cname)), dtype=np.uint64))
    v = zk.halo2.IpaProverVirtual(cname, ps.to_device(zk, ps.rand_field(sf, n, 1)), ps.to_device(zk, ps.rand_field(sf, n, 2)), dummy, new_buffer)
    for j in range(rounds):
        v.fold(ps._monts(sf, [us[j]])[0])
    dummy.free()
    return v


def check_three_way(zk, cname, k, seed=41):
    """collapses after 1, 3, 6 and all k rounds: tables built explicitly == tables off == the literal folds; with tables on, the
    shares of the range entry tile the output"""
    r = pyref.FIELDS[_sf(cname)][0]
    n = 1 << k
    rng = pyref.Rng(seed)
    gens = ps.bases_for(cname, n, seed=35)
    us = [1 + rng.below(r - 1) for _ in range(k)]
    g_after = _folded(zk, cname, gens, us)
    off, on = zk.Bases(cname, gens), _with_tables(zk, cname, gens)
    for rounds in sorted({1, 3, 6, k}):
        v = _weights(zk, cname, n, us, rounds)
        cur = n >> rounds
        g_off = _collapse(zk, cname, off, v.W, n, cur)
        g_on = _collapse(zk, cname, on, v.W, n, cur)
        assert (g_off == g_after[rounds]).all(), (cname, k, rounds, "tables off vs literal folds")
        assert (g_on == g_after[rounds]).all(), (cname, k, rounds, "tables on vs literal folds")
        a = max(1, cur // 3)
        parts = [_collapse(zk, cname, on, v.W, n, cur, first, count) for first, count in ((0, a), (a, cur - a)) if count]
        assert (np.concatenate(parts) == g_after[rounds]).all(), (cname, k, rounds, "ranges with tables")
        v.free()
    assert on.has_shift_tables() and not off.has_shift_tables()      # a small handle never builds tables by itself
    off.free()
    on.free()


def crafted_weights(cname):
    """the chunk edges: 0, 1, r - 1, 2^64 - 1, 2^64, 2^128 - 1, 2^192, and the largest value below the modulus whose low three
    chunks are all 2^64 - 1 (a carry across every chunk boundary into the narrow top window), then eight seeded ones"""
    r = pyref.FIELDS[_sf(cname)][0]
    top = (((r >> 192) - 1) << 192) | ((1 << 192) - 1)
    assert top < r and all((top >> (64 * j)) & ((1 << 64) - 1) == (1 << 64) - 1 for j in range(3))
    rng = pyref.Rng(77)
    return [0, 1, r - 1, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 192, top] + [rng.below(r) for _ in range(8)]


def check_crafted_weights(zk, cname, seed=43):
    """T = 16 weights written straight into W (only W[t cur] is read), 16 survivors, each against the oracle's MSM over its 16
    original points; survivor 3 has only identity points, survivor 5 has identities under the weights 2^64 and 2^192 (an identity
    stays an identity in every table)"""
    sf = _sf(cname)
    T = cur = 16
    m0 = T * cur
    L = orc.coord_limbs(cname)
    gens = ps.bases_for(cname, m0, seed=37).copy()
    wt = crafted_weights(cname)
    gens[3::cur] = 0
    gens[4 * cur + 5] = 0
    gens[6 * cur + 5] = 0
    W = np.zeros((m0, 4), dtype=np.uint64)          # everything the collapse must not read stays zero
    W[::cur] = ps._monts(sf, wt)
    d_W = ps.to_device(zk, W)
    wsc = orc.ints_to_array(wt, 4)
    exp = np.zeros((cur, 2 * L), dtype=np.uint64)
    for i in range(cur):
        keep = [t for t in range(T) if gens[t * cur + i].any()]
        if keep:
            exp[i] = orc.msm_ark(cname, np.ascontiguousarray(gens[i::cur][keep]), np.ascontiguousarray(wsc[keep]), threads=4)
    assert not exp[3].any()
    off, on = zk.Bases(cname, gens), _with_tables(zk, cname, gens)
    assert (_collapse(zk, cname, off, d_W, m0, cur) == exp).all(), (cname, "crafted weights, tables off")
    assert (_collapse(zk, cname, on, d_W, m0, cur) == exp).all(), (cname, "crafted weights, tables on")
    off.free()
    on.free()


def check_wider_handle(zk, cname, k, seed=47):
    """a handle with twice as many points as the argument's m0: the tables' rows are the HANDLE's length apart"""
    r = pyref.FIELDS[_sf(cname)][0]
    m0 = 1 << k
    rng = pyref.Rng(seed)
    gens = ps.bases_for(cname, 2 * m0, seed=39)
    us = [1 + rng.below(r - 1) for _ in range(3)]
    v = _weights(zk, cname, m0, us, 3)
    narrow, wide = zk.Bases(cname, gens[:m0]), _with_tables(zk, cname, gens)
    cur = m0 >> 3
    exp = _collapse(zk, cname, narrow, v.W, m0, cur)
    assert (_collapse(zk, cname, wide, v.W, m0, cur) == exp).all(), (cname, k, "wider handle")
    Wt = [1]
    for u in us:                                   # W_t = the product of the challenges t's bits select, first challenge = top bit
        Wt = [x for w in Wt for x in (w, w * u % r)]
    i = cur - 1
    assert (exp[i] == orc.msm_ark(cname, np.ascontiguousarray(gens[i:m0:cur]), orc.ints_to_array(Wt, 4), threads=4)).all(), (cname, k, "oracle")
    v.free()
    narrow.free()
    wide.free()


def check_refresh(zk, cname, k, seed=53):
    """adopt a device buffer, build tables, collapse; rewrite a few points in place and refresh: the tables are gone, the result is
    the table-free result over the new points, and so is the result over tables built again"""
    r = pyref.FIELDS[_sf(cname)][0]
    n = 1 << k
    rng = pyref.Rng(seed)
    gens = ps.bases_for(cname, n, seed=35)
    other = ps.bases_for(cname, 8, seed=51)
    us = [1 + rng.below(r - 1) for _ in range(3)]
    v = _weights(zk, cname, n, us, 3)
    cur = n >> 3
    d = ps.to_device(zk, gens.copy())
    adopted = zk.Bases(cname, device_tensor=d, n=n)
    adopted.precompute_shifts()
    assert adopted.has_shift_tables()
    plain = zk.Bases(cname, gens)
    assert (_collapse(zk, cname, adopted, v.W, n, cur) == _collapse(zk, cname, plain, v.W, n, cur)).all(), (cname, "before the refresh")
    plain.free()
    idx = [0, 1, cur, n // 2 + 3, n - 2, n - 1]
    new = gens.copy()
    new[idx] = other[:len(idx)]
    if isinstance(d, np.ndarray):
        d[idx] = other[:len(idx)]
    else:
        import torch
        d[torch.tensor(idx, device=d.device)] = torch.from_numpy(other[:len(idx)].view(np.int64)).to(d.device)
        torch.cuda.synchronize()
    adopted.refresh(0, n)
    assert not adopted.has_shift_tables()
    plain = zk.Bases(cname, new)
    exp = _collapse(zk, cname, plain, v.W, n, cur)
    assert (_collapse(zk, cname, adopted, v.W, n, cur) == exp).all(), (cname, "after the refresh, no tables")
    adopted.precompute_shifts()
    assert adopted.has_shift_tables()
    assert (_collapse(zk, cname, adopted, v.W, n, cur) == exp).all(), (cname, "after the refresh, tables built again")
    v.free()
    plain.free()
    adopted.free()


def check_automatic(zk, cname, k=16, small_k=10, rounds=6, seed=59):
    """GPU tier.  The first collapse over a 2^16-point handle leaves no tables, the second builds them, both give the same points; a
    2^10-point handle never builds any"""
    r = pyref.FIELDS[_sf(cname)][0]
    L = orc.coord_limbs(cname)
    rng = pyref.Rng(seed)
    us = [1 + rng.below(r - 1) for _ in range(rounds)]
    for kk, builds in ((k, True), (small_k, False)):
        n = 1 << kk
        d_pts = ps.to_device(zk, np.zeros((n, 2 * L), dtype=np.uint64))
        zk.fixed_base_msm_device(cname, ps.to_device(zk, ps.scalars_for(cname, n, seed)), d_pts, n)
        ps.to_host(zk, d_pts)
        srs = zk.Bases(cname, device_tensor=d_pts, n=n)
        v = _weights(zk, cname, n, us, rounds)
        cur = n >> rounds
        first = _collapse(zk, cname, srs, v.W, n, cur)
        assert not srs.has_shift_tables(), (cname, kk, "the first collapse must not build tables")
        second = _collapse(zk, cname, srs, v.W, n, cur)
        assert srs.has_shift_tables() == builds, (cname, kk, "tables after the second collapse")
        third = _collapse(zk, cname, srs, v.W, n, cur)
        assert srs.has_shift_tables() == builds
        assert (first == second).all() and (first == third).all(), (cname, kk, "tables on vs off")
        v.free()
        srs.free()
