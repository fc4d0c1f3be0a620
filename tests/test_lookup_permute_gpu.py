"""GPU tier (-m gpu): zk_halo2_permute_expression_pair_device, the lookup argument's permute_expression_pair on a real
MI355X, against oracle.pyref_halo2.permute_expression_pair element by element, with the lookup product over the permuted
pair closing to 1.  2^20 - 6 usable rows (the bench's 5 blinding rows + 1) give 2^21 keys = 512 sort chunks: the offsets
scan runs past one workgroup's 256 chunks there."""
import numpy as np
import pytest

import lookup_permute_cases as lc
from oracle import pyref
from parity_suite import _monts, to_device, to_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zk():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    import contangle_zkcp_amd as zk
    zk._lib = None
    zk.load()
    zk.init(0)
    info = zk.backend_info()
    assert info.startswith("hip gfx950"), info
    yield zk
    zk.shutdown()


@pytest.mark.parametrize("dist", ["range_check", "random_dups"])
def test_permute_2_20(zk, dist):
    lc.check_dist(zk, "PallasFp", dist, (1 << 20) - 6)


@pytest.mark.parametrize("name", lc.FIELDS)
@pytest.mark.parametrize("dist", lc.DISTRIBUTIONS)
def test_permute_2_16_all_fields(zk, name, dist):
    lc.check_dist(zk, name, dist, 1 << 16, close=(dist in ("range_check", "random_dups")))


def test_permute_2_22_random(zk):
    lc.check_dist(zk, "PallasFp", "random_dups", (1 << 22) - 6, close=False)


def test_theta_compressed_two_column_lookup(zk):
    """a two-column lookup compressed on the device with the existing vector ops, A = a0 + theta a1, S = t0 + theta t1,
    then permuted and closed"""
    name, u = "Bn254Fr", (1 << 18) - 6
    p = pyref.FIELDS[name][0]
    rng = pyref.Rng(0x7E7A)
    pairs = [(rng.below(p), rng.below(1 << 10)) for _ in range(2000)]
    rows = pairs + [pairs[rng.below(len(pairs))] for _ in range(u - len(pairs))]
    picks = [pairs[rng.below(len(pairs))] for _ in range(u)]
    theta = rng.below(p)
    comp = lambda col: [(x + theta * y) % p for x, y in col]
    cols = [to_device(zk, _monts(name, [r[c] for r in src])) for src in (picks, rows) for c in (0, 1)]
    th = _monts(name, [theta])[0]
    for lo, hi in ((0, 1), (2, 3)):
        zk.vec_op(name, "scale", cols[hi], scalar=th)
        zk.vec_op(name, "add", cols[lo], cols[hi])
    A, S = cols[0], cols[2]
    inputs, table = comp(picks), comp(rows)
    assert (to_host(zk, A) == _monts(name, inputs)).all() and (to_host(zk, S) == _monts(name, table)).all()
    a_exp, s_exp = lc.h2.permute_expression_pair(name, inputs, table, u)
    in_host, tab_host = _monts(name, inputs), _monts(name, table)
    a_out, s_out = to_device(zk, lc._sentinel(u)), to_device(zk, lc._sentinel(u))
    zk.halo2.permute_expression_pair_device(name, A, S, u, a_out, s_out)
    lc.verify(zk, name, inputs, table, u, A, S, a_out, s_out, a_exp, s_exp, in_host, tab_host)


def test_two_streams_in_flight(zk):
    import torch
    cases = [("PallasFp", "random_dups", (1 << 19) - 6), ("Bls381Fr", "range_check", (1 << 19) - 6)]
    streams = [torch.cuda.Stream() for _ in cases]
    runs = []
    for (name, dist, u), s in zip(cases, streams):
        inputs, table = lc.make_case(name, dist, u, seed=11)
        in_host, tab_host = _monts(name, inputs), _monts(name, table)
        d_in, d_tab = to_device(zk, in_host), to_device(zk, tab_host)
        a_out, s_out = to_device(zk, lc._sentinel(u)), to_device(zk, lc._sentinel(u))
        torch.cuda.synchronize()
        runs.append((name, inputs, table, u, d_in, d_tab, a_out, s_out, in_host, tab_host))
    # each call synchronises its own stream at the end; run them from two host threads so both are in flight together
    import threading
    errs = []

    def go(r, s):
        try:
            zk.halo2.permute_expression_pair_device(r[0], r[4], r[5], r[3], r[6], r[7], stream=s.cuda_stream)
        except Exception as e:       # reported below
            errs.append(e)
    ths = [threading.Thread(target=go, args=(r, s)) for r, s in zip(runs, streams)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    for name, inputs, table, u, d_in, d_tab, a_out, s_out, in_host, tab_host in runs:
        a_exp, s_exp = lc.h2.permute_expression_pair(name, inputs, table, u)
        lc.verify(zk, name, inputs, table, u, d_in, d_tab, a_out, s_out, a_exp, s_exp, in_host, tab_host, close=False)


def test_input_not_in_table_2_20(zk):
    lc.check_missing(zk, "PallasFp", "between", (1 << 20) - 6, repeats=1000)
