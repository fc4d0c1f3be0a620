"""Cases of the lookup argument's permute_expression_pair on the device (zk_halo2_permute_expression_pair_device), shared by
tests/test_lookup_permute_emu.py (CPU tier, the emulator build) and tests/test_lookup_permute_gpu.py (-m gpu).  Every check
compares A' and S' element by element with oracle.pyref_halo2.permute_expression_pair."""
import numpy as np

from oracle import pyref
from oracle import pyref_halo2 as h2
from parity_suite import _monts, to_device, to_host

FIELDS = ["PallasFp", "PallasFq", "Bn254Fr", "Bls381Fr"]
DISTRIBUTIONS = ["range_check", "random_dups", "all_equal", "no_repeats", "extremes", "top_limb", "low_byte"]
SENTINEL = 0xA5A5_5A5A_DEAD_BEEF


def make_case(name, dist, u, seed=1):
    """(inputs, table) as Python integers, u of each, for a lookup that holds (every input value is in the table)"""
    p = pyref.FIELDS[name][0]
    rng = pyref.Rng(seed * 1000003 + u)
    pick = lambda vals: [vals[rng.below(len(vals))] for _ in range(u)]
    if dist == "range_check":
        # the reference's 10-bit range check: table 0..1023 then zeros (padding), ~70 % of the inputs 0
        m = min(1024, u)
        table = list(range(m)) + [0] * (u - m)
        inputs = [0 if rng.below(10) < 7 else rng.below(m) for _ in range(u)]
    elif dist == "random_dups":
        # theta-compressed values: a few hundred (or thousand) distinct full-width values, repeated
        vals = [rng.below(p) for _ in range(max(1, min(u // 3, 300 if u < 100000 else 3000)))]
        table = vals + pick(vals)[: u - len(vals)]
        inputs = pick(vals)
    elif dist == "all_equal":
        v = rng.below(p)
        table = [rng.below(p) for _ in range(u - 1)] + [v]
        inputs = [v] * u
    elif dist == "no_repeats":
        table = [rng.below(p) for _ in range(u)]
        inputs = list(table)
        for i in range(u - 1, 0, -1):
            j = rng.below(i + 1)
            inputs[i], inputs[j] = inputs[j], inputs[i]
    elif dist == "extremes":
        vals = [p - 1, 0] if u >= 2 else [p - 1]
        table = vals + pick(vals + [1, p - 2])[: u - len(vals)]
        inputs = pick(vals)
    elif dist == "top_limb":
        # values that differ only in bits 192.. : the low six 8-bit digits of every key are dead (and skipped)
        vals = [(rng.below(1 << 60) + 1) << 192 for _ in range(min(u, 40))]
        table = vals + pick(vals)[: u - len(vals)]
        inputs = pick(vals)
    elif dist == "low_byte":
        # values that differ only in their lowest byte: every digit above the second is dead
        base = rng.below(p >> 8) << 8
        vals = [base + j for j in range(min(u, 256))]
        table = vals + pick(vals)[: u - len(vals)]
        inputs = pick(vals)
    else:
        raise ValueError(dist)
    assert len(table) == u and len(inputs) == u
    return inputs, table


def _sentinel(n):
    return np.full((n, 4), SENTINEL, dtype=np.uint64)


def _first_diff(got, exp):
    bad = np.flatnonzero((got != exp).any(axis=1))
    return "%d rows differ, first at %d" % (len(bad), bad[0]) if len(bad) else "equal"


def run_and_check(zk, name, inputs, table, u, pad=3, host_mirror=False, close=True, stream=0, seed=7, check=True):
    """run the device call on columns of u + pad rows (the pad rows hold values outside the table: they must not be read),
    outputs pre-filled with a sentinel; check A', S' against the oracle, the pad rows of the outputs untouched, the inputs
    unchanged, optionally the host mirror, and that the lookup product over the permuted pair closes to 1"""
    p = pyref.FIELDS[name][0]
    rng = pyref.Rng(seed)
    a_exp, s_exp = h2.permute_expression_pair(name, inputs, table, u)
    in_table = set(table[:u])
    outside = [v for v in (rng.below(p) for _ in range(pad + 8)) if v not in in_table][:pad]
    in_host = _monts(name, list(inputs) + outside)
    tab_host = _monts(name, list(table) + outside)
    d_in, d_tab = to_device(zk, in_host), to_device(zk, tab_host)
    a_out, s_out = to_device(zk, _sentinel(u + pad)), to_device(zk, _sentinel(u + pad))
    zk.halo2.permute_expression_pair_device(name, d_in, d_tab, u, a_out, s_out, stream=stream)
    if not check:
        return d_in, d_tab, a_out, s_out, a_exp, s_exp
    verify(zk, name, inputs, table, u, d_in, d_tab, a_out, s_out, a_exp, s_exp, in_host, tab_host, host_mirror, close)


def verify(zk, name, inputs, table, u, d_in, d_tab, a_out, s_out, a_exp, s_exp, in_host, tab_host, host_mirror=False, close=True):
    p = pyref.FIELDS[name][0]
    ga, gs = to_host(zk, a_out), to_host(zk, s_out)
    ea, es = _monts(name, a_exp), _monts(name, s_exp)
    assert (ga[:u] == ea).all(), (name, u, "A'", _first_diff(ga[:u], ea))
    assert (gs[:u] == es).all(), (name, u, "S'", _first_diff(gs[:u], es))
    assert (ga[u:] == SENTINEL).all() and (gs[u:] == SENTINEL).all(), "rows from usable_rows on are the caller's"
    assert (to_host(zk, d_in) == in_host).all() and (to_host(zk, d_tab) == tab_host).all(), "the inputs are not modified"
    if host_mirror:
        ha, hs = zk.halo2.permute_expression_pair(name, in_host, tab_host, u)
        assert (ha == ea).all() and (hs == es).all(), (name, u, "host mirror")
    if close:
        rng = pyref.Rng(u)
        beta, gamma = rng.below(p), rng.below(p)
        z_out = to_device(zk, np.zeros((u, 4), dtype=np.uint64))
        cols = [to_device(zk, c) for c in (in_host[:u], tab_host[:u], ga[:u], gs[:u])]
        last = zk.halo2.lookup_product(name, *cols, _monts(name, [beta])[0], _monts(name, [gamma])[0], z_out)
        assert (last == _monts(name, [1])[0]).all(), (name, u, "the lookup product over the permuted pair closes to 1")


def check_dist(zk, name, dist, u, host_mirror=False, close=True, seed=1):
    inputs, table = make_case(name, dist, u, seed)
    run_and_check(zk, name, inputs, table, u, host_mirror=host_mirror, close=close)


def missing_case(name, where, u, repeats=1, seed=3):
    """a range-check-like lookup with one input value that is not in the table: below the table's minimum, above its
    maximum or in between; `repeats` inputs carry it"""
    rng = pyref.Rng(seed)
    lo = 1000
    table = [lo + 2 * rng.below(200) for _ in range(u)]          # even values in [1000, 1400)
    inputs = [table[rng.below(u)] for _ in range(u)]
    bad = {"below": 5, "above": 5000, "between": min(table) + 1}[where]
    for k in range(repeats):
        inputs[(k * 7919) % u] = bad
    return inputs, table


def check_missing(zk, name, where, u, repeats=1):
    """ZK_ERR_LOOKUP -> ValueError, and a correct call right afterwards succeeds"""
    inputs, table = missing_case(name, where, u, repeats)
    d_in, d_tab = to_device(zk, _monts(name, inputs)), to_device(zk, _monts(name, table))
    a_out, s_out = to_device(zk, np.zeros((u, 4), dtype=np.uint64)), to_device(zk, np.zeros((u, 4), dtype=np.uint64))
    try:
        zk.halo2.permute_expression_pair_device(name, d_in, d_tab, u, a_out, s_out)
        raise AssertionError("an input value outside the table must be refused (%s, %d repeats)" % (where, repeats))
    except ValueError:
        pass
    ok_inputs = [table[(i * 31) % u] for i in range(u)]
    run_and_check(zk, name, ok_inputs, table, u, close=False)
