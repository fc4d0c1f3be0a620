"""TEST INFRASTRUCTURE -- an independent restatement of bench.py's default work-list (the device side of one halo2_proofs 0.2
create_proof, phases 0-9 of bench_halo2's docstring) on Python integers, from the bench's seeded inputs to every proof element
`bench.py --dump-outputs` writes.  Written from that docstring and from upstream semantics, not from bench.py's step(): the two
agree only if the glue between the library calls (column order, rotation scales, point sets, Horner directions, the sub-coset
recombination, the IPA's p' and b) is right.

Commitments are computed in the exponent: the bench's SRS is P_i = [k_i] G with known k_i (synth.scalars_for), so every
commitment is [sum_i s_i k_i mod r] G -- one scalar multiplication, independent of every MSM implementation.  The IPA folds
the generators' logarithms as scalars, which is the same for every generator schedule (fold / virtual / collapse).

Imports: oracle/pyref*.py, the C oracle's best_fft, and contangle-zkcp_amd/synth.py (input generation only), loaded on its
own -- never the product package's __init__, halo2.py or bench.py.

`python -m oracle.pyref_halo2_worklist --write` regenerates tests/golden/halo2_worklist_*.json.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

try:
    from . import pyref, pyref_halo2
    from . import zk_oracle as orc
except ImportError:
    import pyref
    import pyref_halo2
    import zk_oracle as orc

_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_DIR)
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

# bench.py's circuit constants (the reference circuit's column layout), restated; tests compare them with bench.py via ast
N_INST, N_FIXED, N_PERM_COLS, PERM_CHUNK, N_H_PIECES = 3, 8, 16, 7, 8
NCOL = 13
GATE_DEGREE = 9                 # degree-9 gates: quotient_poly_degree 8, extended_k = k + 3
BLINDING_FACTORS = 5            # the "last" row is omega^-(BLINDING_FACTORS + 1)

SEEDS = {"instance": "0x1D0 + c", "advice": "0xC0DE + c", "lookup A, S, A', S'": "0xA0 .. 0xA3", "sigma (Lagrange)": "0x51 + c",
         "fixed (extended coset, natural order)": "0xF1 + c", "fixed / sigma / random coefficients": "0xAB00 + table row",
         "s (opening blinding polynomial)": "0xBB5", "beta, gamma, delta, y": "0xC1 .. 0xC4", "x, x1, x2, x3, x4, xi": "0xE0 .. 0xE5",
         "IPA u_j": "0xD0 + j", "SRS g_lagrange": "scalars_for(curve, n, 0x5EED)", "SRS g": "scalars_for(curve, n, 0x5EEE)"}

# Where the bench's work-list stands in for an upstream step (halo2_proofs 0.2).  The reference follows the bench here; `upstream`
# names the entries for which upstream_switch computes upstream's value instead (the arrays it changes are listed).
BENCH_SHORTCUTS = [
    {"name": "key_material_random", "bench": "bench.py:392-398, :425-427",
     "upstream": "plonk/keygen.rs keygen_pk (fixed_cosets, permutation pk: polys / cosets)",
     "what": "the fixed columns on the extended coset, the fixed / sigma coefficient forms and the sigma Lagrange values are "
             "independent seeded vectors, not transforms of one another"},
    {"name": "lagrange_srs_random", "bench": "bench.py:375", "upstream": "poly/commitment.rs Params::new (g_lagrange = the Lagrange form of g)",
     "what": "g_lagrange is an independent seeded SRS, not the inverse transform of g"},
    {"name": "lookup_permuted_random", "bench": "bench.py:391, :504",
     "upstream": "plonk/lookup/prover.rs permute_expression_pair",
     "what": "A' and S' are seeded vectors, not a permutation of A and S (Z_L does not close to 1)"},
    {"name": "challenges_fixed", "bench": "bench.py:399-401",
     "upstream": "transcript.rs squeeze_challenge_scalar (theta, beta, gamma, y, x, x_1..x_4, xi, z, u_j)",
     "what": "every challenge is a seeded field element; there is no transcript; delta is seeded, not the field's DELTA"},
    {"name": "no_blinding", "bench": "bench.py:344-346",
     "upstream": "plonk/prover.rs (blinding rows of advice / Z), vanishing/prover.rs, poly/commitment/prover.rs (s(x_3) = 0, L/R blinding)",
     "what": "no blinding rows or blinds: every row is a witness row, commitments carry no [r] W term, L_j / R_j carry no "
             "[value z] U + [r] W terms, and the opening's s is not shifted to vanish at x_3"},
    {"name": "p_prime_constant_term", "bench": "bench.py:640", "upstream": "poly/commitment/prover.rs create_proof: p_prime_poly[0] -= v",
     "what": "p'[0] -= v is not applied: the argument runs on p' = s xi + p itself"},
    {"name": "query_order", "bench": "bench.py:409-423", "upstream": "poly/multiopen.rs construct_intermediate_sets",
     "what": "the multiopen's point sets are taken in the order S0 = {x}, S1 = {x, wx}, S2 = {x, w^-1 x}, S3 = {x, wx, w^last x} and "
             "their polynomials in the table order below, not in the order of upstream's query list"},
    {"name": "gate_set_synthetic", "bench": "bench.py:441", "upstream": "plonk/vanishing / plonk/prover.rs (the circuit's gates, lookup and permutation expressions)",
     "what": "the quotient's numerator is synth.quotient_program (fixed columns stand in for the selectors and sigma cosets, "
             "the lookup's input and table expressions)"},
    {"name": "perm_chunk_link", "bench": "bench.py:518-519",
     "upstream": "plonk/permutation/prover.rs Argument::commit: last_z = z[n - (blinding_factors + 1)]",
     "what": "each permutation chunk's Z starts from the previous chunk's value after ALL n rows (the product over every row), "
             "where upstream starts it from the previous Z at the last usable row, omega^last = omega^-(blinding + 1) -- the "
             "row the S3 openings use",
     "upstream_switch": True,
     "changes": ["product_commitments", "h_commitments", "evals_at_x", "evals_at_omega_x", "evals_at_omega_last_x",
                 "q_commitment", "q_evals_at_x3", "v", "ipa_L", "ipa_R", "ipa_vl", "ipa_vr", "ipa_a"]},
]

OUTPUT_NAMES = ["instance_advice_commitments", "lookup_permuted_commitments", "product_commitments", "random_commitment", "h_commitments",
                "evals_at_x", "evals_at_omega_x", "evals_at_omega_inv_x", "evals_at_omega_last_x",
                "q_commitment", "q_evals_at_x3", "s_commitment", "v", "ipa_L", "ipa_R", "ipa_vl", "ipa_vr", "ipa_a"]
POINT_OUTPUTS = {"instance_advice_commitments", "lookup_permuted_commitments", "product_commitments", "random_commitment",
                 "h_commitments", "q_commitment", "s_commitment", "ipa_L", "ipa_R"}
SINGLE_OUTPUTS = {"random_commitment", "q_commitment", "s_commitment", "v"}       # written as one row (1-D) by the bench

CONFIGS = {"vesta_k8": ("Vesta", 8), "pallas_k8": ("Pallas", 8), "vesta_k12": ("Vesta", 12)}
SCALAR_FIELD = {"Vesta": "PallasFp", "Pallas": "PallasFq"}


def _load_synth():
    """contangle-zkcp_amd/synth.py on its own: its two imports from the package (FIELD_NAMES, field_modulus) are supplied from
    pyref, so neither the package's __init__ nor the HIP library is loaded"""
    name = "_worklist_inputs"
    if name + ".synth" in sys.modules:
        return sys.modules[name + ".synth"]
    pkg = types.ModuleType(name)
    pkg.__path__ = []
    pkg.FIELD_NAMES = {f: i for i, f in enumerate(pyref.FIELD_IDS[:4])}
    pkg.field_modulus = lambda f: pyref.FIELDS[f][0]
    sys.modules[name] = pkg
    spec = importlib.util.spec_from_file_location(name + ".synth", os.path.join(ROOT, "contangle-zkcp_amd", "synth.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name + ".synth"] = mod
    spec.loader.exec_module(mod)
    return mod


def source_sha256():
    return hashlib.sha256(open(os.path.abspath(__file__).replace(".pyc", ".py"), "rb").read()).hexdigest()


# ------------------------------------------------------------------ field helpers
def _words_to_int(row):
    return sum(int(w) << (64 * i) for i, w in enumerate(row))


def _int_to_words(v, nl=4):
    return ["%016x" % ((v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF) for i in range(nl)]


class Field:
    def __init__(self, name):
        self.name = name
        self.p, self.g, _ = pyref.FIELDS[name]
        self.Rinv = pow(1 << 256, -1, self.p)

    def stored(self, arr):
        """synth.rand_field words read as Montgomery residues (what the library and montgomery=True MSMs see) -> values"""
        return [_words_to_int(r) * self.Rinv % self.p for r in np.asarray(arr, dtype=np.uint64).tolist()]

    def mont_words(self, v):
        return _int_to_words(v % self.p * (1 << 256) % self.p)

    def fft(self, a, omega, logn):
        """upstream best_fft (the C oracle's restatement) on values: the Montgomery form is linear, so it commutes"""
        p = self.p
        arr = np.array([[(v * (1 << 256) % p >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in a], dtype=np.uint64)
        om = np.array([(omega * (1 << 256) % p >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        out = orc.halo2_best_fft(self.name, arr, om, logn, threads=os.cpu_count() or 4)
        return [v * self.Rinv % p for v in (_words_to_int(r) for r in out.tolist())]


def horner(p, poly, x):
    acc = 0
    for c in reversed(poly):
        acc = (acc * x + c) % p
    return acc


class Domain:
    """halo2_proofs 0.2 poly/domain.rs EvaluationDomain::new(j, k), restated"""

    def __init__(self, F, j, k):
        p = F.p
        self.F, self.k, self.n = F, k, 1 << k
        self.quotient_poly_degree = j - 1
        ek = k
        while (1 << ek) < self.n * self.quotient_poly_degree:
            ek += 1
        self.extended_k, self.ne = ek, 1 << ek
        self.omega = pyref.root_of_unity(F.name, k)
        self.omega_inv = pow(self.omega, -1, p)
        self.extended_omega = pyref.root_of_unity(F.name, ek)
        self.zeta = pow(F.g, (p - 1) // 3, p)                      # pasta FieldExt::ZETA = GENERATOR^((p - 1) / 3)
        self.zeta_inv = pow(self.zeta, -1, p)                      # = ZETA^2
        orig, step = pow(self.zeta, self.n, p), pow(self.extended_omega, self.n, p)
        self.t_evaluations, cur = [], orig
        while True:
            self.t_evaluations.append(cur)
            cur = cur * step % p
            if cur == orig:
                break
        assert len(self.t_evaluations) == 1 << (ek - k)
        self.t_evaluations = [pow((t - 1) % p, -1, p) for t in self.t_evaluations]

    def lagrange_to_coeff(self, a):
        ninv = pow(self.n, -1, self.F.p)
        return [v * ninv % self.F.p for v in self.F.fft(a, self.omega_inv, self.k)]

    def _distribute_powers_zeta(self, a, into_coset):
        pw = (self.zeta, self.zeta_inv) if into_coset else (self.zeta_inv, self.zeta)
        return [v if i % 3 == 0 else v * pw[i % 3 - 1] % self.F.p for i, v in enumerate(a)]

    def coeff_to_extended(self, a):
        a = self._distribute_powers_zeta(a, True) + [0] * (self.ne - self.n)
        return self.F.fft(a, self.extended_omega, self.extended_k)

    def extended_to_coeff(self, a):
        p = self.F.p
        neinv = pow(self.ne, -1, p)
        a = [v * neinv % p for v in self.F.fft(a, pow(self.extended_omega, -1, p), self.extended_k)]
        return self._distribute_powers_zeta(a, False)[:self.n * self.quotient_poly_degree]

    def divide_by_vanishing_poly(self, a):
        t = self.t_evaluations
        return [v * t[i % len(t)] % self.F.p for i, v in enumerate(a)]


# ------------------------------------------------------------------ the work-list
def coefficient_table():
    """the resident coefficient table of the openings, grouped by point set in the order S0 | S2 | S1 | S3 (bench_halo2 phase 7-8):
    the polynomial behind each row and the four sets as (first row, count, point names)"""
    synth = _load_synth()
    rot = synth.rotated_advice(NCOL)
    s0 = ([("inst", c) for c in range(N_INST)] + [("adv", c) for c in range(NCOL) if c not in rot] + [("fixed", c) for c in range(N_FIXED)]
          + [("random", 0), ("h", 0)] + [("sigma", c) for c in range(N_PERM_COLS)] + [("lk", "S'")])
    s2 = [("lk", "A'")]
    s1 = [("adv", c) for c in rot] + [("lk", "Z"), ("zp", 2)]
    s3 = [("zp", 0), ("zp", 1)]
    names = s0 + s2 + s1 + s3
    sets = [(0, len(s0), ("x",)), (len(s0) + len(s2), len(s1), ("x", "wx")), (len(s0), len(s2), ("x", "w^-1x")),
            (len(s0) + len(s2) + len(s1), len(s3), ("x", "wx", "w^last x"))]
    return names, sets


def _label(nm):
    return "%s%s" % nm


def generate(curve, k, upstream=()):
    """-> {name: [[64-bit word hex, ...] per row]}, {eval array: [polynomial label per row]}.  upstream: names of BENCH_SHORTCUTS
    entries with upstream_switch whose upstream value is computed instead of the bench's"""
    for u in upstream:
        assert any(s["name"] == u and s.get("upstream_switch") for s in BENCH_SHORTCUTS), u
    synth = _load_synth()
    sf = SCALAR_FIELD[curve]
    F = Field(sf)
    r = F.p
    bq = pyref.FIELDS[pyref.CURVES[curve][0]][0]
    G = pyref.CURVES[curve][3:5]
    n = 1 << k
    dom = Domain(F, GATE_DEGREE, k)
    ne, ek = dom.ne, dom.extended_k
    assert ek == k + 3
    rf = lambda seed, cnt=n: F.stored(synth.rand_field(sf, cnt, seed))
    one = lambda seed: rf(seed, 1)[0]

    # ---- SRS logarithms (canonical scalars: the fixed-base generation takes them as integers)
    srs_lag = [_words_to_int(row) for row in synth.scalars_for(curve, n, 0x5EED).tolist()]
    srs_g = [_words_to_int(row) for row in synth.scalars_for(curve, n, 0x5EEE).tolist()]

    def point(e):
        P = pyref.ec_mul(curve, e % r, G)
        assert P is not None, "a commitment is the identity: the dump has no encoding for it"
        return [w for c in P for w in _int_to_words(c * (1 << 256) % bq)]

    commit = lambda vals, logs: point(sum(v * g for v, g in zip(vals, logs)))

    # ---- inputs
    inst = [rf(0x1D0 + c) for c in range(N_INST)]
    adv = [rf(0xC0DE + c) for c in range(NCOL)]
    lk_a, lk_s, lk_ap, lk_sp = (rf(0xA0 + j) for j in range(4))
    sigma = [rf(0x51 + c) for c in range(N_PERM_COLS)]
    fixed_ext = [rf(0xF1 + c, ne) for c in range(N_FIXED)]
    beta, gamma, delta, y = (one(0xC1 + j) for j in range(4))
    x, x1, x2, x3, x4, xi = (one(0xE0 + j) for j in range(6))
    us = [one(0xD0 + j) for j in range(k)]
    names, sets = coefficient_table()
    row = {nm: i for i, nm in enumerate(names)}
    coef = {nm: rf(0xAB00 + row[nm]) for nm in names if nm[0] in ("fixed", "sigma", "random")}
    s_poly = rf(0xBB5)
    out = {}

    # ---- 0, 1: instance and advice commitments (Lagrange basis), coefficient forms and extended cosets
    out["instance_advice_commitments"] = [commit(v, srs_lag) for v in inst + adv]
    lag = {("inst", c): inst[c] for c in range(N_INST)}
    lag.update({("adv", c): adv[c] for c in range(NCOL)})
    lag[("lk", "A'")], lag[("lk", "S'")] = lk_ap, lk_sp
    # ---- 2: the lookup's permuted columns
    out["lookup_permuted_commitments"] = [commit(lk_ap, srs_lag), commit(lk_sp, srs_lag)]
    # ---- 3: the permutation's grand product in chunks of PERM_CHUNK columns: the 13 advice columns, then the 3 instance columns
    pcols = adv + inst
    z_first, zp = 1, []
    for c in range(3):
        lo, hi = c * PERM_CHUNK, min(N_PERM_COLS, (c + 1) * PERM_CHUNK)
        f = pyref_halo2.permutation_factors(sf, pcols[lo:hi], sigma[lo:hi], beta, gamma, delta, dom.omega, lo)
        z, total = pyref_halo2.prefix_product(sf, f, first=z_first)
        zp.append(z)
        z_first = z[n - (BLINDING_FACTORS + 1)] if "perm_chunk_link" in upstream else total
    # ---- 4: the lookup's grand product
    zl, _ = pyref_halo2.prefix_product(sf, pyref_halo2.lookup_factors(sf, lk_a, lk_s, lk_ap, lk_sp, beta, gamma))
    out["product_commitments"] = [commit(z, srs_lag) for z in zp + [zl]]
    for c in range(3):
        lag[("zp", c)] = zp[c]
    lag[("lk", "Z")] = zl
    for nm, v in lag.items():
        coef[nm] = dom.lagrange_to_coeff(v)
    ext = {nm: dom.coeff_to_extended(coef[nm]) for nm in lag}
    # ---- 5: the vanishing argument's random polynomial (coefficient basis)
    out["random_commitment"] = commit(coef[("random", 0)], srs_g)
    # ---- 6: the quotient.  Columns in quotient_program's documented order: advice, fixed, A', S', Z_lookup, Z_perm x3, instance
    prog = synth.quotient_program(NCOL, N_FIXED, N_INST)
    columns = ([ext[("adv", c)] for c in range(NCOL)] + fixed_ext + [ext[("lk", "A'")], ext[("lk", "S'")], ext[("lk", "Z")]]
               + [ext[("zp", c)] for c in range(3)] + [ext[("inst", c)] for c in range(N_INST)])
    consts = [y, 5, 1, beta, gamma]
    rot_scale = ne // n                                            # omega = extended_omega^(ne / n): one row = rot_scale extended rows
    num = [pyref_halo2.eval_program(sf, prog, columns, consts, ne, rot_scale, i) for i in range(ne)]
    h = dom.extended_to_coeff(dom.divide_by_vanishing_poly(num))
    pieces = [h[q * n:(q + 1) * n] for q in range(N_H_PIECES)]
    out["h_commitments"] = [commit(pc, srs_g) for pc in pieces]
    # ---- 7: h(X) = sum_q x^(n q) h_q, then every polynomial at x and its rotations
    xn = pow(x, n, r)
    coef[("h", 0)] = [sum(pieces[q][i] * pow(xn, q, r) for q in range(N_H_PIECES)) % r for i in range(n)]
    pts = {"x": x, "wx": x * dom.omega % r, "w^-1x": x * dom.omega_inv % r,
           "w^last x": x * pow(dom.omega_inv, BLINDING_FACTORS + 1, r) % r}
    table = [coef[nm] for nm in names]
    evals, labels = {}, {}
    for key, pt in (("evals_at_x", "x"), ("evals_at_omega_x", "wx"), ("evals_at_omega_inv_x", "w^-1x"), ("evals_at_omega_last_x", "w^last x")):
        rows = sorted(i for first, cnt, ps in sets if pt in ps for i in range(first, first + cnt))     # table order
        assert rows == list(range(rows[0], rows[-1] + 1))
        evals[key] = [F.mont_words(horner(r, table[i], pts[pt])) for i in rows]
        labels[key] = [_label(names[i]) for i in rows]
    out.update(evals)
    # ---- 8: multiopen.  q_s = each set's polynomials folded with x_1 (the first one the leading term); q' = sum over the sets, in
    # set order with x_2 (the first set leading), of q_s / prod (X - point); p = q' x_4^4 + q_0 x_4^3 + ... + q_3
    q = []
    for first, cnt, _ in sets:
        acc = [0] * n
        for i in range(first, first + cnt):
            acc = [(a_ * x1 + b_) % r for a_, b_ in zip(acc, table[i])]
        q.append(acc)
    qprime = pyref_halo2.multiopen_quotient(sf, q, [[pts[pn] for pn in ps] for _, _, ps in sets], x2, n)
    out["q_commitment"] = commit(qprime, srs_g)
    out["q_evals_at_x3"] = [F.mont_words(horner(r, qs, x3)) for qs in q]
    p_poly = qprime
    for qs in q:
        p_poly = [(a_ * x4 + b_) % r for a_, b_ in zip(p_poly, qs)]
    # ---- 9: the inner-product argument on p' = s xi + p at x_3, b = powers of x_3, G' = the SRS g (logarithms folded as scalars)
    out["s_commitment"] = commit(s_poly, srs_g)
    pp = [(s_ * xi + a_) % r for s_, a_ in zip(s_poly, p_poly)]
    out["v"] = F.mont_words(horner(r, pp, x3))
    b = [pow(x3, i, r) for i in range(n)]
    g = list(srs_g)
    Ls, Rs, vls, vrs = [], [], [], []
    for j in range(k):
        half = len(pp) // 2
        Ls.append(commit(pp[half:], g[:half]))
        Rs.append(commit(pp[:half], g[half:]))
        vls.append(F.mont_words(pyref_halo2.inner_product(sf, pp[half:], b[:half])))
        vrs.append(F.mont_words(pyref_halo2.inner_product(sf, pp[:half], b[half:])))
        u, ui = us[j], pow(us[j], -1, r)
        pp = [(pp[i] + pp[i + half] * ui) % r for i in range(half)]
        b = [(b[i] + b[i + half] * u) % r for i in range(half)]
        g = [(g[i] + g[i + half] * u) % r for i in range(half)]
    out.update({"ipa_L": Ls, "ipa_R": Rs, "ipa_vl": vls, "ipa_vr": vrs, "ipa_a": [F.mont_words(pp[0])]})
    for nm in SINGLE_OUTPUTS:
        out[nm] = [out[nm]]
    assert sorted(out) == sorted(OUTPUT_NAMES)
    return out, labels


def golden_path(config):
    return os.path.join(GOLDEN_DIR, "halo2_worklist_%s.json" % config)


def golden_document(config):
    curve, k = CONFIGS[config]
    arrays, labels = generate(curve, k)
    return {"generator": "oracle/pyref_halo2_worklist.py", "generator_sha256": source_sha256(), "curve": curve, "scalar_field": SCALAR_FIELD[curve],
            "logn": k, "seeds": SEEDS, "encoding": "rows of little-endian 64-bit words (hex): points affine x | y in Montgomery base-field "
            "limbs, field elements canonical Montgomery limbs; single elements are one row",
            "bench_shortcuts": [s["name"] for s in BENCH_SHORTCUTS], "eval_rows": labels, "arrays": arrays}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--write", action="store_true", help="write tests/golden/halo2_worklist_*.json")
    ap.add_argument("--config", action="append", choices=sorted(CONFIGS), help="only these (default: all)")
    args = ap.parse_args()
    for cfg in args.config or list(CONFIGS):
        doc = golden_document(cfg)
        text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
        if args.write:
            with open(golden_path(cfg), "w") as f:
                f.write(text)
            print("wrote", golden_path(cfg))
        else:
            print(cfg, hashlib.sha256(text.encode()).hexdigest()[:16])


if __name__ == "__main__":
    main()
