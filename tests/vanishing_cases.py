"""The halo2 quotient against the identity a verifier checks, shared by tests/test_vanishing_emu.py (CPU tier, the emulator build)
and tests/test_vanishing_gpu.py (-m gpu).

The other quotient tests compare the device with a restatement of the same computation (pyref_halo2.eval_program on the same
extended values and the same rot_scale, oracle/pyref_halo2_worklist.py).  Here nothing on the right-hand side shares the
device's conventions.  For a gate program whose numerator vanishes on H = <omega>:

  (i)   h = numerator / (X^n - 1) is a polynomial: every coefficient above d (n - 1) - n is zero (d = degree(program));
  (ii)  h(x) (x^n - 1) = the program at a random x, built from the column polynomials at x omega^r (r mod n: a rotation
        keeps its polynomial meaning however it wraps);
  (iii) the folded quotient sum_q x^(n q) h_q(X) -- what the evaluation phase opens -- satisfies (ii) at the same x;
  (iv)  every route to h gives the same coefficients, bit for bit.

A numerator vanishes on H when the program carries its own value as one more column: aux[i] = the program at row i of H
(cyclic rotations), and the program ends in ("col", aux, 0) ("sub",).  For k <= 12 aux comes from pyref_halo2.eval_program on
Python integers; above that from zk_expr_eval_device on the base domain -- then aux is NOT independent of the device, but the
x-identity still is: its right-hand side is computed in Python from the column polynomials.  The lookup argument needs no aux
column: its permuted columns and grand product (permute_expression_pair_device, lookup_product) make both constraints hold.

Column values at a point come from the barycentric formula on Python integers (n <= 2^12), v(z) = (z^n - 1) / n sum_i v_i
omega^i / (z - omega^i), or on larger domains from lagrange_to_coeff and eval_polynomials on the device (pinned elsewhere).

The routes to h:
  (a) "saturated"   the whole coset, the saturated evaluator, divide_by_vanishing_poly, extended_to_coeff;
  (b) "never"       the whole coset with lazy_out and the lazy interpreter (expr_configure("never"));
  (c) "always"      as (b) with the kernel compiled for the program (hiprtc; the GPU build only), "auto" likewise;
  (d) ("part", QP, src, mode)   QP sub-cosets from coeff_to_extended_part (src "part") or coeff_to_extended(parts=QP) (src
        "whole"), evaluate_expression at extended_k - log2 QP with rot_scale_part(QP), divide_by_vanishing_poly_part,
        part_to_coeff, and h from part_mix.
The whole-coset routes fold the quotient with vec_fold_many over its pieces; the sub-coset routes with fold_scalars over the
slices of the folded coefficients (both the bench's way)."""
import numpy as np

from oracle import pyref
from oracle import pyref_halo2 as h2
from parity_suite import _ints, _monts, rand_field, to_device, to_host

FIELDS = ["PallasFp", "PallasFq", "Bn254Fr", "Bls381Fr"]
PY_AUX_MAX_K = 12           # aux and the column values at a point on Python integers up to here
PY_EXT_MAX = 1 << 14        # h(x) by Horner and h from part_mix on Python integers up to this many extended rows


def degree(program):
    """a column is 1, a constant 0; add / sub / neg / scale take the larger operand, mul adds"""
    st = []
    for o in program:
        if o[0] == "col":
            st.append(1)
        elif o[0] == "const":
            st.append(0)
        elif o[0] in ("neg", "scale"):
            st.append(st.pop())
        else:
            b, a = st.pop(), st.pop()
            st.append(a + b if o[0] == "mul" else max(a, b))
    assert len(st) == 1, "not a program"
    return st[0]


def extended_ratio(d):
    """2^(extended_k - k) of EvaluationDomain(field, d + 1, k): the smallest power of two >= d (1 for d <= 1)"""
    r = 1
    while r < d:
        r *= 2
    return r


def new_buffer(zk, shape):
    if zk.backend_info().startswith("emu"):
        return np.zeros(shape, dtype=np.uint64)
    import torch
    return torch.empty(shape, dtype=torch.int64, device="cuda")


def _all(x):
    return bool(x.all())


def _sync(zk):
    if not zk.backend_info().startswith("emu"):
        import torch
        torch.cuda.synchronize()


def _mont(p, v):
    return np.array([((v % p) << 256) % p >> (64 * i) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def _int(field, limbs):
    return _ints(field, np.ascontiguousarray(limbs, dtype=np.uint64).reshape(1, 4))[0]


def eval_at(field, program, value, consts):
    """the program at one point: value(c, r) is column c's polynomial at x omega^r"""
    p = pyref.FIELDS[field][0]
    st = []
    for o in program:
        if o[0] == "col":
            st.append(value(o[1], o[2]))
        elif o[0] == "const":
            st.append(consts[o[1]] % p)
        elif o[0] == "neg":
            st.append(-st.pop() % p)
        elif o[0] == "scale":
            st.append(st.pop() * consts[o[1]] % p)
        else:
            b, a = st.pop(), st.pop()
            st.append((a + b) % p if o[0] == "add" else (a - b) % p if o[0] == "sub" else a * b % p)
    assert len(st) == 1
    return st[0]


def barycentric_weights(p, wpow, z):
    """(c, w) with v(z) = c sum_i v_i w_i for every v given by its values on H: c = (z^n - 1) / n, w_i = omega^i / (z - omega^i);
    wpow[i] = omega^i; one batch inversion"""
    n = len(wpow)
    den = [(z - w) % p for w in wpow]
    pre, acc = [], 1
    for d in den:
        assert d, "z lies in H"
        pre.append(acc)
        acc = acc * d % p
    inv = pow(acc, -1, p)
    w = [0] * n
    for i in range(n - 1, -1, -1):
        w[i] = wpow[i] * inv % p * pre[i] % p
        inv = inv * den[i] % p
    return (pow(z, n, p) - 1) * pow(n, -1, p) % p, w


def barycentric(p, vals, wpow, z):
    """v(z) for the polynomial with v(omega^i) = vals[i]"""
    c, w = barycentric_weights(p, wpow, z)
    return c * sum(v * wi for v, wi in zip(vals, w)) % p


def horner(p, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


class Case:
    """a program' (ending in the aux column, or the lookup program) over Lagrange columns on H = 2^k rows, its domain
    EvaluationDomain(field, degree + 1, k), the columns' coefficients on the device and two random points x"""

    def __init__(self, zk, field, prog, lag, consts, k, seed=1):
        self.zk, self.field, self.prog, self.k = zk, field, prog, k
        self.p = p = pyref.FIELDS[field][0]
        self.n = n = 1 << k
        self.ncols = len(lag)
        self.d = degree(prog)
        self.dom = zk.halo2.EvaluationDomain(field, self.d + 1, k)
        self.ratio = self.dom.extended_len() // n
        assert self.ratio == extended_ratio(self.d), (self.d, self.ratio)
        self.consts = [c % p for c in consts]
        self.consts_mont = _monts(field, self.consts) if consts else np.zeros((0, 4), dtype=np.uint64)
        self.lag = lag                                            # Montgomery uint64 [n, 4] per column (host)
        self.lag_int = [_ints(field, c) for c in lag] if k <= PY_AUX_MAX_K else None
        self.d_lag = [to_device(zk, c) for c in lag]
        self.d_coef = new_buffer(zk, (max(1, self.ncols), n, 4))
        for c in range(self.ncols):
            self.dom.lagrange_to_coeff(self.d_lag[c], out=self.d_coef[c])
        self.omega = _int(field, self.dom.omega)
        rng = pyref.Rng(seed * 7 + k)
        self.xs = [rng.below(p) for _ in range(2)]
        self._rhs = {}

    # ---- the right-hand side: the program at x from the column polynomials at x omega^r (Python, or eval_polynomials)
    def _values(self, x):
        p, n = self.p, self.n
        pts = sorted({o[2] % n for o in self.prog if o[0] == "col"})
        vals = {}
        if self.lag_int is not None:
            wpow = [1] * n
            for i in range(1, n):
                wpow[i] = wpow[i - 1] * self.omega % p
            for r in pts:
                cz, w = barycentric_weights(p, wpow, x * pow(self.omega, r, p) % p)
                for c in range(self.ncols):
                    vals[(c, r)] = cz * sum(v * wi for v, wi in zip(self.lag_int[c], w)) % p
        else:
            for r in pts:
                z = _mont(p, x * pow(self.omega, r, p))
                got = self.zk.halo2.eval_polynomials(self.field, self.d_coef[: self.ncols], z)
                for c in range(self.ncols):
                    vals[(c, r)] = _int(self.field, got[c])
        return vals

    def rhs(self, x):
        """program'(x)"""
        if x not in self._rhs:
            vals = self._values(x)
            self._rhs[x] = eval_at(self.field, self.prog, lambda c, r: vals[(c, r % self.n)], self.consts)
        return self._rhs[x]

    # ---- the checks
    def poly_at(self, buf, x):
        """the polynomial with coefficients `buf` (a device buffer) at x"""
        if int(buf.shape[0]) <= PY_EXT_MAX:
            return horner(self.p, _ints(self.field, np.ascontiguousarray(to_host(self.zk, buf))), x)
        return _int(self.field, self.zk.halo2.eval_polynomial(self.field, buf, _mont(self.p, x)))

    def check(self, h, folded=None):
        """{"degree": (i), "identity": (ii) at both points, "fold": (iii)} for coefficients h (device buffer of extended_len)
        and folded[t], the folded quotient for x_t"""
        p, n = self.p, self.n
        lo = max(0, self.d * (n - 1) - n + 1)
        out = {"degree": _all(h[lo:] == 0)}
        out["identity"] = all(self.poly_at(h, x) * (pow(x, n, p) - 1) % p == self.rhs(x) for x in self.xs)
        if folded is not None:
            out["fold"] = all(self.poly_at(f, x) * (pow(x, n, p) - 1) % p == self.rhs(x) for f, x in zip(folded, self.xs))
        return out

    # ---- the program the device runs
    def device_program(self, fault):
        if fault == "rot_neg":
            return [("col", o[1], -o[2]) if o[0] == "col" else o for o in self.prog]
        return self.prog

    def _evaluate(self, cols, log_n, rot_scale, out, mode, fault):
        H = self.zk.halo2
        lazy = mode != "saturated"
        if lazy:
            H.expr_configure(mode)
        try:
            H.evaluate_expression(self.field, self.device_program(fault), cols, self.consts_mont, log_n,
                                  rot_scale * (2 if fault == "rot_scale_x2" else 1), out, lazy=lazy)
        finally:
            if lazy:
                H.expr_configure("auto")

    def _fold_pieces(self, h):
        """vec_fold_many over the quotient's n-coefficient pieces, the last one leading: one folded polynomial per x"""
        out = []
        for x in self.xs:
            f = new_buffer(self.zk, (self.n, 4))
            self.zk.halo2.vec_fold_many(self.field, f, h.reshape(self.ratio, self.n, 4), _mont(self.p, pow(x, self.n, self.p)), reverse=True)
            out.append(f)
        return out

    def route_whole(self, mode, fault=None):
        """routes (a) / (b) / (c): (h, folded)"""
        dom, ne = self.dom, self.dom.extended_len()
        cols = []
        for c in range(self.ncols):
            b = new_buffer(self.zk, (ne, 4))
            dom.coeff_to_extended(b, coeffs=self.d_coef[c], lazy_out=mode != "saturated")
            cols.append(b)
        h = new_buffer(self.zk, (ne, 4))
        self._evaluate(cols, dom.extended_k, self.ratio, h, mode, fault)
        del cols
        if mode == "saturated":
            dom.divide_by_vanishing_poly(h)
        else:
            dom.divide_by_vanishing_poly_part(h, 0, 1)
        dom.extended_to_coeff(h)
        return h, self._fold_pieces(h)

    def route_parts(self, parts, src="part", mode="never", fault=None):
        """route (d): (h, folded)"""
        zk, dom, ne = self.zk, self.dom, self.dom.extended_len()
        H, p = zk.halo2, self.p
        m = ne // parts
        lazy = mode != "saturated"
        hp = new_buffer(zk, (parts, m, 4))
        whole = None
        if src == "whole":
            whole = []
            for c in range(self.ncols):
                b = new_buffer(zk, (ne, 4))
                dom.coeff_to_extended(b, coeffs=self.d_coef[c], lazy_out=lazy, parts=parts)
                whole.append(b.reshape(parts, m, 4))
        for j in range(parts):
            if whole is not None:
                cols = [b[j] for b in whole]
            else:
                cols = []
                for c in range(self.ncols):
                    b = new_buffer(zk, (m, 4))
                    dom.coeff_to_extended_part(self.d_coef[c], b, j, parts, lazy_out=lazy)
                    cols.append(b)
            self._evaluate(cols, dom.extended_k - (parts.bit_length() - 1), dom.rot_scale_part(parts), hp[j], mode, fault)
            dom.divide_by_vanishing_poly_part(hp[j], j, parts)
        del whole
        if fault == "swap_parts":
            t = hp[0].copy() if isinstance(hp, np.ndarray) else hp[0].clone()
            hp[0] = hp[1]
            hp[1] = t
        for j in range(parts):
            dom.part_to_coeff(hp[j], j, parts)
        c = dom.part_mix(parts)
        if ne <= PY_EXT_MAX:                       # h from part_mix on Python integers
            A = [np.array(_ints(self.field, np.ascontiguousarray(to_host(zk, hp[j]))), dtype=object) for j in range(parts)]
            hv = []
            for i in range(parts):
                hv.extend(int(v) for v in sum(c[i][j] * A[j] for j in range(parts)) % p)
            h = to_device(zk, _monts(self.field, hv))
        else:                                      # ... or with vec_muladd on the device
            h = new_buffer(zk, (ne, 4))
            for i in range(parts):
                dst = h[i * m:(i + 1) * m]
                dst[...] = hp[0]
                zk.vec_op(self.field, "scale", dst, scalar=_mont(p, c[i][0]))
                for j in range(1, parts):
                    H.vec_muladd(self.field, hp[j], dst, _mont(p, c[i][j]), out=dst)
        # the folded quotient the bench's way: fold_scalars over the n-coefficient slices of the A_j
        r = m // self.n
        slices = hp.reshape(parts * r, self.n, 4)
        folded = []
        for x in self.xs:
            e = dom.fold_scalars(parts, pow(x, self.n, p))
            f = new_buffer(zk, (self.n, 4))
            f[...] = slices[0]
            zk.vec_op(self.field, "scale", f, scalar=_mont(p, e[0][0]))
            for j in range(parts):
                for s in range(r):
                    if j or s:
                        H.vec_muladd(self.field, slices[j * r + s], f, _mont(p, e[j][s]), out=f)
            folded.append(f)
        return h, folded

    def route(self, spec, fault=None):
        """spec: "saturated" / "never" / "always" / "auto" (the whole coset) or ("part", QP, src, mode).  fault, for the negative
        controls: "rot_scale_x2" (the device is given twice the rot_scale), "rot_neg" (every rotation negated), "swap_parts"
        (sub-cosets 0 and 1 swapped before part_to_coeff)"""
        if isinstance(spec, tuple):
            return self.route_parts(spec[1], src=spec[2], mode=spec[3], fault=fault)
        return self.route_whole(spec, fault=fault)


def part_routes(ratio, modes=("never",), srcs=("part", "whole")):
    """route (d) for QP = 2 .. ratio"""
    out = []
    qp = 2
    while qp <= ratio:
        out += [("part", qp, s, m) for s in srcs for m in modes]
        qp *= 2
    return out


def check_routes(case, routes, call=None):
    """(i) - (iii) on every route, (iv) bit for bit against the first; call(spec) -> (h, folded) runs a route (default:
    case.route)"""
    first = None
    for spec in routes:
        h, folded = (call or case.route)(spec)
        res = case.check(h, folded)
        assert all(res.values()), (case.field, case.k, spec, res)
        hh = to_host(case.zk, h).copy() if isinstance(h, np.ndarray) else h
        ff = [to_host(case.zk, f).copy() if isinstance(f, np.ndarray) else f for f in folded]
        if first is None:
            first = (spec, hh, ff)
        else:
            assert _all(hh == first[1]), (case.field, case.k, spec, "h differs from", first[0])
            assert all(_all(a == b) for a, b in zip(ff, first[2])), (case.field, case.k, spec, "folded quotient differs from", first[0])
    _sync(case.zk)


# ------------------------------------------------------------------------------------------------------------ cases
def aux_case(zk, field, prog, n_cols, n_consts, k, seed=1, corrupt=None):
    """random Lagrange columns, the aux column that makes `prog` vanish on H, program' = prog - aux.  corrupt = (column, row):
    one Lagrange value changed AFTER aux was computed (a negative control)"""
    p = pyref.FIELDS[field][0]
    n = 1 << k
    lag = [rand_field(field, n, seed * 1000 + c) for c in range(n_cols)]
    rng = pyref.Rng(seed * 31 + k)
    consts = [rng.below(p) for _ in range(n_consts)]
    if k <= PY_AUX_MAX_K:
        ci = [_ints(field, c) for c in lag]
        aux = _monts(field, [h2.eval_program(field, prog, ci, consts, n, 1, i) for i in range(n)])
    else:                                  # not independent of the device (see the module docstring)
        out = new_buffer(zk, (n, 4))
        zk.halo2.evaluate_expression(field, prog, [to_device(zk, c) for c in lag], _monts(field, consts) if consts else np.zeros((0, 4), dtype=np.uint64),
                                     k, 1, out)
        aux = np.ascontiguousarray(to_host(zk, out)).copy()
    lag.append(aux)
    if corrupt is not None:                # (column n_cols is aux itself)
        c, i = corrupt
        lag[c] = lag[c].copy()
        lag[c][i] = _monts(field, [_int(field, lag[c][i]) + 1])[0]
    return Case(zk, field, prog + [("col", n_cols, 0), ("sub",)], lag, consts, k, seed)


def bench_program():
    from contangle_zkcp_amd import synth
    return synth.quotient_program(13, 8, 3), 30, 5


def corpus_programs(k, max_degree=15):
    """tests/expr_programs.py's corpus (its +-(n - 1) rotations for this n) whose degree is at most max_degree: (name, ops, n_cols,
    n_consts).  The corpus' rot_scale belongs to its own tests: here every rotation is a rotation of H"""
    import expr_programs as xp
    return [(q.name, q.ops, q.n_cols, q.n_consts) for q in xp.corpus(k) if degree(q.ops) <= max_degree and q.n_cols < xp.EXPR_MAX_COLS
            and len(q.ops) + 2 <= xp.EXPR_MAX_OPS]


# the two lookup constraints of synth.quotient_program over columns A, S, A', S', Z; consts beta, gamma, y
LOOKUP_PROGRAM = [("col", 4, 1), ("col", 2, 0), ("const", 0), ("add",), ("mul",), ("col", 3, 0), ("const", 1), ("add",), ("mul",),
                  ("col", 4, 0), ("col", 0, 0), ("const", 0), ("add",), ("mul",), ("col", 1, 0), ("const", 1), ("add",), ("mul",), ("sub",),
                  ("scale", 2), ("col", 2, 0), ("col", 3, 0), ("sub",), ("col", 2, 0), ("col", 2, -1), ("sub",), ("mul",), ("add",)]


def lookup_case(zk, field, dist, k, seed=1, swap_rows=False):
    """a genuine lookup on all 2^k rows: A, S from lookup_permute_cases, (A', S') = permute_expression_pair_device, Z from
    lookup_product (z_0 = 1, z_{i+1} = z_i f_i, closing to 1: the relation holds cyclically on H).  swap_rows: two rows of A' that
    hold different values swapped after Z was computed (a negative control)"""
    import lookup_permute_cases as lc
    p = pyref.FIELDS[field][0]
    n = 1 << k
    inputs, table = lc.make_case(field, dist, n, seed)
    a, s = _monts(field, inputs), _monts(field, table)
    d_a, d_s = to_device(zk, a), to_device(zk, s)
    ap, sp = zk.halo2.permute_expression_pair_device(field, d_a, d_s, n)
    rng = pyref.Rng(seed * 13 + k)
    beta, gamma, y = rng.below(p), rng.below(p), rng.below(p)
    z = new_buffer(zk, (n, 4))
    last = zk.halo2.lookup_product(field, d_a, d_s, ap, sp, _mont(p, beta), _mont(p, gamma), z)
    assert (last == _mont(p, 1)).all(), "the lookup product closes to 1"
    cols = [a, s] + [np.ascontiguousarray(to_host(zk, c)).copy() for c in (ap, sp, z)]
    assert (cols[4][0] == _mont(p, 1)).all(), "z_0 = 1"
    if swap_rows:
        A = cols[2]
        i = 0
        j = next(t for t in range(1, n) if (A[t] != A[i]).any())
        A[[i, j]] = A[[j, i]]
    return Case(zk, field, LOOKUP_PROGRAM, cols, [beta, gamma, y], k, seed)


def assert_detected(case, spec, fault=None):
    """a negative control: the checker reports failure of both (i) and (ii)"""
    h, folded = case.route(spec, fault=fault)
    res = case.check(h, folded)
    assert not res["degree"] and not res["identity"], (case.field, case.k, spec, fault, res)
