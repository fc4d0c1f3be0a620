"""Mirror of halo2_proofs 0.2 on the commitment / quotient path:

  arithmetic.rs    best_multiexp(coeffs, bases) -> C::Curve    coeffs are field elements as stored (Montgomery)
                   best_fft(a, omega, log_n)                   no scaling, no coset logic; caller supplies omega or omega^-1
  poly/domain.rs   EvaluationDomain::new(j, k), lagrange_to_coeff, coeff_to_extended, extended_to_coeff,
                   divide_by_vanishing_poly, and the constants it derives (omega, extended_omega, g_coset = ZETA,
                   ifft divisors, t_evaluations)

The reference's halo2 crate (circuits-halo2/src/encryption.rs:254-296) never reaches these -- it only runs
MockProver -- so they are exercised here as the shape donor for the 2^20-row synthetic workload.
Same names, argument meaning and assertion behaviour as upstream; the arithmetic runs in the HIP library.
"""
import ctypes

import numpy as np

from . import (ZK_ERR_INVALID_ARG, ZK_ERR_LOOKUP, Bases, ZkError, _call, _check, _np64, _ptr, base_limbs, cp, curve_id, field_id, field_inverse,
               field_modulus, i32, i64, load, msm, msm_batch, msm_submit, multiplicative_generator, ntt, ntt_points_device, ptr, root_of_unity,
               scalar_field, u32, u64, vec_op, vp)

def best_multiexp(coeffs, bases):
    if int(coeffs.shape[0]) != bases.n:
        raise AssertionError("assertion failed: coeffs.len() == bases.len()")   # halo2: assert_eq!
    return msm(bases, coeffs, montgomery=True)


def best_multiexp_batch(columns, bases, stream=0):
    """the commitments of several columns against the same `Params::g_lagrange` (upstream: a loop of commit_lagrange
    calls with no data dependence between them); columns: device buffer [count, n, 4]"""
    if int(columns.shape[1]) != bases.n:
        raise AssertionError("assertion failed: coeffs.len() == bases.len()")
    return msm_batch(bases, columns, montgomery=True, stream=stream)


def best_fft(field, a, omega, log_n):
    if int(a.shape[0]) != 1 << log_n:
        raise AssertionError("assertion failed: a.len() == 1 << log_n")
    return ntt(field, a, omega)


def best_fft_points(curve, d_points, omega, log_n, out=None, stream=0):
    """best_fft(a, omega, log_n) with G = a curve (Pallas, Vesta): the DFT of 2^log_n affine points resident on the device with
    scalar-field twiddles, no scaling.  In place, or into `out` with d_points left alone."""
    if int(d_points.shape[0]) != 1 << log_n:
        raise AssertionError("assertion failed: a.len() == 1 << log_n")
    if out is not None and int(out.shape[0]) != 1 << log_n:
        raise AssertionError("assertion failed: out.len() == 1 << log_n")
    return ntt_points_device(curve, d_points, d_points if out is None else out, log_n, omega, False, stream)


class Params:
    """halo2_proofs 0.2 poly/commitment.rs Params<C>, the part that lives on the device: k, n, g and g_lagrange as resident
    bases.  `from_g` does what Params::new does after it has hashed g: g_lagrange = best_fft(g, omega_k^-1) times n^-1,
    normalised, i.e. g_lagrange[i] = [1/n] sum_j [omega^(-ij)] g_j, the key for which commit_lagrange(evals) ==
    commit(coeffs).  Generating g itself (hash_to_curve("Halo2-Parameters"): BLAKE2b, simplified SWU, isogeny) is not done
    here and stays with the caller, and so do w and u: the caller hands them in (affine Montgomery host points) when it
    verifies openings (MSM.eval needs both); committing and key generation never look at them."""

    def __init__(self, curve, k, d_g, d_g_lagrange, u=None, w=None):
        self.curve, self.k, self.n = curve_id(curve), int(k), 1 << int(k)
        self.u = None if u is None else _np64(u).copy()
        self.w = None if w is None else _np64(w).copy()
        self.d_g, self.d_g_lagrange = d_g, d_g_lagrange
        self.g = Bases(curve, device_tensor=d_g, n=self.n)                    # zk_bases_adopt_device: no copy
        self.g_lagrange = Bases(curve, device_tensor=d_g_lagrange, n=self.n)

    @classmethod
    def from_g(cls, curve, k, g, stream=0, u=None, w=None):
        """g: 2^k affine points (Montgomery u64 limbs [n, 8], identity = (0, 0)), a host array or a device tensor"""
        from .groth16 import _new_buffer, _synchronize, _upload
        n = 1 << int(k)
        if int(g.shape[0]) != n:
            raise AssertionError("assertion failed: g.len() == 1 << k")
        d_g = _upload(g) if isinstance(g, np.ndarray) else g
        field = scalar_field(curve)
        omega_inv = field_inverse(field, root_of_unity(field, int(k)))
        d_gl = _new_buffer(tuple(d_g.shape))
        ntt_points_device(curve, d_g, d_gl, int(k), omega_inv, True, stream)
        _synchronize()          # the adopted vectors are read by MSMs on any stream
        return cls(curve, k, d_g, d_gl, u=u, w=w)

    def commit(self, coeffs):
        """commit(poly) without blinding: best_multiexp(coeffs, g); coeffs Montgomery, host or device"""
        return best_multiexp(coeffs, self.g)

    def commit_lagrange(self, evals):
        """commit_lagrange(poly) without blinding: best_multiexp(evals, g_lagrange)"""
        return best_multiexp(evals, self.g_lagrange)

    def commit_lagrange_batch(self, columns, stream=0):
        return best_multiexp_batch(columns, self.g_lagrange, stream=stream)

    def free(self):
        self.g.free()
        self.g_lagrange.free()


def coeff_to_extended(field, d_ext, k, omega_ext, zeta, stream=0):
    """halo2_proofs 0.2 EvaluationDomain::coeff_to_extended: `d_ext` is a device buffer of the EXTENDED length whose first
    2^k entries hold the coefficients; they are taken as zero-extended (`a.resize(extended_len, 0)` upstream -- the padding
    is neither written nor read here), shifted onto the zeta coset (`distribute_powers_zeta`) and transformed in place."""
    return ntt(field, d_ext, omega_ext, stream=stream, coset_pre=zeta, in_log=k)


def _mont_limbs(x, p):
    v = (x << 256) % p
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def zeta(field):
    """pasta_curves 0.4 `FieldExt::ZETA` = GENERATOR^((p - 1) / 3), a primitive cube root of unity, Montgomery"""
    p = field_modulus(field)
    g = multiplicative_generator(field)
    gi = sum(int(w) << (64 * i) for i, w in enumerate(g.tolist())) * pow(1 << 256, -1, p) % p
    assert (p - 1) % 3 == 0
    return _mont_limbs(pow(gi, (p - 1) // 3, p), p)


class EvaluationDomain:
    """halo2_proofs 0.2 poly/domain.rs EvaluationDomain<G>::new(j, k): n = 2^k rows, gates of degree j; the quotient is
    computed on the extended domain of size 2^extended_k, extended_k = k + ceil(log2(j - 1)), on the coset ZETA * H_ext."""

    def __init__(self, field, j, k):
        self.field = field_id(field)
        self.k = k
        self.quotient_poly_degree = j - 1
        self.n = 1 << k
        extended_k = k
        while (1 << extended_k) < self.n * self.quotient_poly_degree:
            extended_k += 1
        self.extended_k = extended_k
        self.omega = root_of_unity(field, k)                       # ROOT_OF_UNITY^(2^(S - k))
        self.omega_inv = field_inverse(field, self.omega)
        self.extended_omega = root_of_unity(field, extended_k)
        self.extended_omega_inv = field_inverse(field, self.extended_omega)
        self.g_coset = zeta(field)                                 # ZETA
        self.g_coset_inv = field_inverse(field, self.g_coset)      # = ZETA^2
        p = field_modulus(field)
        self._p = p
        # t_evaluations[i] = 1 / ((ZETA * extended_omega^i)^n - 1), i < 2^(extended_k - k): the vanishing polynomial X^n - 1
        # takes only that many distinct values on the coset
        to_int = lambda a: sum(int(w) << (64 * i) for i, w in enumerate(a.tolist())) * pow(1 << 256, -1, p) % p
        zi, wi = to_int(self.g_coset), to_int(self.extended_omega)
        m = 1 << (extended_k - k)
        self.t_evaluations = np.stack([_mont_limbs(pow((pow(zi * pow(wi, i, p) % p, self.n, p) - 1) % p, -1, p), p) for i in range(m)])

    def extended_len(self):
        return 1 << self.extended_k

    # ---- device buffers (torch tensors; numpy under the CPU test emulator), in place
    def lagrange_to_coeff(self, a, stream=0, out=None):
        """ifft(a, omega_inv, k, ifft_divisor): best_fft with omega^-1, then every element times n^-1.  out: write the
        coefficients there and leave the Lagrange values alone (upstream returns a new Polynomial; the prover keeps both)"""
        if int(a.shape[0]) != self.n:
            raise AssertionError("assertion failed: a.values.len() == 1 << self.k")
        if out is not None:
            if int(out.shape[0]) != self.n:
                raise AssertionError("assertion failed: out.len() == 1 << self.k")
            return ntt(self.field, out, self.omega_inv, scale_by_n_inv=True, stream=stream, src=a)
        return ntt(self.field, a, self.omega_inv, scale_by_n_inv=True, stream=stream, device=True)

    def coeff_to_lagrange(self, a, stream=0):
        if int(a.shape[0]) != self.n:
            raise AssertionError("assertion failed: a.values.len() == 1 << self.k")
        return ntt(self.field, a, self.omega, stream=stream, device=True)

    def coeff_to_extended(self, a_ext, stream=0, coeffs=None, lazy_out=False, parts=1):
        """`a_ext`: buffer of extended_len() whose first n entries are the coefficients (the rest is treated as the zeros
        upstream's `resize` appends): distribute_powers_zeta(into_coset) ; best_fft(extended_omega).  coeffs: take the n
        coefficients from that buffer instead (it is left untouched: the openings evaluate it later).
        parts: store the result sub-coset by sub-coset -- a_ext.view(parts, extended_len / parts)[j] is what
        coeff_to_extended_part(.., j, parts) computes (ZK_NTT_OUT_SUBCOSETS: the same transform, other store addresses)"""
        if int(a_ext.shape[0]) != self.extended_len():
            raise AssertionError("assertion failed: a.len() == extended_len")
        self._part_check(0, parts)
        flags = (2 if lazy_out else 0) | ((parts.bit_length() - 1) << 4)
        if coeffs is not None:
            if int(coeffs.shape[0]) != self.n:
                raise AssertionError("assertion failed: a.len() == 1 << self.k")
            return ntt(self.field, a_ext, self.extended_omega, stream=stream, coset_pre=self.g_coset, in_log=self.k, src=coeffs,
                       scale_by_n_inv=flags)
        return ntt(self.field, a_ext, self.extended_omega, stream=stream, coset_pre=self.g_coset,
                   in_log=self.k if self.extended_k > self.k else None, device=True, scale_by_n_inv=flags)

    def extended_to_coeff(self, a_ext, stream=0):
        """best_fft(extended_omega_inv) ; times extended_ifft_divisor ; distribute_powers_zeta(out of the coset).  Upstream
        then truncates to n * quotient_poly_degree coefficients: use the first quotient_len() entries."""
        if int(a_ext.shape[0]) != self.extended_len():
            raise AssertionError("assertion failed: a.values.len() == extended_len")
        return ntt(self.field, a_ext, self.extended_omega_inv, scale_by_n_inv=True, stream=stream, coset_post=self.g_coset_inv, device=True)

    # ---- the extended coset in `parts` sub-cosets (one per GPU of a sharded prover): sub-coset j holds the extended
    # evaluations e = i * parts + j, i.e. the points ZETA extended_omega^j (extended_omega^parts)^i.  Every column's values on
    # sub-coset j are ONE transform of size extended_len / parts (coset generator ZETA extended_omega^j), rotations by r
    # rows stay inside the sub-coset (shift r * rot_scale_part), and the vanishing polynomial takes 2^(extended_k - k) / parts
    # values there -- so the quotient numerator shards with no exchange until h itself (32 bytes per extended row).
    def _part_check(self, part, parts):
        m = 1 << (self.extended_k - self.k)
        if parts < 1 or parts > m or (parts & (parts - 1)) or not 0 <= part < parts:
            raise AssertionError("parts must be a power of two <= 2^(extended_k - k) and 0 <= part < parts")

    def part_len(self, parts):
        return self.extended_len() // parts

    def rot_scale_part(self, parts):
        return (1 << (self.extended_k - self.k)) // parts

    def _part_constants(self, part, parts):
        key = (part, parts)
        if not hasattr(self, "_parts"):
            self._parts = {}
        if key not in self._parts:
            p = self._p
            to_int = lambda a: sum(int(w) << (64 * i) for i, w in enumerate(a.tolist())) * pow(1 << 256, -1, p) % p
            wi, zi = to_int(self.extended_omega), to_int(self.g_coset)
            g = zi * pow(wi, part, p) % p
            self._parts[key] = (_mont_limbs(g, p), _mont_limbs(pow(wi, parts, p), p))
        return self._parts[key]

    def coeff_to_extended_part(self, coeffs, out, part, parts, stream=0, lazy_out=False):
        """out[i] = the polynomial `coeffs` (n coefficients, untouched) at ZETA extended_omega^(i parts + part), i < extended_len / parts.
        lazy_out: in the lazy-limb radix (x R' mod p) for evaluate_expression(lazy=True)"""
        self._part_check(part, parts)
        if int(coeffs.shape[0]) != self.n or int(out.shape[0]) != self.part_len(parts):
            raise AssertionError("assertion failed: coeffs.len() == n && out.len() == extended_len / parts")
        g, w = self._part_constants(part, parts)
        return ntt(self.field, out, w, stream=stream, coset_pre=g, in_log=self.k, src=coeffs, scale_by_n_inv=2 if lazy_out else 0)

    def part_to_coeff(self, a_part, part, parts, stream=0):
        """in place, the inverse of coeff_to_extended_part for a polynomial of degree < extended_len / parts =: m -- and for a
        longer one (the quotient: degree < extended_len) the sub-coset's FOLDED coefficients
            A_part[r] = sum_i (g^m)^i h[i m + r],   g = ZETA extended_omega^part   (g^m is the same for every point of the sub-coset)
        from which quotient_pieces_from_parts recovers h: inverse transform of size m, times 1 / m, times g^-r."""
        self._part_check(part, parts)
        if int(a_part.shape[0]) != self.part_len(parts):
            raise AssertionError("assertion failed: a.len() == extended_len / parts")
        key = ("inv", part, parts)
        if key not in self.__dict__.setdefault("_parts", {}):
            g, w = self._part_constants(part, parts)
            self._parts[key] = (field_inverse(self.field, g), field_inverse(self.field, w))
        ginv, winv = self._parts[key]
        return ntt(self.field, a_part, winv, scale_by_n_inv=True, stream=stream, coset_post=ginv, device=True)

    def part_mix(self, parts):
        """c[i][j] (Python integers) with  h[i m : (i + 1) m] = sum_j c[i][j] A_j  for the folded coefficients A_j of part_to_coeff:
        A_j = sum_i (ZETA^m theta^j)^i h^(i), theta = extended_omega^m a primitive parts-th root of unity, so the h^(i) are an inverse
        DFT of size `parts` over the sub-cosets, scaled: c[i][j] = ZETA^(-m i) theta^(-i j) / parts."""
        self._part_check(0, parts)
        p = self._p
        to_int = lambda a: sum(int(w) << (64 * i) for i, w in enumerate(a.tolist())) * pow(1 << 256, -1, p) % p
        m = self.part_len(parts)
        theta = pow(to_int(self.extended_omega), m, p)
        zm_inv = pow(pow(to_int(self.g_coset), m, p), -1, p)
        pinv = pow(parts, -1, p)
        return [[pinv * pow(zm_inv, i, p) * pow(theta, (-i * j) % parts, p) % p for j in range(parts)] for i in range(parts)]

    def piece_scalars(self, parts):
        """the quotient's pieces of n coefficients (upstream commits each: h(X) = sum_q X^(n q) h_q) as combinations of the n-coefficient
        slices of the folded sub-coset coefficients: piece q = i r + s (r = m / n slices per part) = sum_j c[i][j] A_j[s n : (s + 1) n].
        Returns [(q, [(j, s, c_ij), ...])]: by linearity the same combination of the slices' COMMITMENTS is the piece's commitment."""
        c = self.part_mix(parts)
        r = self.part_len(parts) // self.n
        return [(i * r + s, [(j, s, c[i][j]) for j in range(parts)]) for i in range(parts) for s in range(r)]

    def fold_scalars(self, parts, xn_int):
        """e[j][s] with  sum_q xn^q h_q = sum_{j, s} e[j][s] A_j[s n : (s + 1) n]  (the folded quotient the evaluation phase opens)"""
        c = self.part_mix(parts)
        p = self._p
        r = self.part_len(parts) // self.n
        xr = pow(xn_int, r, p)
        return [[pow(xn_int, s, p) * sum(pow(xr, i, p) * c[i][j] for i in range(parts)) % p for s in range(r)] for j in range(parts)]

    def divide_by_vanishing_poly_part(self, a_part, part, parts, stream=0):
        """a[i] *= t_evaluations[(i parts + part) mod 2^(extended_k - k)]"""
        self._part_check(part, parts)
        m = 1 << (self.extended_k - self.k)
        tbl = np.stack([self.t_evaluations[(i * parts + part) % m] for i in range(m // parts)])
        return vec_op(self.field, "scale_periodic", a_part, b=tbl, stream=stream)

    def quotient_len(self):
        return self.n * self.quotient_poly_degree

    def divide_by_vanishing_poly(self, a_ext, stream=0):
        """a[i] *= t_evaluations[i mod 2^(extended_k - k)]  (the inverse of X^n - 1 on the coset, periodic)"""
        if int(a_ext.shape[0]) != self.extended_len():
            raise AssertionError("assertion failed: a.values.len() == extended_len")
        return vec_op(self.field, "scale_periodic", a_ext, b=self.t_evaluations, stream=stream)


def combine_commitments(curve, points_jac, rows, to_device=None, stream=0):
    """sum_k scalar_k * points[index_k] for every row of `rows` = [[(index, integer scalar), ...], ...]: the commitments of the quotient's
    pieces from the commitments of the sub-cosets' folded coefficients (EvaluationDomain.piece_scalars) -- commitments are linear, so
    the pieces never have to exist as vectors before they are committed.  A batched MSM over a throwaway handle of len(points) bases
    (to_device: host array -> device buffer; without it one host-scalar MSM per row).  Returns [len(rows), 3 * limbs] Jacobian."""
    from . import point_to_affine
    aff = np.stack([point_to_affine(curve, pj) for pj in points_jac])
    cols = np.zeros((len(rows), len(points_jac), 4), dtype=np.uint64)
    for q, terms in enumerate(rows):
        for idx, sc in terms:
            cols[q, idx] = [(int(sc) >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]
    bases = Bases(curve, aff)
    try:
        if to_device is not None:
            return msm_batch(bases, to_device(cols), stream=stream)
        return np.stack([msm(bases, cols[q]) for q in range(len(rows))])
    finally:
        bases.free()


# ------------------------------------------------------------------ prover steps beyond commit / FFT
class ExprOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_uint8), ("pad", ctypes.c_uint8), ("rot", ctypes.c_int16), ("arg", ctypes.c_uint32)]


EXPR_CODES = {"col": 0, "const": 1, "add": 2, "sub": 3, "mul": 4, "neg": 5, "scale": 6}

pp = ptr(vp)
SIGNATURES = {
    "zk_batch_invert_device": [i32, vp, u64, vp],
    "zk_prefix_product_device": [i32, vp, vp, u64, vp, vp, vp],
    "zk_halo2_permutation_product_device": [i32, u32, pp, pp, u32, vp, vp, vp, u32, vp, vp, vp, vp],
    "zk_halo2_lookup_product_device": [i32, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp],
    "zk_halo2_permute_expression_pair_device": [i32, vp, vp, u64, vp, vp, vp],
    "zk_inner_product_device": [i32, vp, vp, u64, vp, vp],
    "zk_vec_fold_device": [i32, vp, u64, vp, vp],
    "zk_ipa_fold_bases_device": [i32, vp, u64, vp, vp],
    "zk_ipa_virtual_scalars_device": [i32, vp, vp, u64, u64, vp, vp, vp],
    "zk_ipa_update_weights_device": [i32, vp, u64, u64, vp, vp],
    "zk_ipa_collapse_device": [i32, u64, vp, u64, u64, vp, vp],
    "zk_ipa_collapse_range_device": [i32, u64, vp, u64, u64, u64, u64, vp, vp],
    "zk_ipa_round_device": [i32, u64, vp, vp, vp, u64, u64, vp, vp, vp, vp],
    "zk_poly_eval_device": [i32, vp, u64, vp, vp, vp],
    "zk_vec_muladd_device": [i32, vp, vp, u64, vp, vp],
    "zk_vec_muladd_to_device": [i32, vp, vp, vp, u64, vp, vp],
    "zk_poly_eval_batch_device": [i32, vp, u64, u32, u64, vp, vp, vp],
    "zk_kate_division_device": [i32, vp, vp, u64, vp, vp],
    "zk_vec_powers_device": [i32, vp, u64, vp, vp],
    "zk_vec_fold_many_device": [i32, vp, vp, i64, u32, u64, vp, vp],
    "zk_ipa_fold_round_device": [i32, vp, vp, vp, u64, u64, vp, vp],
    "zk_expr_eval_device": [i32, ptr(ExprOp), u32, pp, u32, vp, u32, u32, u32, vp, vp],
    "zk_expr_eval_lazy_device": [i32, ptr(ExprOp), u32, pp, u32, vp, u32, u32, u32, vp, vp],
    "zk_expr_configure": [i32],
    "zk_expr_specialised_source": [i32, ptr(ExprOp), u32, u32, u32, cp, u64, ptr(u64)],
    "zk_halo2_assembly_new": [u64, u32, ptr(u64)],
    "zk_halo2_assembly_copy": [u64, vp, u64, ptr(u64)],
    "zk_halo2_assembly_mapping": [u64, vp],
    "zk_halo2_assembly_free": [u64],
    "zk_halo2_permutation_sigmas_device": [i32, u32, u32, vp, vp, vp, vp],
    "zk_halo2_ipa_s_device": [i32, u32, u32, vp, vp, vp, i32, vp],
    "zk_halo2_ipa_compute_b": [i32, u32, vp, vp, vp],
    "zk_halo2_mock_eval_device": [i32, u32, ptr(ExprOp), vp, u32, pp, vp, u32, vp, u32, vp, vp, vp],
    "zk_halo2_mock_lookup_device": [i32, u32, vp, vp, vp, vp, u64, vp, vp],
    "zk_halo2_mock_permutation_device": [i32, u32, u32, pp, vp, vp, vp, vp],
    "zk_halo2_mock_failures_device": [vp, u64, u64, vp, vp, vp, vp],
}
PROVER_EXPORTS = list(SIGNATURES)
_plib = load        # the bound handle (tests and tools take it for raw calls)


def _ptr_array(bufs):
    return (ctypes.c_void_p * len(bufs))(*[ctypes.cast(_ptr(b), ctypes.c_void_p).value for b in bufs])


def permute_expression_pair(field, inputs_mont, table_mont, usable_rows):
    """plonk/lookup/prover.rs permute_expression_pair -- a CPU step upstream (a sort and a BTreeMap) and here: host arrays of
    Montgomery limbs [n, 4] in, (A', S') of usable_rows each out (the caller appends its blinding rows and uploads).  Values are
    ordered as canonical integers (the field's Ord); raises ValueError where upstream returns ConstraintSystemFailure."""
    p = field_modulus(field)
    r_inv = pow(1 << 256, -1, p)

    def canon(arr):            # Montgomery limbs -> canonical limbs, via Python integers (a host step; sizes are one column)
        a = _np64(arr)[:usable_rows].astype(object)
        v = (a[:, 0] + (a[:, 1] << 64) + (a[:, 2] << 128) + (a[:, 3] << 192)) * r_inv % p
        return np.stack([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], axis=1).astype(np.uint64)

    def to_mont(c):
        a = c.astype(object)
        v = ((a[:, 0] + (a[:, 1] << 64) + (a[:, 2] << 128) + (a[:, 3] << 192)) << 256) % p
        return np.stack([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], axis=1).astype(np.uint64)

    order = lambda c: np.lexsort((c[:, 0], c[:, 1], c[:, 2], c[:, 3]))     # most significant limb last = primary key
    ci, ct = canon(inputs_mont), canon(table_mont)
    a = ci[order(ci)]
    t = ct[order(ct)]
    first = np.ones(usable_rows, dtype=bool)
    first[1:] = (a[1:] != a[:-1]).any(axis=1)
    # the table's multiset: unique values and counts (t is sorted)
    tb = np.ones(len(t), dtype=bool)
    tb[1:] = (t[1:] != t[:-1]).any(axis=1)
    tvals = t[tb]
    tcnt = np.diff(np.append(np.flatnonzero(tb), len(t)))
    key = lambda c: [tuple(int(x) for x in row[::-1]) for row in c]
    index = {k: i for i, k in enumerate(key(tvals))}
    for k in key(a[first]):
        i = index.get(k)
        if i is None or tcnt[i] == 0:
            raise ValueError("ConstraintSystemFailure: a lookup input is not in the table")
        tcnt[i] -= 1
    s_perm = np.zeros((usable_rows, 4), dtype=np.uint64)
    s_perm[first] = a[first]
    leftovers = np.repeat(tvals, tcnt, axis=0)                     # ascending
    repeated = np.flatnonzero(~first)
    assert len(leftovers) == len(repeated)
    s_perm[repeated[::-1]] = leftovers                              # upstream pops the repeated rows from the last one down
    return to_mont(a), to_mont(s_perm)


def permute_expression_pair_device(field, inputs, table, usable_rows, a_out=None, s_out=None, stream=0):
    """permute_expression_pair on device buffers (zk_halo2_permute_expression_pair_device): rows [0, usable_rows) of the
    Montgomery columns `inputs` and `table` in, (A', S') out -- rows [0, usable_rows) written, later rows left alone.  Outputs
    of usable_rows rows are allocated beside the inputs when none are given.  Raises ValueError where upstream returns
    ConstraintSystemFailure, like the host routine above."""
    def alloc():
        if isinstance(inputs, np.ndarray):
            return np.zeros((usable_rows, 4), dtype=np.uint64)
        import torch
        return torch.empty((usable_rows, 4), dtype=torch.int64, device=inputs.device)
    a_out = alloc() if a_out is None else a_out
    s_out = alloc() if s_out is None else s_out
    st = _plib().zk_halo2_permute_expression_pair_device(field_id(field), _ptr(inputs), _ptr(table), int(usable_rows), _ptr(a_out), _ptr(s_out),
                                                          ctypes.c_void_p(stream))
    if st == ZK_ERR_LOOKUP:
        raise ValueError("ConstraintSystemFailure: a lookup input is not in the table")
    _check(st, "zk_halo2_permute_expression_pair_device")
    return a_out, s_out


def batch_invert(field, a, stream=0):
    """arithmetic.rs BatchInvert on a device buffer, in place; zeros stay zero"""
    _call("zk_batch_invert_device", field_id(field), _ptr(a), int(a.shape[0]), ctypes.c_void_p(stream))
    return a


def prefix_product(field, a, out=None, first=None, want_total=False, stream=0):
    """out[i] = first * prod_{j<i} a[j] (in place when out is None) -> out, or (out, total)"""
    out = a if out is None else out
    tot = np.zeros(4, dtype=np.uint64)
    _call("zk_prefix_product_device", field_id(field), _ptr(a), _ptr(out), int(a.shape[0]), _ptr(_np64(first)) if first is not None else None,
          _ptr(tot) if want_total else None, ctypes.c_void_p(stream))
    return (out, tot) if want_total else out


def permutation_product(field, columns, sigmas, beta, gamma, delta, k, z_out, first_column_index=0, z_first=None, stream=0):
    """plonk/permutation/prover.rs Argument::commit, one chunk (<= 8 columns): fills z_out with Z and returns the value
    after the last row (the next chunk's z_first)"""
    last = np.zeros(4, dtype=np.uint64)
    keep = [_np64(x) for x in (beta, gamma, delta)]
    zf = _np64(z_first) if z_first is not None else None
    _call("zk_halo2_permutation_product_device", field_id(field), len(columns), _ptr_array(columns), _ptr_array(sigmas), first_column_index,
          _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), k, _ptr(zf) if zf is not None else None, _ptr(z_out), _ptr(last), ctypes.c_void_p(stream))
    return last


def lookup_product(field, a, s, a_perm, s_perm, beta, gamma, z_out, stream=0):
    """plonk/lookup/prover.rs commit_product; returns Z after the last row (must be 1 for a valid lookup)"""
    last = np.zeros(4, dtype=np.uint64)
    keep = [_np64(beta), _np64(gamma)]
    _call("zk_halo2_lookup_product_device", field_id(field), _ptr(a), _ptr(s), _ptr(a_perm), _ptr(s_perm), _ptr(keep[0]), _ptr(keep[1]),
          int(a.shape[0]), _ptr(z_out), _ptr(last), ctypes.c_void_p(stream))
    return last


def inner_product(field, a, b, stream=0):
    out = np.zeros(4, dtype=np.uint64)
    _call("zk_inner_product_device", field_id(field), _ptr(a), _ptr(b), int(a.shape[0]), _ptr(out), ctypes.c_void_p(stream))
    return out


def vec_muladd(field, a, b, s, stream=0, out=None):
    """a[i] = a[i] * s + b[i] (multiopen: folding the polynomials of a point set with powers of x_1); out: write there instead
    and leave a alone (upstream clones the first polynomial of a fold)"""
    ss = _np64(s)
    if out is not None:
        _call("zk_vec_muladd_to_device", field_id(field), _ptr(out), _ptr(a), _ptr(b), int(a.shape[0]), _ptr(ss), ctypes.c_void_p(stream))
        return out
    _call("zk_vec_muladd_device", field_id(field), _ptr(a), _ptr(b), int(a.shape[0]), _ptr(ss), ctypes.c_void_p(stream))
    return a


def eval_polynomial(field, d_poly, x, stream=0):
    """arithmetic.rs eval_polynomial: p(x) for a device-resident coefficient vector; x, result: Montgomery limbs"""
    xx = _np64(x)
    out = np.zeros(4, dtype=np.uint64)
    _call("zk_poly_eval_device", field_id(field), _ptr(d_poly), int(d_poly.shape[0]), _ptr(xx), _ptr(out), ctypes.c_void_p(stream))
    return out


def eval_polynomials(field, d_polys, x, stream=0):
    """d_polys: device buffer [count, n, 4]; every polynomial at the same x in one launch -> [count, 4]"""
    xx = _np64(x)
    count, n = int(d_polys.shape[0]), int(d_polys.shape[1])
    out = np.zeros((count, 4), dtype=np.uint64)
    _call("zk_poly_eval_batch_device", field_id(field), _ptr(d_polys), n, count, n, _ptr(xx), _ptr(out), ctypes.c_void_p(stream))
    return out


def vec_fold_many(field, out, polys, s, stream=0, reverse=False):
    """out[j] = sum_i s^(count - 1 - i) polys[i][j] (Horner over the rows of `polys` [count, n, 4], one pass); reverse: walk the rows
    from the last to the first (h(X) = sum_i (x^n)^i h_i: the last piece is the leading one)"""
    ss = _np64(s)
    count, n = int(polys.shape[0]), int(polys.shape[1])
    first = polys[count - 1] if reverse else polys[0]
    _call("zk_vec_fold_many_device", field_id(field), _ptr(out), _ptr(first), -n if reverse else n, count, n, _ptr(ss), ctypes.c_void_p(stream))
    return out


def ipa_fold_round(field, p, b, half, u, w=None, m0=0, stream=0):
    """the three folds of one argument round in one launch (w: the fold-free form's weight vector over m0 generators)"""
    uu = _np64(u)
    _call("zk_ipa_fold_round_device", field_id(field), _ptr(p), _ptr(b), _ptr(w) if w is not None else None, half, m0, _ptr(uu),
          ctypes.c_void_p(stream))


def vec_powers(field, out, x, stream=0):
    """out[i] = x^i (the vector b of the inner-product argument: powers of x_3)"""
    xx = _np64(x)
    _call("zk_vec_powers_device", field_id(field), _ptr(out), int(out.shape[0]), _ptr(xx), ctypes.c_void_p(stream))
    return out


def kate_division(field, a, x, out=None, stream=0):
    """arithmetic.rs kate_division: (a(X) - a(x)) / (X - x) as len(a) coefficients (the last one zero: upstream returns one fewer
    and the multiopen prover resizes); in place unless `out` is given"""
    xx = _np64(x)
    out = a if out is None else out
    _call("zk_kate_division_device", field_id(field), _ptr(a), _ptr(out), int(a.shape[0]), _ptr(xx), ctypes.c_void_p(stream))
    return out


def vec_fold(field, a, half, c, stream=0):
    """a[i] += c a[i + half] for i < half"""
    cc = _np64(c)
    _call("zk_vec_fold_device", field_id(field), _ptr(a), half, _ptr(cc), ctypes.c_void_p(stream))
    return a


def ipa_fold_bases(curve, g, half, u, stream=0):
    """parallel_generator_collapse: g[i] <- affine(g[i] + [u] g[i + half]); g: device buffer [2 * half, 2 * limbs]"""
    uu = _np64(u)
    _call("zk_ipa_fold_bases_device", curve_id(curve), _ptr(g), half, _ptr(uu), ctypes.c_void_p(stream))
    return g


def _expr_ops(program):
    """the program as zk_expr_op records.  ctypes truncates an out-of-range integer without an error (a rotation of 40000 would
    become -25536 in the int16 field), so every field is range-checked here first: a program that cannot be written as it is
    stated is refused, never evaluated as a different one"""
    ops = (ExprOp * len(program))()
    for k, o in enumerate(program):
        if not isinstance(o, (tuple, list)) or not o or o[0] not in EXPR_CODES or len(o) != {"col": 3, "const": 2, "scale": 2}.get(o[0], 1):
            raise ZkError(ZK_ERR_INVALID_ARG, "expression op %d %r" % (k, o))
        arg, rot = (int(o[1]) if len(o) > 1 else 0), (int(o[2]) if len(o) > 2 else 0)
        if not 0 <= arg < 1 << 32 or not -(1 << 15) <= rot < 1 << 15:
            raise ZkError(ZK_ERR_INVALID_ARG, "expression op %d %r: index or rotation out of range" % (k, o))
        ops[k].op, ops[k].rot, ops[k].arg = EXPR_CODES[o[0]], rot, arg
    return ops


def evaluate_expression(field, program, columns, consts, log_n_ext, rot_scale, out, stream=0, lazy=False):
    """program: list of ("col", column, rotation) / ("const", i) / ("add",) / ("sub",) / ("mul",) / ("neg",) / ("scale", i).
    lazy: the columns hold x R' mod p (coeff_to_extended(..., lazy_out=True) / to_lazy_form) and the evaluation runs on lazy
    29-bit limbs; constants and the output stay in the usual Montgomery form"""
    ops = _expr_ops(program)
    cs = _np64(consts).reshape(-1, 4) if len(consts) else np.zeros((1, 4), dtype=np.uint64)
    _call("zk_expr_eval_lazy_device" if lazy else "zk_expr_eval_device", field_id(field), ops, len(program), _ptr_array(columns), len(columns),
          _ptr(cs), len(consts), log_n_ext, rot_scale, _ptr(out), ctypes.c_void_p(stream))
    return out


def expr_configure(jit="auto"):
    """zk_expr_configure: the lazy evaluator's specialised (hiprtc-compiled) kernel: "auto" (2^16 rows and more), "always", "never" """
    _call("zk_expr_configure", {"auto": 0, "always": 1, "never": 2}[jit])


def expr_specialised_source(field, program, n_columns, n_consts):
    """the HIP source of the kernel zk_expr_eval_lazy_device compiles for `program` (no device needed)"""
    ops = _expr_ops(program)
    n = ctypes.c_uint64(0)
    fid = field_id(field)
    _check(_plib().zk_expr_specialised_source(fid, ops, len(program), n_columns, n_consts, None, 0, ctypes.byref(n)), "zk_expr_specialised_source")
    buf = ctypes.create_string_buffer(n.value + 1)
    _check(_plib().zk_expr_specialised_source(fid, ops, len(program), n_columns, n_consts, buf, n.value + 1, ctypes.byref(n)), "zk_expr_specialised_source")
    return buf.value.decode()


def to_lazy_form(field, a, stream=0):
    """x R -> x R' (R' = 2^261 for the 256-bit fields: times 2^5) in place: key material (fixed columns on the extended coset) for
    evaluate_expression(lazy=True)"""
    p = field_modulus(field)
    return vec_op(field, "scale", a, scalar=_mont_limbs(32, p), stream=stream)


class IpaProver:
    """poly/commitment/prover.rs create_proof, the k rounds of the inner-product argument on device buffers.  The caller
    owns the transcript: `round()` returns L_j, R_j (before the U / W blinding terms) and <p'_hi, b_lo>, <p'_lo, b_hi>;
    after hashing them into its transcript the caller feeds the challenge to `fold(u_j)`."""

    def __init__(self, curve, d_p, d_b, d_g, stream=0):
        """d_p, d_b: device buffers [n, 4] (p' coefficients and the powers of x_3, Montgomery); d_g: [n, 2 * limbs] affine
        generators (a working copy: it is folded in place).  The generator vector is adopted ONCE as a bases handle; every
        round's two MSMs address its halves through zk_msm_opts.base_offset, and the fold refreshes the handle's derived
        copy for the half that survives."""
        self.curve, self.field = curve_id(curve), scalar_field(curve)
        self.p, self.b, self.g, self.stream = d_p, d_b, d_g, stream
        self.n = int(d_p.shape[0])
        assert self.n & (self.n - 1) == 0 and int(d_b.shape[0]) == self.n and int(d_g.shape[0]) == self.n
        self.bases = Bases(self.curve, device_tensor=d_g, n=self.n)

    def round(self, sharded=False):
        """sharded: every rank of a torch.distributed job holds the same p', b, G' and sums its own scalar windows of the
        two MSMs; one all_gather combines them (contangle-zkcp_amd/dist.py)"""
        half = self.n // 2
        if sharded:
            from . import dist as zkdist
            L, R = zkdist.msm_many_sharded([(self.bases, self.p[half:self.n], True, 0), (self.bases, self.p[:half], True, half)], stream=self.stream)
        else:
            tl = msm_submit(self.bases, self.p[half:self.n], montgomery=True, stream=self.stream)                    # L = <p'_hi, G'_lo>
            tr = msm_submit(self.bases, self.p[:half], montgomery=True, stream=self.stream, base_offset=half)        # R = <p'_lo, G'_hi>
        vl = inner_product(self.field, self.p[half:self.n], self.b[:half], stream=self.stream)
        vr = inner_product(self.field, self.p[:half], self.b[half:self.n], stream=self.stream)
        if not sharded:
            L, R = tl.collect(), tr.collect()
        return L, R, vl, vr

    def fold(self, u):
        half = self.n // 2
        vec_fold(self.field, self.p, half, field_inverse(self.field, u), stream=self.stream)
        vec_fold(self.field, self.b, half, u, stream=self.stream)
        ipa_fold_bases(self.curve, self.g, half, u, stream=self.stream)
        self.bases.refresh(0, half, stream=self.stream)
        self.n = half

    def free(self):
        self.bases.free()


class IpaProverVirtual:
    """The same argument with the generators left alone: every round's L, R are MSMs over the ORIGINAL generators (a resident
    `Bases`, e.g. the SRS itself) with scalars p'[i] W[idx]; W collects the challenges.  2 n-point MSMs (half of the scalars
    zero) per round in one batched call, instead of a 255-bit scalar multiplication per surviving generator.

    `collapse()` materialises the generators that the rounds so far would have left (zk_ipa_collapse_device: the
    surviving points as multi-scalar multiplications that share their scalars) and continues over them: the first rounds
    cost one full-size MSM each, the remaining ones only what their own size costs."""

    def __init__(self, curve, d_p, d_b, bases, new_buffer, stream=0, buffers=None):
        """new_buffer(shape) -> zero device buffer (torch on the GPU, numpy under the test emulator).
        buffers = (S [2, n, 4], W [n, 4]): caller-owned scratch reused across proofs (no allocation inside the argument);
        every entry is rewritten on the stream before it is read"""
        self.curve, self.field = curve_id(curve), scalar_field(curve)
        self.p, self.b, self.bases, self.stream = d_p, d_b, bases, stream
        self.new_buffer = new_buffer
        self.m0 = self.n = int(d_p.shape[0])
        assert self.n & (self.n - 1) == 0 and int(d_b.shape[0]) == self.n and bases.n >= self.n
        self._own_bases = None
        self._g = None
        self._buffers = buffers
        if buffers is not None:
            assert int(buffers[0].shape[0]) == 2 and int(buffers[0].shape[1]) >= self.n and int(buffers[1].shape[0]) >= self.n
        self._fresh_weights()

    def _fresh_weights(self):
        one = _mont_limbs(1, field_modulus(self.field))
        if self._buffers is not None:       # prefixes of the caller's buffers; W = 1 everywhere as the powers of 1, on the stream
            self.S = self._buffers[0].reshape(-1)[: 2 * self.m0 * 4].reshape(2, self.m0, 4)
            self.W = self._buffers[1][: self.m0]
            vec_powers(self.field, self.W, one, stream=self.stream)
            return
        self.S = self.new_buffer((2, self.m0, 4))
        self.W = self.new_buffer((self.m0, 4))
        ones = np.tile(one, (self.m0, 1))
        if isinstance(self.W, np.ndarray):
            self.W[:] = ones
        else:
            import torch
            self.W.copy_(torch.from_numpy(ones.view(np.int64)))

    def round(self, sharded=False):
        half = self.n // 2
        if sharded:
            from . import dist as zkdist
            sharded = self.m0 >= zkdist.SHARD_MIN_POINTS      # small rounds: every rank computes them whole, no collective
        if not sharded:     # the whole round in one call: scalars, inner products and both MSMs enqueued together
            nl = _plib().zk_curve_base_limbs64(self.curve)
            lr = np.zeros((2, 3 * nl), dtype=np.uint64)
            v = np.zeros((2, 4), dtype=np.uint64)
            _call("zk_ipa_round_device", self.curve, self.bases.handle, _ptr(self.p), _ptr(self.b), _ptr(self.W), self.m0, self.n, _ptr(self.S),
                  _ptr(lr), _ptr(v), ctypes.c_void_p(self.stream))
            return lr[0], lr[1], v[0], v[1]
        _call("zk_ipa_virtual_scalars_device", self.field, _ptr(self.p), _ptr(self.W), self.m0, self.n, _ptr(self.S[0]), _ptr(self.S[1]),
              ctypes.c_void_p(self.stream))
        L, R = zkdist.msm_batch_sharded(self.bases, self.S, montgomery=True, stream=self.stream)
        vl = inner_product(self.field, self.p[half:self.n], self.b[:half], stream=self.stream)
        vr = inner_product(self.field, self.p[:half], self.b[half:self.n], stream=self.stream)
        return L, R, vl, vr

    def fold(self, u):
        half = self.n // 2
        if half < self.m0:
            ipa_fold_round(self.field, self.p, self.b, half, u, w=self.W, m0=self.m0, stream=self.stream)
        else:      # (a single generator left over: nothing to weight)
            ipa_fold_round(self.field, self.p, self.b, half, u, stream=self.stream)
        self.n = half

    def collapse(self, sharded=False):
        """G' of the rounds done so far, as a device buffer [n, 2 * limbs] of affine points; the later rounds run over it.
        sharded: the ranks of a torch.distributed job (all holding the same state) compute n / world survivors each and
        exchange them with one all_gather."""
        nl = _plib().zk_curve_base_limbs64(self.curve)
        g = self.new_buffer((self.n, 2 * nl))
        world, rank = 1, 0
        if sharded:
            import torch.distributed as tdist
            if tdist.is_initialized():
                world, rank = tdist.get_world_size(), tdist.get_rank()
        if world > 1 and self.n % world == 0 and self.n // world >= 64:
            import torch
            share = self.n // world
            mine = g[rank * share:(rank + 1) * share]
            _call("zk_ipa_collapse_range_device", self.curve, self.bases.handle, _ptr(self.W), self.m0, self.n, rank * share, share, _ptr(mine),
                  ctypes.c_void_p(self.stream))
            # (the call above synchronises the stream: `mine` is complete)
            if isinstance(g, np.ndarray):                                   # the CPU test emulator: "device" memory is host memory
                t = torch.from_numpy(np.ascontiguousarray(mine).view(np.int64))
                outs = [torch.empty_like(t) for _ in range(world)]
                tdist.all_gather(outs, t)
                for r, o in enumerate(outs):
                    g[r * share:(r + 1) * share] = o.numpy().view(np.uint64).reshape(share, 2 * nl)
            elif tdist.get_backend() == "nccl":                             # RCCL over xGMI, device to device (the same
                t = mine.reshape(-1).clone()                                # all_gather form as dist._gather_add)
                outs = [torch.empty_like(t) for _ in range(world)]
                tdist.all_gather(outs, t)
                g.view(-1).copy_(torch.cat(outs))
                torch.cuda.synchronize()                                    # g is adopted as a bases handle next (another stream)
            else:                                                           # gloo rehearsal on a GPU box: staged through the host
                t = mine.cpu()
                outs = [torch.empty_like(t) for _ in range(world)]
                tdist.all_gather(outs, t)
                g.copy_(torch.cat(outs).to(g.device))
                torch.cuda.synchronize()
        else:
            _call("zk_ipa_collapse_device", self.curve, self.bases.handle, _ptr(self.W), self.m0, self.n, _ptr(g), ctypes.c_void_p(self.stream))
        if self._own_bases is not None:
            self._own_bases.free()
        self._g = g                                   # adopted, not copied: kept alive here
        self._own_bases = self.bases = Bases(self.curve, device_tensor=g, n=self.n)
        self.m0 = self.n
        self._fresh_weights()
        return g

    def free(self):
        if self._own_bases is not None:
            self._own_bases.free()
            self._own_bases = None

    def folded_generator(self):
        """G' after the rounds so far are all done (n == 1): MSM(G0, W) -- what upstream's collapsed g_prime[0] is"""
        return msm(self.bases, self.W, montgomery=True, stream=self.stream)


# ------------------------------------------------------------------ key generation (plonk/keygen.rs, plonk/permutation/keygen.rs)
def delta(field):
    """pasta_curves 0.4 `FieldExt::DELTA` = GENERATOR^(2^S), S the field's two-adicity (generator 5, S = 32 on both Pasta fields):
    a generator of the odd-order subgroup, so the cosets delta^c H label the permutation argument's columns.  Montgomery limbs --
    the `delta` argument of permutation_product."""
    p = field_modulus(field)
    g = multiplicative_generator(field)
    gi = sum(int(w) << (64 * i) for i, w in enumerate(g.tolist())) * pow(1 << 256, -1, p) % p
    s = ((p - 1) & -(p - 1)).bit_length() - 1
    return _mont_limbs(pow(gi, 1 << s, p), p)


class BoundsFailure(ValueError):
    """upstream's Error::BoundsFailure from Assembly::copy; `applied` = how many copies of the call went in before it"""

    def __init__(self, applied):
        ValueError.__init__(self, "BoundsFailure: copy %d names a row or a column outside the permutation" % applied)
        self.applied = applied


class Assembly:
    """plonk/permutation/keygen.rs Assembly over `ncols` columns of `n` rows: Assembly::new's identity mapping, then `copy` in the
    caller's order -- the permutation depends on that order and is upstream's, cell for cell (the larger cycle absorbs the smaller,
    the left one on a tie; mapping[left] and mapping[right] are swapped).  Lives in host memory inside the library: the walk of a
    cycle is sequential by definition, and a Python loop per copy would take minutes at 2^24 cells.  Columns are the indices of
    the permutation argument's column list (upstream looks the Column up there).  Which cells a circuit copies -- synthesis and
    floor planning -- is the caller's business."""

    def __init__(self, n, ncols):
        h = ctypes.c_uint64(0)
        _call("zk_halo2_assembly_new", int(n), int(ncols), ctypes.byref(h))
        self.handle, self.n, self.ncols = h.value, int(n), int(ncols)

    def copy(self, left_column, left_row, right_column, right_row):
        self.copy_many([(left_column, left_row, right_column, right_row)])

    def copy_many(self, quads):
        """quads: [count, 4] (left_column, left_row, right_column, right_row), applied in order; the first one out of bounds raises
        BoundsFailure (its .applied = the number applied before it; the rest are not looked at).  Returns the number applied."""
        # a value that does not fit 32 bits is out of bounds, not another cell: it becomes 2^32 - 1, which no assembly has
        if isinstance(quads, np.ndarray) and quads.dtype.kind in "iu":
            q = quads.reshape(-1, 4)
            if q.dtype != np.uint32:
                q = q if q.dtype == np.uint64 else q.astype(np.int64)
                q = np.where((q < 0) | (q > 0xFFFFFFFF), 0xFFFFFFFF, q).astype(np.uint32)
        else:
            q = np.array([[v if 0 <= v < 1 << 32 else 0xFFFFFFFF for v in map(int, quad)] for quad in quads], dtype=np.uint32).reshape(-1, 4)
        q = np.ascontiguousarray(q)
        done = ctypes.c_uint64(0)
        st = _plib().zk_halo2_assembly_copy(self.handle, _ptr(q), int(q.shape[0]), ctypes.byref(done))
        if st == ZK_ERR_INVALID_ARG:
            raise BoundsFailure(done.value)
        _check(st, "zk_halo2_assembly_copy")
        return done.value

    def mapping(self):
        """[ncols, n] uint64, mapping[c][r] = column << 32 | row of the cell (c, r) maps to"""
        out = np.zeros((self.ncols, self.n), dtype=np.uint64)
        _call("zk_halo2_assembly_mapping", self.handle, _ptr(out))
        return out

    def free(self):
        if self.handle:
            _call("zk_halo2_assembly_free", self.handle)
            self.handle = 0


def permutation_sigmas(field, k, mapping, sigmas=None, stream=0):
    """Assembly::build_vk / build_pk, the columns themselves: sigmas[c][j] = DELTA^col omega^row for mapping[c][j] = col << 32 | row
    (zk_halo2_permutation_sigmas_device).  mapping: [ncols, 2^k] uint64, host (uploaded) or device; sigmas: device [ncols, 2^k, 4],
    allocated when not given.  A mapping that names a cell outside the ncols x 2^k grid raises ZkError(ZK_ERR_INVALID_ARG)."""
    from .groth16 import _new_buffer, _upload
    ncols, n = int(mapping.shape[0]), int(mapping.shape[1])
    if n != 1 << k:
        raise AssertionError("assertion failed: mapping.len() == 1 << k")
    d_map = _upload(mapping) if isinstance(mapping, np.ndarray) else mapping
    sigmas = _new_buffer((ncols, n, 4)) if sigmas is None else sigmas
    dl = delta(field)
    _call("zk_halo2_permutation_sigmas_device", field_id(field), int(k), ncols, _ptr(d_map), _ptr(dl), _ptr(sigmas), ctypes.c_void_p(stream))
    return sigmas


class PermutationVerifyingKey:
    """plonk/permutation.rs VerifyingKey: commitments[c] = commit_lagrange(permutations[c]), host, Jacobian like msm()"""

    def __init__(self, commitments):
        self.commitments = commitments


class PermutationProvingKey:
    """plonk/permutation.rs ProvingKey, resident: permutations [ncols, n, 4] (Lagrange; the `sigmas` of permutation_product as it
    is), polys [ncols, n, 4] (coefficients), cosets [ncols, extended_len, 4] or None"""

    def __init__(self, permutations, polys, cosets):
        self.permutations, self.polys, self.cosets = permutations, polys, cosets


class VerifyingKey:
    """plonk.rs VerifyingKey, the computed part: domain, fixed_commitments, permutation.commitments.  Upstream commits with
    Blind::default(), which adds [1] W; `Params` here leaves w to the caller, so every commitment is the multi-scalar part only
    (add W to each for upstream's points).  The key's transcript representation (hashing it into the transcript) is not built."""

    def __init__(self, domain, fixed_commitments, permutation, blinding_factors):
        self.domain, self.fixed_commitments, self.permutation, self.blinding_factors = domain, fixed_commitments, permutation, blinding_factors


class ProvingKey:
    """plonk.rs ProvingKey, resident on the device: fixed_values / fixed_polys [nfixed, n, 4], fixed_cosets [nfixed, extended_len, 4],
    permutation (PermutationProvingKey), l0 / l_last / l_active_row [extended_len, 4] (None with cosets=None) and their
    coefficient forms l0_poly / l_last_poly / l_active_row_poly [n, 4] (not kept upstream; a prover that evaluates the quotient
    sub-coset by sub-coset extends from them)"""

    def __init__(self, vk):
        self.vk = vk
        self.fixed_values = self.fixed_polys = self.fixed_cosets = self.permutation = None
        self.l0 = self.l_last = self.l_active_row = self.l0_poly = self.l_last_poly = self.l_active_row_poly = None

    def free(self):
        """drop the resident buffers"""
        ProvingKey.__init__(self, self.vk)


def _fixed_values(field, n, fixed):
    """the fixed columns as one resident [nfixed, n, 4] buffer; a (numerators, denominators) pair is batch_invert_assigned's
    num / den with a zero denominator giving 0"""
    from .groth16 import _new_buffer, _upload

    def check(a):
        if int(a.shape[0]) != n:
            raise AssertionError("assertion failed: a.values.len() == 1 << self.k")
        return a

    def store(dst, src):
        if isinstance(dst, np.ndarray):
            dst[:] = _np64(src)
        elif isinstance(src, np.ndarray):
            import torch
            dst.copy_(torch.from_numpy(_np64(src).view(np.int64)))
        else:
            dst.copy_(src)

    out = _new_buffer((max(len(fixed), 1), n, 4))[:len(fixed)]
    for i, col in enumerate(fixed):
        if isinstance(col, (tuple, list)):
            num, den = check(col[0]), check(col[1])
            store(out[i], den)
            batch_invert(field, out[i])
            vec_op(field, "mul", out[i], b=_upload(num) if isinstance(num, np.ndarray) else num)
        else:
            store(out[i], check(col))
    return out


def _keygen_checks(params, asm, blinding_factors):
    if asm.n != params.n:
        raise AssertionError("assertion failed: assembly.n == params.n")
    if params.n < blinding_factors + 3:          # upstream: cs.minimum_rows() -> Error::NotEnoughRowsAvailable
        raise ValueError("NotEnoughRowsAvailable: n = %d < blinding_factors + 3 = %d" % (params.n, blinding_factors + 3))


def keygen_vk(params, degree, fixed, asm, blinding_factors, stream=0):
    """plonk/keygen.rs keygen_vk after synthesis: `fixed` = the fixed columns (selectors already compressed into them by the caller;
    each a host or device [n, 4] Montgomery array, or a (numerators, denominators) pair of such -- upstream's Assigned cells),
    `asm` = the permutation Assembly, `degree` = cs.degree().  Commitments are computed on the device over params.g_lagrange and
    carry no blinding term (see VerifyingKey).  Out of scope: circuit synthesis and floor planning, compress_selectors, hashing
    g / w / u, the verifying key's transcript representation."""
    _keygen_checks(params, asm, blinding_factors)
    field = scalar_field(params.curve)
    domain = EvaluationDomain(field, degree, params.k)
    values = _fixed_values(field, params.n, fixed)
    nl = load().zk_curve_base_limbs64(params.curve)
    fixed_commitments = params.commit_lagrange_batch(values, stream=stream) if len(fixed) else np.zeros((0, 3 * nl), dtype=np.uint64)
    sigmas = permutation_sigmas(field, params.k, asm.mapping(), stream=stream)
    return VerifyingKey(domain, fixed_commitments, PermutationVerifyingKey(params.commit_lagrange_batch(sigmas, stream=stream)), blinding_factors)


def keygen_pk(params, vk, fixed, asm, cosets="mont", stream=0):
    """plonk/keygen.rs keygen_pk after synthesis, the key resident on the device (ProvingKey): fixed_values -> fixed_polys
    (lagrange_to_coeff) -> fixed_cosets (coeff_to_extended); the permutation columns likewise (Assembly::build_pk); l0 (row 0),
    l_last (row n - blinding_factors - 1) and l_active_row = 1 - (l_last + l_blind) on the extended coset.  l_active_row is
    computed as the extension of the active rows' indicator column: extension is linear and the constant 1 extends to 1, so that
    is the same polynomial and the same canonical values as upstream's pass over three extended vectors.
    cosets: "mont" = Montgomery form; "lazy" = the R' radix evaluate_expression(lazy=True) reads (ZK_NTT_OUT_R29; equal to
    to_lazy_form of the "mont" result); None = no extended forms at all (27 x 256 MB at k = 20, extended_k = 23: a prover that
    evaluates the quotient by sub-coset extends from the coefficient forms instead).
    Out of scope: circuit synthesis and floor planning, compress_selectors, hashing g / w / u, the key's transcript representation."""
    from .groth16 import _new_buffer
    if cosets not in ("mont", "lazy", None):
        raise ZkError(ZK_ERR_INVALID_ARG, "cosets must be \"mont\", \"lazy\" or None")
    bf = vk.blinding_factors
    _keygen_checks(params, asm, bf)
    field, domain, n = vk.domain.field, vk.domain, params.n
    ext = domain.extended_len()
    lazy = cosets == "lazy"

    def forms(values):
        count = int(values.shape[0])
        polys = _new_buffer((max(count, 1), n, 4))[:count]
        ext_forms = _new_buffer((max(count, 1), ext, 4))[:count] if cosets else None
        for i in range(count):
            domain.lagrange_to_coeff(values[i], stream=stream, out=polys[i])
            if cosets:
                domain.coeff_to_extended(ext_forms[i], stream=stream, coeffs=polys[i], lazy_out=lazy)
        return polys, ext_forms

    pk = ProvingKey(vk)
    pk.fixed_values = _fixed_values(field, n, fixed)
    pk.fixed_polys, pk.fixed_cosets = forms(pk.fixed_values)
    sigmas = permutation_sigmas(field, params.k, asm.mapping(), stream=stream)
    pk.permutation = PermutationProvingKey(sigmas, *forms(sigmas))
    one = _mont_limbs(1, field_modulus(field))
    ind = np.zeros((3, n, 4), dtype=np.uint64)
    ind[0, 0] = one                      # l0
    ind[1, n - bf - 1] = one             # l_last
    ind[2, :n - bf - 1] = one            # 1 - (l_last + l_blind): l_blind covers the last blinding_factors rows
    polys, ext_forms = forms(_fixed_values(field, n, list(ind)))
    pk.l0_poly, pk.l_last_poly, pk.l_active_row_poly = polys[0], polys[1], polys[2]
    if cosets:
        pk.l0, pk.l_last, pk.l_active_row = ext_forms[0], ext_forms[1], ext_forms[2]
    return pk


# ------------------------------------------------------------------ verification (poly/commitment/verifier.rs, poly/commitment/msm.rs)
IPA_S_MAX_COUNT = 8            # csrc/zk_ipa_verify_kernels.h: proofs per pass of zk_halo2_ipa_s_device (a larger count is chunked inside)


def _aligned16(a):
    """the array as contiguous uint64 limbs at a 16-byte aligned address (the host pointers of zk_halo2_ipa_s_device)"""
    a = _np64(a)
    if a.ctypes.data % 16 == 0:
        return a
    buf = np.empty(a.size + 2, dtype=np.uint64)
    off = (-buf.ctypes.data % 16) // 8
    out = buf[off:off + a.size].reshape(a.shape)
    out[...] = a
    return out


def _to_int(limbs, p):
    """Montgomery limbs -> the canonical Python integer"""
    return sum(int(w) << (64 * i) for i, w in enumerate(_np64(limbs).reshape(-1).tolist())) * pow(1 << 256, -1, p) % p


def compute_s(field, u, init, out=None, accumulate=False, stream=0):
    """verifier.rs compute_s for a batch (zk_halo2_ipa_s_device): out[i] (= or +=) sum_p init[p] prod_j u[p][j]^bit_(k-1-j)(i).
    u: [count, k, 4] (or [k, 4]) Montgomery host limbs, u[p][0] the first round's challenge; init: [count, 4] (or [4]).
    out: device buffer [2^k, 4], allocated (and then written, not accumulated into) when None.  One pass over `out`."""
    from .groth16 import _new_buffer
    uu = _np64(u)
    uu = uu.reshape(1, -1, 4) if uu.ndim == 2 else uu
    ii = _np64(init).reshape(-1, 4)
    count, k = int(uu.shape[0]), int(uu.shape[1])
    if int(ii.shape[0]) != count:
        raise ZkError(ZK_ERR_INVALID_ARG, "compute_s: one init per proof")
    if out is None:
        if not 0 < k <= 32:
            raise ZkError(ZK_ERR_INVALID_ARG, "compute_s: k")
        out, accumulate = _new_buffer((1 << k, 4)), False
    elif int(out.shape[0]) != 1 << k:
        raise AssertionError("assertion failed: s.len() == 1 << k")
    uu, ii = _aligned16(uu), _aligned16(ii)
    _call("zk_halo2_ipa_s_device", field_id(field), k, count, _ptr(uu), _ptr(ii), _ptr(out), int(bool(accumulate)), ctypes.c_void_p(stream))
    return out


def compute_b(field, x, u):
    """verifier.rs compute_b(x, u) = prod_j (1 + u_j x^(2^(k-1-j))) on host limbs (zk_halo2_ipa_compute_b); u: [k, 4]"""
    uu, xx = _np64(u).reshape(-1, 4), _np64(x)
    out = np.zeros(4, dtype=np.uint64)
    _call("zk_halo2_ipa_compute_b", field_id(field), int(uu.shape[0]), _ptr(xx), _ptr(uu), _ptr(out))
    return out


class MSM:
    """poly/commitment/msm.rs MSM<C>: a multi-scalar multiplication that is still being put together.  g_scalars lives on the
    device ([n, 4] Montgomery, None until first needed, upstream's Option) because the opening check adds n scalars to it and
    the SRS it multiplies is resident; w_scalar, u_scalar (None = upstream's None) and the listed terms are a handful of host
    values, kept as Python integers.  Scalars come in as Montgomery limbs, points as affine Montgomery host limbs."""

    def __init__(self, params, stream=0):
        self.params, self.stream = params, stream
        self.field = scalar_field(params.curve)
        self.p = field_modulus(self.field)
        self.g_scalars = None
        self.w_scalar = self.u_scalar = None
        self.other_scalars, self.other_bases = [], []

    def _g(self):
        if self.g_scalars is None:
            from .groth16 import _new_buffer
            self.g_scalars = _new_buffer((self.params.n, 4))
        return self.g_scalars

    def _int(self, s):
        return s % self.p if isinstance(s, int) else _to_int(s, self.p)

    def append_term(self, scalar, point):
        self.other_scalars.append(self._int(scalar))
        self.other_bases.append(_np64(point).copy())

    def add_constant_term(self, constant):
        """g_scalars[0] += constant: a one-element zk_vec_op_device on the head of the resident vector"""
        from .groth16 import _upload
        c = _mont_limbs(self._int(constant), self.p).reshape(1, 4)
        vec_op(self.field, "add", self._g()[:1], b=_upload(c), stream=self.stream)

    def add_to_g_scalars(self, scalars):
        """scalars: device buffer [n, 4]"""
        if int(scalars.shape[0]) != self.params.n:
            raise AssertionError("assertion failed: scalars.len() == self.params.n")
        vec_op(self.field, "add", self._g(), b=scalars, stream=self.stream)

    def add_to_w_scalar(self, scalar):
        self.w_scalar = ((self.w_scalar or 0) + self._int(scalar)) % self.p

    def add_to_u_scalar(self, scalar):
        self.u_scalar = ((self.u_scalar or 0) + self._int(scalar)) % self.p

    def scale(self, factor):
        f = self._int(factor)
        if self.g_scalars is not None:
            vec_op(self.field, "scale", self.g_scalars, scalar=_mont_limbs(f, self.p), stream=self.stream)
        self.other_scalars = [s * f % self.p for s in self.other_scalars]
        if self.w_scalar is not None:
            self.w_scalar = self.w_scalar * f % self.p
        if self.u_scalar is not None:
            self.u_scalar = self.u_scalar * f % self.p

    def add_msm(self, other):
        self.other_scalars += other.other_scalars
        self.other_bases += [b.copy() for b in other.other_bases]
        if other.g_scalars is not None:
            self.add_to_g_scalars(other.g_scalars)
        if other.w_scalar is not None:
            self.add_to_w_scalar(other.w_scalar)
        if other.u_scalar is not None:
            self.add_to_u_scalar(other.u_scalar)

    def eval(self):
        """true when sum other + [w_scalar] W + [u_scalar] U + sum_i [g_scalars[i]] G_i is the identity: ONE zk_msm_device over
        params.g with the resident g_scalars, one small host-scalar MSM over the listed terms, U and W, and the sum and the
        identity test on host limbs"""
        from . import point_add, point_to_affine
        scalars, bases = list(self.other_scalars), list(self.other_bases)
        for s, pt, name in ((self.w_scalar, self.params.w, "w"), (self.u_scalar, self.params.u, "u")):
            if s is not None:
                if pt is None:
                    raise ZkError(ZK_ERR_INVALID_ARG, "MSM.eval: the params carry no %s" % name)
                scalars.append(s)
                bases.append(pt)
        nl = load().zk_curve_base_limbs64(self.params.curve)
        acc = np.zeros(3 * nl, dtype=np.uint64)                    # z = 0: the identity
        if self.g_scalars is not None:
            acc = msm(self.params.g, self.g_scalars, montgomery=True, stream=self.stream)
        if scalars:
            small = Bases(self.params.curve, np.stack(bases))
            try:
                part = msm(small, np.stack([_mont_limbs(s, self.p) for s in scalars]), montgomery=True)
            finally:
                small.free()
            acc = point_add(self.params.curve, acc, part)
        return not point_to_affine(self.params.curve, acc).any()


class IpaProof:
    """the opening proof in transcript order: S, then xi, z, then (L_j, R_j, u_j) for each of the k rounds, then c, f.  Points
    are affine Montgomery host limbs, scalars Montgomery limbs; the challenges are the ones the caller's transcript squeezed."""

    def __init__(self, s_commitment, xi, z, rounds, c, f):
        self.s_commitment, self.xi, self.z, self.rounds, self.c, self.f = s_commitment, xi, z, list(rounds), c, f


class Accumulator:
    """verifier.rs Accumulator: the claimed folded generator g and the challenges that a later compute_g must reproduce"""

    def __init__(self, g, challenges_packed):
        self.g, self.challenges_packed = g, challenges_packed


class Guard:
    """verifier.rs Guard: the verifier's state before the one linear-time step, which is either done here (use_challenges) or
    deferred behind a claimed g (use_g; compute_g is what checks such a claim later)"""

    def __init__(self, msm_, neg_c, challenges):
        self.msm, self.neg_c, self.challenges = msm_, neg_c, challenges      # neg_c: Python integer; challenges: [k, 4] Montgomery

    def use_challenges(self):
        """msm.add_to_g_scalars(compute_s(u, neg_c)), fused: the kernel adds into the resident g_scalars in its one pass"""
        m = self.msm
        fresh = m.g_scalars is None
        compute_s(m.field, self.challenges, _mont_limbs(self.neg_c, m.p), out=m._g(), accumulate=not fresh, stream=m.stream)
        return m

    def use_g(self, g):
        self.msm.append_term(self.neg_c, g)
        return self.msm, Accumulator(_np64(g).copy(), self.challenges)

    def compute_g(self):
        """best_multiexp(compute_s(u, 1), params.g) as an affine point"""
        from . import point_to_affine
        m = self.msm
        s = compute_s(m.field, self.challenges, _mont_limbs(1, m.p), stream=m.stream)
        return point_to_affine(m.params.curve, msm(m.params.g, s, montgomery=True, stream=m.stream))


def _proof_challenges(params, msm_, proof):
    """-> (u as integers, u as [k, 4] limbs); the round count and u_j != 0 checked"""
    if len(proof.rounds) != params.k:
        raise ZkError(ZK_ERR_INVALID_ARG, "verify_proof: %d rounds for k = %d" % (len(proof.rounds), params.k))
    limbs = np.stack([_np64(r[2]) for r in proof.rounds])
    ints = [_to_int(r[2], msm_.p) for r in proof.rounds]
    if not all(ints):
        raise ZkError(ZK_ERR_INVALID_ARG, "verify_proof: a zero challenge has no inverse")
    return ints, limbs


def _append_proof_terms(params, msm_, proof, x, v, weight=1):
    """steps 1-5 of verify_proof on the host scalars, every scalar times `weight` (an integer); the constant term -v * weight is
    RETURNED, not applied -> (constant, neg_c * weight, challenges [k, 4])"""
    p = msm_.p
    ints, limbs = _proof_challenges(params, msm_, proof)
    msm_.append_term(weight * _to_int(proof.xi, p), proof.s_commitment)
    for (l, r, _), uj in zip(proof.rounds, ints):
        msm_.append_term(weight * pow(uj, -1, p), l)
        msm_.append_term(weight * uj, r)
    c, b = _to_int(proof.c, p), _to_int(compute_b(msm_.field, x, limbs), p)
    msm_.add_to_u_scalar(-c * b * _to_int(proof.z, p) * weight)
    msm_.add_to_w_scalar(-_to_int(proof.f, p) * weight)
    return -_to_int(v, p) * weight % p, -c * weight % p, limbs


def commitment_verify_proof(params, msm_, proof, x, v):
    """poly/commitment/verifier.rs verify_proof(params, msm, proof, x, v) -> Guard, for an msm into which the caller has put the
    commitment being opened (append_term(1, P)).  The transcript stays with the caller: `proof` (IpaProof, or anything with its
    attributes) carries the points and scalars read from it and the challenges squeezed from it.
    Deviation from upstream: a challenge u_j = 0 raises ZkError(ZK_ERR_INVALID_ARG) -- upstream's batch_invert leaves the zero
    in place as its own 'inverse' and goes on; a transcript hash yields 0 with probability 2^-255, so no honest proof is refused.
    len(proof.rounds) != params.k raises ZkError too.  Both are raised before the msm is touched."""
    constant, neg_c, limbs = _append_proof_terms(params, msm_, proof, x, v)
    msm_.add_constant_term(constant)
    return Guard(msm_, neg_c, limbs)


def batch_msm(params, items, weights, stream=0):
    """the MSM of the batching strategy (halo2's BatchVerifier) over items = [(commitment P, proof, x, v)]: what
        for item, r in zip(items, weights): msm.scale(r); msm.append_term(1, P); msm = verify_proof(..).use_challenges()
    leaves, with the g_scalars work fused: proof p's scalars are scaled on the host by t_p = prod_{q > p} r_q, and ONE
    zk_halo2_ipa_s_device call of count = len(items) with init_p = -c_p t_p writes the whole vector in one pass (upstream and the
    loop above: k doubling passes plus a scale pass per proof)."""
    if len(items) != len(weights) or not items:
        raise ZkError(ZK_ERR_INVALID_ARG, "verify_batch: one weight per item, at least one item")
    m = MSM(params, stream=stream)
    tails = [1] * len(items)
    for q in range(len(items) - 2, -1, -1):
        tails[q] = tails[q + 1] * _to_int(weights[q + 1], m.p) % m.p
    constant, inits, challenges = 0, [], []
    for (commitment, proof, x, v), t in zip(items, tails):
        m.append_term(t, commitment)
        c0, neg_c, limbs = _append_proof_terms(params, m, proof, x, v, weight=t)
        constant = (constant + c0) % m.p
        inits.append(_mont_limbs(neg_c, m.p))
        challenges.append(limbs)
    compute_s(m.field, np.stack(challenges), np.stack(inits), out=m._g(), accumulate=False, stream=stream)
    m.add_constant_term(constant)
    return m


def verify_batch(params, items, weights, stream=0):
    """true when every opening of the batch verifies (up to the soundness of the random weights): batch_msm(..).eval() -- one
    pass for all the g_scalars, one n-point MSM"""
    return batch_msm(params, items, weights, stream=stream).eval()


# ------------------------------------------------------------------ MockProver (dev.rs), after synthesis
MOCK_MAX_PROGRAMS = 1024       # csrc/zk_mock_kernels.h: programs per zk_halo2_mock_eval_device call (more are chunked here)
MOCK_ZERO, MOCK_NONZERO, MOCK_POISON = 0, 1, 2


class _Failure:
    """one VerifyFailure of dev.rs: equal when class and fields are"""
    _fields = ()

    def _key(self):
        return tuple(getattr(self, f) for f in self._fields)

    def __eq__(self, other):
        return type(other) is type(self) and self._key() == other._key()

    def __hash__(self):
        return hash((type(self).__name__,) + tuple(map(str, self._key())))

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (f, getattr(self, f)) for f in self._fields))


class ConstraintNotSatisfied(_Failure):
    """gate: (index, name); poly: index inside the gate; row; cell_values: [((column, rotation), integer), ...] -- the cells the
    polynomial queries at that row, in order of first appearance, as canonical integers"""
    _fields = ("gate", "poly", "row", "cell_values")

    def __init__(self, gate, poly, row, cell_values):
        self.gate, self.poly, self.row, self.cell_values = tuple(gate), int(poly), int(row), list(cell_values)


class ConstraintPoisoned(_Failure):
    """an active constraint reads a poisoned cell (a blinding row of an advice column); once per constraint"""
    _fields = ("gate", "poly")

    def __init__(self, gate, poly):
        self.gate, self.poly = tuple(gate), int(poly)


class Lookup(_Failure):
    _fields = ("lookup", "row")

    def __init__(self, lookup, row):
        self.lookup, self.row = int(lookup), int(row)


class Permutation(_Failure):
    """column: the flat column index (advice ++ fixed ++ instance)"""
    _fields = ("column", "row")

    def __init__(self, column, row):
        self.column, self.row = int(column), int(row)


class VerifyFailures(AssertionError):
    """MockProver.assert_satisfied: carries the list"""

    def __init__(self, failures, truncated):
        AssertionError.__init__(self, "circuit was not satisfied%s:\n  %s" % (" (list truncated)" if truncated else "", "\n  ".join(map(repr, failures[:32]))))
        self.failures, self.truncated = failures, truncated


def _bytes_buffer(count):
    """zero device buffer of status bytes"""
    from .groth16 import _on_emulator
    if _on_emulator():
        return np.zeros(max(count, 1), dtype=np.uint8)
    import torch
    return torch.zeros(max(count, 1), dtype=torch.uint8, device="cuda")


def mock_eval(field, k, programs, columns, poison_from, consts, status=None, values=None, want_values=False, stream=0):
    """zk_halo2_mock_eval_device: `programs` (tuple form, see evaluate_expression) at every row of the 2^k-row domain, three-valued.
    columns: device buffers [2^k, 4]; poison_from: one row per column.  Returns (status [P * 2^k] bytes, values [P, 2^k, 4] or None),
    device buffers."""
    from .groth16 import _new_buffer
    n, P = 1 << k, len(programs)
    ops = _expr_ops([o for prog in programs for o in prog])
    offs = np.zeros(P + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(prog) for prog in programs])
    status = _bytes_buffer(P * n) if status is None else status
    if want_values and values is None:
        values = _new_buffer((max(P, 1), n, 4))
    cs = _np64(consts).reshape(-1, 4) if len(consts) else np.zeros((1, 4), dtype=np.uint64)
    pf = np.ascontiguousarray(poison_from, dtype=np.uint64)
    cols = _ptr_array(columns)
    for lo in range(0, max(P, 1), MOCK_MAX_PROGRAMS):          # (P = 0 goes down once and is refused there)
        hi = min(P, lo + MOCK_MAX_PROGRAMS)
        o = np.ascontiguousarray(offs[lo:hi + 1] - offs[lo]) if P else offs
        sub = ctypes.cast(ctypes.addressof(ops) + int(offs[lo]) * ctypes.sizeof(ExprOp), ctypes.POINTER(ExprOp))
        vout = None if values is None else ctypes.c_void_p(_ptr(values).value + lo * n * 32)
        _call("zk_halo2_mock_eval_device", field_id(field), int(k), sub, _ptr(o), hi - lo, cols, _ptr(pf), len(columns), _ptr(cs), len(consts), vout,
              ctypes.c_void_p(_ptr(status).value + lo * n), ctypes.c_void_p(stream))
    return status, values


def mock_failures(status, count, cap, stream=0):
    """zk_halo2_mock_failures_device: (positions uint64 [m], kinds uint8 [m], total) of the non-zero bytes of status[0 .. count),
    m = min(total, cap), ascending"""
    cap = int(min(cap, count))
    pos, kinds, total = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint8), ctypes.c_uint64(0)
    _call("zk_halo2_mock_failures_device", _ptr(status), int(count), cap, _ptr(pos), _ptr(kinds), ctypes.byref(total), ctypes.c_void_p(stream))
    m = min(total.value, cap)
    return pos[:m], kinds[:m], total.value


def _program_cells(program):
    """the (column, rotation) queries of a program, in order of first appearance"""
    seen = []
    for o in program:
        if o[0] == "col" and (int(o[1]), int(o[2])) not in seen:
            seen.append((int(o[1]), int(o[2])))
    return seen


class MockProver:
    """halo2_proofs 0.2 dev.rs MockProver, after synthesis: does this assignment satisfy these gates, lookups and copy constraints?
    The semantics (Poison cells in the advice columns' blinding rows, three-valued evaluation, the order of the list, where this
    knowingly differs from upstream) are DESIGN.md §5 "MockProver".

      advice, fixed   device columns [n, 4] Montgomery (a list of them, or one [count, n, 4] buffer)
      instance        per column at most `usable` values -- Python integers, or Montgomery limbs [m, 4] -- zero-padded on upload;
                      more than that is upstream's InstanceTooLarge (ValueError)
      gates           [(name, [program, ...]), ...]; programs in the tuple form of evaluate_expression over the flat column space
                      advice ++ fixed ++ instance
      lookups         [(input_programs, table_programs), ...], equally long lists.  One expression wide: the membership test runs
                      on the device (zk_halo2_mock_lookup_device).  Wider: the expressions are evaluated on the device, the
                      tuples are compared ON THE HOST with Python integers (the device path for tuples is DESIGN.md's follow-up).
      permutation     (flat column indices, Assembly or [ncols, n] uint64 mapping array)
      consts          Montgomery limbs [count, 4], shared by all programs"""

    def __init__(self, field, k, blinding_factors, advice, fixed, instance=(), gates=(), lookups=(), permutation=None, consts=(), stream=0):
        from .groth16 import _upload
        self.field, self.k, self.n, self.blinding_factors, self.stream = field_id(field), int(k), 1 << int(k), int(blinding_factors), stream
        if self.n < self.blinding_factors + 3:       # upstream: cs.minimum_rows() -> Error::NotEnoughRowsAvailable
            raise ValueError("NotEnoughRowsAvailable: n = %d < blinding_factors + 3 = %d" % (self.n, self.blinding_factors + 3))
        self.usable = self.n - (self.blinding_factors + 1)
        p = field_modulus(field)

        def columns_of(group):
            cols = [group[i] for i in range(len(group))]
            for c in cols:
                if tuple(c.shape) != (self.n, 4):
                    raise AssertionError("assertion failed: column.len() == 1 << k")
            return cols

        inst = np.zeros((len(instance), self.n, 4), dtype=np.uint64)
        for i, col in enumerate(instance):
            if len(col) > self.usable:
                raise ValueError("InstanceTooLarge: instance column %d has %d values, %d rows are usable" % (i, len(col), self.usable))
            if isinstance(col, np.ndarray) and col.ndim == 2:
                inst[i, :len(col)] = _np64(col)
            else:
                for r, v in enumerate(col):
                    inst[i, r] = _mont_limbs(int(v) % p, p)
        self._instance = _upload(inst) if len(instance) else None
        self.columns = columns_of(advice) + columns_of(fixed) + ([self._instance[i] for i in range(len(instance))] if len(instance) else [])
        self.n_advice, self.n_fixed, self.n_instance = len(advice), len(fixed), len(instance)
        self.poison_from = np.array([self.usable] * self.n_advice + [self.n] * (self.n_fixed + self.n_instance), dtype=np.uint64)
        self.consts = _np64(consts).reshape(-1, 4) if len(consts) else np.zeros((0, 4), dtype=np.uint64)
        self.gates = [(name, [list(prog) for prog in polys]) for name, polys in gates]
        self.lookups = [([list(q) for q in ins], [list(q) for q in tab]) for ins, tab in lookups]
        for _, polys in self.gates:
            for prog in polys:
                self._check_program(prog)
        for ins, tab in self.lookups:
            if len(ins) != len(tab) or not ins:
                raise ZkError(ZK_ERR_INVALID_ARG, "a lookup is a pair of equally long, non-empty lists of programs")
            for prog in ins + tab:
                self._check_program(prog)
        self.permutation = None
        if permutation is not None:
            idx, asm = permutation
            mapping = asm.mapping() if isinstance(asm, Assembly) else asm
            if any(not 0 <= int(c) < len(self.columns) for c in idx) or tuple(mapping.shape) != (len(idx), self.n):
                raise ZkError(ZK_ERR_INVALID_ARG, "permutation: column indices / mapping shape")
            self.permutation = ([int(c) for c in idx], _upload(mapping) if isinstance(mapping, np.ndarray) else mapping)
        self.failure_counts, self.truncated = {}, False

    def _check_program(self, prog):
        _expr_ops(prog)                              # the range checks of every field of every op
        for o in prog:
            if o[0] == "col" and int(o[1]) >= len(self.columns):
                raise ZkError(ZK_ERR_INVALID_ARG, "expression op %r: no such column" % (o,))
            if o[0] in ("const", "scale") and int(o[1]) >= len(self.consts):
                raise ZkError(ZK_ERR_INVALID_ARG, "expression op %r: no such constant" % (o,))

    def _eval(self, programs, want_values=False):
        return mock_eval(self.field, self.k, programs, self.columns, self.poison_from, self.consts, want_values=want_values, stream=self.stream)

    def _cell_values(self, wanted):
        """wanted: [(column, row), ...] -> integers; one gather per column group"""
        from .groth16 import _download
        if not wanted:
            return []
        p = field_modulus(self.field)
        r_inv = pow(1 << 256, -1, p)
        out = [None] * len(wanted)
        by_col = {}
        for i, (c, r) in enumerate(wanted):
            by_col.setdefault(c, []).append((i, r))
        for c, items in by_col.items():
            rows = np.array([r for _, r in items], dtype=np.int64)
            col = self.columns[c]
            if isinstance(col, np.ndarray):
                got = col[rows]
            else:
                import torch
                got = _download(col[torch.from_numpy(rows).to(col.device)])
            for (i, _), limbs in zip(items, _np64(got).tolist()):
                out[i] = sum(w << (64 * j) for j, w in enumerate(limbs)) * r_inv % p
        return out

    def _verify_gates(self, cap):
        index = [(g, j) for g, (_, polys) in enumerate(self.gates) for j in range(len(polys))]
        if not index:
            return [], 0
        status, _ = self._eval([self.gates[g][1][j] for g, j in index])
        pos, kinds, total = mock_failures(status, len(index) * self.n, cap, self.stream)
        found, poisoned, wanted = [], set(), []
        for q, kind in zip(pos.tolist(), kinds.tolist()):
            g, j = index[q // self.n]
            row = q % self.n
            if kind == MOCK_POISON:
                if (g, j) not in poisoned:               # once per constraint, at the position of its first poisoned row
                    poisoned.add((g, j))
                    found.append((g, row, j, None))
            else:
                cells = _program_cells(self.gates[g][1][j])
                found.append((g, row, j, (len(wanted), cells)))
                wanted.extend((c, (row + rot) % self.n) for c, rot in cells)
        values = self._cell_values(wanted)
        out = []
        for g, row, j, cells in sorted(found, key=lambda f: f[:3]):
            gate = (g, self.gates[g][0])
            if cells is None:
                out.append(ConstraintPoisoned(gate, j))
            else:
                out.append(ConstraintNotSatisfied(gate, j, row, list(zip(cells[1], values[cells[0]:cells[0] + len(cells[1])]))))
        return out, total

    def _verify_lookups(self, cap):
        from .groth16 import _download
        if not self.lookups:
            return [], 0
        n, u = self.n, self.usable
        programs, first = [], []
        for ins, tab in self.lookups:
            first.append(len(programs))
            programs.extend(ins + tab)
        status, values = self._eval(programs, want_values=True)
        out_status = _bytes_buffer(len(self.lookups) * n)
        host = {}
        sbase, obase = _ptr(status).value, _ptr(out_status).value
        for li, (ins, tab) in enumerate(self.lookups):
            a = first[li]
            if len(ins) == 1:
                _call("zk_halo2_mock_lookup_device", self.field, self.k, _ptr(values[a]), ctypes.c_void_p(sbase + a * n), _ptr(values[a + 1]),
                      ctypes.c_void_p(sbase + (a + 1) * n), u, ctypes.c_void_p(obase + li * n), ctypes.c_void_p(self.stream))
            else:                                        # HOST PATH: tuples of Python integers; Poison is its own component value
                w = len(ins)
                vals = _np64(_download(values[a:a + 2 * w]))[:, :u].astype(object)
                ints = vals[..., 0] + (vals[..., 1] << 64) + (vals[..., 2] << 128) + (vals[..., 3] << 192)
                st = status[a * n:(a + 2 * w) * n]
                st = (st if isinstance(st, np.ndarray) else st.cpu().numpy()).reshape(2 * w, n)[:, :u]      # (after _download's synchronisation)
                comp = lambda e, r: None if st[e, r] == MOCK_POISON else ints[e, r]
                table = {tuple(comp(w + e, r) for e in range(w)) for r in range(u)}
                host[li] = [r for r in range(u) if tuple(comp(e, r) for e in range(w)) not in table]
        pos, _, total = mock_failures(out_status, len(self.lookups) * n, cap, self.stream)
        found = [(int(q) // n, int(q) % n) for q in pos.tolist()]
        for li, rows in host.items():
            found.extend((li, r) for r in rows)
            total += len(rows)
        found.sort()
        return [Lookup(li, r) for li, r in found[:cap]], total

    def _verify_permutation(self, cap):
        if self.permutation is None:
            return [], 0
        idx, mapping = self.permutation
        status = _bytes_buffer(len(idx) * self.n)
        pf = np.ascontiguousarray(self.poison_from[idx], dtype=np.uint64)
        _call("zk_halo2_mock_permutation_device", self.field, self.k, len(idx), _ptr_array([self.columns[c] for c in idx]), _ptr(pf), _ptr(mapping),
              _ptr(status), ctypes.c_void_p(self.stream))
        pos, _, total = mock_failures(status, len(idx) * self.n, cap, self.stream)
        return [Permutation(idx[int(q) // self.n], int(q) % self.n) for q in pos.tolist()], total

    def verify(self, max_failures=65536):
        """dev.rs MockProver::verify: gate failures in (gate, row, poly) order, then lookup failures in (lookup, row) order, then
        permutation failures in (column, row) order; [] is upstream's Ok(()).  failure_counts: the totals per class as the device
        counted them -- "gates" = flagged (constraint, row) pairs, every poisoned row of a constraint included; when a class has
        more than max_failures the first ones in device order (program, then row) are reported and `truncated` is set."""
        cap = int(max_failures)
        gates, n_g = self._verify_gates(cap)
        lookups, n_l = self._verify_lookups(cap)
        perm, n_p = self._verify_permutation(cap)
        self.failure_counts = {"gates": n_g, "lookups": n_l, "permutation": n_p}
        self.truncated = any(t > cap for t in (n_g, n_l, n_p))
        return gates + lookups + perm

    def assert_satisfied(self, max_failures=65536):
        failures = self.verify(max_failures)
        if failures:
            raise VerifyFailures(failures, self.truncated)
