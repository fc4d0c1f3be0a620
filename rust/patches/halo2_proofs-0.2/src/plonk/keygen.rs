//! REPLACES, in halo2_proofs 0.2.0 `src/plonk/keygen.rs`, what `keygen_vk` and `keygen_pk` do AFTER the circuit has been
//! synthesised into their `Assembly` (fixed columns, selectors compressed into further fixed columns, the permutation assembly):
//! the fixed columns' commitments, coefficient and extended forms, the permutation key (permutation/keygen.rs) and the three key
//! columns l0, l_last, l_active_row, all on resident buffers.  Synthesis, floor planning, `compress_selectors` and the key's
//! transcript representation are upstream's, unchanged.  NOT COMPILED here.
//!
//! upstream                                                     here
//!   batch_invert_assigned(fixed)                                numerators * (1 / denominators) with zk_batch_invert_device
//!                                                               (a zero denominator gives 0 on both sides)
//!   params.commit_lagrange(poly, Blind::default()) per column   one zk_msm_batch_device over g_lagrange (+ [1] W upstream's way)
//!   domain.lagrange_to_coeff / coeff_to_extended per column     zk_ntt_oop_device twice per column (ZK_NTT_OUT_R29 for the lazy form)
//!   l_active_row = 1 - (l_last + l_blind) on the extended coset the extension of the active rows' indicator column: the same
//!                                                               polynomial (extension is linear and the constant 1 extends to 1),
//!                                                               so the same canonical values, without a pass over three vectors
use zkcp_amd_sys as zk;

use super::super::arithmetic::{limbs_of, CurveAffine, FieldExt};
use super::super::poly::EvaluationDomain;

/// `fixed`: nfixed x n Montgomery elements, resident.  Returns (fixed_polys, fixed_cosets, commitments as 12 u64 Jacobian each).
#[allow(clippy::too_many_arguments)]
pub fn fixed_key_device<C: CurveAffine>(domain: &EvaluationDomain<C::Scalar>, curve: i32, field: i32, g_lagrange_handle: u64,
                                        fixed: &zk::DeviceBuf, nfixed: usize, lazy: bool, stream: *mut core::ffi::c_void)
                                        -> (zk::DeviceBuf, zk::DeviceBuf, Vec<u64>) {
    let (n, ext) = (1usize << domain.k(), domain.extended_len());
    let mut commitments = vec![0u64; 12 * nfixed];
    zk::check(unsafe { zk::zk_msm_batch_device(curve, g_lagrange_handle, fixed.ptr() as _, n as u64, nfixed as u32, n as u64, 1, core::ptr::null(),
                                               commitments.as_mut_ptr() as _, stream) }, "zk_msm_batch_device").unwrap();
    let (mut polys, mut cosets) = (zk::DeviceBuf::zeroed(nfixed * n * 4), zk::DeviceBuf::zeroed(nfixed * ext * 4));
    let (w_inv, w_ext, zeta) = (limbs_of(&domain.get_omega_inv()), limbs_of(&domain.get_extended_omega()), limbs_of(&C::Scalar::ZETA));
    for i in 0..nfixed {
        zk::check(unsafe { zk::zk_ntt_oop_device(field, fixed.ptr_at(i * n * 4) as _, polys.ptr_at(i * n * 4), domain.k(), domain.k(),
                                                 w_inv.as_ptr() as _, 1, core::ptr::null(), core::ptr::null(), stream) }, "zk_ntt_oop_device").unwrap();
        zk::check(unsafe { zk::zk_ntt_oop_device(field, polys.ptr_at(i * n * 4) as _, cosets.ptr_at(i * ext * 4), domain.extended_k(), domain.k(),
                                                 w_ext.as_ptr() as _, if lazy { 2 } else { 0 }, zeta.as_ptr() as _, core::ptr::null(), stream) },
                  "zk_ntt_oop_device").unwrap();
    }
    (polys, cosets, commitments)
}

/// an `Assigned` column given as numerators and denominators: den <- 1 / den (zeros stay zero), num <- num * den
pub fn assigned_column_device(field: i32, num: &mut zk::DeviceBuf, den: &mut zk::DeviceBuf, n: usize, stream: *mut core::ffi::c_void) {
    zk::check(unsafe { zk::zk_batch_invert_device(field, den.ptr(), n as u64, stream) }, "zk_batch_invert_device").unwrap();
    zk::check(unsafe { zk::zk_vec_op_device(field, 0, num.ptr(), den.ptr() as _, core::ptr::null(), n as u64, core::ptr::null(), stream) },
              "zk_vec_op_device").unwrap();
}

/// l0, l_last, l_active_row on the extended coset: three indicator columns (row 0; row n - blinding_factors - 1; the rows before
/// that one) through the two transforms.  `cs.minimum_rows()` has been checked by the caller, as upstream.
pub fn key_columns_device<F: FieldExt>(domain: &EvaluationDomain<F>, field: i32, blinding_factors: usize, lazy: bool,
                                       stream: *mut core::ffi::c_void) -> [zk::DeviceBuf; 3] {
    let (n, ext) = (1usize << domain.k(), domain.extended_len());
    let last = n - blinding_factors - 1;
    let one = limbs_of(&F::one());
    let (w_inv, w_ext, zeta) = (limbs_of(&domain.get_omega_inv()), limbs_of(&domain.get_extended_omega()), limbs_of(&F::ZETA));
    let column = |rows: core::ops::Range<usize>| {
        let mut host = vec![0u64; n * 4];
        for r in rows { host[4 * r..4 * r + 4].copy_from_slice(&one); }
        let mut lagrange = zk::DeviceBuf::upload(&host);
        let out = zk::DeviceBuf::zeroed(ext * 4);
        zk::check(unsafe { zk::zk_ntt_device(field, lagrange.ptr(), domain.k(), w_inv.as_ptr() as _, 1, stream) }, "zk_ntt_device").unwrap();
        zk::check(unsafe { zk::zk_ntt_oop_device(field, lagrange.ptr() as _, out.ptr(), domain.extended_k(), domain.k(), w_ext.as_ptr() as _,
                                                 if lazy { 2 } else { 0 }, zeta.as_ptr() as _, core::ptr::null(), stream) }, "zk_ntt_oop_device").unwrap();
        out
    };
    [column(0..1), column(last..last + 1), column(0..last)]
}
