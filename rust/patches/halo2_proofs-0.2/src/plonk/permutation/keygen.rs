//! REPLACES `Assembly` in halo2_proofs 0.2.0 `src/plonk/permutation/keygen.rs`: `new` / `copy` keep their signatures and their
//! exact permutation (the larger cycle absorbs the smaller, the left one on a tie, then mapping[left] <-> mapping[right]) but the
//! three tables live inside the library, and `build_vk` / `build_pk` produce the permutation columns, their coefficient and
//! extended forms and their commitments on resident buffers: one kernel for delta^col omega^row over all ncols x n cells, the NTT
//! entry points for the two transforms, one batched MSM for the commitments.  NOT COMPILED here.
//! The Python mirror contangle-zkcp_amd/halo2.py (`Assembly`, `keygen_vk`, `keygen_pk`) is the tested statement of the same calls.
use zkcp_amd_sys as zk;

use super::super::super::arithmetic::{limbs_of, CurveAffine, FieldExt};
use super::super::super::poly::EvaluationDomain;
use super::super::{Any, Column, Error};
use super::Argument;

pub struct Assembly {
    columns: Vec<Column<Any>>,
    handle: u64,
    n: usize,
}

impl Assembly {
    pub(crate) fn new(n: usize, p: &Argument) -> Self {
        let mut handle = 0u64;
        zk::check(unsafe { zk::zk_halo2_assembly_new(n as u64, p.columns.len() as u32, &mut handle) }, "zk_halo2_assembly_new").unwrap();
        Assembly { columns: p.columns.clone(), handle, n }
    }

    pub(crate) fn copy(&mut self, left_column: Column<Any>, left_row: usize, right_column: Column<Any>, right_row: usize) -> Result<(), Error> {
        let index = |c: &Column<Any>| self.columns.iter().position(|x| x == c).ok_or(Error::ColumnNotInPermutation(*c));
        let quad = [index(&left_column)? as u32, left_row as u32, index(&right_column)? as u32, right_row as u32];
        if left_row >= self.n || right_row >= self.n {
            return Err(Error::BoundsFailure);
        }
        let mut applied = 0u64;
        zk::check(unsafe { zk::zk_halo2_assembly_copy(self.handle, quad.as_ptr(), 1, &mut applied) }, "zk_halo2_assembly_copy")
            .map_err(|_| Error::BoundsFailure)
    }

    /// mapping -> a device buffer of ncols x n words (col << 32 | row)
    fn mapping_device(&self) -> zk::DeviceBuf {
        let mut host = vec![0u64; self.columns.len() * self.n];
        zk::check(unsafe { zk::zk_halo2_assembly_mapping(self.handle, host.as_mut_ptr() as _) }, "zk_halo2_assembly_mapping").unwrap();
        zk::DeviceBuf::upload(&host)
    }

    /// permutations (Lagrange), polys (coefficients) and -- unless `cosets` is None -- cosets (extended, `lazy` = the R' radix) of
    /// every column, each ncols x its length in one buffer, and the commitments (12 u64 Jacobian each; upstream adds the
    /// Blind::default() term [1] W on the CPU afterwards).  build_vk keeps the commitments, build_pk the three buffers.
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn build_device<C: CurveAffine>(&self, domain: &EvaluationDomain<C::Scalar>, curve: i32, field: i32, g_lagrange_handle: u64,
                                               cosets: Option<bool>, stream: *mut core::ffi::c_void)
                                               -> (zk::DeviceBuf, zk::DeviceBuf, Option<zk::DeviceBuf>, Vec<u64>) {
        let (n, ncols, ext) = (self.n, self.columns.len(), domain.extended_len());
        let mapping = self.mapping_device();
        let delta = limbs_of(&C::Scalar::DELTA);
        let mut permutations = zk::DeviceBuf::zeroed(ncols * n * 4);
        zk::check(unsafe { zk::zk_halo2_permutation_sigmas_device(field, domain.k(), ncols as u32, mapping.ptr() as _, delta.as_ptr() as _,
                                                                  permutations.ptr(), stream) }, "zk_halo2_permutation_sigmas_device").unwrap();
        let mut commitments = vec![0u64; 12 * ncols];
        zk::check(unsafe { zk::zk_msm_batch_device(curve, g_lagrange_handle, permutations.ptr() as _, n as u64, ncols as u32, n as u64, 1,
                                                   core::ptr::null(), commitments.as_mut_ptr() as _, stream) }, "zk_msm_batch_device").unwrap();
        let mut polys = zk::DeviceBuf::zeroed(ncols * n * 4);
        let mut ext_buf = cosets.map(|_| zk::DeviceBuf::zeroed(ncols * ext * 4));
        let (w_inv, w_ext, zeta) = (limbs_of(&domain.get_omega_inv()), limbs_of(&domain.get_extended_omega()), limbs_of(&C::Scalar::ZETA));
        for c in 0..ncols {
            let (src, dst) = (permutations.ptr_at(c * n * 4), polys.ptr_at(c * n * 4));
            zk::check(unsafe { zk::zk_ntt_oop_device(field, src as _, dst, domain.k(), domain.k(), w_inv.as_ptr() as _, 1, core::ptr::null(),
                                                     core::ptr::null(), stream) }, "zk_ntt_oop_device").unwrap();
            if let (Some(lazy), Some(buf)) = (cosets, ext_buf.as_mut()) {
                zk::check(unsafe { zk::zk_ntt_oop_device(field, dst as _, buf.ptr_at(c * ext * 4), domain.extended_k(), domain.k(), w_ext.as_ptr() as _,
                                                         if lazy { 2 } else { 0 }, zeta.as_ptr() as _, core::ptr::null(), stream) },
                          "zk_ntt_oop_device").unwrap();
            }
        }
        (permutations, polys, ext_buf, commitments)
    }
}

impl Drop for Assembly {
    fn drop(&mut self) {
        unsafe { zk::zk_halo2_assembly_free(self.handle) };
    }
}
