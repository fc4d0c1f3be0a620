//! REPLACES `MSM` in halo2_proofs 0.2.0 `src/poly/commitment/msm.rs`: the same eight operations, with `g_scalars` resident on the
//! device (the opening check adds 2^k scalars to it and the SRS it multiplies is resident already) and `eval` as ONE n-point
//! `zk_msm_device` over `params.g`, one small `zk_msm` over the listed terms plus U and W, and the sum and the identity test on
//! host limbs.  `scale` / `add_msm` / `add_to_g_scalars` on the vector are `zk_vec_op_device`; `add_constant_term` is that call
//! on one element.  NOT COMPILED here.
//! The Python mirror contangle-zkcp_amd/halo2.py (`MSM`) is the tested statement of the same calls.
use zkcp_amd_sys as zk;

use super::super::super::arithmetic::{limbs_of, point_limbs_of, CurveAffine};
use super::Params;
use ff::Field;

const VEC_ADD: i32 = 2;
const VEC_SCALE: i32 = 3;

pub struct MSM<'a, C: CurveAffine> {
    pub(crate) params: &'a Params<C>,
    /// 4 n words, Montgomery; None until first needed
    pub(crate) g_scalars: Option<zk::DeviceBuf>,
    w_scalar: Option<C::Scalar>,
    u_scalar: Option<C::Scalar>,
    other_scalars: Vec<C::Scalar>,
    other_bases: Vec<C>,
}

impl<'a, C: CurveAffine> MSM<'a, C> {
    pub fn new(params: &'a Params<C>) -> Self {
        MSM { params, g_scalars: None, w_scalar: None, u_scalar: None, other_scalars: vec![], other_bases: vec![] }
    }

    pub(crate) fn g_scalars_device(&mut self) -> &mut zk::DeviceBuf {
        let n = self.params.n as usize;
        self.g_scalars.get_or_insert_with(|| zk::DeviceBuf::zeroed(4 * n))
    }

    fn vec_op(&mut self, op: i32, b: *const core::ffi::c_void, n: u64, scalar: *const core::ffi::c_void) {
        let (field, stream) = (self.params.field_id(), self.params.stream());
        let g = self.g_scalars_device().ptr();
        zk::check(unsafe { zk::zk_vec_op_device(field, op, g, b, core::ptr::null(), n, scalar, stream) }, "zk_vec_op_device").unwrap();
    }

    pub fn add_msm(&mut self, other: &Self) {
        self.other_scalars.extend(other.other_scalars.iter());
        self.other_bases.extend(other.other_bases.iter());
        if let Some(g) = &other.g_scalars {
            self.vec_op(VEC_ADD, g.ptr() as _, self.params.n, core::ptr::null());
        }
        if let Some(w) = &other.w_scalar {
            self.add_to_w_scalar(*w);
        }
        if let Some(u) = &other.u_scalar {
            self.add_to_u_scalar(*u);
        }
    }

    pub fn append_term(&mut self, scalar: C::Scalar, point: C) {
        self.other_scalars.push(scalar);
        self.other_bases.push(point);
    }

    /// g_scalars[0] += constant: one element of the resident vector, nothing copied to the host
    pub fn add_constant_term(&mut self, constant: C::Scalar) {
        let c = zk::DeviceBuf::upload(&limbs_of(&constant));
        self.vec_op(VEC_ADD, c.ptr() as _, 1, core::ptr::null());
    }

    /// scalars: 4 n words on the device
    pub fn add_to_g_scalars(&mut self, scalars: &zk::DeviceBuf) {
        self.vec_op(VEC_ADD, scalars.ptr() as _, self.params.n, core::ptr::null());
    }

    pub fn add_to_w_scalar(&mut self, scalar: C::Scalar) {
        self.w_scalar = self.w_scalar.map_or(Some(scalar), |a| Some(a + scalar));
    }

    pub fn add_to_u_scalar(&mut self, scalar: C::Scalar) {
        self.u_scalar = self.u_scalar.map_or(Some(scalar), |a| Some(a + scalar));
    }

    pub fn scale(&mut self, factor: C::Scalar) {
        if self.g_scalars.is_some() {
            let f = limbs_of(&factor);
            self.vec_op(VEC_SCALE, core::ptr::null(), self.params.n, f.as_ptr() as _);
        }
        for s in self.other_scalars.iter_mut() {
            *s *= &factor;
        }
        self.w_scalar = self.w_scalar.map(|a| a * &factor);
        self.u_scalar = self.u_scalar.map(|a| a * &factor);
    }

    pub fn eval(self) -> bool {
        let (curve, stream) = (self.params.curve_id(), self.params.stream());
        let mut acc = [0u64; 12]; // z = 0: the identity
        if let Some(g) = &self.g_scalars {
            zk::check(unsafe { zk::zk_msm_device(curve, self.params.g_handle(), g.ptr() as _, self.params.n, 1, core::ptr::null(),
                                                 acc.as_mut_ptr() as _, stream) }, "zk_msm_device").unwrap();
        }
        let (mut scalars, mut bases) = (self.other_scalars, self.other_bases);
        if let Some(w) = self.w_scalar {
            scalars.push(w);
            bases.push(self.params.w);
        }
        if let Some(u) = self.u_scalar {
            scalars.push(u);
            bases.push(self.params.u);
        }
        if !scalars.is_empty() {
            let s: Vec<u64> = scalars.iter().flat_map(|x| limbs_of(x)).collect();
            let b: Vec<u64> = bases.iter().flat_map(|x| point_limbs_of(x)).collect();
            let (mut handle, mut part) = (0u64, [0u64; 12]);
            zk::check(unsafe { zk::zk_bases_upload(curve, b.as_ptr() as _, scalars.len() as u64, &mut handle) }, "zk_bases_upload").unwrap();
            let st = unsafe { zk::zk_msm(curve, handle, s.as_ptr() as _, scalars.len() as u64, 1, core::ptr::null(), part.as_mut_ptr() as _) };
            unsafe { zk::zk_bases_free(handle) };
            zk::check(st, "zk_msm").unwrap();
            let sum = acc;
            zk::check(unsafe { zk::zk_point_add(curve, sum.as_ptr() as _, part.as_ptr() as _, acc.as_mut_ptr() as _) }, "zk_point_add").unwrap();
        }
        let mut aff = [0u64; 8];
        zk::check(unsafe { zk::zk_point_to_affine(curve, acc.as_ptr() as _, aff.as_mut_ptr() as _) }, "zk_point_to_affine").unwrap();
        aff.iter().all(|w| *w == 0)
    }
}
