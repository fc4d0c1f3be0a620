//! REPLACES `verify_proof`, `Guard`, `compute_s` and `compute_b` in halo2_proofs 0.2.0 `src/poly/commitment/verifier.rs`: the
//! transcript reads and the handful of host scalars stay as upstream has them; `Guard::use_challenges` adds compute_s(u, neg_c)
//! to the resident `g_scalars` in ONE pass (`zk_halo2_ipa_s_device`; upstream: k doubling passes on CPU threads and an
//! n-element add), and `compute_g` is that kernel with init = 1 followed by one `zk_msm_device`.  A batching strategy that keeps
//! many proofs behind one MSM passes all their challenge vectors to one call (count = the number of proofs, init_p = -c_p times the
//! product of the later weights).  NOT COMPILED here.
//! The Python mirror contangle-zkcp_amd/halo2.py (`commitment_verify_proof`, `Guard`, `verify_batch`) is the tested statement.
use zkcp_amd_sys as zk;

use super::super::super::arithmetic::{limbs_of, point_from_limbs, CurveAffine};
use super::super::super::transcript::{EncodedChallenge, TranscriptRead};
use super::super::Error;
use super::{Params, MSM};
use ff::Field;

#[derive(Debug, Clone)]
pub struct Guard<'a, C: CurveAffine, E: EncodedChallenge<C>> {
    msm: MSM<'a, C>,
    neg_c: C::Scalar,
    u: Vec<C::Scalar>,
    u_packed: Vec<E>,
}

#[derive(Debug, Clone)]
pub struct Accumulator<C: CurveAffine, E: EncodedChallenge<C>> {
    pub g: C,
    pub u_packed: Vec<E>,
}

/// one element's Montgomery words at the 16-byte alignment zk_halo2_ipa_s_device asks of its host pointers
#[repr(C, align(16))]
#[derive(Clone, Copy)]
struct Limbs([u64; 4]);

/// the challenges as k x 4 Montgomery words, u_0 first
fn challenge_limbs<F: ff::PrimeField>(u: &[F]) -> Vec<Limbs> {
    u.iter().map(|x| Limbs(limbs_of(x))).collect()
}

impl<'a, C: CurveAffine, E: EncodedChallenge<C>> Guard<'a, C, E> {
    pub fn use_challenges(mut self) -> MSM<'a, C> {
        let (field, stream, k) = (self.msm.params.field_id(), self.msm.params.stream(), self.u.len() as u32);
        let accumulate = self.msm.g_scalars.is_some() as i32;
        let (u, init) = (challenge_limbs(&self.u), Limbs(limbs_of(&self.neg_c)));
        let g = self.msm.g_scalars_device().ptr();
        zk::check(unsafe { zk::zk_halo2_ipa_s_device(field, k, 1, u.as_ptr() as _, &init as *const Limbs as _, g, accumulate, stream) },
                  "zk_halo2_ipa_s_device").unwrap();
        self.msm
    }

    pub fn use_g(mut self, g: C) -> (MSM<'a, C>, Accumulator<C, E>) {
        self.msm.append_term(self.neg_c, g);
        (self.msm, Accumulator { g, u_packed: self.u_packed })
    }

    pub fn compute_g(&self) -> C {
        let params = self.msm.params;
        let (u, one) = (challenge_limbs(&self.u), Limbs(limbs_of(&C::Scalar::one())));
        let s = zk::DeviceBuf::zeroed(4 * params.n as usize);
        zk::check(unsafe { zk::zk_halo2_ipa_s_device(params.field_id(), self.u.len() as u32, 1, u.as_ptr() as _, &one as *const Limbs as _, s.ptr(), 0,
                                                     params.stream()) }, "zk_halo2_ipa_s_device").unwrap();
        let (mut jac, mut aff) = ([0u64; 12], [0u64; 8]);
        zk::check(unsafe { zk::zk_msm_device(params.curve_id(), params.g_handle(), s.ptr() as _, params.n, 1, core::ptr::null(),
                                             jac.as_mut_ptr() as _, params.stream()) }, "zk_msm_device").unwrap();
        zk::check(unsafe { zk::zk_point_to_affine(params.curve_id(), jac.as_ptr() as _, aff.as_mut_ptr() as _) }, "zk_point_to_affine").unwrap();
        point_from_limbs(&aff)
    }
}

pub fn verify_proof<'a, C: CurveAffine, E: EncodedChallenge<C>, T: TranscriptRead<C, E>>(
    params: &'a Params<C>, mut msm: MSM<'a, C>, transcript: &mut T, x: C::Scalar, v: C::Scalar,
) -> Result<Guard<'a, C, E>, Error> {
    let k = params.k as usize;
    msm.add_constant_term(-v);
    let s_poly_commitment = transcript.read_point().map_err(|_| Error::OpeningError)?;
    let xi = *transcript.squeeze_challenge_scalar::<()>();
    msm.append_term(xi, s_poly_commitment);
    let z = *transcript.squeeze_challenge_scalar::<()>();
    let mut rounds = vec![];
    for _ in 0..k {
        let l = transcript.read_point().map_err(|_| Error::OpeningError)?;
        let r = transcript.read_point().map_err(|_| Error::OpeningError)?;
        let u_j_packed = transcript.squeeze_challenge();
        let u_j = *u_j_packed.as_challenge_scalar::<()>();
        rounds.push((l, r, u_j, /* to be inverted */ u_j, u_j_packed));
    }
    // (upstream's batch_invert leaves a zero challenge in place; the library's mirror refuses it instead)
    for round in rounds.iter_mut() {
        round.3 = Option::from(round.3.invert()).ok_or(Error::OpeningError)?;
    }
    let (mut u, mut u_packed) = (Vec::with_capacity(k), Vec::with_capacity(k));
    for (l, r, u_j, u_j_inv, u_j_packed) in rounds {
        msm.append_term(u_j_inv, l);
        msm.append_term(u_j, r);
        u.push(u_j);
        u_packed.push(u_j_packed);
    }
    let c = transcript.read_scalar().map_err(|_| Error::SamplingError)?;
    let neg_c = -c;
    let f = transcript.read_scalar().map_err(|_| Error::SamplingError)?;
    let b = compute_b(params.field_id(), x, &u);
    msm.add_to_u_scalar(neg_c * &b * &z);
    msm.add_to_w_scalar(-f);
    Ok(Guard { msm, neg_c, u, u_packed })
}

/// prod_j (1 + u_j x^(2^(k-1-j))): k products on host limbs
fn compute_b<F: ff::PrimeField>(field: i32, x: F, u: &[F]) -> F {
    let (xl, ul, mut out) = (limbs_of(&x), challenge_limbs(u), [0u64; 4]);
    zk::check(unsafe { zk::zk_halo2_ipa_compute_b(field, u.len() as u32, xl.as_ptr() as _, ul.as_ptr() as _, out.as_mut_ptr() as _) },
              "zk_halo2_ipa_compute_b").unwrap();
    super::super::super::arithmetic::field_from_limbs(&out)
}
