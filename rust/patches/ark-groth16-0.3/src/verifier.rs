//! REPLACES `prepare_inputs` and `verify_proof_with_prepared_inputs` in ark-groth16 0.3.0 `src/verifier.rs`, and adds the checked
//! read of a verifying key that keeps `gamma_abc_g1` on the device (the reference's buyer: `read_verifying_key` at
//! lib/src/utils.rs:112-118, then `Groth16::verify` at lib/src/zk/encryption.rs:152, sample_entries.rs:126, property.rs:177).
//! Upstream's `prepare_inputs` is a serial loop of full scalar multiplications, `g_ic.add_assign(&b.mul(i.into_repr()))`, over
//! 2 + n public inputs (the whole ciphertext is public: n = 196 608 in the reference's test); here it is one MSM over the
//! resident points.  Upstream's `VerifyingKey::deserialize` takes a square root and a multiplication by r per point, one point
//! after another; here one GPU lane does that per point.  NOT COMPILED here.
//! `DeviceVec` is the fork's own thin RAII wrapper over hipMalloc / hipMemcpy (hip-sys), omitted for brevity.
use ark_ec::{AffineCurve, PairingEngine};
use ark_ff::PrimeField;
use ark_relations::r1cs::{Result as R1CSResult, SynthesisError};
use ark_serialize::{CanonicalDeserialize, CanonicalSerialize, SerializationError};
use zkcp_amd_sys as zk;

use crate::device::DeviceVec;
use crate::Proof;

fn limbs<T>(v: &T) -> *const core::ffi::c_void { v as *const T as *const _ }   // Fq / Fr / affine points are Montgomery limbs in memory

/// VerifyingKey<E> with gamma_abc_g1 resident: the checked decode's output, adopted as a bases handle over gamma_abc_g1[1..]
pub struct DeviceVerifyingKey<E: PairingEngine> {
    pub alpha_g1: E::G1Affine,
    pub beta_g2: E::G2Affine,
    pub gamma_g2: E::G2Affine,
    pub delta_g2: E::G2Affine,
    pub gamma_abc_0: E::G1Affine,
    pub gamma_abc_len: usize,
    pub gamma_abc_dev: DeviceVec,
    pub gamma_abc_tail: u64,
    /// e(alpha_g1, beta_g2) as zk_pairing_product writes it (PreparedVerifyingKey::alpha_g1_beta_g2)
    pub alpha_g1_beta_g2: Vec<u64>,
}

/// `VerifyingKey::<E>::deserialize(bytes)` -- compressed and checked.  `pairing`, `g1`: library ids of E and E::G1Affine.
pub fn read_verifying_key_on_device<E: PairingEngine>(bytes: &[u8], pairing: i32, g1: i32, stream: *mut core::ffi::c_void)
                                                      -> Result<DeviceVerifyingKey<E>, SerializationError> {
    let mut rd = bytes;
    // the four single members go through upstream's own checked readers (four points)
    let alpha_g1 = E::G1Affine::deserialize(&mut rd)?;
    let beta_g2 = E::G2Affine::deserialize(&mut rd)?;
    let gamma_g2 = E::G2Affine::deserialize(&mut rd)?;
    let delta_g2 = E::G2Affine::deserialize(&mut rd)?;
    let n = u64::deserialize(&mut rd)? as usize;
    let ps = unsafe { zk::zk_ark_point_size(g1, 1) } as usize;
    if n == 0 || rd.len() != n * ps { return Err(SerializationError::InvalidData); }
    let limbs64 = unsafe { zk::zk_curve_base_limbs64(g1) } as usize;
    let gamma_abc_dev = DeviceVec::zeroed(n * 2 * limbs64 * 8, stream);
    let (mut bad, mut why) = (0u64, 0u64);
    let st = unsafe { zk::zk_ark_points_decode_checked_device(g1, rd.as_ptr(), n as u64, 1, gamma_abc_dev.ptr(), &mut bad, &mut why, stream) };
    if st != 0 { return Err(SerializationError::InvalidData); }     // point `bad`: 1 non-canonical, 2 flags, 3 curve, 4 subgroup
    let gamma_abc_0 = E::G1Affine::deserialize(&mut &rd[..ps])?;
    let mut gamma_abc_tail = 0u64;
    if n > 1 {
        let tail = unsafe { (gamma_abc_dev.ptr() as *const u8).add(2 * limbs64 * 8) } as *const core::ffi::c_void;
        zk::check(unsafe { zk::zk_bases_adopt_device(g1, tail, (n - 1) as u64, &mut gamma_abc_tail) }, "zk_bases_adopt_device").unwrap();
    }
    let mut alpha_g1_beta_g2 = vec![0u64; 12 * limbs64];
    zk::check(unsafe { zk::zk_pairing_product(pairing, limbs(&alpha_g1), limbs(&beta_g2), 1, alpha_g1_beta_g2.as_mut_ptr() as _) },
              "zk_pairing_product").unwrap();
    Ok(DeviceVerifyingKey { alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_0, gamma_abc_len: n, gamma_abc_dev, gamma_abc_tail, alpha_g1_beta_g2 })
}

/// `prepare_inputs(pvk, public_inputs)`: gamma_abc_g1[0] + sum_i x_i gamma_abc_g1[i + 1] through the MSM entry
pub fn prepare_inputs<E: PairingEngine>(vk: &DeviceVerifyingKey<E>, public_inputs: &[E::Fr], g1: i32, stream: *mut core::ffi::c_void)
                                        -> R1CSResult<E::G1Affine> {
    if public_inputs.len() + 1 != vk.gamma_abc_len { return Err(SynthesisError::MalformedVerifyingKey); }
    let d_x = DeviceVec::from_host(public_inputs, stream);          // Fr is Montgomery limbs in memory: scalars_are_montgomery = 1 inside
    let mut g_ic = E::G1Affine::prime_subgroup_generator();         // overwritten
    let st = unsafe { zk::zk_groth16_prepare_inputs(g1, vk.gamma_abc_tail, limbs(&vk.gamma_abc_0), vk.gamma_abc_len as u64, d_x.ptr(),
                                                   public_inputs.len() as u64, &mut g_ic as *mut E::G1Affine as _, stream) };
    zk::check(st, "zk_groth16_prepare_inputs").map_err(|_| SynthesisError::MalformedVerifyingKey)?;
    Ok(g_ic)
}

/// `verify_proof_with_prepared_inputs`: e(A, B) e(g_ic, -gamma_g2) e(C, -delta_g2) == e(alpha_g1, beta_g2), on the host
pub fn verify_proof_with_prepared_inputs<E: PairingEngine>(vk: &DeviceVerifyingKey<E>, proof: &Proof<E>, g_ic: &E::G1Affine, pairing: i32)
                                                           -> R1CSResult<bool> {
    let pts = zk::zk_groth16_vk_points { alpha_g1: limbs(&vk.alpha_g1), beta_g2: limbs(&vk.beta_g2), gamma_g2: limbs(&vk.gamma_g2),
                                         delta_g2: limbs(&vk.delta_g2) };
    let mut ok = 0u64;
    let st = unsafe { zk::zk_groth16_verify(pairing, &pts, vk.alpha_g1_beta_g2.as_ptr() as _, limbs(g_ic), limbs(&proof.a), limbs(&proof.b),
                                           limbs(&proof.c), &mut ok) };
    zk::check(st, "zk_groth16_verify").map_err(|_| SynthesisError::UnexpectedIdentity)?;
    Ok(ok != 0)
}
