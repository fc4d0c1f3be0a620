//! REPLACES the body of `generate_parameters` in ark-groth16 0.3.0 `src/generator.rs` from the point where the constraint
//! system has been synthesised in setup mode: the Lagrange coefficients at tau, the QAP at tau
//! (`LibsnarkReduction::instance_map_with_evaluation`), the key scalars and the five fixed-base multiplications all run on
//! resident buffers; only the trapdoor scalars go in and only affine points come out (call site
//! lib/src/zk/encryption.rs:169 through `Groth16::setup`).  NOT COMPILED here.
//! `DeviceVec` is the fork's own thin RAII wrapper over hipMalloc / hipMemcpy (hip-sys), omitted for brevity.
use ark_ec::{AffineCurve, PairingEngine, ProjectiveCurve};
use ark_ff::{Field, PrimeField, Zero};
use ark_relations::r1cs::{ConstraintMatrices, Result as R1CSResult, SynthesisError};
use ark_serialize::{CanonicalDeserialize, CanonicalSerialize};
use zkcp_amd_sys as zk;

use crate::device::DeviceVec;
use crate::{ProvingKey, VerifyingKey};

fn limbs<T: CanonicalSerialize>(v: &T) -> *const core::ffi::c_void { v as *const T as *const _ }   // Fr / Fq are Montgomery limbs in memory

/// one matrix of `cs.to_matrices()` in CSR form, resident through zk_r1cs_matrix_upload
fn upload<F: PrimeField>(field: i32, rows: &[Vec<(F, usize)>], n_cols: usize) -> u64 {
    let mut row_ptr = vec![0u64; rows.len() + 1];
    let (mut col, mut val) = (Vec::<u32>::new(), Vec::<F>::new());
    for (i, row) in rows.iter().enumerate() {
        for (c, j) in row { val.push(*c); col.push(*j as u32); }
        row_ptr[i + 1] = col.len() as u64;
    }
    let mut h = 0u64;
    let st = unsafe { zk::zk_r1cs_matrix_upload(field, row_ptr.as_ptr(), col.as_ptr(), val.as_ptr() as _, rows.len() as u64, n_cols as u64, &mut h) };
    zk::check(st, "zk_r1cs_matrix_upload").unwrap();
    h
}

/// [k_i] base for the resident Montgomery scalars, as affine points read back through the uncompressed wire format
fn fixed_base<G: AffineCurve>(curve: i32, base: &G, scalars: *const core::ffi::c_void, n: usize, stream: *mut core::ffi::c_void) -> Vec<G> {
    let limbs64 = unsafe { zk::zk_curve_base_limbs64(curve) } as usize;
    let out = DeviceVec::zeroed(n * 2 * limbs64 * 8, stream);
    let st = unsafe { zk::zk_fixed_base_msm_device(curve, base as *const G as _, scalars, n as u64, 1, out.ptr(), stream) };
    zk::check(st, "zk_fixed_base_msm_device").unwrap();
    let host: Vec<u64> = out.to_host(stream);
    let ps = unsafe { zk::zk_ark_point_size(curve, 0) } as usize;
    let mut bytes = vec![0u8; n * ps];
    zk::check(unsafe { zk::zk_ark_points_encode(curve, host.as_ptr() as _, n as u64, 0, bytes.as_mut_ptr()) }, "zk_ark_points_encode").unwrap();
    bytes.chunks(ps).map(|b| G::deserialize_unchecked(b).unwrap()).collect()
}

/// `field`, `g1`, `g2`: library ids of E::Fr, E::G1Affine, E::G2Affine.  t is sampled outside the domain by the caller, as upstream.
#[allow(clippy::too_many_arguments)]
pub fn generate_parameters_on_device<E: PairingEngine>(matrices: &ConstraintMatrices<E::Fr>, alpha: E::Fr, beta: E::Fr, gamma: E::Fr,
                                                       delta: E::Fr, t: E::Fr, g1_generator: E::G1Projective, g2_generator: E::G2Projective,
                                                       field: i32, g1: i32, g2: i32, stream: *mut core::ffi::c_void) -> R1CSResult<ProvingKey<E>> {
    let num_inputs = matrices.num_instance_variables;
    let n_vars = num_inputs + matrices.num_witness_variables;
    let m = (matrices.num_constraints + num_inputs).next_power_of_two();
    let log_m = m.trailing_zeros();
    zk::init_once();
    let (ha, hb, hc) = (upload(field, &matrices.a, n_vars), upload(field, &matrices.b, n_vars), upload(field, &matrices.c, n_vars));
    // evaluate_all_lagrange_coefficients + instance_map_with_evaluation: u, v, w of every variable at t; zt = t^m - 1
    let (u, v, w) = (DeviceVec::zeroed(n_vars * 32, stream), DeviceVec::zeroed(n_vars * 32, stream), DeviceVec::zeroed(n_vars * 32, stream));
    let mut zt = E::Fr::zero();
    let st = unsafe { zk::zk_groth16_qap_at_device(field, ha, hb, hc, num_inputs as u64, log_m, limbs(&t), u.ptr(), v.ptr(), w.ptr(), n_vars as u64,
                                                   &mut zt as *mut E::Fr as _, stream) };
    zk::check(st, "zk_groth16_qap_at_device").map_err(|_| SynthesisError::PolynomialDegreeTooLarge)?;
    // (beta a + alpha b + c) / gamma for the inputs, / delta for the rest, over w in place; the powers of t times zt / delta
    let h = DeviceVec::zeroed((m - 1) * 32, stream);
    let st = unsafe { zk::zk_groth16_key_scalars_device(field, u.ptr(), v.ptr(), w.ptr(), n_vars as u64, num_inputs as u64, log_m, limbs(&alpha),
                                                        limbs(&beta), limbs(&gamma), limbs(&delta), limbs(&t), limbs(&zt), w.ptr(), h.ptr(), stream) };
    zk::check(st, "zk_groth16_key_scalars_device").map_err(|_| SynthesisError::UnexpectedIdentity)?;   // gamma or delta has no inverse
    for handle in [ha, hb, hc] { zk::check(unsafe { zk::zk_r1cs_matrix_free(handle) }, "zk_r1cs_matrix_free").unwrap(); }
    let (g1a, g2a) = (g1_generator.into_affine(), g2_generator.into_affine());
    let a_query = fixed_base::<E::G1Affine>(g1, &g1a, u.ptr(), n_vars, stream);
    let b_g1_query = fixed_base::<E::G1Affine>(g1, &g1a, v.ptr(), n_vars, stream);
    let b_g2_query = fixed_base::<E::G2Affine>(g2, &g2a, v.ptr(), n_vars, stream);
    let h_query = fixed_base::<E::G1Affine>(g1, &g1a, h.ptr(), m - 1, stream);
    let mut gamma_abc_g1 = fixed_base::<E::G1Affine>(g1, &g1a, w.ptr(), n_vars, stream);
    let l_query = gamma_abc_g1.split_off(num_inputs);
    // the single elements: upstream's scalar multiplications, unchanged
    let vk = VerifyingKey::<E> { alpha_g1: g1_generator.mul(alpha.into_repr()).into_affine(), beta_g2: g2_generator.mul(beta.into_repr()).into_affine(),
                                 gamma_g2: g2_generator.mul(gamma.into_repr()).into_affine(), delta_g2: g2_generator.mul(delta.into_repr()).into_affine(),
                                 gamma_abc_g1 };
    let _ = E::Fr::one();
    Ok(ProvingKey { vk, beta_g1: g1_generator.mul(beta.into_repr()).into_affine(), delta_g1: g1_generator.mul(delta.into_repr()).into_affine(),
                    a_query, b_g1_query, b_g2_query, h_query, l_query })
}
