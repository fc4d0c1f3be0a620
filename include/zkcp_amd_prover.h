/*
 * zkcp_amd_prover -- the callers and data formats either side of the MSM / NTT path:
 * what a patched ark-groth16 / halo2_proofs needs beyond zkcp_amd.h to keep a whole proof on the device and to exchange
 * keys and proofs with the unmodified reference.
 *
 *   zk_ark_*                   <-  ark-serialize 0.3 CanonicalSerialize / CanonicalDeserialize of ark-ec 0.3 GroupAffine,
 *                                  Vec<T>, ark-groth16 0.3 ProvingKey / VerifyingKey / Proof -- the formats the reference
 *                                  writes and reads at lib/src/utils.rs:85-118 (serialize_unchecked / deserialize_unchecked
 *                                  of the proving key, ark_to_bytes / ark_from_bytes of the verifying key) and
 *                                  circuits-ark/src/utils.rs:12-22 (ark_to_bytes(proof) at lib/src/zk/encryption.rs:80).
 *
 * Same conventions as zkcp_amd.h (which this header includes): plain pointers and sizes, Montgomery field elements as
 * little-endian u64 limbs, affine points (x, y) with infinity = (0, 0), negative zk_status on error.
 */
#ifndef ZKCP_AMD_PROVER_H
#define ZKCP_AMD_PROVER_H

#include "zkcp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ZK_PAIRING_BN254 = 0,       /* ark-bn254 0.3: G1 = ZK_BN254_G1, G2 = ZK_BN254_G2 */
    ZK_PAIRING_BLS12_381 = 1    /* ark-bls12-381 0.3 -- the reference's PairingEngine (lib/src/lib.rs:21-24) */
} zk_pairing_t;

/* ---- ark-serialize 0.3 wire formats (host memory on both sides) ----
 * A point is serialized as x (and y when uncompressed) in canonical, non-Montgomery little-endian bytes with the two
 * SWFlags bits in the top of the last byte: bit 7 = y is the larger of (y, -y), bit 6 = infinity.
 *   compressed = 1: CanonicalSerialize::serialize            (48 B G1 / 96 B G2 on BLS12-381; 32 / 64 on BN254)
 *   compressed = 0: serialize_uncompressed = serialize_unchecked (96 / 192; 64 / 128); infinity is (0, 1) + flag
 * Decoding uncompressed points follows deserialize_unchecked (no curve / subgroup check) unless check_on_curve is set;
 * decoding compressed points recovers y (p = 3 mod 4 square roots; complex method on Fq2) and fails with
 * ZK_ERR_INVALID_ARG on a non-canonical coordinate, an invalid flag pair or an x that is not on the curve. */
int zk_ark_point_size(zk_curve_t c, int compressed);
int zk_ark_points_encode(zk_curve_t c, const void *affine_mont, uint64_t n, int compressed, uint8_t *out);
int zk_ark_points_decode(zk_curve_t c, const uint8_t *in, uint64_t n, int compressed, int check_on_curve, void *affine_mont_out);

/* The CHECKED decoders: GroupAffine::deserialize (compressed = 1) / the checked deserialize_uncompressed (compressed = 0) of
 * ark-ec 0.3 -- what CanonicalDeserialize::deserialize runs for every element of a Vec, e.g. read_verifying_key at
 * lib/src/utils.rs:112-118.  Per point, in this order: canonical coordinates (reason 1), a valid flag pair (2), the infinity
 * flag (decoded as (0, 0) like zk_ark_points_decode), y recovered by the square root and chosen by the sign flag, or the curve
 * equation for an uncompressed point (3), and is_in_correct_subgroup_assuming_on_curve, [r] P == O (4).  A refused input returns
 * ZK_ERR_INVALID_ARG with *first_bad_index = the smallest refused index and *reason as above (both optional, zeroed on entry);
 * the output rows are then unspecified and the library stays usable.
 *   zk_ark_points_decode_checked         host memory on both sides; BN254 and BLS12-381, G1 and G2 (ZK_ERR_UNSUPPORTED for the
 *                                        Pasta curves, which have no arkworks wire format); large vectors use all host threads
 *   zk_ark_points_decode_checked_device  ZK_BN254_G1 and ZK_BLS12_381_G1: encoded bytes in host memory -> affine Montgomery points
 *                                        in device memory (16-B aligned, n rows, the layout zk_bases_adopt_device takes), one GPU
 *                                        lane per point.  One copy to the device, one launch; synchronises hip_stream once, at
 *                                        the end, to read the status word.  Staging: n encoded points in the stream's scratch. */
int zk_ark_points_decode_checked(zk_curve_t c, const uint8_t *in, uint64_t n, int compressed, void *affine_mont_out, uint64_t *first_bad_index,
                                 uint64_t *reason);
int zk_ark_points_decode_checked_device(zk_curve_t c, const uint8_t *in_host, uint64_t n, int compressed, void *affine_mont_out_dev,
                                        uint64_t *first_bad_index, uint64_t *reason, void *hip_stream);

/* Fr elements: canonical little-endian 32 bytes (ark-ff 0.3 Fp256::serialize) <-> Montgomery limbs */
int zk_ark_scalars_encode(zk_field_t f, const void *mont, uint64_t n, uint8_t *out);
int zk_ark_scalars_decode(zk_field_t f, const uint8_t *in, uint64_t n, void *mont_out);

/* Layout of ProvingKey::<E>::serialize_unchecked (ark-groth16 0.3; field order vk { alpha_g1, beta_g2, gamma_g2, delta_g2,
 * gamma_abc_g1 }, beta_g1, delta_g1, a_query, b_g1_query, b_g2_query, h_query, l_query; a Vec is a u64 length followed by
 * its items): byte offset of the first point and number of points of every member, so that a key file the reference's
 * `compile` wrote (lib/src/utils.rs:85-102) can be uploaded member by member without an intermediate copy. */
typedef struct {
    uint64_t offset, count;
} zk_ark_span;
typedef struct {
    zk_ark_span alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, beta_g1, delta_g1, a_query, b_g1_query, b_g2_query, h_query, l_query;
    uint64_t total_bytes;
} zk_ark_pk_index;
int zk_ark_proving_key_index(zk_pairing_t p, const uint8_t *buf, uint64_t len, zk_ark_pk_index *out);

/* decode n uncompressed points (a query vector located with zk_ark_proving_key_index) into a resident bases handle */
int zk_bases_upload_ark(zk_curve_t c, const uint8_t *uncompressed_points, uint64_t n, uint64_t *handle_out);

/* ark-groth16 0.3 Proof { a: G1, b: G2, c: G1 }, compressed: 192 bytes on BLS12-381 (128 on BN254) -- what the reference
 * stores as `proof_of_encryption` (lib/src/zk/verifiable_encryption.rs:23-27) */
int zk_ark_proof_size(zk_pairing_t p);
int zk_ark_proof_encode(zk_pairing_t p, const void *a_g1_affine_mont, const void *b_g2_affine_mont, const void *c_g1_affine_mont, uint8_t *out);
int zk_ark_proof_decode(zk_pairing_t p, const uint8_t *in, void *a_g1_affine_mont, void *b_g2_affine_mont, void *c_g1_affine_mont);

/* ---- Groth16 around the MSM / NTT path (ark-groth16 0.3 create_proof; call sites
 * lib/src/zk/encryption.rs:76, verifiable_encryption.rs:92, sample_entries.rs:86, property.rs:133) ----
 *
 * R1CS matrices (ark-relations 0.3 ConstraintMatrices { a, b, c }: one Vec<(coeff, variable index)> per constraint) are
 * fixed per circuit like the proving key: uploaded once in CSR form (row_ptr: n_rows + 1 offsets; col_idx / val per term,
 * val in Montgomery form), resident on the home device.
 *   Rows: a row may have no term (row_ptr[i + 1] == row_ptr[i]; its product is 0), n_rows may be 0 (row_ptr = {0}) and so may
 *   the number of terms (col_idx_host / val_mont_host are then not read).  Terms need not be sorted by column, and a column may
 *   occur more than once in a row: like upstream's evaluate_constraint the products sum every term, so duplicates add up.  A
 *   coefficient of 0 is an ordinary term.
 *   Refused with ZK_ERR_INVALID_ARG: row_ptr[0] != 0, a decreasing row_ptr, a col_idx >= n_cols, n_cols >= 2^32. */
int zk_r1cs_matrix_upload(zk_field_t f, const uint64_t *row_ptr_host, const uint32_t *col_idx_host, const void *val_mont_host,
                          uint64_t n_rows, uint64_t n_cols, uint64_t *handle_out);
int zk_r1cs_matrix_free(uint64_t handle);
/* out[i] = <row i, z> for i < n_rows, 0 for n_rows <= i < out_len  (upstream: evaluate_constraint per row).  z holds n_cols
 * elements.  out_len >= n_rows, else ZK_ERR_INVALID_ARG and nothing is written; every one of the out_len elements is written
 * (the caller's buffer need not be cleared), so out_len = the domain size gives the zero-padded evaluation vector directly. */
int zk_r1cs_matvec_device(uint64_t matrix, const void *z_mont_dev, void *out_mont_dev, uint64_t out_len, void *hip_stream);
/* R1CStoQAP::witness_map from the full assignment z (instance variables first, z[0] = 1), all in HBM:
 *   a = A z, b = B z, c = C z on the first num_constraints rows; a[num_constraints + j] = z[j] for j < num_inputs;
 *   then the seven NTTs and the pointwise glue of zk_groth16_witness_map_device.  a_dev / b_dev / c_dev are caller
 *   buffers of 2^log_m elements; on return a_dev holds h.  All three matrices must have the same number of rows
 *   and num_constraints + num_inputs <= 2^log_m. */
int zk_groth16_witness_map_r1cs_device(zk_field_t f, uint64_t matrix_a, uint64_t matrix_b, uint64_t matrix_c, const void *z_mont_dev,
                                       uint64_t num_inputs, uint32_t log_m, void *a_dev, void *b_dev, void *c_dev, void *hip_stream);

/* The last step of create_proof: the proof from the five MSM results, the key's single elements and the blinding r, s.
 *   A = a_query[0] + a_acc + alpha_g1 + r delta_g1
 *   B = b_g2_query[0] + b_g2_acc + beta_g2 + s delta_g2          (B1 likewise in G1, used for C only)
 *   C = s A + r B1 - r s delta_g1 + l_acc + h_acc
 * Points of the key are affine (x, y) Montgomery; the *_acc are the Jacobian outputs of zk_msm* over query[1..] ; r, s are
 * Fr elements in Montgomery form.  Host arithmetic (a handful of scalar multiplications), like upstream. */
typedef struct {
    const void *alpha_g1, *beta_g1, *delta_g1;
    const void *beta_g2, *delta_g2;
    const void *a_query0, *b_g1_query0, *b_g2_query0;
    const void *a_acc, *b_g1_acc, *l_acc, *h_acc;
    const void *b_g2_acc;
    const void *r, *s;
} zk_groth16_assembly;
int zk_groth16_assemble_proof(zk_pairing_t p, const zk_groth16_assembly *in, void *a_g1_affine_out, void *b_g2_affine_out,
                              void *c_g1_affine_out);

/* ---- Groth16 verification (ark-groth16 0.3 verifier.rs; the reference's buyer reaches Groth16::verify at
 * lib/src/zk/encryption.rs:152, sample_entries.rs:126, property.rs:177 after read_verifying_key) ----
 * prepare_inputs, g_ic = gamma_abc_g1[0] + sum_i x_i gamma_abc_g1[i + 1], is one zk_msm_device over the resident gamma_abc_g1[1..]
 * (the output of zk_ark_points_decode_checked_device adopted with zk_bases_adopt_device) with scalars_are_montgomery = 1, plus
 * one zk_point_add; upstream runs a serial loop of scalar multiplications.  What is left is the pairing check, on the host:
 *
 * gt_out = final_exponentiation(prod_{i < n} miller_loop(g1[i], g2[i])): the optimal ate pairing, e(P, Q) = f^((p^12 - 1) / r)
 * exactly, as 12 Fq coefficients in Montgomery limbs in ark's Fp12 order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ... over
 * Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v); xi = 1 + u on BLS12-381, 9 + u on BN254).
 * g1 / g2: n affine Montgomery points each; a pair with the identity (0, 0) in either slot contributes 1; n = 0 gives 1.  The
 * points must lie in their r-order subgroups (the checked decoders above establish that); other input gives an unspecified value. */
int zk_pairing_product(zk_pairing_t p, const void *g1_affine, const void *g2_affine, uint64_t n, void *gt_out);
/* verifier.rs prepare_inputs: g_ic = gamma_abc_g1[0] + sum_{i < n_inputs} x_i gamma_abc_g1[i + 1], affine Montgomery, host memory.
 * gamma_abc_tail_bases: a bases handle over gamma_abc_g1[1..] (gamma_abc_len - 1 points; not looked at when n_inputs = 0);
 * gamma_abc0_affine: gamma_abc_g1[0], host; inputs_mont_dev: the public inputs as Montgomery Fr elements in device memory.
 * n_inputs + 1 != gamma_abc_len is upstream's MalformedVerifyingKey: ZK_ERR_INVALID_ARG, and nothing is launched.
 * One zk_msm_device (scalars_are_montgomery = 1) on hip_stream and one host addition. */
int zk_groth16_prepare_inputs(zk_curve_t g1, uint64_t gamma_abc_tail_bases, const void *gamma_abc0_affine, uint64_t gamma_abc_len,
                              const void *inputs_mont_dev, uint64_t n_inputs, void *g_ic_affine_out, void *hip_stream);
/* verify_proof_with_prepared_inputs: *ok = (e(A, B) e(g_ic, -gamma_g2) e(C, -delta_g2) == e(alpha_g1, beta_g2)).
 * alpha_g1_beta_g2: the right-hand side as zk_pairing_product writes it (PreparedVerifyingKey caches it), NULL = compute it.
 * prepared_inputs_g1 = g_ic, affine.  A false proof gives *ok = 0 and returns ZK_OK; errors are for malformed arguments. */
typedef struct {
    const void *alpha_g1, *beta_g2, *gamma_g2, *delta_g2;
} zk_groth16_vk_points;
int zk_groth16_verify(zk_pairing_t p, const zk_groth16_vk_points *vk, const void *alpha_g1_beta_g2, const void *prepared_inputs_g1,
                      const void *a_g1, const void *b_g2, const void *c_g1, uint64_t *ok);

/* ---- Groth16 key generation (ark-groth16 0.3 generator.rs generate_parameters; the reference's `compile` reaches it through
 * Groth16::setup at lib/src/zk/encryption.rs:169, sample_entries.rs:141, property.rs:192) ----
 * From the resident matrices to the scalars of the key's point vectors; the points themselves are zk_fixed_base_msm_device over
 * those scalars (scalars_are_montgomery = 1).  Device buffers of Montgomery elements, trapdoor scalars in host memory.
 * Every entry refuses with ZK_ERR_INVALID_ARG before it launches anything and leaves the library usable.
 *
 * out[j] = sum_{i < min(x_len, n_rows)} M[i][j] x[i] for j < n_cols, 0 for n_cols <= j < out_len (out_len >= n_cols): the product
 * with the TRANSPOSED matrix -- upstream walks the rows and scatters `u[index] += coeff * x[i]`.  There are no 256-bit field
 * atomics, so this is a gather over a column-major copy of the matrix, which the first such call on a handle builds on the
 * device (histogram of col_idx, scan, scatter; synchronises hip_stream once) and zk_r1cs_matrix_free releases. */
int zk_r1cs_matvec_transposed_device(uint64_t matrix, const void *x_mont_dev, uint64_t x_len, void *out_mont_dev, uint64_t out_len,
                                     void *hip_stream);
/* ark-poly 0.3 Radix2EvaluationDomain::evaluate_all_lagrange_coefficients(tau) on the size-2^log_m domain, tau outside it:
 *   out[i] = L_i(tau) = (tau^m - 1) / m * w^i / (tau - w^i), i < m;  zt_out_host (optional) = tau^m - 1 = evaluate_vanishing_polynomial.
 * tau^m = 1 is refused (upstream samples tau outside the domain; that branch is not provided). */
int zk_lagrange_coefficients_device(zk_field_t f, uint32_t log_m, const void *tau_mont_host, void *out_dev, void *zt_out_mont_host,
                                    void *hip_stream);
/* r1cs_to_qap.rs LibsnarkReduction::instance_map_with_evaluation: with L = the Lagrange coefficients at tau (stream scratch),
 *   u[j] = sum_i A[i][j] L_i + (j < num_inputs ? L_{num_constraints + j} : 0),  v[j] = sum_i B[i][j] L_i,  w[j] = sum_i C[i][j] L_i
 * for j < n_vars (n_vars >= every matrix's n_cols; the tail is zero).  Same preconditions as zk_groth16_witness_map_r1cs_device:
 * equal row counts, num_constraints + num_inputs <= 2^log_m; num_inputs <= n_vars. */
int zk_groth16_qap_at_device(zk_field_t f, uint64_t matrix_a, uint64_t matrix_b, uint64_t matrix_c, uint64_t num_inputs, uint32_t log_m,
                             const void *tau_mont_host, void *u_dev, void *v_dev, void *w_dev, uint64_t n_vars, void *zt_out_mont_host,
                             void *hip_stream);
/* generate_parameters, the scalars that are not u or v themselves (a_query = u, b_g1_query = b_g2_query = v):
 *   abc_dev[j] = (beta u[j] + alpha v[j] + w[j]) / gamma for j < num_inputs (gamma_abc_g1), / delta for the rest (l_query), n_vars
 *                elements in one pass; abc_dev may be one of u_dev, v_dev, w_dev;
 *   h_dev[i]   = tau^i * zt / delta, i < 2^log_m - 1 (h_query).
 * gamma = 0, delta = 0 or zt = 0 is refused (upstream unwraps the inverses). */
int zk_groth16_key_scalars_device(zk_field_t f, const void *u_dev, const void *v_dev, const void *w_dev, uint64_t n_vars, uint64_t num_inputs,
                                  uint32_t log_m, const void *alpha_mont_host, const void *beta_mont_host, const void *gamma_mont_host,
                                  const void *delta_mont_host, const void *tau_mont_host, const void *zt_mont_host, void *abc_dev,
                                  void *h_dev, void *hip_stream);

/* ---- halo2_proofs 0.2 prover steps beyond commit / FFT, device buffers, Montgomery elements ----
 * The reference's circuit (circuits-halo2/src/encryption.rs:83-161: 13 advice + 8 fixed columns, a lookup table, a
 * permutation over the equality-enabled columns) is the shape donor; these are the per-row products a create_proof over
 * it runs between the column commitments and the opening.  Blinding rows / scalars and the transcript stay with the
 * caller (RNG and hashing on the CPU), like upstream's structure. */

/* arithmetic.rs BatchInvert: a[i] <- 1 / a[i], zeros stay zero */
int zk_batch_invert_device(zk_field_t f, void *a_dev, uint64_t n, void *hip_stream);
/* out[i] = first * prod_{j < i} in[j] (in == out allowed); first NULL = 1; total_out_host (optional, synchronises) =
 * first * prod of all -- the running value the next chunk of a permutation argument starts from */
int zk_prefix_product_device(zk_field_t f, const void *in_dev, void *out_dev, uint64_t n, const void *first_mont_host,
                             void *total_out_mont_host, void *hip_stream);
/* plonk/permutation/prover.rs Argument::commit, one chunk of <= 8 columns (chunk_len = degree - 2) on the 2^k-row domain:
 *   Z(0) = z_first (NULL = 1);  Z(i + 1) = Z(i) prod_c (v_c(i) + beta delta^(first_column_index + c) omega^i + gamma)
 *                                              / prod_c (v_c(i) + beta sigma_c(i) + gamma)
 * columns_dev / sigmas_dev: host arrays of ncols device pointers (Lagrange form).  z_out_dev gets Z(0 .. 2^k);
 * z_last_out_host (optional, synchronises) the value after the last row. */
int zk_halo2_permutation_product_device(zk_field_t f, uint32_t ncols, const void *const *columns_dev, const void *const *sigmas_dev,
                                        uint32_t first_column_index, const void *beta, const void *gamma, const void *delta, uint32_t k,
                                        const void *z_first, void *z_out_dev, void *z_last_out_host, void *hip_stream);
/* plonk/lookup/prover.rs commit_product: Z(0) = 1, Z(i + 1) = Z(i) (A_i + beta)(S_i + gamma) / ((A'_i + beta)(S'_i + gamma));
 * A', S' are the permuted input / table expressions (zk_halo2_permute_expression_pair_device below) */
int zk_halo2_lookup_product_device(zk_field_t f, const void *a_dev, const void *s_dev, const void *a_perm_dev, const void *s_perm_dev,
                                   const void *beta, const void *gamma, uint64_t n, void *z_out_dev, void *z_last_out_host, void *hip_stream);
/* plonk/lookup/prover.rs permute_expression_pair, the deterministic part: the compressed input expression A and table
 * expression S (Montgomery, n x 4 u64, 16-B aligned) -> the permuted pair A', S'.  Reads rows [0, usable_rows) of each input
 * and writes exactly rows [0, usable_rows) of each output; rows from usable_rows on are left to the caller's blinding rows.
 * The inputs are not modified.
 *   A'  the inputs sorted by the field's Ord (canonical integers, not Montgomery limbs);
 *   S'  at the first row of every run of equal values in A' that value; the leftover table values, ascending, fill the
 *       repeated-input rows from the last one up (upstream's repeated_input_rows.pop()).
 * An input value that is not in the table returns ZK_ERR_LOOKUP (upstream: Error::ConstraintSystemFailure); A', S' are then
 * unspecified and the library stays usable.  All work is enqueued on hip_stream; the call synchronises it once, at the end,
 * to read the status word.  ZK_ERR_INVALID_ARG: null or misaligned pointers, outputs that overlap each other or either
 * input, usable_rows >= 2^31.  usable_rows = 0 does nothing.  Scratch: about 160 B per usable row, owned by the stream. */
int zk_halo2_permute_expression_pair_device(zk_field_t f, const void *inputs_dev, const void *table_dev, uint64_t usable_rows,
                                            void *a_perm_dev, void *s_perm_dev, void *hip_stream);
/* ---- halo2_proofs 0.2 key generation (plonk/keygen.rs keygen_vk / keygen_pk, plonk/permutation/keygen.rs Assembly) ----
 * Every transform of the key goes through the NTT entry points of zkcp_amd.h (ZK_NTT_OUT_R29 for the lazy form), every commitment
 * through zk_msm_batch_device, Assigned fixed columns through zk_batch_invert_device (a zero denominator gives 0, upstream's rule);
 * what is left is the copy-constraint permutation and its columns.  Circuit synthesis, floor planning, compress_selectors and the
 * key's transcript representation stay with the caller.
 *
 * plonk/permutation/keygen.rs Assembly::new(n, columns): mapping[c][r] = aux[c][r] = (c, r), sizes[c][r] = 1 over ncols columns of
 * n rows, in host memory (the walk of a cycle is sequential by definition).  ncols x n must stay below 2^32 cells (16 B a cell). */
int zk_halo2_assembly_new(uint64_t n, uint32_t ncols, uint64_t *handle_out);
/* Assembly::copy(left_column, left_row, right_column, right_row) for `count` quadruples of quads_host, applied in order: a copy
 * inside one cycle does nothing; otherwise the larger cycle (the left one on a tie) absorbs the other and mapping[left], mapping[right]
 * are swapped, so the permutation depends on the order of the calls exactly as upstream's does.  A row >= n or a column >= ncols
 * (upstream: Error::BoundsFailure) stops the walk with ZK_ERR_INVALID_ARG: the earlier copies stay applied, the rest are not
 * looked at, and *applied_out (optional) = how many were applied.  ZK_ERR_BAD_HANDLE for an unknown or freed handle. */
int zk_halo2_assembly_copy(uint64_t handle, const uint32_t *quads_host, uint64_t count, uint64_t *applied_out);
/* the permutation as it stands: ncols x n words, mapping_out_host[c * n + r] = column << 32 | row of the cell that (c, r) maps to */
int zk_halo2_assembly_mapping(uint64_t handle, void *mapping_out_host);
int zk_halo2_assembly_free(uint64_t handle);
/* Assembly::build_vk / build_pk, the permutation columns in Lagrange form on the 2^k-row domain:
 *   sigmas_dev[c * n + j] = delta^col * omega^row   for mapping_dev[c * n + j] = col << 32 | row   (upstream: deltaomega[col][row])
 * delta: FieldExt::DELTA in Montgomery form, host; omega: the domain's generator.  Column c is sigmas_dev + c * n, usable as it is
 * as a sigmas_dev entry of zk_halo2_permutation_product_device.  The mapping is device data the library did not produce: a cell
 * whose row >= n or column >= ncols is never used as an index, gets 0 in its own slot, and the call returns ZK_ERR_INVALID_ARG;
 * the library stays usable.  Also ZK_ERR_INVALID_ARG, before anything is launched: null or misaligned (16 B) pointers, buffers
 * that overlap, ncols = 0, k above the field's two-adicity, 2^k * ncols >= 2^32.  Synchronises hip_stream once, at the end, to
 * read the status word. */
int zk_halo2_permutation_sigmas_device(zk_field_t f, uint32_t k, uint32_t ncols, const void *mapping_dev, const void *delta_mont_host,
                                       void *sigmas_dev, void *hip_stream);

/* poly/commitment/prover.rs create_proof, the scalar side of one round: compute_inner_product, and the folds
 * p'[i] += u^-1 p'[i + half], b[i] += u b[i + half] as a[i] += c a[i + half] */
int zk_inner_product_device(zk_field_t f, const void *a_dev, const void *b_dev, uint64_t n, void *out_mont_host, void *hip_stream);
int zk_vec_fold_device(zk_field_t f, void *a_dev, uint64_t half, const void *c_mont_host, void *hip_stream);
/* poly/multiopen/prover.rs: a[i] = a[i] * s + b[i] -- one Horner step of folding the polynomials queried at the same point set with
 * powers of x_1 (and the per-set quotients with x_4), on resident coefficient vectors.  s: Montgomery, host. */
int zk_vec_muladd_device(zk_field_t f, void *a_dev, const void *b_dev, uint64_t n, const void *s_mont_host, void *hip_stream);
/* ... out[i] = a[i] * s + b[i] into a third buffer (out == a or out == b allowed; otherwise disjoint): the first step of such a fold starts
 * from two resident polynomials and must clobber neither (upstream clones; this saves the copy) */
int zk_vec_muladd_to_device(zk_field_t f, void *out_dev, const void *a_dev, const void *b_dev, uint64_t n, const void *s_mont_host, void *hip_stream);
/* arithmetic.rs eval_polynomial: p(x) = sum_i coeffs[i] x^i for a resident coefficient vector (the evaluations create_proof
 * writes to the transcript: every committed polynomial at x and at its rotations omega^r x).  x, the result: Montgomery, host. */
int zk_poly_eval_device(zk_field_t f, const void *coeffs_dev, uint64_t n, const void *x_mont_host, void *out_mont_host, void *hip_stream);
/* ... `count` polynomials of n coefficients (polynomial q at element offset q * stride_elems) at the same x: one launch, one copy */
int zk_poly_eval_batch_device(zk_field_t f, const void *coeffs_dev, uint64_t n, uint32_t count, uint64_t stride_elems, const void *x_mont_host,
                              void *out_mont_host, void *hip_stream);
/* out[j] = sum_{i < count} s^(count - 1 - i) src_i[j] with src_i = first_dev + i * stride_elems (stride may be negative: walk the
 * polynomials backwards): the Horner fold of `count` resident polynomials in one pass, each read once (the x_1 fold of a point set
 * in poly/multiopen/prover.rs; h(X) = sum_i x^(n i) h_i in plonk/vanishing/prover.rs with first = the LAST piece, stride = -n).
 * out_dev may be one of the sources or disjoint from all of them. */
int zk_vec_fold_many_device(zk_field_t f, void *out_dev, const void *first_dev, int64_t stride_elems, uint32_t count, uint64_t n,
                            const void *s_mont_host, void *hip_stream);
/* one round's three folds of the inner-product argument in one launch: p'[i] += u^-1 p'[i + half], b[i] += u b[i + half] for i < half,
 * and (w_dev != NULL, the fold-free form) W[idx] *= u where idx < m0 has bit `half` set.  u != 0. */
int zk_ipa_fold_round_device(zk_field_t f, void *p_dev, void *b_dev, void *w_dev, uint64_t half, uint64_t m0, const void *u_mont_host,
                             void *hip_stream);
/* out[i] = x^i, i < n: the vector b of poly/commitment/prover.rs create_proof (powers of x_3), built from per-call power tables of x */
int zk_vec_powers_device(zk_field_t f, void *out_dev, uint64_t n, const void *x_mont_host, void *hip_stream);
/* arithmetic.rs kate_division(a, x): the quotient of (a(X) - a(x)) / (X - x) as n coefficients (upstream returns n - 1 and
 * poly/multiopen/prover.rs resizes to n: q[n - 1] = 0); the multiopen argument divides every point set's folded polynomial by
 * (X - x_j) for each point of the set in turn, which leaves the quotient by the set's vanishing polynomial.  q_dev == a_dev
 * (in place) or disjoint.  A three-phase suffix scan (q[j] = a[j + 1] + x q[j + 1]), ~3 products per coefficient. */
int zk_kate_division_device(zk_field_t f, const void *a_dev, void *q_dev, uint64_t n, const void *x_mont_host, void *hip_stream);
/* ... and the generator side (parallel_generator_collapse): g[i] <- affine(g[i] + [u] g[i + half]), i < half; g holds
 * 2 * half affine points (x, y) Montgomery on the device, u an element of the curve's scalar field (Montgomery, host) */
int zk_ipa_fold_bases_device(zk_curve_t c, void *g_affine_dev, uint64_t half, const void *u_mont_host, void *hip_stream);

/* The same rounds WITHOUT folding the generators (a fold is one ~255-bit scalar multiplication per surviving point and round;
 * an MSM is ~16 bucket additions per point): with W[idx] the product of the challenges whose fold put idx in an upper half,
 *   L = MSM(G0, S_L), R = MSM(G0, S_R) over the ORIGINAL m0 generators (the resident SRS handle, one zk_msm_batch_device call)
 *   S_L[idx] = p'[i + cur/2] W[idx] for i = idx mod cur < cur/2 (else 0);  S_R[idx] = p'[i - cur/2] W[idx] for i >= cur/2 (else 0)
 * zk_ipa_virtual_scalars_device fills S_L, S_R (m0 elements each); after the round's challenge u (and the p', b folds)
 * zk_ipa_update_weights_device multiplies W[idx] by u where idx has bit cur/2 set.  W starts as all ones; the folded
 * generator at the end is MSM(G0, W) (the prover does not need it). */
int zk_ipa_virtual_scalars_device(zk_field_t f, const void *p_dev, const void *w_dev, uint64_t m0, uint64_t cur, void *sl_dev, void *sr_dev,
                                  void *hip_stream);
int zk_ipa_update_weights_device(zk_field_t f, void *w_dev, uint64_t m0, uint64_t bit, const void *u_mont_host, void *hip_stream);
/* One whole fold-free round in one call (zk_ipa_virtual_scalars_device + two zk_inner_product_device + zk_msm_batch_device without
 * a host round trip per value): s_dev = scratch for 2 * m0 scalars; lr_out_host = L, R as Jacobian points (2 x 3 coordinates);
 * v_out_mont_host = <p'_hi, b_lo>, <p'_lo, b_hi>. */
int zk_ipa_round_device(zk_curve_t c, uint64_t bases_handle, const void *p_dev, const void *b_dev, const void *w_dev, uint64_t m0,
                        uint64_t cur, void *s_dev, void *lr_out_host, void *v_out_mont_host, void *hip_stream);
/* ... and to leave the fold-free form after r of those rounds: the generators r calls of parallel_generator_collapse would
 * have produced, g_out[i] = sum_{t < m0 / cur} W[t cur] G0[t cur + i] for i < cur (affine (x, y) Montgomery, identity (0, 0)),
 * as cur multi-scalar multiplications that share their m0 / cur <= 4096 scalars.  The later rounds then run over g_out
 * (zk_bases_adopt_device) with fresh weights: a few full-size rounds cost a full-size MSM each, the many small ones do not.
 * Synchronises hip_stream: g_out is complete on return. */
int zk_ipa_collapse_device(zk_curve_t c, uint64_t bases_handle, const void *w_dev, uint64_t m0, uint64_t cur, void *g_out_affine_dev,
                           void *hip_stream);
/* ... outputs [first, first + count) only, written to g_out_range_dev[0 .. count): a rank's share when several GPUs split the step
 * (the shares are exchanged with one all_gather: contangle-zkcp_amd/halo2.py IpaProverVirtual.collapse) */
int zk_ipa_collapse_range_device(zk_curve_t c, uint64_t bases_handle, const void *w_dev, uint64_t m0, uint64_t cur, uint64_t first,
                                 uint64_t count, void *g_out_range_dev, void *hip_stream);

/* Shift tables for the collapse above: [2^64] G_i, [2^128] G_i, [2^192] G_i beside the handle's points (3 x the lazy-limb copy more:
 * 192 MiB for a 2^20-point Pasta key), so that every 255-bit weight is four 64-bit scalars over four points -- 11 six-bit windows
 * instead of 52 five-bit ones, and 60 doublings per survivor instead of 255.  The generators of poly/commitment/prover.rs
 * create_proof are Params::g, the same from proof to proof: call this once where the key is loaded (poly/commitment.rs
 * Params::new / Params::read).  One inversion per table entry; synchronises.  Without the call the library builds the tables by
 * itself at the SECOND collapse over a handle of at least 2^16 points (the first runs without them, so does every collapse over a
 * smaller or short-lived handle, and so does everything when the allocation fails).  zk_bases_refresh drops the tables: call
 * again after rewriting the points.  ZK_IPA_SHIFT_TABLES=0 in the environment (read once) turns tables off: nothing is built,
 * here or automatically.  The collapse returns canonical affine points: the same bits with or without tables. */
int zk_bases_precompute_shifts(zk_curve_t c, uint64_t bases_handle);
/* *present = 1 when every device's copy of the handle holds shift tables at the moment, else 0 */
int zk_bases_shift_tables(uint64_t bases_handle, uint64_t *present);

/* ---- halo2 verification (halo2_proofs 0.2 poly/commitment/verifier.rs verify_proof / Guard, poly/commitment/msm.rs MSM) ----
 * The opening check ends in ONE multi-scalar multiplication over the whole SRS, whose scalars are compute_s of the k round
 * challenges.  That vector is built here; the MSM is zk_msm_device over the resident g with scalars_are_montgomery = 1, the few
 * listed terms (S, L_j, R_j, U, W) are one small zk_msm, the partial sums meet in zk_point_add and the identity test is
 * zk_point_to_affine == (0, 0).  The MSM / Guard bookkeeping is contangle-zkcp_amd/halo2.py (MSM, commitment_verify_proof, Guard,
 * verify_batch); the transcript stays with the caller.
 *
 * verifier.rs compute_s(u, init), for `count` proofs in one pass over the vector (Guard::use_challenges adds compute_s(u, neg_c)
 * to MSM::g_scalars; with many proofs behind one MSM -- the BatchVerifier strategy -- every proof adds its own):
 *   s_dev[i] (= or +=, by `accumulate`) sum_{p < count} init_p * prod_{j < k} u_{p,j}^bit_(k-1-j)(i),   i < 2^k
 * u_mont_host: count x k elements, proof-major, u_{p,0} (the first round's challenge, the top bit of i) first; init_mont_host: count
 * elements; both host memory, 16-B aligned, read before the call returns.  s_dev: 2^k elements, device, 16-B aligned; each is
 * written once, and read once only when accumulating.  With init = 1 this is the final weight vector of the fold-free prover
 * (k calls of zk_ipa_update_weights_device on a vector of ones).  A zero challenge is just a product.  Up to 8 proofs share one
 * pass; a larger count is chunked inside, later chunks accumulating.  Scratch, owned by the stream: 32 B x (2^min(k, 8) +
 * 2^(k - min(k, 8))) per proof of a chunk.  Does not synchronise hip_stream.  ZK_ERR_INVALID_ARG, before anything is launched: a
 * null or misaligned (16 B) pointer, count = 0, k = 0, k above the field's two-adicity. */
int zk_halo2_ipa_s_device(zk_field_t f, uint32_t k, uint32_t count, const void *u_mont_host, const void *init_mont_host, void *s_dev,
                          int accumulate, void *hip_stream);
/* verifier.rs compute_b(x, u) = prod_{j < k} (1 + u_j x^(2^(k-1-j))) = sum_i compute_s(u, 1)[i] x^i: k products on host limbs
 * (Montgomery in and out).  ZK_ERR_INVALID_ARG: a null pointer, k = 0, k above the field's two-adicity. */
int zk_halo2_ipa_compute_b(zk_field_t f, uint32_t k, const void *x_mont_host, const void *u_mont_host, void *out_mont_host);

/* The quotient numerator: one stack program evaluated at every row of the extended domain (plonk/prover.rs: each gate's
 * Expression over advice / fixed / instance columns with rotations, folded with y).  A rotation by r rows is a shift of
 * r * rot_scale positions (rot_scale = 2^(extended_k - k)), cyclic.  The program must leave exactly one value; it is
 * validated on the host (operand indices, stack depth <= 8, <= 512 ops, <= 64 columns, <= 32 constants). */
typedef struct {
    uint8_t op;     /* ZK_EXPR_* */
    uint8_t pad;
    int16_t rot;    /* ZK_EXPR_COL: rotation in rows */
    uint32_t arg;   /* ZK_EXPR_COL: column index; ZK_EXPR_CONST / ZK_EXPR_SCALE: constant index */
} zk_expr_op;
#define ZK_EXPR_COL 0
#define ZK_EXPR_CONST 1
#define ZK_EXPR_ADD 2
#define ZK_EXPR_SUB 3
#define ZK_EXPR_MUL 4
#define ZK_EXPR_NEG 5
#define ZK_EXPR_SCALE 6
int zk_expr_eval_device(zk_field_t f, const zk_expr_op *program_host, uint32_t n_ops, const void *const *columns_dev, uint32_t n_columns,
                        const void *consts_mont_host, uint32_t n_consts, uint32_t log_n_ext, uint32_t rot_scale, void *out_dev,
                        void *hip_stream);

/* The same evaluation on lazy 29-bit limbs (one MAD per partial product, carry-free additions): the columns must hold x R' mod p
 * with R' = 2^261 -- what the NTT entry points write when their scale argument has ZK_NTT_OUT_R29 set (zkcp_amd.h), or
 * zk_vec_op_device(scale) by 2^5 for key material -- as canonical 256-bit words.  Constants come in the usual Montgomery form and
 * the OUTPUT is in the usual form too.  The host walks the program once to place the carry steps and pick the subtraction
 * biases (the bound discipline of csrc/zk_field29.h); same validation and limits as zk_expr_eval_device. */
int zk_expr_eval_lazy_device(zk_field_t f, const zk_expr_op *program_host, uint32_t n_ops, const void *const *columns_r29_dev, uint32_t n_columns,
                             const void *consts_mont_host, uint32_t n_consts, uint32_t log_n_ext, uint32_t rot_scale, void *out_dev,
                             void *hip_stream);

/* ---- MockProver::verify on the device (halo2_proofs 0.2 dev.rs; the reference's only halo2 call is MockProver::run(12, ..) at
 * circuits-halo2/src/encryption.rs:335) ----
 * Does an assignment satisfy a circuit?  Four entries: the three-valued evaluation of gate / lookup expressions, the lookup
 * membership test, the copy-constraint check, and the compaction of a status array into a failure list.  The semantics -- Poison
 * cells, where they deliberately differ from upstream -- are DESIGN.md §5 "MockProver"; contangle-zkcp_amd/halo2.py MockProver puts them together.
 * Every entry refuses with ZK_ERR_INVALID_ARG before it launches anything (null or misaligned pointers, overlapping outputs, k above
 * the field's two-adicity or above 30, an invalid program, poison_from > 2^k, usable_rows > 2^k) and leaves the library usable.
 *
 * zk_halo2_mock_eval_device: n_programs stack programs (the zk_expr_op set above, rotations in rows, cyclic mod 2^k) at every row of
 * the 2^k-row domain, in one launch.  A value is Real(v) or Poison: the cell of column c at a row >= poison_from[c] is Poison; neg
 * keeps the kind; add / sub with a Poison side are Poison; Real(0) * Poison = Real(0) in either order, Real(non-zero) * Poison and
 * Poison * Poison are Poison; scale by the constant 0 makes Poison Real(0), any other constant leaves it Poison.
 *   programs_host   the programs back to back; offsets_host[p] .. offsets_host[p + 1] are program p's ops (n_programs + 1 entries,
 *                   offsets_host[0] = 0, increasing).  Each program: the validation and limits of zk_expr_eval_device (<= 512 ops,
 *                   stack <= 8, <= 64 columns, <= 32 constants, exactly one value left); at most 1024 programs a call.
 *   columns_dev     host array of n_columns device pointers, each 2^k Montgomery elements, 16-B aligned; poison_from_host: n_columns
 *                   rows, each <= 2^k (2^k = never); consts_mont_host: n_consts elements, canonical Montgomery
 *   status_out_dev  n_programs x 2^k bytes, 16-B aligned: status[p * 2^k + i] = 0 Real zero, 1 Real non-zero, 2 Poison
 *   values_out_dev  optional (NULL), n_programs x 2^k elements, 16-B aligned: the value, 0 at a Poison entry
 * Stored cells are taken mod p (a word in [p, 2p) counts as its residue), so the zero test is exact.  Reads the host arrays before it
 * returns (one synchronisation of hip_stream, before the launch); the kernel itself is only enqueued.  Scratch: 8 B per op. */
int zk_halo2_mock_eval_device(zk_field_t f, uint32_t k, const zk_expr_op *programs_host, const uint32_t *offsets_host, uint32_t n_programs,
                              const void *const *columns_dev, const uint64_t *poison_from_host, uint32_t n_columns, const void *consts_mont_host,
                              uint32_t n_consts, void *values_out_dev, uint8_t *status_out_dev, void *hip_stream);
/* A lookup one expression wide, exact: status_out_dev[r] = 1 iff the input of row r < usable_rows is not among the table values of
 * rows [0, usable_rows), else 0; usable_rows bytes are written, rows from usable_rows on are neither read nor written.
 * inputs_dev / table_dev: Montgomery elements, 16-B aligned (the values_out of the evaluator); inputs_status_dev / table_status_dev
 * (optional, NULL = all Real): the evaluator's status bytes, where 2 marks a Poison entry.  Poison compares as upstream's derived
 * order has it, equal to Poison and above every field element: a Poison input passes iff the table holds a Poison entry.
 * The table's canonical values are sorted by the LSD passes of zk_halo2_permute_expression_pair_device, then one lane per input row
 * searches them.  Does not synchronise.  Scratch: 64 B per usable row, owned by the stream.  usable_rows = 0 does nothing. */
int zk_halo2_mock_lookup_device(zk_field_t f, uint32_t k, const void *inputs_dev, const uint8_t *inputs_status_dev, const void *table_dev,
                                const uint8_t *table_status_dev, uint64_t usable_rows, uint8_t *status_out_dev, void *hip_stream);
/* The copy constraints: over the permutation's ncols columns (columns_dev: host array of device pointers, 2^k Montgomery elements
 * each; poison_from_host as above) and the Assembly mapping (mapping_dev: ncols x 2^k words, column << 32 | row, device, 16-B aligned
 * -- what zk_halo2_assembly_mapping hands out),
 *   status_out_dev[c * 2^k + r] = 1 iff mapping[c][r] != (c, r) and (either end is Poison or the two stored values differ), else 0.
 * Stored values are compared as stored.  The mapping is device data the library did not produce: a word that names a row >= 2^k or a
 * column >= ncols is never used as an index, its cell gets 0, and the call returns ZK_ERR_INVALID_ARG; the library stays usable (the
 * contract of zk_halo2_permutation_sigmas_device).  ncols = 0 or 2^k * ncols >= 2^32 is refused.  Synchronises hip_stream twice: after
 * copying the tables, and at the end to read the status word. */
int zk_halo2_mock_permutation_device(zk_field_t f, uint32_t k, uint32_t ncols, const void *const *columns_dev, const uint64_t *poison_from_host,
                                     const void *mapping_dev, uint8_t *status_out_dev, void *hip_stream);
/* The failure list of a status array: positions_out_host[q] / kinds_out_host[q] = the index and the byte of the q-th non-zero byte of
 * status_dev[0 .. n_status) for q < min(*total_out_host, cap), ascending; *total_out_host = the number of non-zero bytes.  Entries past
 * min(total, cap) of the two host arrays are not touched.  status_dev: 16-B aligned (it is read 16 bytes at a time).  The same list
 * on every run: positions come from a reduce / scan / emit sequence, not from atomics.  Synchronises hip_stream once, at the end.
 * Scratch: 12 B per 4096 status bytes and 9 B per reported entry. */
int zk_halo2_mock_failures_device(const uint8_t *status_dev, uint64_t n_status, uint64_t cap, uint64_t *positions_out_host, uint8_t *kinds_out_host,
                                  uint64_t *total_out_host, void *hip_stream);

/* A gate expression is fixed per proving key: for evaluations of 2^16 rows and more zk_expr_eval_lazy_device writes the annotated
 * program out as straight-line HIP (the stack resolved at generation time: no interpreter, no LDS), compiles it once per
 * (program, device) with hiprtc -- ~10 s for the reference circuit's 268 operations; the headers it includes ship next to the
 * library (csrc/, or $ZKCP_AMD_CSRC) -- and runs that: about half the instructions per row.  Same operations, same carry steps,
 * same results.  jit_mode: 0 = that rule (default), 1 = always, 2 = never (the interpreter kernel).  If the specialised kernel
 * cannot be built the interpreter runs. */
int zk_expr_configure(int jit_mode);
/* The HIP source zk_expr_eval_lazy_device would compile for this program (no device needed: diagnostics, and the CPU test tier
 * cross-compiles it).  *len_out = its length; at most cap - 1 bytes and a terminating 0 are written to out (out may be NULL). */
int zk_expr_specialised_source(zk_field_t f, const zk_expr_op *program_host, uint32_t n_ops, uint32_t n_columns, uint32_t n_consts, char *out,
                               uint64_t cap, uint64_t *len_out);

/* ---- Poseidon, the Merkle tree over it, and the ElGamal c2 stream ("Poseidon") ----
 * The reference's seller path outside Groth16::prove: EncryptCircuit::encrypt hashes the shared point and adds the digest to the whole
 * plaintext; SampleEntries::new builds a Poseidon Merkle tree over the ciphertext and opens one path.  The library holds no parameter
 * set: the caller states one and gets a handle.
 *   permutation   round i of full_rounds + partial_rounds: s[j] += ark[i][j]; s[j] = s[j]^alpha for every j in the first and last
 *                 full_rounds / 2 rounds, for j = 0 only in between; s = mds s
 *   hash          of `arity` elements: s = init; the elements are added into s[rate_offset ..), `rate` at a time, a permutation after
 *                 every block (the last included, none extra after a full one); the digest is s[rate_offset].
 *                 ark-sponge 0.3 (PoseidonSponge, CRH, TwoToOneCRH at width 3): rate 2, rate_offset 1, init NULL.
 *                 halo2_gadgets ConstantLength<L> at width 3: rate 2, rate_offset 0, init = (0, 0, L * 2^64).
 * Every element is 4 u64 words, Montgomery; device pointers are 16-B aligned.  ark_mont_host: (full_rounds + partial_rounds) x width,
 * mds_mont_host: width x width (row-major), init_mont_host: width elements or NULL for zeros, all canonical.
 * ZK_ERR_INVALID_ARG, before anything is launched: a null pointer; width outside 2 .. 5; rate = 0 or rate_offset + rate > width; odd
 * full_rounds; full_rounds + partial_rounds = 0 or > 256; alpha = 0; a constant >= p; arity = 0 or > 64; log_n = 0 or > 30; a path
 * index >= 2^log_n; an output overlapping an input.  ZK_ERR_BAD_HANDLE: a handle that was freed or never made.  The library stays
 * usable after every refusal.  create / free / the two *_host entries (the same arithmetic on the CPU's 64-bit multiplier, one
 * thread) need neither a device nor zk_init; the *_device entries return ZK_ERR_NOT_INITIALIZED without one, enqueue on hip_stream
 * and do not synchronise it.  A handle's table goes to a device once, at its first *_device call there; handles outlive zk_shutdown. */
int zk_poseidon_create(zk_field_t f, uint32_t width, uint32_t rate, uint32_t rate_offset, uint32_t full_rounds, uint32_t partial_rounds,
                       uint64_t alpha, const void *ark_mont_host, const void *mds_mont_host, const void *init_mont_host, uint64_t *handle_out);
int zk_poseidon_free(uint64_t handle);
/* count states of `width` elements each, permuted in place */
int zk_poseidon_permute_host(uint64_t handle, void *states_mont_host, uint64_t count);
int zk_poseidon_permute_device(uint64_t handle, void *states_dev, uint64_t count, void *hip_stream);
/* out[i] = hash of in[i * arity .. (i + 1) * arity), i < count.  Inputs must be canonical (< p), as in every vector entry. */
int zk_poseidon_hash_host(uint64_t handle, const void *in_mont_host, uint32_t arity, uint64_t count, void *out_mont_host);
int zk_poseidon_hash_device(uint64_t handle, const void *in_dev, uint32_t arity, uint64_t count, void *out_dev, void *hip_stream);
/* ark MerkleTree::new over n = 2^log_n leaves of leaf_arity elements each (leaf and two-to-one parameters the same, identity digest
 * converter).  nodes_dev: 2n - 1 elements.  Level 0 = the leaf digests at nodes[0 .. n); node i of level j + 1 = hash of
 * (level_j[2i], level_j[2i + 1]); level j starts at 2n - 2^(log_n - j + 1); the root is nodes[2n - 2].  (Upstream's heap order is not
 * mirrored.)  One launch for the leaves, one per level of more than 256 nodes, one for all the levels above: 13 for 2^20 leaves. */
int zk_poseidon_merkle_tree_device(uint64_t handle, const void *leaves_dev, uint32_t leaf_arity, uint32_t log_n, void *nodes_dev, void *hip_stream);
/* out[c * log_n + j] = level_j[(indices[c] >> j) ^ 1], j < log_n: the siblings of leaf indices[c], bottom-up.  The index list is read
 * before the call returns. */
int zk_merkle_paths_device(zk_field_t f, const void *nodes_dev, uint32_t log_n, const uint64_t *indices_host, uint64_t count, void *out_dev,
                           void *hip_stream);
/* out[i] = a[i] + s, i < n (encrypt: s = dh; decrypt: s = -dh).  out_dev may be a_dev itself; any other overlap is refused. */
int zk_vec_add_scalar_device(zk_field_t f, void *out_dev, const void *a_dev, uint64_t n, const void *scalar_mont_host, void *hip_stream);

/* ---- EncryptCircuit (circuits-ark/src/encryption.rs; DESIGN.md section 5, "EncryptCircuit") ----
 * The per-element section of the circuit's assignment, in one launch.  For i < n, with dh the Poseidon digest of the shared point:
 *   m[i]  = msg[i] for i < msg_len, else 0
 *   c2[i] = m[i] + dh for i < msg_len, else 0
 *   b[i]  = 1 if c2[i] != 0, else 0               ("the ciphertext element is not empty")
 *   k[i]  = 1 / c2[i], or 1 where c2[i] = 0       (the multiplier of upstream's is_neq gadget)
 * Elements are 4 u64 words, Montgomery, canonical.  One field inversion per lane is shared among the 16 elements the lane owns.  The four
 * outputs are n elements each, independent of one another: in practice four segments of the assignment.  msg_dev may be NULL when
 * msg_len = 0.  Does not synchronise.
 * ZK_ERR_INVALID_ARG, before anything is launched: a null or not 16-B aligned pointer; two outputs, or an output and msg, that share
 * an address; msg_len > n; n > 2^40; dh >= p. */
int zk_encrypt_witness_device(zk_field_t f, const void *msg_dev, uint64_t msg_len, uint64_t n, const void *dh_mont_host, void *c2_dev, void *m_dev,
                              void *b_dev, void *k_dev, void *hip_stream);
/* bytes_to_plaintext_chunks_direct (utils.rs:60-72): out[i] = byte i as a field element (Montgomery) for i < len, 0 for len <= i < n.
 * Bytes from n on are not read.  Does not synchronise. */
int zk_plaintext_from_bytes_device(zk_field_t f, const uint8_t *bytes_dev, uint64_t len, void *out_dev, uint64_t n, void *hip_stream);
/* ConstraintSystem::is_satisfied, naming the row: *first_row_out_host = the smallest i with <A_i, z> <B_i, z> != <C_i, z>, UINT64_MAX
 * when every row holds.  a, b, c: handles of zk_r1cs_matrix_upload with equal row counts; z_dev: z_len >= their column counts
 * canonical Montgomery elements; scratch_dev: scratch_elems >= 3 rows + ZK_R1CS_CHECK_SCRATCH_ELEMS elements, 16-B aligned, apart
 * from z.  Three mat-vecs and one compare kernel that reduces by minimum in a fixed order (the same row on every run); synchronises
 * hip_stream once, at the end. */
#define ZK_R1CS_CHECK_SCRATCH_ELEMS 256
int zk_r1cs_first_unsatisfied_device(zk_field_t f, uint64_t a, uint64_t b, uint64_t c, const void *z_dev, uint64_t z_len, void *scratch_dev,
                                     uint64_t scratch_elems, uint64_t *first_row_out_host, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* ZKCP_AMD_PROVER_H */
