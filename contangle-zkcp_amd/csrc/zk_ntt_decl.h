// Launch sequences of the scalar-field side (NTT, pointwise, polynomial helpers): the static members of FieldLaunch<F>,
// instantiated per field by the one line of zk_ntt_inst.cc.  Kept apart from zk_internal.h so that adding a field-side
// entry point does not rebuild the (slow) curve units.
#pragma once
#include <string>
#include "zk_internal.h"
#include "zkcp_amd_prover.h"
namespace zk {
constexpr uint32_t R1CS_LONG_ROW = 64;   // rows with more terms are summed by a whole workgroup (zk_r1cs_kernels.h)
// one R1CS matrix (A, B or C of ark-relations' ConstraintMatrices) in CSR form, resident on the home device
struct R1csMatrix {
    int field = 0;
    uint64_t n_rows = 0, n_cols = 0, nnz = 0, n_long = 0;
    void *row_ptr = nullptr, *col = nullptr, *val = nullptr, *long_rows = nullptr;
    // the column-major companion (zk_setup_kernels.h): built on the device at the first transposed product, freed with the handle.
    // col_ptr: n_cols + 1 u32 offsets; t_row / t_val: row index and coefficient per term; long_cols: columns over R1CS_LONG_ROW terms
    bool t_ready = false;
    uint64_t n_long_cols = 0;
    void *col_ptr = nullptr, *t_row = nullptr, *t_val = nullptr, *long_cols = nullptr;
};
struct PoseidonShape;
// Every member is declared here and defined in one of the .inl files that zk_ntt.inl pulls in; the explicit instantiation of the
// class in zk_ntt_inst.cc instantiates them all, so a new launch sequence needs this declaration and its definition, nothing else.
template <class F>
struct FieldLaunch {
    static int ntt_run(DeviceCtx& dc, int field, Fe<F>* a, uint32_t logn, const Fe<F>& omega, int scale_flag, hipStream_t st,
                       const Fe<F>* g_pre = nullptr, const Fe<F>* g_post = nullptr, uint32_t in_log = 0, const Fe<F>* src0 = nullptr);
    static int coset_run(DeviceCtx& dc, int field, Fe<F>* a, uint32_t logn, const Fe<F>& gshift, hipStream_t st);
    static int vec_op_run(Fe<F>* a, const Fe<F>* b, const Fe<F>* c, uint64_t n, int op, const Fe<F>& s, hipStream_t st);
    static int scale_periodic_run(Fe<F>* a, uint64_t n, const Fe<F>* table_host, uint32_t m, hipStream_t st);
    // halo2 prover steps beyond commit / FFT (zk_poly.inl)
    static int batch_invert_run(Fe<F>* a, uint64_t n, hipStream_t st);
    static int prefix_product_run(DeviceCtx& dc, const Fe<F>* in, Fe<F>* out, uint64_t n, const Fe<F>& first, Fe<F>** total_dev, hipStream_t st);
    static int perm_product_run(DeviceCtx& dc, int field, uint32_t ncols, const void* const* cols, const void* const* sigmas, uint32_t first_col,
                                const Fe<F>& beta, const Fe<F>& gamma, const Fe<F>& delta, uint32_t k, const Fe<F>& omega, const Fe<F>& first, Fe<F>* z_out,
                                void* total_host, hipStream_t st);
    static int lookup_product_run(DeviceCtx& dc, const Fe<F>* A, const Fe<F>* S, const Fe<F>* Ap, const Fe<F>* Sp, const Fe<F>& beta, const Fe<F>& gamma,
                                  uint64_t n, const Fe<F>& first, Fe<F>* z_out, void* total_host, hipStream_t st);
    // plonk/lookup/prover.rs permute_expression_pair (zk_lookup.inl): A', S' of the first u rows; *lookup_failed = 1 when an input
    // value is not in the table (synchronises the stream once, at the end)
    static int permute_expression_pair_run(DeviceCtx& dc, const Fe<F>* A, const Fe<F>* S, uint32_t u, Fe<F>* a_out, Fe<F>* s_out, int* lookup_failed,
                                           hipStream_t st);
    static int inner_product_run(DeviceCtx& dc, const Fe<F>* a, const Fe<F>* b, uint64_t n, void* out_host, hipStream_t st);
    static int vec_muladd_run(Fe<F>* out, const Fe<F>* a, const Fe<F>* b, uint64_t n, const Fe<F>& s, hipStream_t st);
    static int poly_eval_run(DeviceCtx& dc, const Fe<F>* c, uint64_t n, uint32_t count, uint64_t stride, const Fe<F>& x, int field, void* out_host, hipStream_t st);
    static int vec_fold_many_run(Fe<F>* out, const Fe<F>* first, int64_t stride, uint32_t count, uint64_t n, const Fe<F>& s, hipStream_t st);
    static int ipa_fold_round_run(Fe<F>* p, Fe<F>* b, Fe<F>* W, uint64_t half, uint64_t m0, const Fe<F>& u, hipStream_t st);
    static int vec_powers_run(DeviceCtx& dc, Fe<F>* out, uint64_t n, const Fe<F>& x, hipStream_t st);
    static int kate_division_run(DeviceCtx& dc, const Fe<F>* a, Fe<F>* q, uint64_t n, const Fe<F>& x, hipStream_t st);
    static int vec_fold_run(Fe<F>* a, uint64_t half, const Fe<F>& c, hipStream_t st);
    static int ipa_virtual_scalars_run(const Fe<F>* p, const Fe<F>* W, Fe<F>* SL, Fe<F>* SR, uint64_t m0, uint64_t cur, hipStream_t st);
    static int ipa_round_begin_run(DeviceCtx& dc, const Fe<F>* p, const Fe<F>* b, const Fe<F>* W, Fe<F>* SL, Fe<F>* SR, uint64_t m0, uint64_t cur, hipStream_t st);
    static int ipa_round_end_run(DeviceCtx& dc, hipStream_t st, void* vl_host, void* vr_host);
    static int ipa_update_weights_run(Fe<F>* W, uint64_t m0, uint64_t bit, const Fe<F>& u, hipStream_t st);
    static int expr_eval_run(DeviceCtx& dc, const zk_expr_op* prog, uint32_t n_ops, const void* const* cols, uint32_t n_cols, const Fe<F>* consts,
                             uint32_t n_consts, uint32_t log_n, uint32_t rot_scale, Fe<F>* out, hipStream_t st);
    static int expr_source_run(const zk_expr_op* prog, uint32_t n_ops, uint32_t n_cols, uint32_t n_consts, std::string& out);
    static int expr_eval_lazy_run(DeviceCtx& dc, const zk_expr_op* prog, uint32_t n_ops, const void* const* cols, uint32_t n_cols, const Fe<F>* consts,
                                  uint32_t n_consts, uint32_t log_n, uint32_t rot_scale, Fe<F>* out, hipStream_t st);
    static int r1cs_matvec_run(const R1csMatrix& m, const Fe<F>* z, Fe<F>* out, uint64_t out_len, hipStream_t st);
    // Groth16 key generation (zk_setup.inl)
    static int r1cs_transpose_run(R1csMatrix& m, hipStream_t st);
    static int r1cs_matvec_t_run(const R1csMatrix& m, const Fe<F>* x, uint64_t x_len, Fe<F>* out, uint64_t out_len, const Fe<F>* extra, uint64_t n_extra,
                                 hipStream_t st);
    static int lagrange_consts(uint32_t logm, const Fe<F>& tau, Fe<F>* w_out, Fe<F>* zt_out, Fe<F>* s_out);
    static int lagrange_run(DeviceCtx& dc, int field, uint32_t logm, const Fe<F>& tau, Fe<F>* out, Fe<F>* zt_out, hipStream_t st);
    static int groth16_qap_at_run(DeviceCtx& dc, int field, const R1csMatrix& ma, const R1csMatrix& mb, const R1csMatrix& mc, uint64_t num_inputs,
                                  uint32_t logm, const Fe<F>& tau, Fe<F>* u, Fe<F>* v, Fe<F>* w, uint64_t n_vars, Fe<F>* zt_out, hipStream_t st);
    static int groth16_key_scalars_run(DeviceCtx& dc, const Fe<F>* u, const Fe<F>* v, const Fe<F>* w, uint64_t n_vars, uint64_t num_inputs, uint32_t logm,
                                       const Fe<F>& alpha, const Fe<F>& beta, const Fe<F>& gamma, const Fe<F>& delta, const Fe<F>& tau, const Fe<F>& zt,
                                       Fe<F>* abc, Fe<F>* h, hipStream_t st);
    // halo2 key generation (zk_keygen.inl)
    static int perm_sigmas_run(DeviceCtx& dc, int field, uint32_t k, uint32_t ncols, const uint64_t* mapping, const Fe<F>& delta, const Fe<F>& omega,
                               Fe<F>* sigmas, int* bad_mapping, hipStream_t st);
    // halo2 opening verification (zk_ipa_verify.inl)
    static int ipa_s_run(DeviceCtx& dc, uint32_t k, uint32_t count, const void* u_host, const void* init_host, Fe<F>* s, int accumulate, hipStream_t st);
    // MockProver::verify (zk_mock.inl)
    static int mock_eval_run(DeviceCtx& dc, uint32_t k, const zk_expr_op* prog, const uint32_t* offs, uint32_t n_programs, const void* const* cols,
                             const uint64_t* poison_from, uint32_t n_cols, const Fe<F>* consts, uint32_t n_consts, Fe<F>* vals, uint8_t* status, hipStream_t st);
    static int mock_failures_run(DeviceCtx& dc, const uint8_t* status, uint64_t N, uint64_t cap, uint64_t* pos_host, uint8_t* kind_host, uint64_t* total_host,
                                 hipStream_t st);
    static int mock_permutation_run(DeviceCtx& dc, uint32_t k, uint32_t ncols, const void* const* cols, const uint64_t* poison_from, const uint64_t* mapping,
                                    uint8_t* status, int* bad_mapping, hipStream_t st);
    static int mock_lookup_run(DeviceCtx& dc, const Fe<F>* A, const uint8_t* a_status, const Fe<F>* S, const uint8_t* s_status, uint32_t u, uint8_t* status,
                               hipStream_t st);
    static int witness_map_run(DeviceCtx& dc, int field, Fe<F>* a, Fe<F>* b, Fe<F>* c, uint32_t logm, hipStream_t st);
    // Poseidon, the Merkle tree over it and the ElGamal stream (zk_poseidon.inl).  tbl: [ark | mds | init], host memory for the *_host_run
    // twins (no device, no zk_init), the handle's device table otherwise.
    static int poseidon_permute_host_run(const PoseidonShape& sh, const Fe<F>* tbl, Fe<F>* states, uint64_t count);
    static int poseidon_hash_host_run(const PoseidonShape& sh, const Fe<F>* tbl, const Fe<F>* in, uint32_t arity, uint64_t count, Fe<F>* out);
    static int poseidon_permute_run(const PoseidonShape& sh, const Fe<F>* tbl, Fe<F>* states, uint64_t count, hipStream_t st);
    static int poseidon_hash_run(const PoseidonShape& sh, const Fe<F>* tbl, const Fe<F>* in, uint32_t arity, uint64_t count, Fe<F>* out, hipStream_t st);
    static int poseidon_tree_run(const PoseidonShape& sh, const Fe<F>* tbl, const Fe<F>* leaves, uint32_t leaf_arity, uint32_t log_n, Fe<F>* nodes, hipStream_t st);
    static int merkle_paths_run(const Fe<F>* nodes, uint32_t log_n, const uint64_t* idx_host, uint64_t count, Fe<F>* out, hipStream_t st);
    static int vec_add_scalar_run(Fe<F>* out, const Fe<F>* a, uint64_t n, const Fe<F>& s, hipStream_t st);
    // EncryptCircuit: the per-element witness, the plaintext of a byte string, the first unsatisfied row (zk_encrypt.inl)
    static int encrypt_witness_run(const Fe<F>* msg, uint64_t msg_len, uint64_t n, const Fe<F>& dh, Fe<F>* c2, Fe<F>* m, Fe<F>* b, Fe<F>* k, hipStream_t st);
    static int plaintext_from_bytes_run(const uint8_t* bytes, uint64_t len, Fe<F>* out, uint64_t n, hipStream_t st);
    static int r1cs_first_unsatisfied_run(const R1csMatrix& ma, const R1csMatrix& mb, const R1csMatrix& mc, const Fe<F>* z, Fe<F>* scratch,
                                          uint64_t* first_row_out, hipStream_t st);
};
}  // namespace zk
