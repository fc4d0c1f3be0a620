// C ABI, Groth16: the registry of resident R1CS matrices, the witness map, and the scalars of key generation.
#include "zk_api_common.h"
#include "zk_ntt_decl.h"

using namespace zk;

namespace {
// R1CS matrices of the circuits in use (zk_r1cs_matrix_upload): fixed per circuit, resident on the home device
std::mutex g_mat_mu;
std::map<uint64_t, R1csMatrix> g_mats;
uint64_t g_next_mat = 1;
void free_matrix(R1csMatrix& m) {
    for (void* p : {m.row_ptr, m.col, m.val, m.long_rows, m.col_ptr, m.t_row, m.t_val, m.long_cols})
        if (p) hipFree(p);
    m = R1csMatrix();
}
}  // namespace

namespace zk {
void r1cs_release_all() {   // zk_shutdown, g.mu held
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    if (!g.devs.empty()) hipSetDevice(g.devs[0]->device);
    for (auto& kv : g_mats) free_matrix(kv.second);
    g_mats.clear();
}
}  // namespace zk

extern "C" {

API int zk_groth16_witness_map_device(zk_field_t f, void* a, void* b, void* c, uint32_t log_m, void* stream) {
    if (!a || !b || !c || !aligned16(a) || !aligned16(b) || !aligned16(c)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, return FieldLaunch<F>::witness_map_run(dc, (int)f, (Fe<F>*)a, (Fe<F>*)b, (Fe<F>*)c, log_m, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

API int zk_r1cs_matrix_upload(zk_field_t f, const uint64_t* row_ptr, const uint32_t* col, const void* val, uint64_t n_rows, uint64_t n_cols,
                              uint64_t* handle_out) {
    if (!handle_out || !row_ptr || (int)f < 0 || (int)f > (int)ZK_FR_BLS12_381) return ZK_ERR_INVALID_ARG;
    const uint64_t nnz = row_ptr[n_rows];
    if (row_ptr[0] != 0 || (nnz && (!col || !val)) || n_cols >= (1ull << 32)) return ZK_ERR_INVALID_ARG;
    std::vector<uint64_t> long_rows;
    for (uint64_t i = 0; i < n_rows; i++) {
        if (row_ptr[i + 1] < row_ptr[i]) return ZK_ERR_INVALID_ARG;
        if (row_ptr[i + 1] - row_ptr[i] > R1CS_LONG_ROW) long_rows.push_back(i);
    }
    for (uint64_t k = 0; k < nnz; k++)
        if (col[k] >= n_cols) return ZK_ERR_INVALID_ARG;   // a mat-vec must never index past the assignment
    DEVICE_ENTRY(nullptr);
    R1csMatrix m;
    m.field = (int)f;
    m.n_rows = n_rows;
    m.n_cols = n_cols;
    m.nnz = nnz;
    m.n_long = long_rows.size();
    auto put = [&](void** dst, const void* src, size_t bytes) -> int {
        HIP_TRY(hipMalloc(dst, bytes ? bytes : 16));
        if (bytes) HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return ZK_OK;
    };
    int st = put(&m.row_ptr, row_ptr, (n_rows + 1) * 8);
    if (st == ZK_OK) st = put(&m.col, col, nnz * 4);
    if (st == ZK_OK) st = put(&m.val, val, nnz * 32);
    if (st == ZK_OK) st = put(&m.long_rows, long_rows.data(), long_rows.size() * 8);
    if (st != ZK_OK) {
        free_matrix(m);
        return st;
    }
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    const uint64_t h = g_next_mat++;
    g_mats[h] = m;
    *handle_out = h;
    return ZK_OK;
}
API int zk_r1cs_matrix_free(uint64_t handle) {
    DEVICE_ENTRY(nullptr);
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    auto it = g_mats.find(handle);
    if (it == g_mats.end()) return ZK_ERR_BAD_HANDLE;
    hipDeviceSynchronize();
    free_matrix(it->second);
    g_mats.erase(it);
    return ZK_OK;
}
static int find_matrix(uint64_t handle, R1csMatrix* out) {
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    auto it = g_mats.find(handle);
    if (it == g_mats.end()) return ZK_ERR_BAD_HANDLE;
    *out = it->second;
    return ZK_OK;
}
API int zk_r1cs_matvec_device(uint64_t matrix, const void* z, void* out, uint64_t out_len, void* stream) {
    if (!z || !out || !aligned16(z) || !aligned16(out)) return ZK_ERR_INVALID_ARG;
    R1csMatrix m;
    ZK_TRY(find_matrix(matrix, &m));
    DEVICE_ENTRY(nullptr);
    FIELD_SWITCH((zk_field_t)m.field, return FieldLaunch<F>::r1cs_matvec_run(m, (const Fe<F>*)z, (Fe<F>*)out, out_len, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_groth16_witness_map_r1cs_device(zk_field_t f, uint64_t ha, uint64_t hb, uint64_t hc, const void* z, uint64_t num_inputs,
                                           uint32_t log_m, void* a, void* b, void* c, void* stream) {
    if (!z || !a || !b || !c || !aligned16(z) || !aligned16(a) || !aligned16(b) || !aligned16(c) || log_m > 30) return ZK_ERR_INVALID_ARG;
    R1csMatrix ma, mb, mc;
    ZK_TRY(find_matrix(ha, &ma));
    ZK_TRY(find_matrix(hb, &mb));
    ZK_TRY(find_matrix(hc, &mc));
    const uint64_t m = 1ull << log_m, nc = ma.n_rows;
    if (ma.field != (int)f || mb.field != (int)f || mc.field != (int)f || mb.n_rows != nc || mc.n_rows != nc || nc + num_inputs > m ||
        num_inputs > ma.n_cols)
        return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    FIELD_SWITCH(f, {
        hipStream_t st = (hipStream_t)stream;
        ZK_TRY(FieldLaunch<F>::r1cs_matvec_run(ma, (const Fe<F>*)z, (Fe<F>*)a, m, st));
        ZK_TRY(FieldLaunch<F>::r1cs_matvec_run(mb, (const Fe<F>*)z, (Fe<F>*)b, m, st));
        ZK_TRY(FieldLaunch<F>::r1cs_matvec_run(mc, (const Fe<F>*)z, (Fe<F>*)c, m, st));
        // the input-consistency rows: a[num_constraints + j] = z[j]
        if (num_inputs) HIP_TRY(hipMemcpyAsync((Fe<F>*)a + nc, z, num_inputs * sizeof(Fe<F>), hipMemcpyDeviceToDevice, st));
        return FieldLaunch<F>::witness_map_run(dc, (int)f, (Fe<F>*)a, (Fe<F>*)b, (Fe<F>*)c, log_m, st);
    });
    return ZK_ERR_INVALID_ARG;
}

// ark-relations ConstraintSystem::is_satisfied, naming the row: the smallest i with <A_i, z> <B_i, z> != <C_i, z>
API int zk_r1cs_first_unsatisfied_device(zk_field_t f, uint64_t ha, uint64_t hb, uint64_t hc, const void* z, uint64_t z_len, void* scratch,
                                         uint64_t scratch_elems, uint64_t* first_row_out_host, void* stream) {
    if (!z || !scratch || !first_row_out_host || !aligned16(z) || !aligned16(scratch)) return ZK_ERR_INVALID_ARG;
    R1csMatrix ma, mb, mc;
    ZK_TRY(find_matrix(ha, &ma));
    ZK_TRY(find_matrix(hb, &mb));
    ZK_TRY(find_matrix(hc, &mc));
    const uint64_t rows = ma.n_rows;
    if (ma.field != (int)f || mb.field != (int)f || mc.field != (int)f || mb.n_rows != rows || mc.n_rows != rows || z_len < ma.n_cols ||
        z_len < mb.n_cols || z_len < mc.n_cols || scratch_elems < 3 * rows + ZK_R1CS_CHECK_SCRATCH_ELEMS ||
        spans_overlap(z, z_len * 32, scratch, scratch_elems * 32))
        return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    FIELD_SWITCH(f, return FieldLaunch<F>::r1cs_first_unsatisfied_run(ma, mb, mc, (const Fe<F>*)z, (Fe<F>*)scratch, first_row_out_host, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

// ---- Groth16 key generation (ark-groth16 0.3 generator.rs generate_parameters)
// the matrix with its column-major companion, which is built on `st` at the handle's first transposed product
static int find_matrix_transposed(uint64_t handle, hipStream_t st, R1csMatrix* out) {
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    auto it = g_mats.find(handle);
    if (it == g_mats.end()) return ZK_ERR_BAD_HANDLE;
    if (!it->second.t_ready) FIELD_SWITCH((zk_field_t)it->second.field, ZK_TRY(FieldLaunch<F>::r1cs_transpose_run(it->second, st)));
    *out = it->second;
    return ZK_OK;
}
API int zk_r1cs_matvec_transposed_device(uint64_t matrix, const void* x, uint64_t x_len, void* out, uint64_t out_len, void* stream) {
    if (!out || !aligned16(out) || (x_len && (!x || !aligned16(x)))) return ZK_ERR_INVALID_ARG;
    R1csMatrix m;
    ZK_TRY(find_matrix(matrix, &m));
    if (out_len < m.n_cols) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    ZK_TRY(find_matrix_transposed(matrix, (hipStream_t)stream, &m));
    FIELD_SWITCH((zk_field_t)m.field,
                 return FieldLaunch<F>::r1cs_matvec_t_run(m, (const Fe<F>*)x, x_len, (Fe<F>*)out, out_len, nullptr, 0, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_lagrange_coefficients_device(zk_field_t f, uint32_t log_m, const void* tau, void* out, void* zt_out, void* stream) {
    if (!tau || !out || !aligned16(out)) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        Fe<F> t, w, zt, s;
        host_load(t, tau);
        ZK_TRY(FieldLaunch<F>::lagrange_consts(log_m, t, &w, &zt, &s));   // tau in the domain is refused before the library is entered
    });
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> t, zt;
        host_load(t, tau);
        ZK_TRY(FieldLaunch<F>::lagrange_run(dc, (int)f, log_m, t, (Fe<F>*)out, &zt, (hipStream_t)stream));
        if (zt_out) host_store(zt_out, zt);
        return ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_groth16_qap_at_device(zk_field_t f, uint64_t ha, uint64_t hb, uint64_t hc, uint64_t num_inputs, uint32_t log_m, const void* tau, void* u,
                                 void* v, void* w, uint64_t n_vars, void* zt_out, void* stream) {
    if (!tau || !u || !v || !w || !aligned16(u) || !aligned16(v) || !aligned16(w) || log_m > 30) return ZK_ERR_INVALID_ARG;
    R1csMatrix ma, mb, mc;
    ZK_TRY(find_matrix(ha, &ma));
    ZK_TRY(find_matrix(hb, &mb));
    ZK_TRY(find_matrix(hc, &mc));
    const uint64_t m = 1ull << log_m, nc = ma.n_rows;
    if (ma.field != (int)f || mb.field != (int)f || mc.field != (int)f || mb.n_rows != nc || mc.n_rows != nc || nc + num_inputs > m ||
        num_inputs > n_vars || n_vars < ma.n_cols || n_vars < mb.n_cols || n_vars < mc.n_cols)
        return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        Fe<F> t, w0, zt, s;
        host_load(t, tau);
        ZK_TRY(FieldLaunch<F>::lagrange_consts(log_m, t, &w0, &zt, &s));
    });
    DEVICE_ENTRY(nullptr);
    hipStream_t st = (hipStream_t)stream;
    ZK_TRY(find_matrix_transposed(ha, st, &ma));
    ZK_TRY(find_matrix_transposed(hb, st, &mb));
    ZK_TRY(find_matrix_transposed(hc, st, &mc));
    FIELD_SWITCH(f, {
        Fe<F> t, zt;
        host_load(t, tau);
        ZK_TRY(FieldLaunch<F>::groth16_qap_at_run(dc, (int)f, ma, mb, mc, num_inputs, log_m, t, (Fe<F>*)u, (Fe<F>*)v, (Fe<F>*)w, n_vars, &zt, st));
        if (zt_out) host_store(zt_out, zt);
        return ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_groth16_key_scalars_device(zk_field_t f, const void* u, const void* v, const void* w, uint64_t n_vars, uint64_t num_inputs,
                                      uint32_t log_m, const void* alpha, const void* beta, const void* gamma, const void* delta, const void* tau,
                                      const void* zt, void* abc, void* h, void* stream) {
    if (!alpha || !beta || !gamma || !delta || !tau || !zt || log_m > 30 || num_inputs > n_vars) return ZK_ERR_INVALID_ARG;
    if (n_vars && (!u || !v || !w || !abc || !aligned16(u) || !aligned16(v) || !aligned16(w) || !aligned16(abc))) return ZK_ERR_INVALID_ARG;
    if (log_m && (!h || !aligned16(h))) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        Fe<F> g_, d, z;
        host_load(g_, gamma);
        host_load(d, delta);
        host_load(z, zt);
        if (log_m > (uint32_t)F::TWO_ADICITY || fe_is_zero(g_) || fe_is_zero(d) || fe_is_zero(z)) return ZK_ERR_INVALID_ARG;
    });
    DEVICE_ENTRY(abc);
    FIELD_SWITCH(f, {
        Fe<F> a, b, g_, d, t, z;
        host_load(a, alpha);
        host_load(b, beta);
        host_load(g_, gamma);
        host_load(d, delta);
        host_load(t, tau);
        host_load(z, zt);
        return FieldLaunch<F>::groth16_key_scalars_run(dc, (const Fe<F>*)u, (const Fe<F>*)v, (const Fe<F>*)w, n_vars, num_inputs, log_m, a, b, g_, d, t, z,
                                          (Fe<F>*)abc, (Fe<F>*)h, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}

}  // extern "C"
