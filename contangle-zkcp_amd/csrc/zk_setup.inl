// Launch sequences of Groth16 key generation (zk_setup_kernels.h).  Included by zk_ntt.inl, once per scalar field.
#pragma once
#include "zk_setup_kernels.h"
namespace zk {

// The column-major companion of a resident CSR matrix, on the device: histogram of col_idx, exclusive scan, scatter.  Runs once
// per handle (the caller holds the matrix table's lock) and synchronises `st` at the end to read the number of long columns.
template <class F>
int FieldLaunch<F>::r1cs_transpose_run(R1csMatrix& m, hipStream_t st) {
    if (m.t_ready) return ZK_OK;
    if (m.nnz >= (1ull << 32) || m.n_rows >= (1ull << 32)) return ZK_ERR_UNSUPPORTED;   // 32-bit offsets and row indices
    const uint64_t n_ptr = m.n_cols + 1;
    const uint64_t per_wg = (uint64_t)TSCAN_WG * TSCAN_K;
    const uint32_t nblocks = (uint32_t)((n_ptr + per_wg - 1) / per_wg);
    const uint64_t long_cap = m.nnz / (R1CS_LONG_ROW + 1) + 1;
    void *col_ptr = nullptr, *t_row = nullptr, *t_val = nullptr, *long_cols = nullptr, *tmp = nullptr;
    auto fail = [&](int status) {
        for (void* p : {col_ptr, t_row, t_val, long_cols, tmp})
            if (p) hipFree(p);
        return status;
    };
    // tmp: the counters (later the scatter cursors), the scan's block totals, the long-column counter
    const size_t tmp_words = n_ptr + nblocks + 1;
    if (hipMalloc(&col_ptr, n_ptr * 4) != hipSuccess || hipMalloc(&t_row, (m.nnz ? m.nnz : 1) * 4) != hipSuccess ||
        hipMalloc(&t_val, (m.nnz ? m.nnz : 1) * sizeof(Fe<F>)) != hipSuccess || hipMalloc(&long_cols, long_cap * 4) != hipSuccess ||
        hipMalloc(&tmp, tmp_words * 4) != hipSuccess)
        return fail(ZK_ERR_OOM);
    uint32_t* cnt = (uint32_t*)tmp;
    uint32_t* tot = cnt + n_ptr;
    uint32_t* n_long = tot + nblocks;
    if (hipMemsetAsync(tmp, 0, tmp_words * 4, st) != hipSuccess) return fail(ZK_ERR_HIP);
    uint64_t tb = (m.nnz + 255) / 256;
    if (tb > 8192) tb = 8192;
    uint64_t cb = (n_ptr + 255) / 256;
    if (cb > 8192) cb = 8192;
    if (m.nnz) ZK_LAUNCH((r1cs_col_count_kernel<F>), (unsigned)tb, 256, 0, st, (const uint32_t*)m.col, m.nnz, cnt);
    ZK_LAUNCH((u32_scan_block_kernel<F>), nblocks, TSCAN_WG, 0, st, (const uint32_t*)cnt, (uint32_t*)col_ptr, tot, n_ptr);
    ZK_LAUNCH((u32_scan_totals_kernel<F>), 1, TSCAN_WG, 0, st, tot, nblocks);
    ZK_LAUNCH((r1cs_col_finish_kernel<F>), (unsigned)cb, 256, 0, st, (uint32_t*)col_ptr, cnt, (const uint32_t*)tot, m.n_cols, (uint32_t*)long_cols,
              n_long);
    if (m.nnz)
        ZK_LAUNCH((r1cs_col_scatter_kernel<F>), (unsigned)tb, 256, 0, st, (const uint64_t*)m.row_ptr, (const uint32_t*)m.col, (const Fe<F>*)m.val,
                  m.n_rows, m.nnz, cnt, (uint32_t*)t_row, (Fe<F>*)t_val);
    uint32_t nl = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&nl, n_long, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(ZK_ERR_HIP);
    hipFree(tmp);
    m.col_ptr = col_ptr;
    m.t_row = t_row;
    m.t_val = t_val;
    m.long_cols = long_cols;
    m.n_long_cols = nl;
    m.t_ready = true;
    return ZK_OK;
}

// out[j] = sum_{i < x_len} M[i][j] x[i] (+ extra[j], j < n_extra) for j < n_cols; extra[j] or 0 for n_cols <= j < out_len
template <class F>
int FieldLaunch<F>::r1cs_matvec_t_run(const R1csMatrix& m, const Fe<F>* x, uint64_t x_len, Fe<F>* out, uint64_t out_len, const Fe<F>* extra, uint64_t n_extra,
                                      hipStream_t st) {
    if (!m.t_ready || out_len < m.n_cols || n_extra > out_len) return ZK_ERR_INVALID_ARG;
    if (out_len == 0) return ZK_OK;
    uint64_t blocks = (out_len + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    ZK_LAUNCH((r1cs_matvec_t_kernel<F>), (unsigned)blocks, 256, 0, st, (const uint32_t*)m.col_ptr, (const uint32_t*)m.t_row, (const Fe<F>*)m.t_val, x,
              x_len, out, m.n_cols, out_len, extra, n_extra);
    if (m.n_long_cols)
        ZK_LAUNCH((r1cs_matvec_t_long_kernel<F>), (unsigned)m.n_long_cols, 256, 0, st, (const uint32_t*)m.col_ptr, (const uint32_t*)m.t_row,
                  (const Fe<F>*)m.t_val, x, x_len, out, (const uint32_t*)m.long_cols, extra, n_extra);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

// the host constants of the size-2^logm domain at tau: w = its generator, zt = tau^m - 1 (ZK_ERR_INVALID_ARG when tau lies in
// the domain: upstream samples tau outside it and has no use for that branch), s = zt / m
template <class F>
int FieldLaunch<F>::lagrange_consts(uint32_t logm, const Fe<F>& tau, Fe<F>* w_out, Fe<F>* zt_out, Fe<F>* s_out) {
    if (logm > (uint32_t)F::TWO_ADICITY || logm > 30) return ZK_ERR_INVALID_ARG;
    Fe<F> w, tm = tau, one, mm, minv;
    for (int i = 0; i < F::N; i++) w.v[i] = F::ROOT[i];
    for (uint32_t i = logm; i < (uint32_t)F::TWO_ADICITY; i++) fe_sqr(w, w);
    fe_one(one);
    mm = one;
    for (uint32_t i = 0; i < logm; i++) {
        fe_sqr(tm, tm);
        fe_add(mm, mm, mm);
    }
    fe_sub(tm, tm, one);
    if (fe_is_zero(tm)) return ZK_ERR_INVALID_ARG;
    fe_inv(minv, mm);
    *w_out = w;
    *zt_out = tm;
    fe_mul(*s_out, tm, minv);
    return ZK_OK;
}

// ark-poly 0.3 Radix2EvaluationDomain::evaluate_all_lagrange_coefficients(tau), tau outside the domain: out[i] = L_i(tau), i < 2^logm
template <class F>
int FieldLaunch<F>::lagrange_run(DeviceCtx& dc, int field, uint32_t logm, const Fe<F>& tau, Fe<F>* out, Fe<F>* zt_out, hipStream_t st) {
    Fe<F> w, zt, s;
    ZK_TRY(lagrange_consts(logm, tau, &w, &zt, &s));
    const uint64_t m = 1ull << logm;
    PowTables<F> pw;
    ZK_TRY(pow_tables<F>(dc, w, logm, field, st, &pw));
    uint64_t blocks = (m + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    ZK_LAUNCH((lagrange_den_kernel<F>), (unsigned)blocks, 256, 0, st, out, m, tau, pw);
    ZK_TRY(batch_invert_run(out, m, st));
    ZK_LAUNCH((lagrange_scale_kernel<F>), (unsigned)blocks, 256, 0, st, out, m, s, pw);
    HIP_TRY(hipGetLastError());
    if (zt_out) *zt_out = zt;
    return ZK_OK;
}

// r1cs_to_qap.rs LibsnarkReduction::instance_map_with_evaluation: u, v, w (n_vars elements each) from the three resident
// matrices (their column-major companions ready) at tau; the Lagrange vector lives in the stream's scratch
template <class F>
int FieldLaunch<F>::groth16_qap_at_run(DeviceCtx& dc, int field, const R1csMatrix& ma, const R1csMatrix& mb, const R1csMatrix& mc, uint64_t num_inputs,
                                       uint32_t logm, const Fe<F>& tau, Fe<F>* u, Fe<F>* v, Fe<F>* w, uint64_t n_vars, Fe<F>* zt_out, hipStream_t st) {
    const uint64_t m = 1ull << logm, nc = ma.n_rows;
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    ZK_TRY(ws_get(ss->poly_a, m * sizeof(Fe<F>)));
    Fe<F>* L = (Fe<F>*)ss->poly_a.p;
    ZK_TRY(lagrange_run(dc, field, logm, tau, L, zt_out, st));
    // u_j = sum_i A[i][j] L_i + L_{num_constraints + j} for the inputs: the input-consistency rows, added by the same pass
    ZK_TRY(r1cs_matvec_t_run(ma, L, m, u, n_vars, L + nc, num_inputs, st));
    ZK_TRY(r1cs_matvec_t_run(mb, L, m, v, n_vars, nullptr, 0, st));
    ZK_TRY(r1cs_matvec_t_run(mc, L, m, w, n_vars, nullptr, 0, st));
    return ZK_OK;
}

// generator.rs generate_parameters, the scalars of gamma_abc_g1 | l_query (abc, n_vars elements) and of h_query (h, 2^logm - 1)
template <class F>
int FieldLaunch<F>::groth16_key_scalars_run(DeviceCtx& dc, const Fe<F>* u, const Fe<F>* v, const Fe<F>* w, uint64_t n_vars, uint64_t num_inputs, uint32_t logm,
                                            const Fe<F>& alpha, const Fe<F>& beta, const Fe<F>& gamma, const Fe<F>& delta, const Fe<F>& tau, const Fe<F>& zt,
                                            Fe<F>* abc, Fe<F>* h, hipStream_t st) {
    if (logm > 30 || fe_is_zero(gamma) || fe_is_zero(delta) || fe_is_zero(zt)) return ZK_ERR_INVALID_ARG;
    Fe<F> ginv, dinv, s;
    fe_inv(ginv, gamma);
    fe_inv(dinv, delta);
    fe_mul(s, zt, dinv);
    if (n_vars) {
        uint64_t blocks = (n_vars + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        ZK_LAUNCH((groth16_abc_kernel<F>), (unsigned)blocks, 256, 0, st, u, v, w, abc, n_vars, num_inputs, alpha, beta, ginv, dinv);
    }
    const uint64_t nh = (1ull << logm) - 1;
    if (nh) {
        StreamScratch* ss = nullptr;
        ZK_TRY(stream_scratch(dc, st, &ss));
        PowTables<F> pw;
        ZK_TRY(scratch_pow_tables<F>(*ss, tau, logm, st, &pw));
        uint64_t blocks = (nh + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        ZK_LAUNCH((groth16_h_scalars_kernel<F>), (unsigned)blocks, 256, 0, st, h, nh, s, pw);
    }
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
