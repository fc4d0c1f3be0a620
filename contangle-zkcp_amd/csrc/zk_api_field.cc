// C ABI, scalar-field side: NTT and coset helpers, pointwise vector operations, the polynomial and IPA steps of the halo2
// prover, and the gate-expression evaluators.
#include "zk_api_common.h"
#include "zk_ntt_decl.h"

using namespace zk;

extern "C" {

API int zk_ntt_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g.mu);
    g.ntt_profile = on != 0;
    return ZK_OK;
}
API int zk_ntt_profile_read(zk_ntt_totals* out) {
    if (!out) return ZK_ERR_INVALID_ARG;
    {
        std::lock_guard<std::mutex> lk0(g.mu);
        ZK_TRY(require_init());
    }
    memset(out, 0, sizeof *out);
    for (auto& dcp : g.devs) {
        DeviceCtx& dc = *dcp;
        ZK_TRY(bind_device(dc));
        std::lock_guard<std::mutex> lk(dc.mu);
        for (size_t i = 0; i + 1 < dc.ntt_ev_used; i += 2) {
            HIP_TRY(hipEventSynchronize(dc.ntt_ev_pool[i + 1]));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, dc.ntt_ev_pool[i], dc.ntt_ev_pool[i + 1]));
            out->kernel_ms += ms;
            out->launches++;
        }
        out->transforms += dc.ntt_transforms;
        out->algorithmic_bytes += dc.ntt_alg_bytes;
        dc.ntt_ev_used = 0;
        dc.ntt_transforms = 0;
        dc.ntt_alg_bytes = 0;
    }
    hipSetDevice(g.devs[0]->device);
    return ZK_OK;
}

API int zk_ntt_configure(const zk_ntt_opts* opts) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (opts)
        g.ntt_opts = *opts;
    else
        memset(&g.ntt_opts, 0, sizeof g.ntt_opts);
    return ZK_OK;
}

API int zk_ntt_device(zk_field_t f, void* a, uint32_t log_n, const void* omega, int scale, void* stream) {
    if (!a || !omega || !aligned16(a)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> w;
        host_load(w, omega);
        return FieldLaunch<F>::ntt_run(dc, (int)f, (Fe<F>*)a, log_n, w, scale, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt(zk_field_t f, void* a_host, uint32_t log_n, const void* omega, int scale) {
    if (!a_host || !omega || log_n > 30) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    const size_t bytes = (size_t)32 << log_n;
    ZK_TRY(ws_get(dc.scratch_in, bytes));
    HIP_TRY(hipMemcpy(dc.scratch_in.p, a_host, bytes, hipMemcpyHostToDevice));
    FIELD_SWITCH(f, {
        Fe<F> w;
        host_load(w, omega);
        ZK_TRY(FieldLaunch<F>::ntt_run(dc, (int)f, (Fe<F>*)dc.scratch_in.p, log_n, w, scale, (hipStream_t)0));
    });
    HIP_TRY(hipStreamSynchronize((hipStream_t)0));
    HIP_TRY(hipMemcpy(a_host, dc.scratch_in.p, bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
}
API int zk_ntt_coset_device(zk_field_t f, void* a, uint32_t log_n, const void* omega, int scale, const void* g_pre,
                            const void* g_post, void* stream) {
    if (!a || !omega || !aligned16(a)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> w, gp, gq;
        host_load(w, omega);
        if (g_pre) host_load(gp, g_pre);
        if (g_post) host_load(gq, g_post);
        return FieldLaunch<F>::ntt_run(dc, (int)f, (Fe<F>*)a, log_n, w, scale, (hipStream_t)stream, g_pre ? &gp : nullptr, g_post ? &gq : nullptr);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt_extend_device(zk_field_t f, void* a, uint32_t log_n, uint32_t log_in, const void* omega, int scale, const void* g_pre,
                             const void* g_post, void* stream) {
    if (!a || !omega || !aligned16(a) || log_in > log_n || log_n > 30) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        if (log_n > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
        Fe<F> w, gp, gq;
        host_load(w, omega);
        if (g_pre) host_load(gp, g_pre);
        if (g_post) host_load(gq, g_post);
        if (log_n > 0 && log_in == 0) {   // a single coefficient: in_log = 0 means "all" to the pass kernel, so pad explicitly
            HIP_TRY(hipMemsetAsync((Fe<F>*)a + 1, 0, (((size_t)1 << log_n) - 1) * sizeof(Fe<F>), (hipStream_t)stream));
        }
        return FieldLaunch<F>::ntt_run(dc, (int)f, (Fe<F>*)a, log_n, w, scale, (hipStream_t)stream, g_pre ? &gp : nullptr, g_post ? &gq : nullptr, log_in);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt_oop_device(zk_field_t f, const void* src, void* dst, uint32_t log_n, uint32_t log_in, const void* omega, int scale, const void* g_pre,
                          const void* g_post, void* stream) {
    if (!src || !dst || !omega || !aligned16(src) || !aligned16(dst) || log_in > log_n || log_n > 30) return ZK_ERR_INVALID_ARG;
    if (src == dst) return zk_ntt_extend_device(f, dst, log_n, log_in, omega, scale, g_pre, g_post, stream);
    // the buffers must not overlap: the first pass reads src while later tiles of the same pass may already write dst
    if (spans_overlap(src, (uint64_t)32 << log_in, dst, (uint64_t)32 << log_n)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(dst);
    FIELD_SWITCH(f, {
        if (log_n > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
        Fe<F> w, gp, gq;
        host_load(w, omega);
        if (g_pre) host_load(gp, g_pre);
        if (g_post) host_load(gq, g_post);
        if (log_n > 0 && log_in == 0) {   // a single coefficient (in_log = 0 means "all" to the pass kernel): pad explicitly, then in place
            HIP_TRY(hipMemcpyAsync(dst, src, sizeof(Fe<F>), hipMemcpyDeviceToDevice, (hipStream_t)stream));
            HIP_TRY(hipMemsetAsync((Fe<F>*)dst + 1, 0, (((size_t)1 << log_n) - 1) * sizeof(Fe<F>), (hipStream_t)stream));
            return FieldLaunch<F>::ntt_run(dc, (int)f, (Fe<F>*)dst, log_n, w, scale, (hipStream_t)stream, g_pre ? &gp : nullptr, g_post ? &gq : nullptr, log_in);
        }
        return FieldLaunch<F>::ntt_run(dc, (int)f, (Fe<F>*)dst, log_n, w, scale, (hipStream_t)stream, g_pre ? &gp : nullptr, g_post ? &gq : nullptr, log_in,
                          (const Fe<F>*)src);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_coset_mul_device(zk_field_t f, void* a, uint32_t log_n, const void* gm, void* stream) {
    if (!a || !gm || !aligned16(a)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> w;
        host_load(w, gm);
        return FieldLaunch<F>::coset_run(dc, (int)f, (Fe<F>*)a, log_n, w, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_coset_mul(zk_field_t f, void* a_host, uint32_t log_n, const void* gm) {
    if (!a_host || !gm || log_n > 30) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    const size_t bytes = (size_t)32 << log_n;
    ZK_TRY(ws_get(dc.scratch_in, bytes));
    HIP_TRY(hipMemcpy(dc.scratch_in.p, a_host, bytes, hipMemcpyHostToDevice));
    FIELD_SWITCH(f, {
        Fe<F> w;
        host_load(w, gm);
        ZK_TRY(FieldLaunch<F>::coset_run(dc, (int)f, (Fe<F>*)dc.scratch_in.p, log_n, w, (hipStream_t)0));
    });
    HIP_TRY(hipMemcpy(a_host, dc.scratch_in.p, bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
}

API int zk_vec_op_device(zk_field_t f, int op, void* a, const void* b, const void* c, uint64_t n, const void* scalar, void* stream) {
    if (op < 0 || op > 6 || (n && (!a || !aligned16(a)))) return ZK_ERR_INVALID_ARG;
    const bool needs_b = op == 0 || op == 1 || op == 2 || op == 6, needs_c = op == 6, needs_s = op == 3 || op == 6;
    if (n && ((needs_b && (!b || !aligned16(b))) || (needs_c && (!c || !aligned16(c))) || (needs_s && !scalar))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> s;
        fe_one(s);
        if (needs_s) host_load(s, scalar);
        return FieldLaunch<F>::vec_op_run((Fe<F>*)a, (const Fe<F>*)b, (const Fe<F>*)c, n, op, s, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_scale_periodic_device(zk_field_t f, void* a, uint64_t n, const void* table_host, uint32_t m, void* stream) {
    if ((n && (!a || !aligned16(a))) || !table_host) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, return FieldLaunch<F>::scale_periodic_run((Fe<F>*)a, n, (const Fe<F>*)table_host, m, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

// ---- halo2 prover steps beyond commit / FFT (include/zkcp_amd_prover.h)
API int zk_batch_invert_device(zk_field_t f, void* a, uint64_t n, void* stream) {
    if (n && (!a || !aligned16(a))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, return FieldLaunch<F>::batch_invert_run((Fe<F>*)a, n, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_prefix_product_device(zk_field_t f, const void* in, void* out, uint64_t n, const void* first, void* total_host, void* stream) {
    if (n && (!in || !out || !aligned16(in) || !aligned16(out))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> fst;
        fe_one(fst);
        if (first) host_load(fst, first);
        Fe<F>* total = nullptr;
        ZK_TRY(FieldLaunch<F>::prefix_product_run(dc, (const Fe<F>*)in, (Fe<F>*)out, n, fst, &total, (hipStream_t)stream));
        if (total_host) {
            HIP_TRY(hipMemcpyAsync(total_host, total, sizeof(Fe<F>), hipMemcpyDeviceToHost, (hipStream_t)stream));
            HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        }
        return ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_inner_product_device(zk_field_t f, const void* a, const void* b, uint64_t n, void* out_host, void* stream) {
    if (!out_host || (n && (!a || !b || !aligned16(a) || !aligned16(b)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, return FieldLaunch<F>::inner_product_run(dc, (const Fe<F>*)a, (const Fe<F>*)b, n, out_host, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_muladd_device(zk_field_t f, void* a, const void* b, uint64_t n, const void* s, void* stream) {
    if (!s || (n && (!a || !b || !aligned16(a) || !aligned16(b)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> ss;
        host_load(ss, s);
        return FieldLaunch<F>::vec_muladd_run((Fe<F>*)a, (const Fe<F>*)a, (const Fe<F>*)b, n, ss, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_muladd_to_device(zk_field_t f, void* out, const void* a, const void* b, uint64_t n, const void* s, void* stream) {
    if (!s || (n && (!out || !a || !b || !aligned16(out) || !aligned16(a) || !aligned16(b)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> ss;
        host_load(ss, s);
        return FieldLaunch<F>::vec_muladd_run((Fe<F>*)out, (const Fe<F>*)a, (const Fe<F>*)b, n, ss, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_poly_eval_device(zk_field_t f, const void* c, uint64_t n, const void* x, void* out_host, void* stream) {
    return zk_poly_eval_batch_device(f, c, n, 1, n, x, out_host, stream);
}
API int zk_poly_eval_batch_device(zk_field_t f, const void* c, uint64_t n, uint32_t count, uint64_t stride_elems, const void* x, void* out_host,
                                  void* stream) {
    if (!out_host || !x || stride_elems < n || (n && count && (!c || !aligned16(c)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(c);
    FIELD_SWITCH(f, {
        Fe<F> xx;
        host_load(xx, x);
        return FieldLaunch<F>::poly_eval_run(dc, (const Fe<F>*)c, n, count, stride_elems, xx, (int)f, out_host, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_fold_many_device(zk_field_t f, void* out, const void* first, int64_t stride_elems, uint32_t count, uint64_t n, const void* s,
                                void* stream) {
    if (!s || count == 0 || (n && (!out || !first || !aligned16(out) || !aligned16(first)))) return ZK_ERR_INVALID_ARG;
    if (count > 1 && (stride_elems == 0 || (uint64_t)(stride_elems < 0 ? -stride_elems : stride_elems) < n)) return ZK_ERR_INVALID_ARG;
    // out may be one of the sources (every lane reads all of its inputs before it writes) or disjoint from all of them
    for (uint32_t i = 0; i < count; i++) {
        const void* a = (const void*)((intptr_t)first + (intptr_t)i * stride_elems * 32);
        if (a != out && spans_overlap(a, n * 32, out, n * 32)) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> ss;
        host_load(ss, s);
        return FieldLaunch<F>::vec_fold_many_run((Fe<F>*)out, (const Fe<F>*)first, stride_elems, count, n, ss, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ipa_fold_round_device(zk_field_t f, void* p, void* b, void* w, uint64_t half, uint64_t m0, const void* u, void* stream) {
    if (!u || (half && (!p || !b || !aligned16(p) || !aligned16(b))) || (w && !aligned16(w))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(p);
    FIELD_SWITCH(f, {
        Fe<F> uu;
        host_load(uu, u);
        if (fe_is_zero(uu)) return ZK_ERR_INVALID_ARG;
        return FieldLaunch<F>::ipa_fold_round_run((Fe<F>*)p, (Fe<F>*)b, (Fe<F>*)w, half, m0, uu, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_powers_device(zk_field_t f, void* out, uint64_t n, const void* x, void* stream) {
    if (!x || (n && (!out || !aligned16(out)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> xx;
        host_load(xx, x);
        return FieldLaunch<F>::vec_powers_run(dc, (Fe<F>*)out, n, xx, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_kate_division_device(zk_field_t f, const void* a, void* q, uint64_t n, const void* x, void* stream) {
    if (!x || (n && (!a || !q || !aligned16(a) || !aligned16(q)))) return ZK_ERR_INVALID_ARG;
    if (a != q && spans_overlap(a, n * 32, q, n * 32)) return ZK_ERR_INVALID_ARG;   // in place or disjoint
    DEVICE_ENTRY(q);
    FIELD_SWITCH(f, {
        Fe<F> xx;
        host_load(xx, x);
        return FieldLaunch<F>::kate_division_run(dc, (const Fe<F>*)a, (Fe<F>*)q, n, xx, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_fold_device(zk_field_t f, void* a, uint64_t half, const void* c, void* stream) {
    if (!c || (half && (!a || !aligned16(a)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> cc;
        host_load(cc, c);
        return FieldLaunch<F>::vec_fold_run((Fe<F>*)a, half, cc, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ipa_virtual_scalars_device(zk_field_t f, const void* p, const void* w, uint64_t m0, uint64_t cur, void* sl, void* sr, void* stream) {
    if (!p || !w || !sl || !sr || !aligned16(p) || !aligned16(w) || !aligned16(sl) || !aligned16(sr)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(sl);
    FIELD_SWITCH(f, return FieldLaunch<F>::ipa_virtual_scalars_run((const Fe<F>*)p, (const Fe<F>*)w, (Fe<F>*)sl, (Fe<F>*)sr, m0, cur, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_ipa_update_weights_device(zk_field_t f, void* w, uint64_t m0, uint64_t bit, const void* u, void* stream) {
    if (!w || !u || !aligned16(w)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(w);
    FIELD_SWITCH(f, {
        Fe<F> uu;
        host_load(uu, u);
        return FieldLaunch<F>::ipa_update_weights_run((Fe<F>*)w, m0, bit, uu, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_expr_eval_device(zk_field_t f, const zk_expr_op* prog, uint32_t n_ops, const void* const* cols, uint32_t n_cols, const void* consts,
                            uint32_t n_consts, uint32_t log_n, uint32_t rot_scale, void* out, void* stream) {
    if (!prog || !out || !aligned16(out) || (n_cols && !cols) || (n_consts && !consts)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, return FieldLaunch<F>::expr_eval_run(dc, prog, n_ops, cols, n_cols, (const Fe<F>*)consts, n_consts, log_n, rot_scale, (Fe<F>*)out,
                                            (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

API int zk_expr_eval_lazy_device(zk_field_t f, const zk_expr_op* prog, uint32_t n_ops, const void* const* cols, uint32_t n_cols, const void* consts,
                                 uint32_t n_consts, uint32_t log_n, uint32_t rot_scale, void* out, void* stream) {
    if (!prog || !out || !aligned16(out) || (n_cols && !cols) || (n_consts && !consts)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, return FieldLaunch<F>::expr_eval_lazy_run(dc, prog, n_ops, cols, n_cols, (const Fe<F>*)consts, n_consts, log_n, rot_scale, (Fe<F>*)out,
                                                 (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

API int zk_expr_specialised_source(zk_field_t f, const zk_expr_op* prog, uint32_t n_ops, uint32_t n_cols, uint32_t n_consts, char* out, uint64_t cap,
                                   uint64_t* len_out) {
    if (!prog || !len_out) return ZK_ERR_INVALID_ARG;
    std::string src;
    int st = ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, st = FieldLaunch<F>::expr_source_run(prog, n_ops, n_cols, n_consts, src));
    ZK_TRY(st);
    *len_out = src.size();
    if (out && cap) {
        const size_t k = src.size() < cap - 1 ? src.size() : (size_t)cap - 1;
        memcpy(out, src.data(), k);
        out[k] = 0;
    }
    return ZK_OK;
}

API int zk_expr_configure(int jit_mode) {
    if (jit_mode < 0 || jit_mode > 2) return ZK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g.mu);
    g.expr_jit = jit_mode;
    return ZK_OK;
}

}  // extern "C"
