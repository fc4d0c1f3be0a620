// C ABI, halo2 beyond commit / FFT: the permutation and lookup arguments, key generation (the copy-constraint assembly on the
// host, the permutation columns on the device), the opening verifier's helpers and MockProver::verify.
#include "zk_api_common.h"
#include "zk_ntt_decl.h"

using namespace zk;

extern "C" {

API int zk_halo2_permutation_product_device(zk_field_t f, uint32_t ncols, const void* const* cols, const void* const* sigmas, uint32_t first_col,
                                            const void* beta, const void* gamma, const void* delta, uint32_t k, const void* z_first, void* z_out,
                                            void* z_last_host, void* stream) {
    if (!cols || !sigmas || !beta || !gamma || !delta || !z_out || !aligned16(z_out) || ncols == 0 || ncols > 8) return ZK_ERR_INVALID_ARG;
    for (uint32_t c = 0; c < ncols; c++)
        if (!cols[c] || !sigmas[c] || !aligned16(cols[c]) || !aligned16(sigmas[c])) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(z_out);
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY || k > 30) return ZK_ERR_INVALID_ARG;
        Fe<F> b, g_, d, fst, w;
        host_load(b, beta);
        host_load(g_, gamma);
        host_load(d, delta);
        fe_one(fst);
        if (z_first) host_load(fst, z_first);
        for (int i = 0; i < F::N; i++) w.v[i] = F::ROOT[i];
        for (uint32_t i = k; i < (uint32_t)F::TWO_ADICITY; i++) fe_sqr(w, w);
        return FieldLaunch<F>::perm_product_run(dc, (int)f, ncols, cols, sigmas, first_col, b, g_, d, k, w, fst, (Fe<F>*)z_out, z_last_host, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_lookup_product_device(zk_field_t f, const void* a, const void* s, const void* ap, const void* sp, const void* beta,
                                       const void* gamma, uint64_t n, void* z_out, void* z_last_host, void* stream) {
    if (!beta || !gamma || (n && (!a || !s || !ap || !sp || !z_out || !aligned16(a) || !aligned16(s) || !aligned16(ap) || !aligned16(sp) || !aligned16(z_out))))
        return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(z_out);
    FIELD_SWITCH(f, {
        Fe<F> b, g_, one;
        host_load(b, beta);
        host_load(g_, gamma);
        fe_one(one);
        return FieldLaunch<F>::lookup_product_run(dc, (const Fe<F>*)a, (const Fe<F>*)s, (const Fe<F>*)ap, (const Fe<F>*)sp, b, g_, n, one, (Fe<F>*)z_out,
                                     z_last_host, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_permute_expression_pair_device(zk_field_t f, const void* inputs_dev, const void* table_dev, uint64_t usable_rows, void* a_perm_dev,
                                                void* s_perm_dev, void* stream) {
    if (usable_rows >= (1ull << 31)) return ZK_ERR_INVALID_ARG;
    if (usable_rows) {
        const void* ptrs[4] = {inputs_dev, table_dev, a_perm_dev, s_perm_dev};
        for (const void* p : ptrs)
            if (!p || !aligned16(p)) return ZK_ERR_INVALID_ARG;
        const uint64_t bytes = usable_rows * 32;
        if (spans_overlap(a_perm_dev, bytes, s_perm_dev, bytes) || spans_overlap(a_perm_dev, bytes, inputs_dev, bytes) ||
            spans_overlap(a_perm_dev, bytes, table_dev, bytes) || spans_overlap(s_perm_dev, bytes, inputs_dev, bytes) ||
            spans_overlap(s_perm_dev, bytes, table_dev, bytes))
            return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(a_perm_dev);
    FIELD_SWITCH(f, {
        int failed = 0;
        ZK_TRY(FieldLaunch<F>::permute_expression_pair_run(dc, (const Fe<F>*)inputs_dev, (const Fe<F>*)table_dev, (uint32_t)usable_rows, (Fe<F>*)a_perm_dev,
                                              (Fe<F>*)s_perm_dev, &failed, (hipStream_t)stream));
        return failed ? ZK_ERR_LOOKUP : ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
// ---- halo2 key generation: plonk/permutation/keygen.rs Assembly on the host (the walk of a cycle is sequential by definition),
// the permutation columns on the device (zk_keygen.inl)
namespace {
// Assembly { mapping, aux, sizes } over ncols x n cells, cell (c, r) at c * n + r.  mapping holds col << 32 | row, the form
// zk_halo2_assembly_mapping hands out; aux (the cycle's distinguished cell) and sizes are flat 32-bit cell indices / counts.
struct Halo2Assembly {
    uint64_t n = 0;
    uint32_t ncols = 0;
    std::vector<uint64_t> mapping;
    std::vector<uint32_t> aux, sizes;
    uint64_t flat(uint64_t packed) const { return (packed >> 32) * n + (packed & 0xffffffffull); }
    // Assembly::copy; false = Error::BoundsFailure (nothing changed)
    bool copy(uint32_t lc, uint32_t lr, uint32_t rc, uint32_t rr) {
        if (lc >= ncols || rc >= ncols || lr >= n || rr >= n) return false;
        uint64_t left = (uint64_t)lc * n + lr, right = (uint64_t)rc * n + rr;
        if (aux[left] == aux[right]) return true;                    // already in the same cycle
        if (sizes[aux[left]] < sizes[aux[right]]) std::swap(left, right);
        sizes[aux[left]] += sizes[aux[right]];                       // the left cycle absorbs the right one
        const uint32_t head = aux[left];
        uint64_t i = right;
        do {
            aux[i] = head;
            i = flat(mapping[i]);
        } while (i != right);
        std::swap(mapping[left], mapping[right]);
        return true;
    }
};
std::mutex g_asm_mu;
std::map<uint64_t, std::unique_ptr<Halo2Assembly>> g_asms;
uint64_t g_next_asm = 1;
}  // namespace

API int zk_halo2_assembly_new(uint64_t n, uint32_t ncols, uint64_t* handle_out) {
    if (!handle_out || n == 0 || ncols == 0 || n > (1ull << 32) || n * ncols >= (1ull << 32)) return ZK_ERR_INVALID_ARG;
    std::unique_ptr<Halo2Assembly> a;
    const uint64_t cells = n * ncols;
    try {
        a.reset(new Halo2Assembly());
        a->n = n;
        a->ncols = ncols;
        a->mapping.resize(cells);
        a->aux.resize(cells);
        a->sizes.assign(cells, 1u);
    } catch (const std::bad_alloc&) {
        return ZK_ERR_OOM;
    }
    for (uint32_t c = 0; c < ncols; c++)
        for (uint64_t r = 0; r < n; r++) {
            a->mapping[c * n + r] = ((uint64_t)c << 32) | r;
            a->aux[c * n + r] = (uint32_t)(c * n + r);
        }
    std::lock_guard<std::mutex> lk(g_asm_mu);
    const uint64_t h = g_next_asm++;
    g_asms[h] = std::move(a);
    *handle_out = h;
    return ZK_OK;
}
API int zk_halo2_assembly_copy(uint64_t handle, const uint32_t* quads, uint64_t count, uint64_t* applied_out) {
    if (applied_out) *applied_out = 0;
    if (count && !quads) return ZK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_asm_mu);
    auto it = g_asms.find(handle);
    if (it == g_asms.end()) return ZK_ERR_BAD_HANDLE;
    Halo2Assembly& a = *it->second;
    for (uint64_t q = 0; q < count; q++) {
        if (!a.copy(quads[4 * q], quads[4 * q + 1], quads[4 * q + 2], quads[4 * q + 3])) return ZK_ERR_INVALID_ARG;
        if (applied_out) *applied_out = q + 1;
    }
    return ZK_OK;
}
API int zk_halo2_assembly_mapping(uint64_t handle, void* mapping_out) {
    if (!mapping_out) return ZK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_asm_mu);
    auto it = g_asms.find(handle);
    if (it == g_asms.end()) return ZK_ERR_BAD_HANDLE;
    memcpy(mapping_out, it->second->mapping.data(), it->second->mapping.size() * sizeof(uint64_t));
    return ZK_OK;
}
API int zk_halo2_assembly_free(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_asm_mu);
    auto it = g_asms.find(handle);
    if (it == g_asms.end()) return ZK_ERR_BAD_HANDLE;
    g_asms.erase(it);
    return ZK_OK;
}
API int zk_halo2_permutation_sigmas_device(zk_field_t f, uint32_t k, uint32_t ncols, const void* mapping_dev, const void* delta,
                                           void* sigmas_dev, void* stream) {
    if (!mapping_dev || !delta || !sigmas_dev || !aligned16(mapping_dev) || !aligned16(sigmas_dev) || ncols == 0 || k > 30)
        return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
    });
    if (((uint64_t)ncols << k) >= (1ull << 32)) return ZK_ERR_INVALID_ARG;       // the assembly's own limit on the number of cells
    {   // 8 bytes per cell in, 32 out
        const uint64_t cells = (uint64_t)ncols << k;
        if (spans_overlap(mapping_dev, cells * 8, sigmas_dev, cells * 32)) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(sigmas_dev);
    FIELD_SWITCH(f, {
        Fe<F> d, w;
        host_load(d, delta);
        for (int i = 0; i < F::N; i++) w.v[i] = F::ROOT[i];
        for (uint32_t i = k; i < (uint32_t)F::TWO_ADICITY; i++) fe_sqr(w, w);
        int bad = 0;
        ZK_TRY(FieldLaunch<F>::perm_sigmas_run(dc, (int)f, k, ncols, (const uint64_t*)mapping_dev, d, w, (Fe<F>*)sigmas_dev, &bad, (hipStream_t)stream));
        return bad ? ZK_ERR_INVALID_ARG : ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
// ---- halo2 opening verification: poly/commitment/verifier.rs compute_s on the device (zk_ipa_verify.inl), compute_b on host limbs
API int zk_halo2_ipa_s_device(zk_field_t f, uint32_t k, uint32_t count, const void* u_host, const void* init_host, void* s_dev, int accumulate,
                              void* stream) {
    if (!u_host || !init_host || !s_dev || !aligned16(u_host) || !aligned16(init_host) || !aligned16(s_dev) || count == 0 || k == 0)
        return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
    });
    DEVICE_ENTRY(s_dev);
    FIELD_SWITCH(f, return FieldLaunch<F>::ipa_s_run(dc, k, count, u_host, init_host, (Fe<F>*)s_dev, accumulate, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_ipa_compute_b(zk_field_t f, uint32_t k, const void* x, const void* u_host, void* out) {
    if (!x || !u_host || !out || k == 0) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
        Fe<F> cur, acc, one, t;
        host_load(cur, x);
        fe_one(one);
        acc = one;
        for (uint32_t j = k; j-- > 0;) {      // the last round's challenge goes with x^1: cur = x^(2^(k - 1 - j))
            host_load(t, (const unsigned char*)u_host + (size_t)j * sizeof(Fe<F>));
            fe_mul(t, t, cur);
            fe_add(t, t, one);
            fe_mul(acc, acc, t);
            fe_sqr(cur, cur);
        }
        host_store(out, acc);
    });
    return ZK_OK;
}
// ---- MockProver::verify on the device (zk_mock.inl) ----
API int zk_halo2_mock_eval_device(zk_field_t f, uint32_t k, const zk_expr_op* programs, const uint32_t* offsets, uint32_t n_programs,
                                  const void* const* cols, const uint64_t* poison_from, uint32_t n_cols, const void* consts, uint32_t n_consts,
                                  void* values_out, uint8_t* status_out, void* stream) {
    if (!programs || !offsets || !status_out || !aligned16(status_out) || (values_out && !aligned16(values_out)) || (n_cols && (!cols || !poison_from)) ||
        (n_consts && !consts) || k > 30 || n_programs == 0)
        return ZK_ERR_INVALID_ARG;
    if (values_out) {   // 32 bytes per entry in one output, 1 in the other
        const uint64_t entries = (uint64_t)n_programs << k;
        if (spans_overlap(values_out, entries * 32, status_out, entries)) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(status_out);
    FIELD_SWITCH(f, return FieldLaunch<F>::mock_eval_run(dc, k, programs, offsets, n_programs, cols, poison_from, n_cols, (const Fe<F>*)consts, n_consts,
                                            (Fe<F>*)values_out, status_out, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_mock_lookup_device(zk_field_t f, uint32_t k, const void* inputs_dev, const uint8_t* inputs_status, const void* table_dev,
                                    const uint8_t* table_status, uint64_t usable_rows, uint8_t* status_out, void* stream) {
    if (k > 30 || usable_rows > (1ull << k)) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
    });
    if (usable_rows) {
        if (!inputs_dev || !table_dev || !status_out || !aligned16(inputs_dev) || !aligned16(table_dev)) return ZK_ERR_INVALID_ARG;
        const void* ins[4] = {inputs_dev, table_dev, inputs_status, table_status};
        const uint64_t bytes[4] = {usable_rows * 32, usable_rows * 32, usable_rows, usable_rows};
        for (int i = 0; i < 4; i++)
            if (ins[i] && spans_overlap(ins[i], bytes[i], status_out, usable_rows)) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(status_out);
    FIELD_SWITCH(f, return FieldLaunch<F>::mock_lookup_run(dc, (const Fe<F>*)inputs_dev, inputs_status, (const Fe<F>*)table_dev, table_status, (uint32_t)usable_rows,
                                              status_out, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_mock_permutation_device(zk_field_t f, uint32_t k, uint32_t ncols, const void* const* cols, const uint64_t* poison_from,
                                         const void* mapping_dev, uint8_t* status_out, void* stream) {
    if (!cols || !poison_from || !mapping_dev || !status_out || !aligned16(mapping_dev) || ncols == 0 || k > 30) return ZK_ERR_INVALID_ARG;
    if (((uint64_t)ncols << k) >= (1ull << 32)) return ZK_ERR_INVALID_ARG;       // the assembly's own limit on the number of cells
    {
        const uint64_t cells = (uint64_t)ncols << k;
        if (spans_overlap(mapping_dev, cells * 8, status_out, cells)) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(status_out);
    FIELD_SWITCH(f, {
        int bad = 0;
        ZK_TRY(FieldLaunch<F>::mock_permutation_run(dc, k, ncols, cols, poison_from, (const uint64_t*)mapping_dev, status_out, &bad, (hipStream_t)stream));
        return bad ? ZK_ERR_INVALID_ARG : ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_mock_failures_device(const uint8_t* status_dev, uint64_t n_status, uint64_t cap, uint64_t* positions_out, uint8_t* kinds_out,
                                      uint64_t* total_out, void* stream) {
    if (!total_out || (n_status && (!status_dev || !aligned16(status_dev))) || (cap && n_status && (!positions_out || !kinds_out)))
        return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(status_dev);
    return FieldLaunch<PallasFp>::mock_failures_run(dc, status_dev, n_status, cap, positions_out, kinds_out, total_out, (hipStream_t)stream);   // (the bytes carry no field)
}

}  // extern "C"
