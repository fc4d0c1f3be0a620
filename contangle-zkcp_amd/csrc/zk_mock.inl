// Launch sequences of MockProver::verify on the device (zk_mock_kernels.h).  Included by zk_ntt.inl, once per scalar field.
// Scratch (program words, tables, block totals, compacted positions, sort keys) belongs to the caller's stream.
#pragma once
#include "zk_mock_kernels.h"
namespace zk {

// P programs at every row of the 2^k-row domain: status[p n + i], and vals[p n + i] when vals is given.  offs: n_programs + 1 op
// offsets into prog (host).  Every program is validated on the host (expr_validate) before anything is launched.
template <class F>
int FieldLaunch<F>::mock_eval_run(DeviceCtx& dc, uint32_t k, const zk_expr_op* prog, const uint32_t* offs, uint32_t n_programs, const void* const* cols,
                                  const uint64_t* poison_from, uint32_t n_cols, const Fe<F>* consts, uint32_t n_consts, Fe<F>* vals, uint8_t* status, hipStream_t st) {
    if (k > 30 || k > (uint32_t)F::TWO_ADICITY || n_programs == 0 || n_programs > MOCK_MAX_PROGRAMS || offs[0] != 0) return ZK_ERR_INVALID_ARG;
    const uint64_t n = 1ull << k;
    for (uint32_t p = 0; p < n_programs; p++) {
        if (offs[p + 1] <= offs[p] || offs[p + 1] - offs[p] > EXPR_MAX_OPS) return ZK_ERR_INVALID_ARG;
        ZK_TRY(expr_validate(prog + offs[p], offs[p + 1] - offs[p], cols, n_cols, n_consts));
    }
    for (uint32_t c = 0; c < n_cols; c++)
        if (poison_from[c] > n) return ZK_ERR_INVALID_ARG;
    const uint32_t total_ops = offs[n_programs];
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    // [program words | column pointers | constants | offsets | poison_from], every part 16-byte aligned
    const size_t pb = (sizeof(uint64_t) * total_ops + 15) & ~(size_t)15, cb = sizeof(void*) * EXPR_MAX_COLS, kb = sizeof(Fe<F>) * EXPR_MAX_CONSTS;
    const size_t ob = (sizeof(uint32_t) * (n_programs + 1) + 15) & ~(size_t)15, fb = sizeof(uint32_t) * EXPR_MAX_COLS;
    ZK_TRY(ws_get(ss->poly_tot, pb + cb + kb + ob + fb));
    unsigned char* base = (unsigned char*)ss->poly_tot.p;
    std::vector<uint64_t> words(total_ops);
    for (uint32_t j = 0; j < total_ops; j++) words[j] = expr_word(prog[j]);
    std::vector<uint32_t> pf(n_cols ? n_cols : 1, 0);
    for (uint32_t c = 0; c < n_cols; c++) pf[c] = (uint32_t)poison_from[c];      // (n <= 2^30)
    HIP_TRY(hipMemcpyAsync(base, words.data(), sizeof(uint64_t) * total_ops, hipMemcpyHostToDevice, st));
    if (n_cols) HIP_TRY(hipMemcpyAsync(base + pb, cols, sizeof(void*) * n_cols, hipMemcpyHostToDevice, st));
    if (n_consts) HIP_TRY(hipMemcpyAsync(base + pb + cb, consts, sizeof(Fe<F>) * n_consts, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + pb + cb + kb, offs, sizeof(uint32_t) * (n_programs + 1), hipMemcpyHostToDevice, st));
    if (n_cols) HIP_TRY(hipMemcpyAsync(base + pb + cb + kb + ob, pf.data(), sizeof(uint32_t) * n_cols, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the sources are host memory (the caller's and this frame's)
    uint64_t bx = (n + EXPR_WG - 1) / EXPR_WG;
    if (bx > MOCK_GRID_X) bx = MOCK_GRID_X;
    ZK_LAUNCH((mock_eval_kernel<F>), (unsigned)(bx * n_programs), EXPR_WG, 0, st, (const uint64_t*)base, (const uint32_t*)(base + pb + cb + kb), n_programs,
              (uint32_t)bx, (const Fe<F>* const*)(base + pb), (const uint32_t*)(base + pb + cb + kb + ob), n_cols, (const Fe<F>*)(base + pb + cb), n_consts, k,
              vals, status);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

// positions / bytes of the first `cap` non-zero bytes of status[0 .. N), ascending, and their total.  The host arrays get
// min(total, cap) entries; what lies past them is not touched.  Synchronises the stream once, at the end.
template <class F>
int FieldLaunch<F>::mock_failures_run(DeviceCtx& dc, const uint8_t* status, uint64_t N, uint64_t cap, uint64_t* pos_host, uint8_t* kind_host, uint64_t* total_host,
                                      hipStream_t st) {
    *total_host = 0;
    if (N == 0) return ZK_OK;
    if (cap > N) cap = N;
    const uint64_t nblocks64 = (N + FLAGS_CHUNK - 1) / FLAGS_CHUNK;
    if (nblocks64 >= (1ull << 31)) return ZK_ERR_INVALID_ARG;
    const uint32_t nblocks = (uint32_t)nblocks64;
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    // poly_a: [total | block offsets (u64) | block totals (u32)]; poly_b: [positions (u64) x cap | bytes x cap]
    ZK_TRY(ws_get(ss->poly_a, 8 + 12ull * nblocks + 16));
    ZK_TRY(ws_get(ss->poly_b, 9 * cap + 16));
    uint64_t* total_dev = (uint64_t*)ss->poly_a.p;
    uint64_t* offs = total_dev + 1;
    uint32_t* tot = (uint32_t*)(offs + nblocks);
    uint64_t* pos = (uint64_t*)ss->poly_b.p;
    uint8_t* kind = (uint8_t*)(pos + cap);
    ZK_LAUNCH((flags_count_kernel<F>), nblocks, FLAGS_WG, 0, st, status, N, tot);
    ZK_LAUNCH((flags_scan_kernel<F>), 1, FLAGS_WG, 0, st, (const uint32_t*)tot, offs, nblocks, total_dev);
    if (cap) ZK_LAUNCH((flags_emit_kernel<F>), nblocks, FLAGS_WG, 0, st, status, N, (const uint64_t*)offs, cap, pos, kind);
    HIP_TRY(hipGetLastError());
    // the compacted arrays come back through a staging buffer of this frame: the caller's arrays must keep what lies past
    // min(total, cap), and the total is not known before the one synchronisation
    std::vector<uint64_t> pos_stage(cap);
    std::vector<uint8_t> kind_stage(cap);
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, total_dev, sizeof total, hipMemcpyDeviceToHost, st));
    if (cap) {
        HIP_TRY(hipMemcpyAsync(pos_stage.data(), pos, 8 * cap, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(kind_stage.data(), kind, cap, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t m = total < cap ? total : cap;
    if (m) {
        memcpy(pos_host, pos_stage.data(), 8 * m);
        memcpy(kind_host, kind_stage.data(), m);
    }
    *total_host = total;
    return ZK_OK;
}

// status[c n + r] of the copy constraints over the permutation's ncols columns; *bad_mapping = 1 when a mapping word names a
// cell outside the grid (nothing was read through it).  Synchronises the stream once, at the end, to read the status word.
template <class F>
int FieldLaunch<F>::mock_permutation_run(DeviceCtx& dc, uint32_t k, uint32_t ncols, const void* const* cols, const uint64_t* poison_from, const uint64_t* mapping,
                                         uint8_t* status, int* bad_mapping, hipStream_t st) {
    *bad_mapping = 0;
    if (ncols == 0 || k > 30 || k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
    const uint64_t n = 1ull << k, cells = n * ncols;
    std::vector<uint32_t> pf(ncols);
    for (uint32_t c = 0; c < ncols; c++) {
        if (!cols[c] || poison_from[c] > n) return ZK_ERR_INVALID_ARG;
        pf[c] = (uint32_t)poison_from[c];
    }
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    // [column pointers | poison_from | status word]
    const size_t cb = sizeof(void*) * ncols, fb = sizeof(uint32_t) * ncols;
    ZK_TRY(ws_get(ss->poly_tot, cb + fb + sizeof(uint32_t)));
    unsigned char* base = (unsigned char*)ss->poly_tot.p;
    uint32_t* word_dev = (uint32_t*)(base + cb + fb);
    HIP_TRY(hipMemcpyAsync(base, cols, cb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + cb, pf.data(), fb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(word_dev, 0, sizeof(uint32_t), st));
    HIP_TRY(hipStreamSynchronize(st));   // the sources are host memory
    uint64_t blocks = (cells + 255) / 256;
    if (blocks > MOCK_PERM_GRID) blocks = MOCK_PERM_GRID;
    ZK_LAUNCH((mock_permutation_kernel<F>), (unsigned)blocks, 256, 0, st, mapping, (const Fe<F>* const*)base, (const uint32_t*)(base + cb), cells, n, ncols,
              status, word_dev);
    HIP_TRY(hipGetLastError());
    uint32_t word = 0;
    HIP_TRY(hipMemcpyAsync(&word, word_dev, sizeof word, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *bad_mapping = word != 0;
    return ZK_OK;
}

// status[r] = 1 iff input row r < u is not among table rows [0, u); a_status / s_status (optional): the evaluator's status bytes
// of the two expressions, 2 = Poison.  Does not synchronise.
template <class F>
int FieldLaunch<F>::mock_lookup_run(DeviceCtx& dc, const Fe<F>* A, const uint8_t* a_status, const Fe<F>* S, const uint8_t* s_status, uint32_t u, uint8_t* status,
                                    hipStream_t st) {
    if (u == 0) return ZK_OK;
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    LkSort srt;
    ZK_TRY(lk_sort_begin(ss, u, 0, &srt, st));
    ZK_LAUNCH((mock_lookup_keys_kernel<F>), lk_key_blocks(dc, u), LK_WG, 0, st, S, s_status, u, srt.k0, srt.hist);
    ZK_TRY(lk_sort_passes<F>(srt, u, st));
    uint64_t fb = ((uint64_t)u + LK_WG - 1) / LK_WG;
    if (fb > 8192) fb = 8192;
    ZK_LAUNCH((mock_lookup_find_kernel<F>), (unsigned)fb, LK_WG, 0, st, A, a_status, u, (const LkKey*)srt.k0, (const LkKey*)srt.k1,
              (const uint32_t*)srt.meta, status);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
