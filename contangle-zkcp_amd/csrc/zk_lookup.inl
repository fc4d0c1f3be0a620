// Launch sequence of the lookup argument's permute_expression_pair (zk_lookup_kernels.h).  Included by zk_ntt.inl, once
// per scalar field.  Scratch (the two key buffers, the per-pass counts, the run arrays, histogram and meta words) belongs
// to the caller's stream.
#pragma once
#include "zk_lookup_kernels.h"
namespace zk {

// The 256-bit LSD radix sort both callers share (permute_expression_pair below, the lookup check of zk_mock.inl): scratch for
// `total` keys, then -- after the caller's own kernel has written the keys to k0 and their digit histogram to hist -- the plan and
// the passes.  The sorted keys end in k0 or k1 as meta[LK_M_SEL + LK_DIGITS] says.
struct LkSort {
    LkKey *k0, *k1;
    uint32_t *counts, *extra, *hist, *meta;
    uint32_t nblocks;
};
// extra_words: 32-bit words the caller wants after the per-pass counts (lk_runs); hist and meta are cleared on the stream
inline int lk_sort_begin(StreamScratch* ss, uint64_t total, uint64_t extra_words, LkSort* s, hipStream_t st) {
    s->nblocks = (uint32_t)((total + LK_CHUNK - 1) / LK_CHUNK);
    ZK_TRY(ws_get(ss->lk_keys, 2 * total * sizeof(LkKey)));
    ZK_TRY(ws_get(ss->lk_runs, (256ull * s->nblocks + extra_words) * sizeof(uint32_t)));
    ZK_TRY(ws_get(ss->lk_meta, (LK_DIGITS * 256 + LK_META) * sizeof(uint32_t)));
    s->k0 = (LkKey*)ss->lk_keys.p;
    s->k1 = s->k0 + total;
    s->counts = (uint32_t*)ss->lk_runs.p;
    s->extra = s->counts + 256ull * s->nblocks;
    s->hist = (uint32_t*)ss->lk_meta.p;
    s->meta = s->hist + LK_DIGITS * 256;
    HIP_TRY(hipMemsetAsync(s->hist, 0, (LK_DIGITS * 256 + LK_META) * sizeof(uint32_t), st));
    return ZK_OK;
}
template <class F>
int lk_sort_passes(const LkSort& s, uint64_t total, hipStream_t st) {
    const uint32_t nblocks = s.nblocks;
    ZK_LAUNCH((lk_plan_kernel<F>), 1, 64, 0, st, s.hist, s.meta, total);
    // every digit gets its three launches; a dead one (one bucket holds every key) returns at once on the device, so the
    // host never waits for the histogram
    for (uint32_t d = 0; d < LK_DIGITS; d++) {
        ZK_LAUNCH((lk_count_kernel<F>), nblocks, LK_WG, 0, st, s.k0, s.k1, s.meta, d, total, s.counts, nblocks);
        if (nblocks <= LK_SMALL_SCAN) ZK_LAUNCH((lk_offsets_small_kernel<F>), 1, LK_WG, 0, st, s.meta, d, s.hist, s.counts, nblocks);
        else ZK_LAUNCH((lk_offsets_kernel<F>), 256, LK_WG, 0, st, s.meta, d, s.hist, s.counts, nblocks);
        ZK_LAUNCH((lk_scatter_kernel<F>), nblocks, LK_WG, 0, st, s.k0, s.k1, s.meta, d, total, s.counts, nblocks);
    }
    return ZK_OK;
}
// workgroups of a key-building kernel (a grid-stride loop over `total` keys)
inline unsigned lk_key_blocks(const DeviceCtx& dc, uint64_t total) {
    uint64_t kb = (total + LK_WG - 1) / LK_WG;
    const uint64_t kb_max = dc.num_cus > 0 ? 2ull * dc.num_cus : 512;
    return (unsigned)(kb > kb_max ? kb_max : kb);
}

template <class F>
int FieldLaunch<F>::permute_expression_pair_run(DeviceCtx& dc, const Fe<F>* A, const Fe<F>* S, uint32_t u, Fe<F>* a_out, Fe<F>* s_out, int* lookup_failed,
                                                hipStream_t st) {
    static_assert(F::N == 8, "256-bit keys");
    static_assert(F::P[7] < 0x80000000u, "the modulus leaves bit 255 free for the input / table tag");
    *lookup_failed = 0;
    if (u == 0) return ZK_OK;
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    const uint64_t total = 2ull * u;
    // [counts 256 x nblocks | run-scan block sums 3 x nblocks | rpos | astart | lstart | rstart (total each)]
    LkSort srt;
    ZK_TRY(lk_sort_begin(ss, total, 3ull * ((total + LK_CHUNK - 1) / LK_CHUNK) + 4 * total, &srt, st));
    const uint32_t nblocks = srt.nblocks;
    LkKey *k0 = srt.k0, *k1 = srt.k1;
    uint32_t* tot = srt.extra;
    uint32_t* rpos = tot + 3ull * nblocks;
    uint32_t *astart = rpos + total, *lstart = astart + total, *rstart = lstart + total;
    uint32_t *hist = srt.hist, *meta = srt.meta;

    ZK_LAUNCH((lk_keys_kernel<F>), lk_key_blocks(dc, total), LK_WG, 0, st, A, S, u, k0, hist);
    ZK_TRY(lk_sort_passes<F>(srt, total, st));
    ZK_LAUNCH((lk_runs_reduce_kernel<F>), nblocks, LK_WG, 0, st, k0, k1, meta, total, tot);
    ZK_LAUNCH((lk_runs_totals_kernel<F>), 1, LK_WG, 0, st, tot, nblocks, meta);
    ZK_LAUNCH((lk_runs_apply_kernel<F>), nblocks, LK_WG, 0, st, k0, k1, meta, total, tot, rpos, astart, lstart, rstart);
    uint64_t eb = (u + LK_WG - 1) / LK_WG;
    if (eb > 8192) eb = 8192;
    ZK_LAUNCH((lk_emit_kernel<F>), (unsigned)eb, LK_WG, 0, st, k0, k1, meta, u, rpos, astart, lstart, rstart, a_out, s_out);
    HIP_TRY(hipGetLastError());
    uint32_t status = 0;
    HIP_TRY(hipMemcpyAsync(&status, meta + LK_M_STATUS, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *lookup_failed = status != 0;
    return ZK_OK;
}

}  // namespace zk
