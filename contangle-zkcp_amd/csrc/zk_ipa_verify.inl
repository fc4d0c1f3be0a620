// Launch sequence of halo2 opening verification (zk_ipa_verify_kernels.h).  Included by zk_ntt.inl, once per scalar field.
#pragma once
#include "zk_ipa_verify_kernels.h"
namespace zk {

// poly/commitment/verifier.rs compute_s for `count` proofs at once: s[i] (= or +=) sum_p init_p prod_j u_{p,j}^bit_(k-1-j)(i), i < 2^k.
// u_host: count x k elements, proof-major, u_0 first; init_host: count elements (host memory; read before this
// returns).  Per chunk of <= IPA_S_MAX_COUNT proofs: one small launch per proof for its two tables (the challenges travel as the
// kernel argument), then ONE pass over s; later chunks accumulate.  The tables live in the stream's scratch (32 bytes x (2^min(k, 8)
// + 2^(k - 8)) a proof: 129 KB at k = 20) and everything is ordered by the stream: no synchronisation.  A chunk also stays below
// IPA_S_SCRATCH_BYTES of tables where one proof allows it (k >= 22: fewer proofs a pass).
constexpr size_t IPA_S_SCRATCH_BYTES = 64u << 20;
template <class F>
int FieldLaunch<F>::ipa_s_run(DeviceCtx& dc, uint32_t k, uint32_t count, const void* u_host, const void* init_host, Fe<F>* s, int accumulate, hipStream_t st) {
    if (k == 0 || k > (uint32_t)F::TWO_ADICITY || k > IPA_S_MAX_K || count == 0) return ZK_ERR_INVALID_ARG;
    const uint64_t n = 1ull << k;
    const uint32_t lb = k < IPA_S_LOW_BITS ? k : IPA_S_LOW_BITS;
    const uint64_t nlo = 1ull << lb, nrows = n >> lb, per_proof = nlo + nrows;
    uint32_t chunk = IPA_S_MAX_COUNT;
    while (chunk > 1 && (size_t)chunk * per_proof * sizeof(Fe<F>) > IPA_S_SCRATCH_BYTES) chunk >>= 1;
    if (chunk > count) chunk = count;
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    ZK_TRY(ws_get(ss->poly_a, (size_t)chunk * per_proof * sizeof(Fe<F>)));
    Fe<F>* lo = (Fe<F>*)ss->poly_a.p;         // [chunk, nlo]
    Fe<F>* hi = lo + (uint64_t)chunk * nlo;   // [chunk, nrows]
    uint64_t tblocks = (per_proof + 255) / 256, blocks = nrows;
    if (tblocks > 1024) tblocks = 1024;
    if (blocks > 2048) blocks = 2048;         // 8 workgroups a CU: more than are resident at this kernel's registers; the rest on further trips
    IpaChallenges<F> ch;
    for (uint32_t first = 0; first < count; first += chunk) {
        const uint32_t c = count - first < chunk ? count - first : chunk;
        for (uint32_t p = 0; p < c; p++) {
            const unsigned char* up = (const unsigned char*)u_host + (size_t)(first + p) * k * sizeof(Fe<F>);
            for (uint32_t j = 0; j < IPA_S_MAX_K; j++) {
                if (j < k) host_load(ch.u[j], up + (size_t)j * sizeof(Fe<F>));
                else fe_zero(ch.u[j]);
            }
            host_load(ch.init, (const unsigned char*)init_host + (size_t)(first + p) * sizeof(Fe<F>));
            ZK_LAUNCH((ipa_s_tables_kernel<F>), (unsigned)tblocks, 256, 0, st, ch, k, lb, lo + (uint64_t)p * nlo, hi + (uint64_t)p * nrows, nlo, nrows);
            HIP_TRY(hipGetLastError());
        }
        ZK_LAUNCH((ipa_s_kernel<F>), (unsigned)blocks, 256, 0, st, s, n, nrows, (const Fe<F>*)lo, (const Fe<F>*)hi, (uint32_t)nlo, c,
                  (accumulate || first) ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    return ZK_OK;
}

}  // namespace zk
