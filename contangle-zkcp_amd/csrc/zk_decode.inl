// Launch sequence of the checked point decode (zk_decode_kernels.h).  Included by zk_msm.inl, once per curve.
#pragma once
#include "zk_decode_kernels.h"
namespace zk {

// n encoded points in host memory -> d_out (affine Montgomery, the layout zk_bases_adopt_device takes).  The bytes are staged in
// the stream's fb_tmp behind the status word; one copy up, one launch, one word back; synchronises `st` once, to read that word.
// A rejected point gives ZK_ERR_INVALID_ARG with the smallest rejected index and its reason; d_out is then unspecified.
template <class C>
int CurveLaunch<C>::points_decode_checked_run(DeviceCtx& dc, const uint8_t* in_host, uint64_t n, int compressed, Affine<C>* d_out, uint64_t* first_bad,
                                              uint64_t* reason, hipStream_t st) {
    if constexpr (ArkG1<C>::HAS) {
        using Fq = typename C::Fq;
        if (n >= (1ull << 31)) return ZK_ERR_INVALID_ARG;
        if (n == 0) return ZK_OK;
        const size_t bytes = (size_t)n * 4 * Fq::N * (compressed ? 1 : 2);
        StreamScratch* ss = nullptr;
        ZK_TRY(stream_scratch(dc, st, &ss));
        ZK_TRY(ws_get(ss->fb_tmp, 16 + bytes));
        unsigned long long* d_bad = (unsigned long long*)ss->fb_tmp.p;
        uint32_t* d_in = (uint32_t*)((unsigned char*)ss->fb_tmp.p + 16);
        DecodeConsts<C> k;
        uint64_t c = 1;   // p + 1, then >> 2
        for (int i = 0; i < Fq::N; i++) {
            c += Fq::P[i];
            k.sqrt_exp[i] = (uint32_t)c;
            c >>= 32;
        }
        for (int i = 0; i < Fq::N; i++) k.sqrt_exp[i] = (k.sqrt_exp[i] >> 2) | (i + 1 < Fq::N ? k.sqrt_exp[i + 1] << 30 : (uint32_t)c << 30);
        for (int i = 0; i < C::Fr::N; i++) k.order[i] = C::Fr::P[i];
        HIP_TRY(hipMemsetAsync(d_bad, 0xFF, 16, st));
        HIP_TRY(hipMemcpyAsync(d_in, in_host, bytes, hipMemcpyHostToDevice, st));
        uint64_t blocks = (n + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        ZK_LAUNCH((points_decode_checked_kernel<C>), (unsigned)blocks, 256, 0, st, (const uint32_t*)d_in, n, compressed ? 1 : 0, d_out, d_bad, k);
        unsigned long long w = 0;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&w, d_bad, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (w != DECODE_NONE) {
            if (first_bad) *first_bad = (uint64_t)(w >> 3);
            if (reason) *reason = (uint64_t)(w & 7);
            return ZK_ERR_INVALID_ARG;
        }
        return ZK_OK;
    }
    return ZK_ERR_UNSUPPORTED;
}

}  // namespace zk
