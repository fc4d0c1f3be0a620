// Launch sequence of the point FFT (zk_ecfft_kernels.h).  Included by zk_msm.inl, once per curve.
#pragma once
#include "zk_ecfft_kernels.h"
namespace zk {

// omega (Montgomery) has order exactly 2^logn: omega^(n/2) == -1, or omega == 1 for n = 1
template <class F>
bool ecfft_omega_ok(const Fe<F>& omega, uint32_t logn) {
    Fe<F> one, w = omega;
    fe_one(one);
    if (logn == 0) return fe_eq(w, one);
    for (uint32_t i = 0; i + 1 < logn; i++) fe_sqr(w, w);
    fe_add(w, w, one);
    return fe_is_zero(w);
}

// dst[i] = sum_j [omega^(i j)] src[j] (times n^-1 when scale), n = 2^logn; affine in, canonical affine out; src == dst allowed.
// Workspaces: the stream's fb_tmp (n XYZZ points) and fb_table (n / 2 split twiddles).  Does not synchronise.
template <class C>
int CurveLaunch<C>::ntt_points_run(DeviceCtx& dc, const Affine<C>* src, Affine<C>* dst, uint32_t logn, const Fe<typename C::Fr>& omega, int scale, hipStream_t st) {
    if constexpr (Glv<C>::HAS) {
        using Fr = typename C::Fr;
        if (logn > ECFFT_MAX_LOG || !ecfft_omega_ok<Fr>(omega, logn)) return ZK_ERR_INVALID_ARG;
        const uint32_t n = 1u << logn, half = n >> 1;
        StreamScratch* ss = nullptr;
        ZK_TRY(stream_scratch(dc, st, &ss));
        ZK_TRY(ws_get(ss->fb_tmp, (size_t)n * sizeof(XYZZ<C>)));
        ZK_TRY(ws_get(ss->fb_table, (size_t)(half ? half : 1) * sizeof(FoldScalar)));
        XYZZ<C>* ws = (XYZZ<C>*)ss->fb_tmp.p;
        FoldScalar* tw = (FoldScalar*)ss->fb_table.p;
        FoldScalar ks{};
        if (scale && logn) {
            Fe<Fr> ninv;
            fe_one(ninv);
            for (uint32_t i = 0; i < logn; i++) fe_add(ninv, ninv, ninv);
            fe_inv(ninv, ninv);
            fe_from_mont(ninv, ninv);
            ecfft_scalar<C>(ks, ninv);
        }
        if (logn >= 2) {   // (a one-stage transform only uses the twiddle 1)
            EcfftLadder<Fr> lad;
            Fe<Fr> w = omega;
            for (uint32_t k = 0; k < ECFFT_MAX_LOG; k++) {
                lad.p[k] = w;
                fe_sqr(w, w);
            }
            ZK_LAUNCH((ecfft_twiddle_kernel<C>), (half + 255) / 256, 256, 0, st, lad, tw, half);
        }
        ZK_LAUNCH((ecfft_load_kernel<C>), (n + 63) / 64, 64, 0, st, src, ws, n, (int)logn, ks, (scale && logn) ? 1 : 0);
        for (uint32_t s = 0; s < logn; s++) {
            if (logn - 1 - s >= 6)
                ZK_LAUNCH((ecfft_stage_kernel<C, true>), half / 64, 64, 0, st, ws, (const FoldScalar*)tw, half, (int)s, (int)logn);
            else
                ZK_LAUNCH((ecfft_stage_kernel<C, false>), (half + 63) / 64, 64, 0, st, ws, (const FoldScalar*)tw, half, (int)s, (int)logn);
        }
        const uint32_t lanes = (n + FB_K - 1) / FB_K;
        ZK_LAUNCH((xyzz_batch_to_affine_kernel<C>), (lanes + 63) / 64, 64, 0, st, (const XYZZ<C>*)ws, dst, n);
        HIP_TRY(hipGetLastError());
        return ZK_OK;
    }
    return ZK_ERR_UNSUPPORTED;
}

// host points, in place: Jacobian (x, y, z) in, (x, y, 1) or (0, 1, 0) out.  Synchronises the null stream.
template <class C>
int CurveLaunch<C>::ntt_points_host_run(DeviceCtx& dc, void* jac_host, uint32_t logn, const Fe<typename C::Fr>& omega, int scale) {
    if constexpr (Glv<C>::HAS) {
        if (logn > ECFFT_MAX_LOG || !ecfft_omega_ok<typename C::Fr>(omega, logn)) return ZK_ERR_INVALID_ARG;
        const uint32_t n = 1u << logn;
        hipStream_t st = nullptr;
        StreamScratch* ss = nullptr;
        ZK_TRY(stream_scratch(dc, st, &ss));
        ZK_TRY(ws_get(ss->fb_tmp, (size_t)n * sizeof(XYZZ<C>)));
        void *d_jac = nullptr, *d_aff = nullptr;
        auto done = [&](int status) {
            if (d_jac) (void)hipFree(d_jac);
            if (d_aff) (void)hipFree(d_aff);
            return status;
        };
        const size_t jb = (size_t)n * sizeof(Jacobian<C>);
        if (hipMalloc(&d_jac, jb) != hipSuccess || hipMalloc(&d_aff, (size_t)n * sizeof(Affine<C>)) != hipSuccess) {
            (void)hipGetLastError();
            return done(ZK_ERR_OOM);
        }
        if (hipMemcpyAsync(d_jac, jac_host, jb, hipMemcpyHostToDevice, st) != hipSuccess) return done(ZK_ERR_HIP);
        ZK_LAUNCH((ecfft_jac_to_xyzz_kernel<C>), (n + 255) / 256, 256, 0, st, (const Jacobian<C>*)d_jac, (XYZZ<C>*)ss->fb_tmp.p, n);
        const uint32_t lanes = (n + FB_K - 1) / FB_K;
        ZK_LAUNCH((xyzz_batch_to_affine_kernel<C>), (lanes + 63) / 64, 64, 0, st, (const XYZZ<C>*)ss->fb_tmp.p, (Affine<C>*)d_aff, n);
        const int status = ntt_points_run(dc, (const Affine<C>*)d_aff, (Affine<C>*)d_aff, logn, omega, scale, st);
        if (status != ZK_OK) {
            (void)hipStreamSynchronize(st);
            return done(status);
        }
        ZK_LAUNCH((ecfft_affine_to_jac_kernel<C>), (n + 255) / 256, 256, 0, st, (const Affine<C>*)d_aff, (Jacobian<C>*)d_jac, n);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(jac_host, d_jac, jb, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return done(ZK_ERR_HIP);
        return done(ZK_OK);
    }
    return ZK_ERR_UNSUPPORTED;
}

}  // namespace zk
