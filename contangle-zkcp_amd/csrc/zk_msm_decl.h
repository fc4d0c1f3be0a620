// Launch sequences of the curve side (MSM, fixed-base): the static members of CurveLaunch<C>, defined in zk_msm.inl and the
// .inl files it pulls in, instantiated per curve by the one line of zk_msm_inst.cc.
#pragma once
#include "zk_internal.h"
namespace zk {
template <class C>
struct CurveLaunch {
    // enqueue the device work of one MSM on job.stream; the result is produced by job.finish after the job's last event
    static int msm_enqueue(MsmJob& job, const BasesCopy& bc, const Fe<typename C::Fr>* d_scalars, uint64_t n, int mont, const MsmTuning& tu);
    // scalar vectors per job of zk_msm_batch_device: the largest batch the launch plan accepts for this MSM (msm_plan_batch)
    static uint32_t msm_batch_size(const BasesCopy& bc, uint64_t n, const MsmTuning& tu, int num_cus);
    static int bases_prepare_run(BasesCopy& bc, uint64_t n);   // build the resident lazy-limb copy
    static int bases_precompute_run(BasesCopy& bc, uint64_t n, int c);   // window multiples for ZK_MSM_FLAG_PRECOMPUTED
    static int bases_shifts_run(BasesCopy& bc, uint64_t n);   // [2^(64 k)] P_i, k < 4, for the generator collapse
    static int bases_refresh_run(const BasesCopy& bc, uint64_t offset, uint64_t count, hipStream_t st);   // re-derive it for a rewritten range
    static int fixed_base_run(const Fe<typename C::Fr>* d_scalars, uint64_t n, Affine<C>* d_out, hipStream_t st);
    static int fixed_base_msm_run(DeviceCtx& dc, const Affine<C>& base, const Fe<typename C::Fr>* d_scalars, uint64_t n, int mont, Affine<C>* d_out,
                                  hipStream_t st);
    static int ipa_fold_bases_run(DeviceCtx& dc, Affine<C>* g, uint64_t half, const Fe<typename C::Fr>& u_canonical, hipStream_t st);
    static int ipa_collapse_run(DeviceCtx& dc, const BasesCopy& bc, uint64_t base_n, const Fe<typename C::Fr>* w_dev, uint64_t m0, uint64_t cur, uint64_t first,
                                uint64_t count, Affine<C>* g_out, hipStream_t st);
    // the DFT of a vector of curve points (zk_ecfft_kernels.h): Pallas and Vesta, ZK_ERR_UNSUPPORTED elsewhere
    static int ntt_points_run(DeviceCtx& dc, const Affine<C>* src, Affine<C>* dst, uint32_t logn, const Fe<typename C::Fr>& omega_mont, int scale, hipStream_t st);
    static int ntt_points_host_run(DeviceCtx& dc, void* jac_host, uint32_t logn, const Fe<typename C::Fr>& omega_mont, int scale);
    // the checked decode of ark-serialize points (zk_decode_kernels.h): BN254 G1 and BLS12-381 G1, ZK_ERR_UNSUPPORTED elsewhere
    static int points_decode_checked_run(DeviceCtx& dc, const uint8_t* in_host, uint64_t n, int compressed, Affine<C>* d_out, uint64_t* first_bad, uint64_t* reason,
                                         hipStream_t st);
};
}  // namespace zk
