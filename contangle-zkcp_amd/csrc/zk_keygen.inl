// Launch sequence of halo2 key generation (zk_keygen_kernels.h).  Included by zk_ntt.inl, once per scalar field.
#pragma once
#include "zk_keygen_kernels.h"
namespace zk {

// plonk/permutation/keygen.rs Assembly::build_vk / build_pk, the permutation columns in Lagrange form: sigmas[c n + j] =
// delta^col omega^row for mapping[c n + j] = col << 32 | row, n = 2^k.  *bad_mapping = 1 when a cell names a row >= n or a column
// >= ncols (its slot holds 0; nothing was read through it).  Synchronises the stream once, at the end, to read the status word.
template <class F>
int FieldLaunch<F>::perm_sigmas_run(DeviceCtx& dc, int field, uint32_t k, uint32_t ncols, const uint64_t* mapping, const Fe<F>& delta, const Fe<F>& omega,
                                    Fe<F>* sigmas, int* bad_mapping, hipStream_t st) {
    *bad_mapping = 0;
    if (ncols == 0 || k > 30 || k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
    const uint64_t n = 1ull << k, cells = n * ncols;
    PowTables<F> wpow;
    ZK_TRY(pow_tables<F>(dc, omega, k, field, st, &wpow));
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    // [delta^c, c < ncols | status word]
    ZK_TRY(ws_get(ss->poly_tot, (size_t)ncols * sizeof(Fe<F>) + sizeof(uint32_t)));
    Fe<F>* dpow = (Fe<F>*)ss->poly_tot.p;
    uint32_t* status = (uint32_t*)(dpow + ncols);
    std::vector<Fe<F>> dp(ncols);      // (lives until the synchronisation below: the copy may still be reading it)
    fe_one(dp[0]);
    for (uint32_t c = 1; c < ncols; c++) fe_mul(dp[c], dp[c - 1], delta);
    HIP_TRY(hipMemcpyAsync(dpow, dp.data(), (size_t)ncols * sizeof(Fe<F>), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(status, 0, sizeof(uint32_t), st));
    uint64_t blocks = (cells + 255) / 256;
    if (blocks > 4096) blocks = 4096;      // 16 workgroups a CU; the rest of the cells on further trips of the loop
    ZK_LAUNCH((perm_sigma_kernel<F>), (unsigned)blocks, 256, 0, st, mapping, sigmas, cells, n, ncols, (const Fe<F>*)dpow, wpow, status);
    HIP_TRY(hipGetLastError());
    uint32_t word = 0;
    HIP_TRY(hipMemcpyAsync(&word, status, sizeof word, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *bad_mapping = word != 0;
    return ZK_OK;
}

}  // namespace zk
