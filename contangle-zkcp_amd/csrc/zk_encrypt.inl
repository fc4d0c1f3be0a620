// Launch sequences of the EncryptCircuit kernels (zk_encrypt_kernels.h).  Included by zk_ntt.inl, once per scalar field.  Arguments
// are validated by the entry points (zk_api_encrypt.cc).
#pragma once
#include "zk_encrypt_kernels.h"
namespace zk {

// one launch, one tile of ENC_TILE elements per workgroup; does not synchronise
template <class F>
int FieldLaunch<F>::encrypt_witness_run(const Fe<F>* msg, uint64_t msg_len, uint64_t n, const Fe<F>& dh, Fe<F>* c2, Fe<F>* m, Fe<F>* b, Fe<F>* k,
                                        hipStream_t st) {
    if (n == 0) return ZK_OK;
    ZK_LAUNCH((encrypt_witness_kernel<F>), (unsigned)((n + ENC_TILE - 1) / ENC_TILE), ENC_WG, 0, st, msg, msg_len, n, dh, c2, m, b, k);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class F>
int FieldLaunch<F>::plaintext_from_bytes_run(const uint8_t* bytes, uint64_t len, Fe<F>* out, uint64_t n, hipStream_t st) {
    if (n == 0) return ZK_OK;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    ZK_LAUNCH((plaintext_from_bytes_kernel<F>), (unsigned)blocks, 256, 0, st, bytes, len, out, n);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

// scratch: [a: n_rows | b: n_rows | c: n_rows | R1CS_CHECK_MAX_GRID u64 words].  Three mat-vecs, the compare kernel, one copy of at
// most R1CS_CHECK_MAX_GRID words and one synchronisation; the minimum over the workgroups is taken here.
template <class F>
int FieldLaunch<F>::r1cs_first_unsatisfied_run(const R1csMatrix& ma, const R1csMatrix& mb, const R1csMatrix& mc, const Fe<F>* z, Fe<F>* scratch,
                                               uint64_t* first_row_out, hipStream_t st) {
    static_assert(R1CS_CHECK_MAX_GRID * sizeof(uint64_t) <= ZK_R1CS_CHECK_SCRATCH_ELEMS * sizeof(Fe<F>), "the block minima fit the scratch tail");
    const uint64_t rows = ma.n_rows;
    *first_row_out = UINT64_MAX;
    if (rows == 0) return ZK_OK;
    Fe<F>*a = scratch, *b = scratch + rows, *c = scratch + 2 * rows;
    uint64_t* block_min = (uint64_t*)(scratch + 3 * rows);
    ZK_TRY(r1cs_matvec_run(ma, z, a, rows, st));
    ZK_TRY(r1cs_matvec_run(mb, z, b, rows, st));
    ZK_TRY(r1cs_matvec_run(mc, z, c, rows, st));
    uint64_t blocks = (rows + R1CS_CHECK_WG - 1) / R1CS_CHECK_WG;
    if (blocks > R1CS_CHECK_MAX_GRID) blocks = R1CS_CHECK_MAX_GRID;
    ZK_LAUNCH((r1cs_first_unsatisfied_kernel<F>), (unsigned)blocks, R1CS_CHECK_WG, 0, st, (const Fe<F>*)a, (const Fe<F>*)b, (const Fe<F>*)c, rows, block_min);
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> part(blocks);
    HIP_TRY(hipMemcpyAsync(part.data(), block_min, blocks * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint64_t v : part)
        if (v < *first_row_out) *first_row_out = v;
    return ZK_OK;
}

}  // namespace zk
