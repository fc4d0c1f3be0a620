// Launch sequences of the Poseidon kernels (zk_poseidon_kernels.h) and their host twin.  Included by zk_ntt.inl, once per scalar
// field.  Arguments are validated by the entry points (zk_api_poseidon.cc); nothing here synchronises the stream.
#pragma once
#include "zk_host64.h"
#include "zk_poseidon_kernels.h"
namespace zk {

#define POSEIDON_WIDTH_SWITCH(w, ...)                 \
    switch (w) {                                      \
        case 2: { constexpr int T = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int T = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int T = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int T = 5; __VA_ARGS__; } break; \
        default: return ZK_ERR_INVALID_ARG;           \
    }

inline unsigned poseidon_grid(uint64_t count) {
    const uint64_t b = (count + POSEIDON_WG - 1) / POSEIDON_WG;
    return (unsigned)(b < POSEIDON_MAX_GRID ? b : POSEIDON_MAX_GRID);
}

// ---- the host twin: the same permutation and sponge on 64-bit limbs (zk_host64.h), no device, no zk_init ----
template <class F>
int FieldLaunch<F>::poseidon_permute_host_run(const PoseidonShape& sh, const Fe<F>* tbl, Fe<F>* states, uint64_t count) {
    using K = H64<F>;
    static_assert(sizeof(Fe<K>) == sizeof(Fe<F>), "same bytes");
    POSEIDON_WIDTH_SWITCH(sh.width, {
        for (uint64_t i = 0; i < count; i++) {
            Fe<K> s[T];
            memcpy(s, (const unsigned char*)states + i * sizeof s, sizeof s);
            poseidon_permute<K, T>(s, (const Fe<K>*)tbl, sh);
            memcpy((unsigned char*)states + i * sizeof s, s, sizeof s);
        }
    });
    return ZK_OK;
}
template <class F>
int FieldLaunch<F>::poseidon_hash_host_run(const PoseidonShape& sh, const Fe<F>* tbl, const Fe<F>* in, uint32_t arity, uint64_t count, Fe<F>* out) {
    using K = H64<F>;
    POSEIDON_WIDTH_SWITCH(sh.width, {
        for (uint64_t i = 0; i < count; i++) {
            Fe<K> d, x[POSEIDON_MAX_ARITY];          // (the caller's host arrays need not be 16-byte aligned)
            memcpy(x, in + i * arity, sizeof(Fe<K>) * arity);
            poseidon_hash_one<K, T>(&d, x, arity, (const Fe<K>*)tbl, sh);
            memcpy(out + i, &d, sizeof d);
        }
    });
    return ZK_OK;
}

// ---- device ----
template <class F>
int FieldLaunch<F>::poseidon_permute_run(const PoseidonShape& sh, const Fe<F>* tbl, Fe<F>* states, uint64_t count, hipStream_t st) {
    if (count == 0) return ZK_OK;
    POSEIDON_WIDTH_SWITCH(sh.width, ZK_LAUNCH((poseidon_permute_kernel<F, T>), poseidon_grid(count), POSEIDON_WG, 0, st, states, count, tbl, sh));
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}
template <class F>
int FieldLaunch<F>::poseidon_hash_run(const PoseidonShape& sh, const Fe<F>* tbl, const Fe<F>* in, uint32_t arity, uint64_t count, Fe<F>* out, hipStream_t st) {
    if (count == 0) return ZK_OK;
    POSEIDON_WIDTH_SWITCH(sh.width, ZK_LAUNCH((poseidon_hash_kernel<F, T>), poseidon_grid(count), POSEIDON_WG, 0, st, in, arity, count, out, tbl, sh));
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}
// nodes[0 .. 2n - 1): the leaf digests, then every level behind the one below; 1 launch for the leaves, one per level of more than
// 2^POSEIDON_TAIL_LOG nodes, one for all the levels above (a 2^20 tree: 1 + 11 + 1)
template <class F>
int FieldLaunch<F>::poseidon_tree_run(const PoseidonShape& sh, const Fe<F>* tbl, const Fe<F>* leaves, uint32_t leaf_arity, uint32_t log_n, Fe<F>* nodes, hipStream_t st) {
    uint64_t m = 1ull << log_n, off = 0;
    ZK_TRY(poseidon_hash_run(sh, tbl, leaves, leaf_arity, m, nodes, st));
    while (m > 2 * POSEIDON_WG) {
        ZK_TRY(poseidon_hash_run(sh, tbl, nodes + off, 2, m / 2, nodes + off + m, st));
        off += m;
        m /= 2;
    }
    POSEIDON_WIDTH_SWITCH(sh.width, ZK_LAUNCH((poseidon_tree_tail_kernel<F, T>), 1, POSEIDON_WG, 0, st, nodes, off, (uint32_t)m, tbl, sh));
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}
// idx: host, every entry < 2^log_n (checked by the caller); out: count x log_n siblings, bottom-up
template <class F>
int FieldLaunch<F>::merkle_paths_run(const Fe<F>* nodes, uint32_t log_n, const uint64_t* idx, uint64_t count, Fe<F>* out, hipStream_t st) {
    for (uint64_t c0 = 0; c0 < count; c0 += MERKLE_PATHS_PER_LAUNCH) {
        const uint32_t c = (uint32_t)(count - c0 < MERKLE_PATHS_PER_LAUNCH ? count - c0 : MERKLE_PATHS_PER_LAUNCH);
        MerklePathIndices ix;
        for (uint32_t q = 0; q < MERKLE_PATHS_PER_LAUNCH; q++) ix.idx[q] = q < c ? (uint32_t)idx[c0 + q] : 0;
        ZK_LAUNCH((merkle_paths_kernel<F>), (c * log_n + 255) / 256, 256, 0, st, nodes, log_n, ix, c, out + c0 * log_n);
    }
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}
template <class F>
int FieldLaunch<F>::vec_add_scalar_run(Fe<F>* out, const Fe<F>* a, uint64_t n, const Fe<F>& s, hipStream_t st) {
    if (n == 0) return ZK_OK;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    ZK_LAUNCH((vec_add_scalar_kernel<F>), (unsigned)blocks, 256, 0, st, out, a, n, s);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
