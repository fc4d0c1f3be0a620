// Poseidon over the four scalar fields: the permutation, the sponge hash of ark-sponge 0.3 (`PoseidonSponge`, rate slots behind the
// capacity element) and of halo2_gadgets (`ConstantLength<L>`, rate slots first), the Merkle tree of ark-crypto-primitives over it,
// and the c2 stream of the reference's ElGamal encryption.  DESIGN.md section 5 "Poseidon" states the semantics; this is its code.
//
//   round i of RF + RP:  s[j] += ark[i][j];  s[j] = s[j]^alpha (all j in a full round, j = 0 in a partial one);  s = mds s
//   hash of `arity` elements:  s = init; elements are added into s[rate_offset ..) `rate` at a time with a permutation after every
//   block, the last one included; the digest is s[rate_offset]
//
// One lane per permutation, the state in registers (T Fe = 8 T VGPRs), saturated limbs, `fe_mul` = the generated product.  T is a
// template parameter so that every index into the state is a constant.  The round loop is a run-time loop and the full / partial
// switch depends on its counter only.  The S-box is ONE uniform loop for every alpha, square-and-multiply from the top bit down:
// for alpha = 3, 5, 7, 17 that is exactly the short chain (2, 3, 4 and 5 products; 17 = four squarings and one product), so no
// variant has to be selected and there is no select network between variants.
//
// Table (one per handle and device, uploaded once): [ark: (RF + RP) x T | mds: T x T | init: T] Montgomery elements.  Every lane
// reads the same entry, indexed by the round alone, through a `const __restrict__` pointer: scalar loads.
#pragma once
#include "zk_rt.h"
#include "zk_field.h"

namespace zk {

constexpr uint32_t POSEIDON_WG = 256;
constexpr uint32_t POSEIDON_MAX_GRID = 1024;    // workgroups of a grid-stride launch: 2^18 lanes a trip
constexpr uint32_t POSEIDON_TAIL_LOG = 8;       // levels of at most 2^8 nodes are computed by one workgroup in one launch
constexpr uint32_t POSEIDON_MIN_WIDTH = 2, POSEIDON_MAX_WIDTH = 5, POSEIDON_MAX_ROUNDS = 256, POSEIDON_MAX_ARITY = 64;
constexpr uint32_t MERKLE_MAX_LOG_N = 30;
constexpr uint32_t MERKLE_PATHS_PER_LAUNCH = 256;
static_assert(POSEIDON_WG == 1u << POSEIDON_TAIL_LOG, "the tail kernel gives every node of its widest level one lane");

struct PoseidonShape {
    uint32_t width, rate, rate_offset, full_rounds, partial_rounds;
    uint32_t alpha_top;      // index of alpha's highest set bit
    uint64_t alpha;
};

// leaf indices of one merkle_paths_kernel launch, by value in the kernel argument: the caller's list is read before the launch returns
struct MerklePathIndices {
    uint32_t idx[MERKLE_PATHS_PER_LAUNCH];
};

// x = x^alpha.  K is a field (device, emulator) or its 64-bit-limb host view H64<F> (the host twin).
template <class K>
ZK_HD void poseidon_sbox(Fe<K>& x, uint64_t alpha, uint32_t top) {
    Fe<K> r = x;
    for (uint32_t b = top; b-- > 0;) {
        fe_mul(r, r, r);
        if ((alpha >> b) & 1) fe_mul(r, r, x);
    }
    x = r;
}

// o[J ..] = rows J .. of mds s.  One row per instantiation rather than a loop over the rows: at width 5 the doubly unrolled loop is
// past the compiler's size limit for a requested unroll, the row loop stays a loop, and o[] indexed by its counter goes to scratch.
template <class K, int T, int J>
ZK_HD void poseidon_mds_rows(Fe<K> (&o)[T], const Fe<K> (&s)[T], const Fe<K>* __restrict__ mds) {
    if constexpr (J < T) {
        fe_mul(o[J], mds[J * T], s[0]);
        ZK_UNROLL
        for (int k = 1; k < T; k++) {
            Fe<K> t;
            fe_mul(t, mds[J * T + k], s[k]);
            fe_add(o[J], o[J], t);
        }
        poseidon_mds_rows<K, T, J + 1>(o, s, mds);
    }
}

template <class K, int T>
ZK_HD void poseidon_permute(Fe<K> (&s)[T], const Fe<K>* __restrict__ tbl, const PoseidonShape& sh) {
    const uint32_t rounds = sh.full_rounds + sh.partial_rounds, half = sh.full_rounds / 2;
    const Fe<K>* mds = tbl + (size_t)rounds * T;
    for (uint32_t i = 0; i < rounds; i++) {
        const Fe<K>* ark = tbl + (size_t)i * T;
        ZK_UNROLL
        for (int j = 0; j < T; j++) fe_add(s[j], s[j], ark[j]);
        poseidon_sbox(s[0], sh.alpha, sh.alpha_top);
        if (i < half || i >= half + sh.partial_rounds) {
            ZK_UNROLL
            for (int j = 1; j < T; j++) poseidon_sbox(s[j], sh.alpha, sh.alpha_top);
        }
        Fe<K> o[T];
        poseidon_mds_rows<K, T, 0>(o, s, mds);
        ZK_UNROLL
        for (int j = 0; j < T; j++) s[j] = o[j];
    }
}

// the sponge over in[0 .. arity); the digest goes to *out.  The rate slots are named by constants and guarded by the (uniform) shape,
// so the state is never indexed by a run-time value.
template <class K, int T>
ZK_HD void poseidon_hash_one(Fe<K>* out, const Fe<K>* in, uint32_t arity, const Fe<K>* __restrict__ tbl, const PoseidonShape& sh) {
    const Fe<K>* init = tbl + (size_t)(sh.full_rounds + sh.partial_rounds) * T + T * T;
    Fe<K> s[T];
    ZK_UNROLL
    for (int j = 0; j < T; j++) s[j] = init[j];
    for (uint32_t done = 0; done < arity; done += sh.rate) {
        const uint32_t take = arity - done < sh.rate ? arity - done : sh.rate;
        ZK_UNROLL
        for (int j = 0; j < T; j++)
            if ((uint32_t)j >= sh.rate_offset && (uint32_t)j - sh.rate_offset < take) fe_add(s[j], s[j], in[done + (uint32_t)j - sh.rate_offset]);
        poseidon_permute<K, T>(s, tbl, sh);
    }
    ZK_UNROLL
    for (int j = 0; j < T; j++)
        if ((uint32_t)j == sh.rate_offset) *out = s[j];
}

template <class F, int T>
__global__ void __launch_bounds__(POSEIDON_WG) poseidon_permute_kernel(Fe<F>* states, uint64_t count, const Fe<F>* __restrict__ tbl, PoseidonShape sh) {
    for (uint64_t i = (uint64_t)blockIdx.x * POSEIDON_WG + threadIdx.x; i < count; i += (uint64_t)gridDim.x * POSEIDON_WG) {
        Fe<F> s[T];
        ZK_UNROLL
        for (int j = 0; j < T; j++) s[j] = states[i * T + j];
        poseidon_permute<F, T>(s, tbl, sh);
        ZK_UNROLL
        for (int j = 0; j < T; j++) states[i * T + j] = s[j];
    }
}

// out[i] = hash of in[i arity .. (i + 1) arity).  A tree level is this kernel with arity = 2 over the level below.
template <class F, int T>
__global__ void __launch_bounds__(POSEIDON_WG) poseidon_hash_kernel(const Fe<F>* __restrict__ in, uint32_t arity, uint64_t count, Fe<F>* __restrict__ out,
                                                                     const Fe<F>* __restrict__ tbl, PoseidonShape sh) {
    for (uint64_t i = (uint64_t)blockIdx.x * POSEIDON_WG + threadIdx.x; i < count; i += (uint64_t)gridDim.x * POSEIDON_WG)
        poseidon_hash_one<F, T>(out + i, in + i * arity, arity, tbl, sh);
}

// One workgroup: every level above the one that has `m` <= 2 x 256 nodes at nodes[off ..), up to the root.  A level's nodes lie
// directly behind the level below (level j starts at 2n - 2^(log_n - j + 1)).  Every lane reaches every barrier.
template <class F, int T>
__global__ void __launch_bounds__(POSEIDON_WG) poseidon_tree_tail_kernel(Fe<F>* nodes, uint64_t off, uint32_t m, const Fe<F>* __restrict__ tbl, PoseidonShape sh) {
    while (m > 1) {
        const uint32_t half = m / 2;
        if (threadIdx.x < half) poseidon_hash_one<F, T>(nodes + off + m + threadIdx.x, nodes + off + 2 * threadIdx.x, 2, tbl, sh);
        off += m;
        m = half;
        __syncthreads();
    }
}

// out[c log_n + j] = level_j[(idx[c] >> j) ^ 1], j < log_n, c < count <= MERKLE_PATHS_PER_LAUNCH: one lane per sibling
template <class F>
__global__ void __launch_bounds__(256) merkle_paths_kernel(const Fe<F>* __restrict__ nodes, uint32_t log_n, MerklePathIndices ix, uint32_t count,
                                                           Fe<F>* __restrict__ out) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count * log_n) return;
    const uint32_t c = e / log_n, j = e % log_n;
    const uint64_t level = (2ull << log_n) - (2ull << (log_n - j));
    out[e] = nodes[level + ((ix.idx[c] >> j) ^ 1u)];
}

template <class F>
__global__ void __launch_bounds__(256) vec_add_scalar_kernel(Fe<F>* out, const Fe<F>* a, uint64_t n, Fe<F> s) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        Fe<F> x = a[i];
        fe_add(x, x, s);
        out[i] = x;
    }
}

}  // namespace zk
