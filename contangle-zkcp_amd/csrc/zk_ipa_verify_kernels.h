// halo2 opening verification (halo2_proofs 0.2 poly/commitment/verifier.rs, Guard::use_challenges / compute_g): compute_s.
//   upstream: compute_s(u, init) builds s in k doubling passes on CPU threads (s[0] = init; each challenge, last to first, copies the
//             filled prefix times u_j behind itself), n = 2^k elements:
//                 s[i] = init prod_j u_j^bit_(k-1-j)(i),   u_0 -- the first round's challenge -- on the top bit
//   here:     ipa_s_kernel   s[i] (= or +=) sum_{p < count} lo_p[i mod 2^LB] hi_p[i >> LB],   LB = min(k, 8)
//             lo_p[j] = prod over the low LB bits of j, hi_p[h] = init_p prod over the k - LB bits of h (ipa_s_tables_kernel)
// One pass over s for all `count` proofs of a batch: one product and one addition per element and proof, one 32-byte store per
// element, one 32-byte load when accumulating.  The split is at the workgroup's width on purpose.  Element i = 256 row + lane, and
// a workgroup walks whole rows, so through every trip of its loop a lane's low index is its lane number and the row is the high
// index: the low entries are read once, before the loop, and stay in registers (8 VGPRs a proof), and the high entry's address is
// the same for the whole workgroup -- a scalar load that every lane shares.  Neither table is indexed per lane inside the loop, so
// neither LDS nor the vector L1 / L2 path carries table traffic there; the stream of s owns the vector memory path.  (DESIGN.md:
// the table-placement paragraph of the opening-verification section.)
// k < 8: one partial row, the low table has 2^k entries and the high table one entry, init_p.
#pragma once
#include "zk_rt.h"
#include "zk_field.h"

namespace zk {

constexpr uint32_t IPA_S_LOW_BITS = 8;       // = log2 of the workgroup: the low index is the lane number
constexpr uint32_t IPA_S_MAX_COUNT = 8;      // proofs per launch: their low entries live in 64 VGPRs; more is chunked on the host
constexpr uint32_t IPA_S_MAX_K = 32;         // the largest two-adicity of the scalar fields

// one proof's challenges, passed by value as a kernel argument (1056 bytes): the caller's host memory is read before the launch
// returns, so the entry point needs neither a staging copy nor a synchronisation
template <class F>
struct IpaChallenges {
    Fe<F> u[IPA_S_MAX_K];     // u[0] = the first round's challenge (the top bit of the index)
    Fe<F> init;
};

// lo[j], j < nlo = 2^lb: prod_{b < lb, bit b of j} u[k - 1 - b];  hi[h], h < nhi = 2^(k - lb): init prod_{b < k - lb, bit b of h} u[k - 1 - lb - b]
template <class F>
__global__ void __launch_bounds__(256) ipa_s_tables_kernel(IpaChallenges<F> ch, uint32_t k, uint32_t lb, Fe<F>* __restrict__ lo, Fe<F>* __restrict__ hi,
                                                           uint64_t nlo, uint64_t nhi) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nlo + nhi; e += (uint64_t)gridDim.x * blockDim.x) {
        const bool high = e >= nlo;
        const uint64_t idx = high ? e - nlo : e;
        const uint32_t bits = high ? k - lb : lb, top = high ? k - 1 - lb : k - 1;      // (bits = 0 when lb = k: `top` is then unused)
        Fe<F> x;
        if (high) x = ch.init;
        else fe_one(x);
        for (uint32_t b = 0; b < bits; b++)
            if ((idx >> b) & 1) fe_mul(x, x, ch.u[top - b]);
        (high ? hi : lo)[idx] = x;
    }
}

// lo: count x nlo, hi: count x nrows (proof-major); nrows = max(1, n / 256) rows of 256 elements, nlo = min(n, 256)
template <class F>
__global__ void __launch_bounds__(256) ipa_s_kernel(Fe<F>* __restrict__ s, uint64_t n, uint64_t nrows, const Fe<F>* __restrict__ lo,
                                                    const Fe<F>* __restrict__ hi, uint32_t nlo, uint32_t count, int accumulate) {
    const uint32_t lane = threadIdx.x;
    if (lane >= nlo) return;                  // n < 256: the lanes past the end (nothing in this kernel synchronises)
    Fe<F> l[IPA_S_MAX_COUNT];
#pragma unroll
    for (uint32_t p = 0; p < IPA_S_MAX_COUNT; p++)
        if (p < count) l[p] = lo[(uint64_t)p * nlo + lane];
    for (uint64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
        const uint64_t i = row * 256 + lane;  // < n: nlo = 256 and n = 256 nrows, or one partial row and lane < nlo = n
        Fe<F> acc;
        if (accumulate) acc = s[i];
#pragma unroll
        for (uint32_t p = 0; p < IPA_S_MAX_COUNT; p++)
            if (p < count) {
                Fe<F> x = hi[(uint64_t)p * nrows + row];      // the same address in every lane
                fe_mul(x, x, l[p]);
                if (p == 0 && !accumulate) acc = x;
                else fe_add(acc, acc, x);
            }
        s[i] = acc;
    }
}

}  // namespace zk
