// EncryptCircuit on the device (circuits-ark/src/encryption.rs:219-263, 303-317): the per-element section of the assignment, the
// plaintext of utils.rs:60-72, and the satisfaction check of the reference's test (`cs.is_satisfied()`).  DESIGN.md section 5
// "EncryptCircuit" states the layout; this is its code.
//
//   encrypt_witness_kernel          m, c2 = m + dh, b = [c2 != 0], k = c2^-1 (1 where c2 = 0): four segments of z, one launch
//   plaintext_from_bytes_kernel     out[i] = byte i as a field element, 0 from `len` on
//   r1cs_first_unsatisfied_kernel   per workgroup, the smallest row i with a[i] b[i] != c[i]
//
// The witness kernel shares one Fermat inversion among the ENC_K elements a lane owns (Montgomery's trick, as batch_invert_kernel
// with INV_K).  A lane owns the elements tile + lane + 64 j, j < ENC_K, of its workgroup's tile of 1024: at every step the 64 lanes
// of the wave touch 64 consecutive elements, 2 KiB, so every load and store is coalesced without a trip through LDS (a lane that
// owned 16 consecutive elements would store at a 512-byte stride).  The prefix products are parked in k[] itself, which the lane
// overwrites on the way back: no per-lane array, hence no scratch and no LDS.  A lane reads back only what it wrote itself.
// b and the padding of c2 are formed with word masks, not by selecting between structs.
#pragma once
#include "zk_rt.h"
#include "zk_field.h"

namespace zk {

constexpr uint32_t ENC_K = 16;                   // elements per lane and inversion
constexpr uint32_t ENC_WG = 64;                  // one wave per workgroup
constexpr uint32_t ENC_TILE = ENC_K * ENC_WG;    // elements per workgroup; the grid is not capped: one tile per workgroup
constexpr uint32_t R1CS_CHECK_WG = 256, R1CS_CHECK_MAX_GRID = 1024;

template <class F>
__global__ void __launch_bounds__(ENC_WG) encrypt_witness_kernel(const Fe<F>* __restrict__ msg, uint64_t msg_len, uint64_t n, Fe<F> dh, Fe<F>* c2, Fe<F>* m,
                                                                  Fe<F>* b, Fe<F>* k) {
    const uint64_t base = (uint64_t)blockIdx.x * ENC_TILE + threadIdx.x;
    Fe<F> run, one;
    fe_one(one);
    run = one;
    uint32_t cnt = 0;
    for (; cnt < ENC_K; cnt++) {
        const uint64_t i = base + (uint64_t)cnt * ENC_WG;
        if (i >= n) break;
        const bool live = i < msg_len;
        Fe<F> v, x, bit;
        fe_zero(v);
        if (live) v = msg[i];
        m[i] = v;
        fe_add(x, v, dh);
        const uint32_t keep = live ? 0xFFFFFFFFu : 0u;          // padding: c2 = 0, not dh
        ZK_UNROLL
        for (int w = 0; w < F::N; w++) x.v[w] &= keep;
        c2[i] = x;
        const bool nz = !fe_is_zero(x);
        const uint32_t set = nz ? 0xFFFFFFFFu : 0u;
        ZK_UNROLL
        for (int w = 0; w < F::N; w++) bit.v[w] = F::R[w] & set;
        b[i] = bit;
        k[i] = run;                                             // the product of the lane's nonzero elements before this one
        if (nz) fe_mul(run, run, x);                            // a zero contributes a factor 1
    }
    if (cnt == 0) return;
    Fe<F> inv;
    fe_inv(inv, run);
    for (uint32_t q = cnt; q-- > 0;) {
        const uint64_t i = base + (uint64_t)q * ENC_WG;
        Fe<F> x = c2[i];
        if (fe_is_zero(x)) {
            k[i] = one;                                         // upstream's is_neq multiplier of an empty element
            continue;
        }
        Fe<F> pre = k[i], r;
        fe_mul(r, inv, pre);
        fe_mul(inv, inv, x);
        k[i] = r;
    }
}

template <class F>
__global__ void __launch_bounds__(256) plaintext_from_bytes_kernel(const uint8_t* __restrict__ bytes, uint64_t len, Fe<F>* __restrict__ out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        Fe<F> a, r;
        fe_zero(a);
        if (i < len) a.v[0] = bytes[i];
        fe_to_mont(r, a);
        out[i] = r;
    }
}

// block_min[blockIdx.x] = the smallest row of this workgroup's share with a[i] b[i] != c[i], UINT64_MAX when it has none.  A minimum,
// taken in a fixed tree: the same answer on every run.  Every lane reaches every barrier.
template <class F>
__global__ void __launch_bounds__(R1CS_CHECK_WG) r1cs_first_unsatisfied_kernel(const Fe<F>* __restrict__ a, const Fe<F>* __restrict__ b,
                                                                              const Fe<F>* __restrict__ c, uint64_t n_rows,
                                                                              uint64_t* __restrict__ block_min) {
    __shared__ uint64_t part[R1CS_CHECK_WG];
    uint64_t best = UINT64_MAX;
    for (uint64_t i = (uint64_t)blockIdx.x * R1CS_CHECK_WG + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * R1CS_CHECK_WG) {
        Fe<F> x = a[i], y = b[i], w = c[i], xy;
        fe_mul(xy, x, y);
        if (!fe_eq(xy, w) && i < best) best = i;
    }
    part[threadIdx.x] = best;
    __syncthreads();
    for (uint32_t d = R1CS_CHECK_WG / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            const uint64_t o = part[threadIdx.x + d];
            if (o < best) best = o;
            part[threadIdx.x] = best;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) block_min[blockIdx.x] = best;
}

}  // namespace zk
