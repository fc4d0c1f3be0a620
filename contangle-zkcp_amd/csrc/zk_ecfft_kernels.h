// The radix-2 DFT of a vector of curve points with scalar-field twiddles: halo2_proofs 0.2 arithmetic.rs `best_fft` with
// G = a curve, the call in poly/commitment.rs `Params::new` that turns the SRS g into g_lagrange (Pallas and Vesta).
//   upstream: bit-reversal, then log n stages of   t = a[k + j + m] * w^j ; a[k + j + m] = a[k + j] - t ; a[k + j] += t
//             with a full 255-bit double-and-add per butterfly, then a[i] *= n^-1 and batch_normalize
//   here:     ecfft_twiddle_kernel   w^j for j < n / 2 and its GLV split k1 + k2 lambda, once per transform
//             ecfft_load_kernel      ws[i] = [n^-1] src[bitrev i] (or a plain copy): the scaling uses one wave-uniform scalar
//             ecfft_stage_kernel     one stage in place over the XYZZ workspace.  The cost is the scalar multiplication, so the
//                                    lanes are laid out for ITS control flow, not for coalescing: stage s has m = 2^s twiddles,
//                                    each shared by n / 2m butterflies.  While n / 2m >= 64 (UNI) a wave takes 64 butterflies
//                                    of ONE twiddle from 64 different blocks: the GLV halves sit in scalar registers and the
//                                    joint chain of ~129 doublings branches uniformly, as in ipa_fold_bases_kernel.  The
//                                    last six stages (fewer than 64 blocks) run the same chain with per-lane scalars and pay
//                                    the masked additions.  Butterflies whose twiddle is 1 skip the multiplication.
//             xyzz_batch_to_affine_kernel (zk_msm_kernels.h) normalises the workspace into dst.
// The chain runs on lazy 29-bit limbs; the two additions of a butterfly, the negations and phi(x, y) = (beta x, y) are done
// on the saturated words the workspace is stored in (exact, canonical), a few dozen products next to the chain's ~3000.
// Included by zk_ecfft.inl at the end of zk_msm.inl: glv_decompose lives there.
#pragma once
#include "zk_msm_kernels.h"
#include "zk_ntt_kernels.h"

namespace zk {

constexpr uint32_t ECFFT_MAX_LOG = 24;   // = ZK_NTT_POINTS_MAX_LOG_N: 2^23 twiddles, a 2 GiB workspace

#if defined(ZK_EMU)
#define ZK_ECFFT_UNI(v) ((uint32_t)(v))
#else
#define ZK_ECFFT_UNI(v) ZK_UNIFORM32(v)
#endif

// omega^(2^k), k < ECFFT_MAX_LOG - 1 (Montgomery): the kernel argument the twiddle kernel takes its powers from
template <class F>
struct EcfftLadder {
    Fe<F> p[ECFFT_MAX_LOG];
};

// k (canonical) as the scalar of a chain: the GLV halves when the split is short, k itself otherwise
template <class C>
ZK_HD void ecfft_scalar(FoldScalar& ks, const Fe<typename C::Fr>& k) {
    ks = FoldScalar{};
    if (!glv_decompose<C>(k, ks)) {
        ks = FoldScalar{};
        for (int i = 0; i < C::Fr::N && i < 8; i++) ks.k1[i] = k.v[i];
    }
    ks.top_bit = -1;
    for (int b = 255; b >= 0; b--)
        if (((ks.k1[b >> 5] | ks.k2[b >> 5]) >> (b & 31)) & 1) {
            ks.top_bit = b;
            break;
        }
}

// tw[j] = omega^j, j < count
template <class C>
__global__ void __launch_bounds__(256) ecfft_twiddle_kernel(EcfftLadder<typename C::Fr> lad, FoldScalar* __restrict__ tw, uint32_t count) {
    using Fr = typename C::Fr;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    Fe<Fr> w;
    pow_from_table(w, lad.p, j, (int)ECFFT_MAX_LOG - 1);
    fe_from_mont(w, w);
    FoldScalar ks;
    ecfft_scalar<C>(ks, w);
    tw[j] = ks;
}

// acc = [ks] q on lazy limbs: q1 = +-q, q2 = +-phi(q) (already negated as ks asks); one joint chain, one addition site
template <class CK>
__device__ __forceinline__ void ecfft_chain(XYZZ<CK>& acc, const XYZZ<CK>& q1, const XYZZ<CK>& q2, const uint32_t (&k1)[8], const uint32_t (&k2)[8],
                                            int top_bit) {
    xyzz_set_inf(acc);
#pragma unroll 1
    for (int bit = top_bit; bit >= 0; bit--) {
        xyzz_dbl(acc);
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            const uint32_t word = h ? word_at<8>(k2, bit >> 5) : word_at<8>(k1, bit >> 5);
            if ((word >> (bit & 31)) & 1) {
                const XYZZ<CK> q = h ? q2 : q1;
                xyzz_add(acc, q);
            }
        }
    }
}

// r = [ks] b for a point of the workspace (saturated words in and out); the identity stays the identity
template <class C>
__device__ __forceinline__ void ecfft_mul(XYZZ<C>& r, const XYZZ<C>& b, const uint32_t (&k1)[8], const uint32_t (&k2)[8], int neg1, int neg2,
                                          int top_bit) {
    using CK = F29View<C>;
    if (xyzz_is_inf(b)) {
        xyzz_set_inf(r);
        return;
    }
    XYZZ<C> s1 = b, s2 = b;
    Coord<C> beta, ny;
    fe_from_words(beta, Glv<C>::BETA);
    fe_mul(s2.x, s2.x, beta);          // phi(x, y) = (beta x, y) in XYZZ: X' = beta X (unused when the scalar was not split: k2 = 0)
    fe_neg(ny, b.y);
    if (neg1) s1.y = ny;
    if (neg2) s2.y = ny;
    XYZZ<CK> q1, q2, acc;
    fe29_from_std(q1.x, s1.x);
    fe29_from_std(q1.y, s1.y);
    fe29_from_std(q1.zz, s1.zz);
    fe29_from_std(q1.zzz, s1.zzz);
    fe29_from_std(q2.x, s2.x);
    fe29_from_std(q2.y, s2.y);
    q2.zz = q1.zz;
    q2.zzz = q1.zzz;
    ecfft_chain<CK>(acc, q1, q2, k1, k2, top_bit);
    xyzz29_to_std<C>(r, acc);
}

// the host entry point's marshalling: Jacobian (X, Y, Z) -> XYZZ (X, Y, Z^2, Z^3), z = 0 -> the identity; and back from the affine
// result as (x, y, 1) or (0, 1, 0)
template <class C>
__global__ void __launch_bounds__(256) ecfft_jac_to_xyzz_kernel(const Jacobian<C>* __restrict__ in, XYZZ<C>* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Jacobian<C> j = in[i];
    XYZZ<C> r;
    if (fe_is_zero(j.z)) {
        xyzz_set_inf(r);
    } else {
        r.x = j.x;
        r.y = j.y;
        fe_sqr(r.zz, j.z);
        fe_mul(r.zzz, r.zz, j.z);
    }
    out[i] = r;
}
template <class C>
__global__ void __launch_bounds__(256) ecfft_affine_to_jac_kernel(const Affine<C>* __restrict__ in, Jacobian<C>* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<C> p = in[i];
    Jacobian<C> r;
    r.x = p.x;
    r.y = p.y;
    fe_one(r.z);
    if (aff_is_inf(p)) {
        fe_one(r.y);
        fe_zero(r.z);
    }
    out[i] = r;
}

// ws[i] = [ks] src[bitrev(i)] (scale != 0) or src[bitrev(i)]; ks is a kernel argument: wave-uniform
template <class C>
__global__ void __launch_bounds__(64) ecfft_load_kernel(const Affine<C>* __restrict__ src, XYZZ<C>* __restrict__ ws, uint32_t n, int logn,
                                                        FoldScalar ks, int scale) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<C> p = src[bitrev32(i, logn)];
    XYZZ<C> x, r;
    xyzz_from_affine(x, p);
    if (scale)
        ecfft_mul<C>(r, x, ks.k1, ks.k2, ks.neg1, ks.neg2, ks.top_bit);
    else
        r = x;
    ws[i] = r;
}

// stage s (m = 2^s) of the decimation-in-time transform over bit-reversed input, in place: for every block k of 2m points
// and j < m:  t = [w^(j n / 2m)] ws[k + j + m] ;  ws[k + j + m] = ws[k + j] - t ;  ws[k + j] += t.
// UNI: n / 2m >= 64 -- lane = block, wave = twiddle.  Otherwise lane = j inside consecutive blocks (coalesced), per-lane scalars.
template <class C, bool UNI>
__global__ void __launch_bounds__(64) ecfft_stage_kernel(XYZZ<C>* __restrict__ ws, const FoldScalar* __restrict__ tw, uint32_t half, int s, int logn) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= half) return;
    const int lb = logn - 1 - s;                    // log2 of the number of blocks
    uint32_t j, blk;
    if (UNI) {
        j = ZK_ECFFT_UNI(t >> lb);
        blk = t & ((1u << lb) - 1);
    } else {
        j = t & ((1u << s) - 1);
        blk = t >> s;
    }
    const uint64_t ia = ((uint64_t)blk << (s + 1)) + j, ib = ia + ((uint64_t)1 << s);
    XYZZ<C> tp = ws[ib];
    if (j != 0) {
        const FoldScalar* e = tw + ((uint64_t)j << lb);
        uint32_t k1[8], k2[8];
        int neg1, neg2, top;
        if (UNI) {
            for (int i = 0; i < 8; i++) {
                k1[i] = ZK_ECFFT_UNI(e->k1[i]);
                k2[i] = ZK_ECFFT_UNI(e->k2[i]);
            }
            neg1 = (int)ZK_ECFFT_UNI(e->neg1);
            neg2 = (int)ZK_ECFFT_UNI(e->neg2);
            top = (int)ZK_ECFFT_UNI(e->top_bit);
        } else {
            for (int i = 0; i < 8; i++) {
                k1[i] = e->k1[i];
                k2[i] = e->k2[i];
            }
            neg1 = e->neg1;
            neg2 = e->neg2;
            top = e->top_bit;
        }
        const XYZZ<C> b = tp;
        ecfft_mul<C>(tp, b, k1, k2, neg1, neg2, top);
    }
    const XYZZ<C> a = ws[ia];
#pragma unroll 1
    for (int h = 0; h < 2; h++) {                   // a + t, then a - t (one addition site)
        XYZZ<C> r = a;
        xyzz_add(r, tp);
        ws[h ? ib : ia] = r;
        Coord<C> ny;
        fe_neg(ny, tp.y);
        tp.y = ny;
    }
}

}  // namespace zk
