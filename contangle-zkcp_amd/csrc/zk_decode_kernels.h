// Checked decode of ark-serialize 0.3 points on the device: GroupAffine::deserialize (compressed) and the checked
// deserialize_uncompressed of ark-ec 0.3 for the G1 groups of BN254 and BLS12-381 -- what the reference's read_verifying_key
// (lib/src/utils.rs:112-118) runs over gamma_abc_g1, 2 + n points with the whole ciphertext public (196 611 points of BLS12-381
// G1 in the reference's own test).
//   upstream: Vec<T>::deserialize, one element after another: Fq::deserialize_with_flags, get_point_from_x (a square root in Fq),
//             is_in_correct_subgroup_assuming_on_curve (a multiplication by r)
//   here:     points_decode_checked_kernel, one lane per point: both exponents are constants, so every lane of a wave runs the
//             same ~N*32 squarings / doublings with the same multiply / add pattern -- no divergence among valid points
// All arithmetic goes through zk_field.h / zk_curve.h.  A lane that rejects its point reports (index << 3 | reason) with one
// atomicMin on a device word; nothing is indexed with data read from the input, so a bad input cannot fault.
#pragma once
#include "zk_rt.h"
#include "zk_curve.h"

namespace zk {

constexpr int DECODE_NONCANONICAL = 1;      // a coordinate >= p
constexpr int DECODE_FLAGS = 2;             // both SWFlags bits set
constexpr int DECODE_NOT_ON_CURVE = 3;      // x^3 + b is a non-residue / y^2 != x^3 + b
constexpr int DECODE_NOT_IN_SUBGROUP = 4;   // [r] P != O
constexpr unsigned long long DECODE_NONE = ~0ull;

#if defined(ZK_EMU)
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) {
    const unsigned long long o = *p;
    if (v < o) *p = v;
    return o;
}
#endif

// the curves with an arkworks wire format whose base field is 3 mod 4 and whose points sit in Fq
template <class C>
struct ArkG1 {
    static constexpr bool HAS = false;
};
template <>
struct ArkG1<Bn254G1> {
    static constexpr bool HAS = true;
};
template <>
struct ArkG1<Bls381G1> {
    static constexpr bool HAS = true;
};

// the two fixed exponents, little-endian words; a kernel argument, so the bit tests are scalar loads
template <class C>
struct DecodeConsts {
    uint32_t sqrt_exp[C::Fq::N];   // (p + 1) / 4
    uint32_t order[C::Fr::N];      // r
};

// one coordinate: P::N little-endian words (32 / 48 bytes -- the encoded length is exactly the limb array for both fields), the
// two flag bits in the top of the last word when with_flags.  -> false when the value is not canonical; r = the Montgomery form
template <class P>
ZK_HD bool decode_coord(Fe<P>& r, const uint32_t* w, bool with_flags, uint32_t* flags) {
    static_assert((P::BITS + 2 + 7) / 8 == 4 * P::N, "the wire length of a coordinate is its limb array");
    Fe<P> t;
    ZK_UNROLL
    for (int i = 0; i < P::N; i++) t.v[i] = w[i];
    if (with_flags) {
        *flags = t.v[P::N - 1] >> 30;      // bit 1 = y is the larger of (y, -y), bit 0 = infinity
        t.v[P::N - 1] &= 0x3fffffffu;
    }
    uint64_t br = 0;
    ZK_UNROLL
    for (int i = 0; i < P::N; i++) br = (((uint64_t)t.v[i] - P::P[i] - br) >> 32) & 1;
    fe_to_mont(r, t);
    return br != 0;                        // t - p borrows: t < p
}

// ark-ff's Ord on Fp (canonical integers): y > -y
template <class P>
ZK_HD bool decode_larger_than_neg(const Fe<P>& y) {
    Fe<P> ny, a, b;
    fe_neg(ny, y);
    fe_from_mont(a, y);
    fe_from_mont(b, ny);
    bool gt = false, decided = false;
    ZK_UNROLL
    for (int i = P::N - 1; i >= 0; i--) {
        const bool ne = a.v[i] != b.v[i];
        gt = (!decided && ne) ? a.v[i] > b.v[i] : gt;
        decided = decided || ne;
    }
    return gt;
}

// in: n points of pw = N (compressed) or 2 N words; out[i] = the affine Montgomery point ((0, 0) for the infinity flag), left
// alone for a rejected point; *bad = min over the rejected points of (i << 3 | reason)
template <class C>
__global__ void __launch_bounds__(256) points_decode_checked_kernel(const uint32_t* __restrict__ in, uint64_t n, int compressed,
                                                                    Affine<C>* __restrict__ out, unsigned long long* __restrict__ bad,
                                                                    DecodeConsts<C> k) {
    using Fq = typename C::Fq;
    constexpr int N = Fq::N;
    const uint64_t pw = compressed ? N : 2 * N;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t* w = in + i * pw;
        Affine<C> p;
        uint32_t flags = 0;
        int reason = 0;
        bool canon = decode_coord<Fq>(p.x, w, compressed != 0, &flags);
        if (!compressed) canon = decode_coord<Fq>(p.y, w + N, true, &flags) && canon;
        if (!canon) {
            reason = DECODE_NONCANONICAL;
        } else if (flags == 3) {
            reason = DECODE_FLAGS;
        } else if (flags & 1) {
            fe_zero(p.x);
            fe_zero(p.y);
        } else {
            Fe<Fq> rhs, b, t;
            fe_sqr(rhs, p.x);
            fe_mul(rhs, rhs, p.x);
            fe_from_words(b, C::B);
            fe_add(rhs, rhs, b);
            if (compressed) {
                Fe<Fq> y;      // rhs^((p + 1) / 4), most significant bit first (the exponent's top word is not zero)
                fe_one(y);
                for (int j = 32 * N - 1; j >= 0; j--) {
                    fe_sqr(y, y);
                    if ((k.sqrt_exp[j >> 5] >> (j & 31)) & 1u) fe_mul(y, y, rhs);
                }
                fe_sqr(t, y);
                if (!fe_eq(t, rhs)) reason = DECODE_NOT_ON_CURVE;
                Fe<Fq> ny;
                fe_neg(ny, y);
                fe_cmov(y, ny, decode_larger_than_neg(y) != ((flags & 2) != 0));
                p.y = y;
            } else {
                fe_sqr(t, p.y);
                if (!fe_eq(t, rhs)) reason = DECODE_NOT_ON_CURVE;
            }
            if (!reason) {     // [r] P, plain double-and-add from the top bit of r
                XYZZ<C> acc;
                xyzz_set_inf(acc);
                for (int j = 32 * C::Fr::N - 1; j >= 0; j--) {
                    xyzz_dbl(acc);
                    if ((k.order[j >> 5] >> (j & 31)) & 1u) xyzz_add_mixed(acc, p);
                }
                if (!xyzz_is_inf(acc)) reason = DECODE_NOT_IN_SUBGROUP;
            }
        }
        if (reason)
            atomicMin(bad, (unsigned long long)(i << 3) | (unsigned long long)reason);
        else
            out[i] = p;
    }
}

}  // namespace zk
