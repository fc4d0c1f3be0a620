// The optimal ate pairing on BN254 and BLS12-381 and the Groth16 verification equation (include/zkcp_amd_prover.h:
// zk_pairing_product, zk_groth16_verify) -- the tail of ark-groth16 0.3 verify_proof_with_prepared_inputs, reached by the
// reference's buyer at lib/src/zk/encryption.rs:152, sample_entries.rs:126, property.rs:177.  Host arithmetic only, on the
// 64-bit limb view of zk_host64.h: one verification is three Miller loops and one final exponentiation, a few thousand DEPENDENT
// Fq12 products -- latency-bound work with nothing to spread over lanes.
//
// Towers as in ark-bn254 / ark-bls12-381 0.3: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), with
// xi = 1 + u (BLS12-381, M-type twist y^2 = x^3 + 4 xi) or 9 + u (BN254, D-type twist y^2 = x^3 + 3 / xi).  An Fq12 value is
// stored as c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1: ark's Fp12 coefficient order, which is this file's struct layout.
//
// Defined value: e(P, Q) = f^((p^12 - 1) / r) with f the Miller function of the optimal ate pairing (f_{x,Q}(P), conjugated for
// the negative x of BLS12-381; f_{6x+2,Q}(P) and the two Frobenius lines on BN254).  The Miller loop is affine on the twist (one
// Fq2 inversion per step), vertical lines are left out and, on the M-type twist, every line is scaled by w^3: all of these
// factors lie in proper subfields of Fq12 and vanish in the final exponentiation, which is conj(f) / f (= f^(p^6 - 1)) followed
// by plain square-and-multiply over (p^6 + 1) / r.  Speed of this tail is not a target.
#include "zk_internal.h"
#include "zk_host64.h"
#include "zkcp_amd_prover.h"

using namespace zk;

namespace {

template <class Q>
struct Tower {
    using F = Fe<H64<Q>>;
    using F2 = Fe2<H64<Q>>;
    struct F6 {
        F2 c0, c1, c2;
    };
    struct F12 {
        F6 c0, c1;
    };
};

struct Bls381Pairing {
    using G1 = Bls381G1;
    using G2 = Bls381G2;
    using Fq = Bls381Fq;
    static constexpr int XI_C0 = 1;            // xi = 1 + u
    static constexpr bool M_TWIST = true;
    static constexpr bool BN = false;
    static constexpr bool NEGATIVE = true;     // x = -0xd201000000010000
    static constexpr uint64_t LOOP[2] = {0xd201000000010000ull, 0};
    static constexpr int FE_WORDS = 32;        // (p^6 + 1) / r
    static constexpr uint64_t FINAL_EXP[32] = {
        0x8739e1cdc0705d6aull, 0x09a5256de0381a16ull, 0x9cf0f70a61c791e2ull, 0x3a09c4497903f76eull, 0x2d7271563890f133ull, 0x224741b36fec7760ull,
        0x338259c22a12bd40ull, 0x38ee1cd4778e0de7ull, 0xc3b5ef4b188a20b0ull, 0x1d615d49e2764d7bull, 0x816101ddd076117dull, 0xf007c01e7ebe3afcull,
        0x27d7bd90935021c3ull, 0xc3b5e2f557c0b15full, 0x5e886c94c4f82384ull, 0xee6a95db11e63f56ull, 0x2b822f514a9c4f6full, 0x12d6a874d21b73daull,
        0x1304275ef499dffbull, 0x967878febcb95d1full, 0x4744497f8b2f2922ull, 0x85a2e707f0841855ull, 0x9f0c50126c802eecull, 0xfb46e197bd2fa489ull,
        0x548ce0809bc5f61aull, 0xcf56fb1573beaa8cull, 0xad7375a3763bdf7cull, 0xe0ec9031179bdeccull, 0x6579aea83c48c1daull, 0xdbf85ae664cf5bb3ull,
        0x7b6f235c55ca7566ull, 0x000028b314877503ull};
};
struct Bn254Pairing {
    using G1 = Bn254G1;
    using G2 = Bn254G2;
    using Fq = Bn254Fq;
    static constexpr int XI_C0 = 9;            // xi = 9 + u
    static constexpr bool M_TWIST = false;
    static constexpr bool BN = true;
    static constexpr bool NEGATIVE = false;
    static constexpr uint64_t LOOP[2] = {0x9d797039be763ba8ull, 1};   // 6 x + 2, x = 4965661367192848881
    static constexpr int FE_WORDS = 20;        // (p^6 + 1) / r
    static constexpr uint64_t FINAL_EXP[20] = {
        0x5250a54036e3f812ull, 0xa5635f1596789051ull, 0xd1138bf54d5bd1d4ull, 0xa8ce2533be36c7a2ull, 0x94f69f6b84e09bf6ull, 0x42ad1f5e50ef3644ull,
        0x0fcc420e48c3454cull, 0x758e4408ecc9952cull, 0xc901bf1887c6042cull, 0xa733cd65b14bb3b5ull, 0xdf6d76bdcf51b0d8ull, 0xca64c0fd82eb59e1ull,
        0x1d2e5726e39276a1ull, 0xc2d1ea74a391cae9ull, 0x07409206c82d647eull, 0x051c6d1aa5afdd17ull, 0xb37f601919667af5ull, 0x150e578c5084015bull,
        0xfbdea556c23998e4ull, 0x000fd14cc52f5b83ull};
};

template <class E>
struct Engine {
    using Q = typename E::Fq;
    using F = typename Tower<Q>::F;
    using F2 = typename Tower<Q>::F2;
    using F6 = typename Tower<Q>::F6;
    using F12 = typename Tower<Q>::F12;
    static constexpr size_t G1_BYTES = 2 * sizeof(F), G2_BYTES = 2 * sizeof(F2);
    static_assert(sizeof(F12) == 12 * sizeof(F), "twelve Fq coefficients, no padding");

    // ---- Fq2 helpers beyond zk_field.h
    static void mul_fq(F2& r, const F2& a, const F& s) {
        fe_mul(r.c0, a.c0, s);
        fe_mul(r.c1, a.c1, s);
    }
    static void conj2(F2& r, const F2& a) {
        r.c0 = a.c0;
        fe_neg(r.c1, a.c1);
    }
    static void mul_xi(F2& r, const F2& a) {   // (k + u)(a0 + a1 u) = (k a0 - a1) + (k a1 + a0) u
        F k0 = a.c0, k1 = a.c1, t;
        for (int i = 1; i < E::XI_C0; i++) {
            fe_add(k0, k0, a.c0);
            fe_add(k1, k1, a.c1);
        }
        fe_sub(t, k0, a.c1);
        fe_add(r.c1, k1, a.c0);
        r.c0 = t;
    }
    // ---- Fq6
    static void add6(F6& r, const F6& a, const F6& b) {
        fe_add(r.c0, a.c0, b.c0);
        fe_add(r.c1, a.c1, b.c1);
        fe_add(r.c2, a.c2, b.c2);
    }
    static void sub6(F6& r, const F6& a, const F6& b) {
        fe_sub(r.c0, a.c0, b.c0);
        fe_sub(r.c1, a.c1, b.c1);
        fe_sub(r.c2, a.c2, b.c2);
    }
    static void neg6(F6& r, const F6& a) {
        fe_neg(r.c0, a.c0);
        fe_neg(r.c1, a.c1);
        fe_neg(r.c2, a.c2);
    }
    static void mul6(F6& r, const F6& a, const F6& b) {
        F2 t00, t11, t22, t, s, o0, o1, o2;
        fe_mul(t00, a.c0, b.c0);
        fe_mul(t11, a.c1, b.c1);
        fe_mul(t22, a.c2, b.c2);
        fe_mul(t, a.c1, b.c2);      // c0 = a0 b0 + xi (a1 b2 + a2 b1)
        fe_mul(s, a.c2, b.c1);
        fe_add(t, t, s);
        mul_xi(t, t);
        fe_add(o0, t00, t);
        fe_mul(t, a.c0, b.c1);      // c1 = a0 b1 + a1 b0 + xi a2 b2
        fe_mul(s, a.c1, b.c0);
        fe_add(t, t, s);
        mul_xi(s, t22);
        fe_add(o1, t, s);
        fe_mul(t, a.c0, b.c2);      // c2 = a0 b2 + a1 b1 + a2 b0
        fe_mul(s, a.c2, b.c0);
        fe_add(t, t, s);
        fe_add(o2, t, t11);
        r.c0 = o0;
        r.c1 = o1;
        r.c2 = o2;
    }
    static void mul_v(F6& r, const F6& a) {    // (c0, c1, c2) v = (xi c2, c0, c1)
        F2 t;
        mul_xi(t, a.c2);
        r.c2 = a.c1;
        r.c1 = a.c0;
        r.c0 = t;
    }
    static void inv6(F6& r, const F6& a) {
        F2 A, B, C, t, s, f;
        fe_sqr(A, a.c0);            // A = c0^2 - xi c1 c2
        fe_mul(t, a.c1, a.c2);
        mul_xi(t, t);
        fe_sub(A, A, t);
        fe_sqr(B, a.c2);            // B = xi c2^2 - c0 c1
        mul_xi(B, B);
        fe_mul(t, a.c0, a.c1);
        fe_sub(B, B, t);
        fe_sqr(C, a.c1);            // C = c1^2 - c0 c2
        fe_mul(t, a.c0, a.c2);
        fe_sub(C, C, t);
        fe_mul(t, a.c2, B);         // f = c0 A + xi (c2 B + c1 C)
        fe_mul(s, a.c1, C);
        fe_add(t, t, s);
        mul_xi(t, t);
        fe_mul(f, a.c0, A);
        fe_add(f, f, t);
        fe_inv(f, f);
        fe_mul(r.c0, A, f);
        fe_mul(r.c1, B, f);
        fe_mul(r.c2, C, f);
    }
    // ---- Fq12
    static void one12(F12& r) {
        memset(&r, 0, sizeof r);
        fe_one(r.c0.c0.c0);
    }
    static bool eq12(const F12& a, const F12& b) { return memcmp(&a, &b, sizeof a) == 0; }   // reduced limbs: one representation
    static void mul12(F12& r, const F12& a, const F12& b) {
        F6 t0, t1, t2, t3;
        mul6(t0, a.c0, b.c0);
        mul6(t1, a.c1, b.c1);
        mul6(t2, a.c0, b.c1);
        mul6(t3, a.c1, b.c0);
        mul_v(t1, t1);
        add6(r.c0, t0, t1);
        add6(r.c1, t2, t3);
    }
    static void conj12(F12& r, const F12& a) {
        r.c0 = a.c0;
        neg6(r.c1, a.c1);
    }
    static void inv12(F12& r, const F12& a) {   // (c0 - c1 w) / (c0^2 - v c1^2)
        F6 t0, t1;
        mul6(t0, a.c0, a.c0);
        mul6(t1, a.c1, a.c1);
        mul_v(t1, t1);
        sub6(t0, t0, t1);
        inv6(t0, t0);
        mul6(r.c0, a.c0, t0);
        mul6(t1, a.c1, t0);
        neg6(r.c1, t1);
    }
    static void final_exp(F12& r, const F12& f) {
        F12 c, i, g, acc;
        conj12(c, f);
        inv12(i, f);
        mul12(g, c, i);                        // f^(p^6 - 1)
        one12(acc);
        for (int k = 64 * E::FE_WORDS - 1; k >= 0; k--) {
            mul12(acc, acc, acc);
            if ((E::FINAL_EXP[k / 64] >> (k % 64)) & 1) mul12(acc, acc, g);
        }
        r = acc;
    }

    // ---- the Miller loop, affine on the twist
    struct P1 {
        F x, y;
    };
    struct P2 {
        F2 x, y;
    };
    // f <- f * (the line of slope lam through t, at p): with c = lam x_T - y_T and d = -lam x_P,
    //   D-type: y_P + d w + c w^3;  M-type (times w^3): c + d w^2 + y_P w^3
    static void mul_line(F12& f, const F2& lam, const P2& t, const P1& p) {
        F12 l;
        memset(&l, 0, sizeof l);
        F2 c, d;
        fe_mul(c, lam, t.x);
        fe_sub(c, c, t.y);
        mul_fq(d, lam, p.x);
        fe_neg(d, d);
        if (E::M_TWIST) {
            l.c0.c0 = c;
            l.c0.c1 = d;
            l.c1.c1.c0 = p.y;
        } else {
            l.c0.c0.c0 = p.y;
            l.c1.c0 = d;
            l.c1.c1 = c;
        }
        mul12(f, f, l);
    }
    static void step_dbl(F12& f, P2& t, const P1& p) {
        F2 lam, n, d, x3, y3;
        fe_sqr(n, t.x);
        fe_dbl(d, n);
        fe_add(n, n, d);                       // 3 x^2
        fe_dbl(d, t.y);
        fe_inv(d, d);
        fe_mul(lam, n, d);
        mul_line(f, lam, t, p);
        fe_sqr(x3, lam);
        fe_sub(x3, x3, t.x);
        fe_sub(x3, x3, t.x);
        fe_sub(y3, t.x, x3);
        fe_mul(y3, y3, lam);
        fe_sub(y3, y3, t.y);
        t.x = x3;
        t.y = y3;
    }
    static void step_add(F12& f, P2& t, const P2& q, const P1& p, bool update) {
        F2 lam, n, d, x3, y3;
        fe_sub(n, q.y, t.y);
        fe_sub(d, q.x, t.x);
        fe_inv(d, d);
        fe_mul(lam, n, d);
        mul_line(f, lam, t, p);
        if (!update) return;
        fe_sqr(x3, lam);
        fe_sub(x3, x3, t.x);
        fe_sub(x3, x3, q.x);
        fe_sub(y3, t.x, x3);
        fe_mul(y3, y3, lam);
        fe_sub(y3, y3, t.y);
        t.x = x3;
        t.y = y3;
    }
    // a^e in Fq2 for e = (p - 1) / k
    static void pow_pm1_over(F2& r, const F2& a, unsigned k) {
        constexpr int N = Q::N / 2;
        uint64_t e[N];
        unsigned __int128 rem = 0;
        for (int i = N - 1; i >= 0; i--) {     // (p - 1) / k; p is odd, so p - 1 only clears the low bit
            const unsigned __int128 cur = (rem << 64) | (i == 0 ? Q::P64[0] - 1 : Q::P64[i]);
            e[i] = (uint64_t)(cur / k);
            rem = cur % k;
        }
        F2 acc;
        fe_one(acc);
        for (int i = 64 * N - 1; i >= 0; i--) {
            fe_sqr(acc, acc);
            if ((e[i / 64] >> (i % 64)) & 1) fe_mul(acc, acc, a);
        }
        r = acc;
    }
    // f <- f * (the Miller function at p, q); p, q affine, neither the identity, both in their r-torsion subgroups
    static void miller(F12& f_io, const P1& p, const P2& q) {
        F12 f;
        one12(f);
        P2 t = q;
        int top = 127;
        while (!((E::LOOP[top / 64] >> (top % 64)) & 1)) top--;
        for (int i = top - 1; i >= 0; i--) {
            mul12(f, f, f);
            step_dbl(f, t, p);
            if ((E::LOOP[i / 64] >> (i % 64)) & 1) step_add(f, t, q, p, true);
        }
        if (E::BN) {   // the lines through pi(Q) and -pi^2(Q): pi(x, y) = (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2)) on the D-type twist
            F2 xi, g2, g3;
            fe_zero(xi);
            fe_one(xi.c0);
            for (int i = 1; i < E::XI_C0; i++) {
                F o;
                fe_one(o);
                fe_add(xi.c0, xi.c0, o);
            }
            fe_one(xi.c1);
            pow_pm1_over(g2, xi, 3);
            pow_pm1_over(g3, xi, 2);
            P2 q1, q2;
            conj2(q1.x, q.x);
            fe_mul(q1.x, q1.x, g2);
            conj2(q1.y, q.y);
            fe_mul(q1.y, q1.y, g3);
            conj2(q2.x, q1.x);                 // pi twice, then the negation
            fe_mul(q2.x, q2.x, g2);
            conj2(q2.y, q1.y);
            fe_mul(q2.y, q2.y, g3);
            fe_neg(q2.y, q2.y);
            step_add(f, t, q1, p, true);
            step_add(f, t, q2, p, false);
        }
        if (E::NEGATIVE) conj12(f, f);
        mul12(f_io, f_io, f);
    }
    static bool is_zero_bytes(const void* p, size_t n) {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < n; i++)
            if (b[i]) return false;
        return true;
    }
    // prod_i miller(g1[i], +-g2[i]); a pair with the identity (all-zero bytes) in either slot contributes 1
    static void miller_product(F12& f, const void* const* g1, const void* const* g2, const int* negate_g2, int n) {
        one12(f);
        for (int i = 0; i < n; i++) {
            if (is_zero_bytes(g1[i], G1_BYTES) || is_zero_bytes(g2[i], G2_BYTES)) continue;
            P1 p;
            P2 q;
            memcpy(&p, g1[i], G1_BYTES);
            memcpy(&q, g2[i], G2_BYTES);
            if (negate_g2 && negate_g2[i]) fe_neg(q.y, q.y);
            miller(f, p, q);
        }
    }
    static int product(const void* g1, const void* g2, uint64_t n, void* gt_out) {
        std::vector<const void*> a(n), b(n);
        for (uint64_t i = 0; i < n; i++) {
            a[i] = (const unsigned char*)g1 + i * G1_BYTES;
            b[i] = (const unsigned char*)g2 + i * G2_BYTES;
        }
        F12 f, e;
        miller_product(f, a.data(), b.data(), nullptr, (int)n);
        final_exp(e, f);
        memcpy(gt_out, &e, sizeof e);
        return ZK_OK;
    }
    static int verify(const zk_groth16_vk_points* vk, const void* alpha_beta, const void* g_ic, const void* a, const void* b, const void* c, uint64_t* ok) {
        F12 rhs, f, lhs;
        if (alpha_beta) {
            memcpy(&rhs, alpha_beta, sizeof rhs);
        } else {
            const void* p1[1] = {vk->alpha_g1};
            const void* p2[1] = {vk->beta_g2};
            miller_product(f, p1, p2, nullptr, 1);
            final_exp(rhs, f);
        }
        const void* p1[3] = {a, g_ic, c};
        const void* p2[3] = {b, vk->gamma_g2, vk->delta_g2};
        const int neg[3] = {0, 1, 1};
        miller_product(f, p1, p2, neg, 3);
        final_exp(lhs, f);
        *ok = eq12(lhs, rhs) ? 1 : 0;
        return ZK_OK;
    }
};

}  // namespace

extern "C" {
#define API __attribute__((visibility("default")))

API int zk_pairing_product(zk_pairing_t p, const void* g1_affine, const void* g2_affine, uint64_t n, void* gt_out) {
    if (!gt_out || (n && (!g1_affine || !g2_affine)) || n > (1u << 20)) return ZK_ERR_INVALID_ARG;
    if (p == ZK_PAIRING_BN254) return Engine<Bn254Pairing>::product(g1_affine, g2_affine, n, gt_out);
    if (p == ZK_PAIRING_BLS12_381) return Engine<Bls381Pairing>::product(g1_affine, g2_affine, n, gt_out);
    return ZK_ERR_INVALID_ARG;
}

API int zk_groth16_verify(zk_pairing_t p, const zk_groth16_vk_points* vk, const void* alpha_g1_beta_g2, const void* prepared_inputs_g1,
                          const void* a_g1, const void* b_g2, const void* c_g1, uint64_t* ok) {
    if (!vk || !vk->alpha_g1 || !vk->beta_g2 || !vk->gamma_g2 || !vk->delta_g2 || !prepared_inputs_g1 || !a_g1 || !b_g2 || !c_g1 || !ok)
        return ZK_ERR_INVALID_ARG;
    *ok = 0;
    if (p == ZK_PAIRING_BN254) return Engine<Bn254Pairing>::verify(vk, alpha_g1_beta_g2, prepared_inputs_g1, a_g1, b_g2, c_g1, ok);
    if (p == ZK_PAIRING_BLS12_381) return Engine<Bls381Pairing>::verify(vk, alpha_g1_beta_g2, prepared_inputs_g1, a_g1, b_g2, c_g1, ok);
    return ZK_ERR_INVALID_ARG;
}

}  // extern "C"
