// TEST INFRASTRUCTURE: one op table for the field and curve primitives (zk_field.h, zk_field29.h, zk_curve.h, zk_curve29.h),
// shared by the host runner (f29_check.cc, g++) and the device probe (field_probe.hip, hipcc for gfx950), so that the two
// op lists cannot drift.  Every op is a call on rows of u32 words:  op(a[na], b[nb]) -> out[no];  the word counts are
// functions of the target (L = lazy limbs, N = 32-bit words, CW = words of one curve coordinate, CL = lazy limbs of one).
// Compiles as host C++ and as HIP device code; nothing here is part of the product.
#pragma once
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "zk_curve29.h"

namespace zkt {
using namespace zk;

struct Shape {
    int na, nb, no;
    bool ok;
};

template <class P>
constexpr bool has_fq2() {   // the base fields of the G2 twists: Fe2 / Fe29x2 are used over these only
    return std::is_same<P, Bn254Fq>::value || std::is_same<P, Bls381Fq>::value;
}

// ------------------------------------------------------------------------------------------------------------------
// fields.  X(name, words of a, words of b, words of out, available for this field)
// The lazy ops keep the protocol tests/test_f29.py has always used: L limbs of a, L limbs of b (2 L each for the Fq2 ops).
// ------------------------------------------------------------------------------------------------------------------
#define ZK_FIELD_OPS(X)                   \
    X(mul, L, L, L, true)                 \
    X(sqr, L, L, L, true)                 \
    X(mulacc, L, L, L, true)              \
    X(sub4k1, L, L, L, true)              \
    X(sub16k2, L, L, L, true)             \
    X(sub3, L, L, L, true)                \
    X(sub2x, L, L, L, true)               \
    X(norm, L, L, L, true)                \
    X(carry, L, L, L, true)               \
    X(canon, L, L, L, true)               \
    X(tostd, L, L, N, true)               \
    X(fromstd, L, L, L, true)             \
    X(filter, L, L, 3, true)              \
    X(unpack, N, 1, L, true)              \
    X(pack, L, 1, N, true)                \
    X(slots4, 4 * L, 4, 4 * L, true)      \
    X(x2mul4k1, 2 * L, 2 * L, 2 * L, Q2)  \
    X(x2mul8k2, 2 * L, 2 * L, 2 * L, Q2)  \
    X(x2mul16k2, 2 * L, 2 * L, 2 * L, Q2) \
    X(x2sqr8k2, 2 * L, 2 * L, 2 * L, Q2)  \
    X(x2sqr16k2, 2 * L, 2 * L, 2 * L, Q2) \
    X(x2refresh, 2 * L, 2 * L, 2 * L, Q2) \
    X(x2iszero, 2 * L, 2 * L, 1, Q2)      \
    X(fe_add, N, N, N, true)              \
    X(fe_sub, N, N, N, true)              \
    X(fe_neg, N, N, N, true)              \
    X(fe_dbl, N, N, N, true)              \
    X(fe_mul, N, N, N, true)              \
    X(fe_mul_portable, N, N, N, true)     \
    X(fe_sqr, N, N, N, true)              \
    X(fe_to_mont, N, N, N, true)          \
    X(fe_from_mont, N, N, N, true)        \
    X(fe_mul_call, N, N, N, true)         \
    X(fe2_mul, 2 * N, 2 * N, 2 * N, Q2)   \
    X(fe2_sqr, 2 * N, 2 * N, 2 * N, Q2)

enum FieldOp {
#define X(n, A, B, O, av) F_##n,
    ZK_FIELD_OPS(X)
#undef X
        F_COUNT
};

inline const char* field_op_name(int op) {
    switch (op) {
#define X(n, A, B, O, av) \
    case F_##n: return #n;
        ZK_FIELD_OPS(X)
#undef X
    }
    return nullptr;
}

template <class P>
constexpr Shape field_shape(int op) {
    constexpr int L = F29<P>::L, N = P::N;
    constexpr bool Q2 = has_fq2<P>();
    switch (op) {
#define X(n, A, B, O, av) \
    case F_##n: return Shape{A, B, O, av};
        ZK_FIELD_OPS(X)
#undef X
    }
    return Shape{0, 0, 0, false};
}

// calls f(std::integral_constant<int, OP>) for the op if the field has it
template <class P, class Fn>
inline bool field_dispatch(int op, Fn&& f) {
    constexpr bool Q2 = has_fq2<P>();
    (void)Q2;
    switch (op) {
#define X(n, A, B, O, av)                                 \
    case F_##n:                                           \
        if constexpr (av) {                               \
            f(std::integral_constant<int, F_##n>{});      \
            return true;                                  \
        } else                                            \
            return false;
        ZK_FIELD_OPS(X)
#undef X
    }
    return false;
}

template <class P>
ZK_HD void ld29(Fe29<P>& r, const uint32_t* w) {
    ZK_UNROLL
    for (int i = 0; i < F29<P>::L; i++) r.v[i] = w[i];
}
template <class P>
ZK_HD void st29(uint32_t* w, const Fe29<P>& r) {
    ZK_UNROLL
    for (int i = 0; i < F29<P>::L; i++) w[i] = r.v[i];
}
template <class P>
ZK_HD void ld29(Fe29x2<P>& r, const uint32_t* w) {
    ld29(r.c0, w);
    ld29(r.c1, w + F29<P>::L);
}
template <class P>
ZK_HD void st29(uint32_t* w, const Fe29x2<P>& r) {
    st29(w, r.c0);
    st29(w + F29<P>::L, r.c1);
}
template <class P>
ZK_HD void fe_to_words(uint32_t* w, const Fe<P>& r) {
    ZK_UNROLL
    for (int i = 0; i < P::N; i++) w[i] = r.v[i];
}
template <class P>
ZK_HD void fe_to_words(uint32_t* w, const Fe2<P>& r) {
    fe_to_words(w, r.c0);
    fe_to_words(w + P::N, r.c1);
}

template <class P, int OP>
ZK_HD void field_op(const uint32_t* a, const uint32_t* b, uint32_t* o) {
    using K = F29<P>;
    constexpr int L = K::L;
    if constexpr (OP >= F_x2mul4k1 && OP <= F_x2iszero) {
        Fe29x2<P> x, y, r;
        ld29(x, a);
        ld29(y, b);
        if constexpr (OP == F_x2iszero) {
            o[0] = (uint32_t)fe29_is_zero_mod_p(x, b[0], b[1]);
            return;
        }
        if constexpr (OP == F_x2mul4k1) fe29_mul(r, x, y, K::BIAS4K1);
        if constexpr (OP == F_x2mul8k2) fe29_mul(r, x, y, K::BIAS8K2);
        if constexpr (OP == F_x2mul16k2) fe29_mul(r, x, y, K::BIAS16K2);
        if constexpr (OP == F_x2sqr8k2) fe29_sqr(r, x, K::BIAS8K2);
        if constexpr (OP == F_x2sqr16k2) fe29_sqr(r, x, K::BIAS16K2);
        if constexpr (OP == F_x2refresh) fe29_refresh(r, x);
        st29(o, r);
    } else if constexpr (OP >= F_fe_add && OP <= F_fe_mul_call) {
        Fe<P> x, y, r;
        fe_from_words(x, a);
        fe_from_words(y, b);
        if constexpr (OP == F_fe_add) fe_add(r, x, y);
        if constexpr (OP == F_fe_sub) fe_sub(r, x, y);
        if constexpr (OP == F_fe_neg) fe_neg(r, x);
        if constexpr (OP == F_fe_dbl) fe_dbl(r, x);
        if constexpr (OP == F_fe_mul) fe_mul(r, x, y);   // the generated assembly on the device, the portable product on the host
        if constexpr (OP == F_fe_mul_portable) fe_mul_portable(r, x, y);
        if constexpr (OP == F_fe_sqr) fe_sqr(r, x);
        if constexpr (OP == F_fe_to_mont) fe_to_mont(r, x);
        if constexpr (OP == F_fe_from_mont) fe_from_mont(r, x);
        if constexpr (OP == F_fe_mul_call) r = fe_mul_call(x, y);
        fe_to_words(o, r);
    } else if constexpr (OP == F_fe2_mul || OP == F_fe2_sqr) {
        Fe2<P> x, y, r;
        fe_from_words(x, a);
        fe_from_words(y, b);
        if constexpr (OP == F_fe2_mul) fe_mul(r, x, y);
        if constexpr (OP == F_fe2_sqr) fe_sqr(r, x);
        fe_to_words(o, r);
    } else if constexpr (OP == F_unpack) {
        Fe<P> s;
        Fe29<P> r;
        fe_from_words(s, a);
        fe29_unpack(r, s);
        st29(o, r);
    } else if constexpr (OP == F_pack) {
        Fe<P> s;
        Fe29<P> x;
        ld29(x, a);
        fe29_pack(s, x);
        fe_to_words(o, s);
    } else if constexpr (OP == F_slots4) {
        // the shape of profiles/r03_b_expr29_slots.txt: four named register sets selected by an if-chain on a wave-uniform
        // slot number, each loaded from a different operand (a[step]) into slot b[step], then products of the slots
        Fe29<P> c0, c1, c2, c3, r;
        fe29_zero(c0);
        fe29_zero(c1);
        fe29_zero(c2);
        fe29_zero(c3);
        for (int step = 0; step < 4; step++) {
            uint32_t slot = b[step];
#if defined(__HIP_DEVICE_COMPILE__)
            slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
#endif
            Fe29<P> x;
            ld29(x, a + step * L);
            if (slot == 0) c0 = x;
            else if (slot == 1) c1 = x;
            else if (slot == 2) c2 = x;
            else c3 = x;
        }
        fe29_mul(r, c0, c1);
        st29(o, r);
        fe29_mul(r, c2, c3);
        st29(o + L, r);
        st29(o + 2 * L, c2);
        st29(o + 3 * L, c3);
    } else {
        Fe29<P> x, y, r;
        ld29(x, a);
        ld29(y, b);
        if constexpr (OP == F_tostd) {
            Fe<P> s;
            fe29_to_std(s, x);
            fe_to_words(o, s);
            return;
        }
        if constexpr (OP == F_filter) {
            uint32_t k = 0;
            const bool f = fe29_zero_filter(x, b[0], b[1], k);
            o[0] = (uint32_t)f;
            o[1] = k;
            o[2] = (uint32_t)(f && fe29_is_kp(x, k));
            return;
        }
        if constexpr (OP == F_mul) fe29_mul(r, x, y);
        if constexpr (OP == F_sqr) fe29_sqr(r, x);
        if constexpr (OP == F_mulacc) {   // a b + c d with c = b >> 1, d = a >> 1 limb-wise (distinct operands from two vectors)
            Fe29<P> c, d;
            ZK_UNROLL
            for (int i = 0; i < L; i++) c.v[i] = y.v[i] >> 1, d.v[i] = x.v[i] >> 1;
            fe29_mulacc(r, x, y, c, d);
        }
        if constexpr (OP == F_sub4k1) fe29_sub(r, x, y, K::BIAS4K1);
        if constexpr (OP == F_sub16k2) fe29_sub(r, x, y, K::BIAS16K2);
        if constexpr (OP == F_sub3) fe29_sub3(r, x, y, y);
        if constexpr (OP == F_sub2x) fe29_sub2x(r, x, y);
        if constexpr (OP == F_norm) fe29_norm(r, x);
        if constexpr (OP == F_carry) fe29_carry(r, x);
        if constexpr (OP == F_canon) fe29_canon(r, x);
        if constexpr (OP == F_fromstd) {
            Fe<P> s;
            fe_from_words(s, a);
            fe29_from_std(r, s);
        }
        st29(o, r);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// curves.  A target is a curve seen through one form: the saturated limbs of zk_curve.h (C itself) or the lazy view
// F29View<C> of zk_curve29.h (C29 for G1, C29x2 for the G2 twists).  Operands and results cross the boundary as the caller's
// standard-form words (Montgomery, R = 2^(32 N)): the lazy forms convert with fe29_from_std on the way in and with
// xyzz29_to_std / fe29_to_std on the way out.  Every XYZZ result is followed by one word: xyzz_is_inf() of the result in
// the form under test (the literal encoding), xyzz_add_nodbl by a second one: its "needs doubling" return.
// ------------------------------------------------------------------------------------------------------------------
template <class CC>
struct StdOf {
    using type = CC;
};
template <class C>
struct StdOf<C29<C>> {
    using type = C;
};
template <class C>
struct StdOf<C29x2<C>> {
    using type = C;
};
template <class CC>
constexpr bool is_lazy() {
    return CC::EXT >= 29;
}

#define ZK_CURVE_OPS(X)                                   \
    X(xyzz_add_mixed, 4 * CW, 2 * CW, 4 * CW + 1, true)   \
    X(xyzz_dbl, 4 * CW, 1, 4 * CW + 1, true)              \
    X(xyzz_dbl_affine, 2 * CW, 1, 4 * CW + 1, true)       \
    X(xyzz_add, 4 * CW, 4 * CW, 4 * CW + 1, true)         \
    X(xyzz_add_nodbl, 4 * CW, 4 * CW, 4 * CW + 2, true)   \
    X(aff_neg_if, 2 * CW, 1, 2 * CW + 1, true)            \
    X(xyzz29_to_std, 4 * CL, 1, 4 * CW + 1, LAZY)

enum CurveOp {
#define X(n, A, B, O, av) C_##n,
    ZK_CURVE_OPS(X)
#undef X
        C_COUNT
};

inline const char* curve_op_name(int op) {
    switch (op) {
#define X(n, A, B, O, av) \
    case C_##n: return #n;
        ZK_CURVE_OPS(X)
#undef X
    }
    return nullptr;
}

template <class CC>
constexpr Shape curve_shape(int op) {
    using S = typename StdOf<CC>::type;
    constexpr int CW = S::EXT * S::Fq::N, CL = S::EXT * F29<typename S::Fq>::L;
    constexpr bool LAZY = is_lazy<CC>();
    switch (op) {
#define X(n, A, B, O, av) \
    case C_##n: return Shape{A, B, O, av};
        ZK_CURVE_OPS(X)
#undef X
    }
    return Shape{0, 0, 0, false};
}

template <class CC, class Fn>
inline bool curve_dispatch(int op, Fn&& f) {
    constexpr bool LAZY = is_lazy<CC>();
    (void)LAZY;
    switch (op) {
#define X(n, A, B, O, av)                                 \
    case C_##n:                                           \
        if constexpr (av) {                               \
            f(std::integral_constant<int, C_##n>{});      \
            return true;                                  \
        } else                                            \
            return false;
        ZK_CURVE_OPS(X)
#undef X
    }
    return false;
}

template <class CC>
ZK_HD void ld_coord(Coord<CC>& r, const uint32_t* w) {
    if constexpr (is_lazy<CC>()) {
        Coord<typename StdOf<CC>::type> s;
        fe_from_words(s, w);
        fe29_from_std(r, s);
    } else {
        fe_from_words(r, w);
    }
}
template <class CC>
ZK_HD void st_coord(uint32_t* w, const Coord<CC>& r) {
    if constexpr (is_lazy<CC>()) {
        Coord<typename StdOf<CC>::type> s;
        fe29_to_std(s, r);
        fe_to_words(w, s);
    } else {
        fe_to_words(w, r);
    }
}
template <class CC>
ZK_HD void ld_xyzz(XYZZ<CC>& p, const uint32_t* w) {
    constexpr int CW = curve_shape<CC>(C_xyzz_dbl).na / 4;
    ld_coord<CC>(p.x, w);
    ld_coord<CC>(p.y, w + CW);
    ld_coord<CC>(p.zz, w + 2 * CW);
    ld_coord<CC>(p.zzz, w + 3 * CW);
}
template <class CC>
ZK_HD void ld_aff(Affine<CC>& p, const uint32_t* w) {
    constexpr int CW = curve_shape<CC>(C_xyzz_dbl).na / 4;
    ld_coord<CC>(p.x, w);
    ld_coord<CC>(p.y, w + CW);
}
// XYZZ result + the literal-infinity word
template <class CC>
ZK_HD void st_xyzz(uint32_t* w, const XYZZ<CC>& p) {
    using S = typename StdOf<CC>::type;
    constexpr int CW = curve_shape<CC>(C_xyzz_dbl).na / 4;
    XYZZ<S> s;
    if constexpr (is_lazy<CC>()) {
        xyzz29_to_std(s, p);
    } else {
        s = p;
    }
    fe_to_words(w, s.x);
    fe_to_words(w + CW, s.y);
    fe_to_words(w + 2 * CW, s.zz);
    fe_to_words(w + 3 * CW, s.zzz);
    w[4 * CW] = (uint32_t)xyzz_is_inf(p);
}

template <class CC, int OP>
ZK_HD void curve_op(const uint32_t* a, const uint32_t* b, uint32_t* o) {
    constexpr int CW = curve_shape<CC>(C_xyzz_dbl).na / 4;
    if constexpr (OP == C_xyzz_add_mixed) {
        XYZZ<CC> acc;
        Affine<CC> q;
        ld_xyzz<CC>(acc, a);
        ld_aff<CC>(q, b);
        xyzz_add_mixed(acc, q);
        st_xyzz<CC>(o, acc);
    } else if constexpr (OP == C_xyzz_dbl) {
        XYZZ<CC> acc;
        ld_xyzz<CC>(acc, a);
        xyzz_dbl(acc);
        st_xyzz<CC>(o, acc);
    } else if constexpr (OP == C_xyzz_dbl_affine) {
        XYZZ<CC> acc;
        Affine<CC> q;
        ld_aff<CC>(q, a);
        xyzz_dbl_affine(acc, q);
        st_xyzz<CC>(o, acc);
    } else if constexpr (OP == C_xyzz_add) {
        XYZZ<CC> acc, q;
        ld_xyzz<CC>(acc, a);
        ld_xyzz<CC>(q, b);
        xyzz_add(acc, q);
        st_xyzz<CC>(o, acc);
    } else if constexpr (OP == C_xyzz_add_nodbl) {
        XYZZ<CC> acc, q;
        ld_xyzz<CC>(acc, a);
        ld_xyzz<CC>(q, b);
        const bool dbl = xyzz_add_nodbl(acc, q);
        st_xyzz<CC>(o, acc);
        o[4 * CW + 1] = (uint32_t)dbl;
    } else if constexpr (OP == C_aff_neg_if) {
        Affine<CC> q;
        ld_aff<CC>(q, a);
        aff_neg_if(q, b[0] != 0);
        st_coord<CC>(o, q.x);
        st_coord<CC>(o + CW, q.y);
        o[2 * CW] = (uint32_t)aff_is_inf(q);
    } else if constexpr (OP == C_xyzz29_to_std) {
        // lazy limbs in (strict or spread), standard words out: the conversion of the MSM partial sums
        constexpr int CL = curve_shape<CC>(C_xyzz29_to_std).na / 4;
        XYZZ<CC> p;
        ld29(p.x, a);
        ld29(p.y, a + CL);
        ld29(p.zz, a + 2 * CL);
        ld29(p.zzz, a + 3 * CL);
        st_xyzz<CC>(o, p);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// targets: ids and names, in the order of oracle/pyref.py FIELD_IDS / CURVE_IDS.  Field i has id i; curve i has id
// 100 + 2 i in the saturated form and 101 + 2 i in the lazy one (name + "29").
// ------------------------------------------------------------------------------------------------------------------
#define ZK_PROBE_FIELDS(X) X(0, PallasFp) X(1, PallasFq) X(2, Bn254Fr) X(3, Bls381Fr) X(4, Bn254Fq) X(5, Bls381Fq)
#define ZK_PROBE_CURVES(X) X(0, Pallas) X(1, Vesta) X(2, Bn254G1) X(3, Bls381G1) X(4, Bn254G2) X(5, Bls381G2)
constexpr int CURVE_TARGET0 = 100;
template <int I>
struct FieldAt;
template <int I>
struct CurveAt;
#define X(i, P)           \
    template <>           \
    struct FieldAt<i> {   \
        using type = P;   \
    };
ZK_PROBE_FIELDS(X)
#undef X
#define X(i, C)           \
    template <>           \
    struct CurveAt<i> {   \
        using type = C;   \
    };
ZK_PROBE_CURVES(X)
#undef X

}  // namespace zkt
