// TEST INFRASTRUCTURE: the device probe of the field and curve primitives.  The op table of field_ops.h, compiled by hipcc for
// gfx950 with the flags of the product units, one kernel per (target, op), one case per lane.  Built by build_probe() in
// contangle-zkcp_amd/build.py into tests/emu/libzk_field_probe.so: this file is compiled once per field
// (-DZK_PROBE_FIELD=<i>), once per curve and form (-DZK_PROBE_CURVE=<i> -DZK_PROBE_FORM=<0|1>) and once without either for the
// entry point.  tests/test_field_probe_gpu.py drives it; nothing here is part of the product.
//
//   int zk_probe_run(int target, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int nlanes, int mode)
//     a, b, out: host arrays of nlanes rows (na, nb, no words per row: zk_probe_shape).  `out` is copied to the device before
//     the launch and back after it, so the rows of inactive lanes come back as the caller filled them.
//     mode 0: every lane runs its row;  1: odd lanes only (static divergent EXEC);  2: one lane per 64-lane workgroup,
//     lane (5 blk + 1) mod 64, chosen behind a __syncthreads() by a flag read from LDS (the shape of msm_axis_weighted_kernel).
//     Returns 0, a hipError_t (> 0) of the first failing HIP call, -1 for an unknown target, -2 for an unknown op.
#include <hip/hip_runtime.h>

#include "field_ops.h"

using namespace zkt;

constexpr int PROBE_BLOCK = 64;

typedef int (*unit_fn)(int, const uint32_t*, const uint32_t*, uint32_t*, int, int);

#if defined(ZK_PROBE_FIELD) || defined(ZK_PROBE_CURVE)

template <class T, int OP, bool CURVE>
__global__ void __launch_bounds__(PROBE_BLOCK) probe_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                            uint32_t* __restrict__ out, int nlanes, int mode) {
    __shared__ uint32_t flag[PROBE_BLOCK];
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x * PROBE_BLOCK + tid;
    flag[tid] = (mode != 2 || tid == (int)((blockIdx.x * 5u + 1u) % PROBE_BLOCK)) ? 1u : 0u;
    __syncthreads();
    bool active = row < nlanes && flag[tid] != 0;
    if (mode == 1) active = active && (tid & 1);
    if (!active) return;
    if constexpr (CURVE) {
        constexpr Shape s = curve_shape<T>(OP);
        curve_op<T, OP>(a + row * s.na, b + row * s.nb, out + row * s.no);
    } else {
        constexpr Shape s = field_shape<T>(OP);
        field_op<T, OP>(a + row * s.na, b + row * s.nb, out + row * s.no);
    }
}

#define PROBE_HIP(call)                    \
    do {                                   \
        if (err == hipSuccess) err = call; \
    } while (0)

template <class T, int OP, bool CURVE>
static int launch(const Shape& s, const uint32_t* a, const uint32_t* b, uint32_t* out, int nlanes, int mode) {
    uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
    const size_t n = (size_t)nlanes;
    hipError_t err = hipSuccess;
    PROBE_HIP(hipMalloc((void**)&da, n * s.na * 4));
    PROBE_HIP(hipMalloc((void**)&db, n * s.nb * 4));
    PROBE_HIP(hipMalloc((void**)&dout, n * s.no * 4));
    PROBE_HIP(hipMemcpy(da, a, n * s.na * 4, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(db, b, n * s.nb * 4, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(dout, out, n * s.no * 4, hipMemcpyHostToDevice));
    if (err == hipSuccess) {
        const unsigned grid = (unsigned)((n + PROBE_BLOCK - 1) / PROBE_BLOCK);
        hipLaunchKernelGGL((probe_kernel<T, OP, CURVE>), dim3(grid), dim3(PROBE_BLOCK), 0, 0, da, db, dout, nlanes, mode);
        err = hipGetLastError();
    }
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(out, dout, n * s.no * 4, hipMemcpyDeviceToHost));
    // after an error nothing more is launched; the frees are attempted only on a healthy device
    if (err == hipSuccess) {
        PROBE_HIP(hipFree(da));
        PROBE_HIP(hipFree(db));
        PROBE_HIP(hipFree(dout));
    }
    return (int)err;
}

#define PROBE_CAT_(a, b) a##b
#define PROBE_CAT(a, b) PROBE_CAT_(a, b)

#if defined(ZK_PROBE_FIELD)
using Target = FieldAt<ZK_PROBE_FIELD>::type;
extern "C" int PROBE_CAT(zk_probe_unit_f, ZK_PROBE_FIELD)(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int nlanes, int mode) {
    int rc = -2;
    field_dispatch<Target>(op, [&](auto id) {
        constexpr int OP = decltype(id)::value;
        rc = launch<Target, OP, false>(field_shape<Target>(OP), a, b, out, nlanes, mode);
    });
    return rc;
}
#else
using Base = CurveAt<ZK_PROBE_CURVE>::type;
using Target = std::conditional_t<ZK_PROBE_FORM == 1, F29View<Base>, Base>;
extern "C" int PROBE_CAT(PROBE_CAT(PROBE_CAT(zk_probe_unit_c, ZK_PROBE_CURVE), _), ZK_PROBE_FORM)(int op, const uint32_t* a, const uint32_t* b, uint32_t* out,
                                                                                            int nlanes, int mode) {
    int rc = -2;
    curve_dispatch<Target>(op, [&](auto id) {
        constexpr int OP = decltype(id)::value;
        rc = launch<Target, OP, true>(curve_shape<Target>(OP), a, b, out, nlanes, mode);
    });
    return rc;
}
#endif

#else   // the entry point: target id -> unit

#define X(i, P) extern "C" int zk_probe_unit_f##i(int, const uint32_t*, const uint32_t*, uint32_t*, int, int);
ZK_PROBE_FIELDS(X)
#undef X
#define X(i, C)                                                                                  \
    extern "C" int zk_probe_unit_c##i##_0(int, const uint32_t*, const uint32_t*, uint32_t*, int, int); \
    extern "C" int zk_probe_unit_c##i##_1(int, const uint32_t*, const uint32_t*, uint32_t*, int, int);
ZK_PROBE_CURVES(X)
#undef X

#define PROBE_API extern "C" __attribute__((visibility("default")))

PROBE_API int zk_probe_shape(int target, int op, int* na, int* nb, int* no) {
    Shape s{0, 0, 0, false};
    bool known = false;
#define X(i, P) \
    if (target == i) s = field_shape<P>(op), known = true;
    ZK_PROBE_FIELDS(X)
#undef X
#define X(i, C)                                                                      \
    if (target == CURVE_TARGET0 + 2 * i) s = curve_shape<C>(op), known = true;       \
    if (target == CURVE_TARGET0 + 2 * i + 1) s = curve_shape<F29View<C>>(op), known = true;
    ZK_PROBE_CURVES(X)
#undef X
    if (!known) return -1;
    if (!s.ok) return -2;
    *na = s.na, *nb = s.nb, *no = s.no;
    return 0;
}

PROBE_API int zk_probe_run(int target, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int nlanes, int mode) {
    if (nlanes <= 0 || mode < 0 || mode > 2) return -3;
    unit_fn f = nullptr;
#define X(i, P) \
    if (target == i) f = zk_probe_unit_f##i;
    ZK_PROBE_FIELDS(X)
#undef X
#define X(i, C)                                                          \
    if (target == CURVE_TARGET0 + 2 * i) f = zk_probe_unit_c##i##_0;     \
    if (target == CURVE_TARGET0 + 2 * i + 1) f = zk_probe_unit_c##i##_1;
    ZK_PROBE_CURVES(X)
#undef X
    return f ? f(op, a, b, out, nlanes, mode) : -1;
}

#endif
