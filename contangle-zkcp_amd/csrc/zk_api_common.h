// Private to the units of the C ABI (zk_runtime.cc and zk_api_*.cc, one per subsystem): the export and device-entry macros,
// the runtime helpers (zk_runtime.cc) that more than one unit calls, and what zk_shutdown asks of the two registries that own
// device memory.  An entry point goes into the unit of its subsystem; its argument checks come first and touch no device.
#pragma once
#include "zk_internal.h"
#include "zkcp_amd_prover.h"

#define API __attribute__((visibility("default")))

// entry points on device buffers: bind the calling thread to the owner of `a`, serialise the enqueue on that device
#define DEVICE_ENTRY(ptr)                       \
    {                                           \
        std::lock_guard<std::mutex> lk0(g.mu);  \
        ZK_TRY(require_init());                 \
    }                                           \
    DeviceCtx& dc = device_of(ptr);             \
    ZK_TRY(bind_device(dc));                    \
    std::lock_guard<std::mutex> lk(dc.mu)

namespace zk {
DeviceCtx& device_of(const void* p);
int ensure_lib_streams(DeviceCtx& dc);
std::future<int> run_on_device(DeviceCtx& dc, std::function<int()> fn);
int point_add_host(zk_curve_t c, const void* ja, const void* jb, void* jout);
// zk_shutdown (g.mu held): free the resident R1CS matrices (zk_api_groth16.cc) / the device copies of the Poseidon tables
// (zk_api_poseidon.cc)
void r1cs_release_all();
void poseidon_release_tables();

// [a, a + a_bytes) and [b, b + b_bytes) share an address
inline bool spans_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}
// `count` host elements of F::N words each, every one below the modulus
template <class F>
bool canonical_elems(const void* p, size_t count) {
    const uint32_t* w = (const uint32_t*)p;
    for (size_t e = 0; e < count; e++, w += F::N) {
        int i = F::N - 1;
        while (i >= 0 && w[i] == F::P[i]) i--;
        if (i < 0 || w[i] > F::P[i]) return false;
    }
    return true;
}
template <class C>
void jac_to_xyzz(XYZZ<C>& r, const Jacobian<C>& j) {
    if (fe_is_zero(j.z)) {
        xyzz_set_inf(r);
        return;
    }
    r.x = j.x;
    r.y = j.y;
    fe_sqr(r.zz, j.z);
    fe_mul(r.zzz, r.zz, j.z);
}
}  // namespace zk
