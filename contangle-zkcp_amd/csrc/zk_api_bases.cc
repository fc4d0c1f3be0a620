// C ABI, bases handles: the resident copies of a vector of curve points (one per device of the process) and the tables derived
// from them.  The handles live in Ctx::bases; zk_shutdown frees what is left of them.
#include "zk_api_common.h"
#include "zk_msm_decl.h"

using namespace zk;

extern "C" {

// bases: one resident copy per device of the process.  `src_dev` >= 0: `src` is a device pointer on that device index
// (adopted there without a copy, copied to the peers); -1: `src` is host memory.
static int bases_install(zk_curve_t c, const void* src, int src_dev, uint64_t n, uint64_t* handle_out) {
    size_t esz = 0;
    CURVE_SWITCH(c, esz = sizeof(Affine<C>));
    BasesEntry be;
    be.curve = (int)c;
    be.n = n;
    be.per_dev.resize(g.devs.size());
    auto cleanup = [&]() {
        for (size_t d = 0; d < be.per_dev.size(); d++) {
            hipSetDevice(g.devs[d]->device);
            if (be.per_dev[d].owned && be.per_dev[d].dev) hipFree(be.per_dev[d].dev);
            if (be.per_dev[d].dev29) hipFree(be.per_dev[d].dev29);
        }
        hipSetDevice(g.devs[0]->device);
    };
    for (size_t d = 0; d < g.devs.size(); d++) {
        DeviceCtx& dc = *g.devs[d];
        BasesCopy& bc = be.per_dev[d];
        int st = bind_device(dc);
        if (st == ZK_OK) {
            if ((int)d == src_dev) {
                bc.dev = const_cast<void*>(src);
                bc.owned = false;
            } else {
                hipError_t e = hipMalloc(&bc.dev, esz * (n ? n : 1));
                if (e != hipSuccess) {
                    bc.dev = nullptr;
                    st = e == hipErrorOutOfMemory ? ZK_ERR_OOM : ZK_ERR_HIP;
                } else {
                    bc.owned = true;
                    if (n) {
                        if (src_dev < 0)
                            e = hipMemcpy(bc.dev, src, esz * n, hipMemcpyHostToDevice);
                        else
#if defined(ZK_EMU)
                            e = hipMemcpy(bc.dev, src, esz * n, hipMemcpyDeviceToDevice);
#else
                            e = hipMemcpyPeer(bc.dev, dc.device, src, g.devs[src_dev]->device, esz * n);
#endif
                        if (e != hipSuccess) st = ZK_ERR_HIP;
                    }
                }
            }
        }
        if (st == ZK_OK) CURVE_SWITCH(c, st = CurveLaunch<C>::bases_prepare_run(bc, n));
        if (st != ZK_OK) {
            cleanup();
            return st;
        }
    }
    hipSetDevice(g.devs[0]->device);
    const uint64_t h = g.next_handle++;
    g.bases[h] = std::move(be);
    *handle_out = h;
    return ZK_OK;
}

API int zk_bases_upload(zk_curve_t c, const void* host, uint64_t n, uint64_t* handle_out) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    if (!handle_out || (n && !host)) return ZK_ERR_INVALID_ARG;
    return bases_install(c, host, -1, n, handle_out);
}
API int zk_bases_adopt_device(zk_curve_t c, const void* dev, uint64_t n, uint64_t* handle_out) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    if (!handle_out || !dev || !aligned16(dev)) return ZK_ERR_INVALID_ARG;
    return bases_install(c, dev, device_of(dev).index, n, handle_out);
}
API int zk_bases_free(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    auto it = g.bases.find(handle);
    if (it == g.bases.end()) return ZK_ERR_BAD_HANDLE;
    for (size_t d = 0; d < it->second.per_dev.size(); d++) {
        BasesCopy& bc = it->second.per_dev[d];
        hipSetDevice(g.devs[d]->device);
        if (bc.owned || bc.dev29) hipDeviceSynchronize();
        if (bc.owned) hipFree(bc.dev);
        if (bc.dev29) hipFree(bc.dev29);
        if (bc.pre) hipFree(bc.pre);
        if (bc.shift) hipFree(bc.shift);
    }
    hipSetDevice(g.devs[0]->device);
    g.bases.erase(it);
    return ZK_OK;
}

API int zk_bases_precompute(uint64_t handle, int window_bits) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    auto it = g.bases.find(handle);
    if (it == g.bases.end()) return ZK_ERR_BAD_HANDLE;
    BasesEntry& be = it->second;
    const zk_curve_t c = (zk_curve_t)be.curve;
    const int cw = msm_pick_c(be.n, window_bits, true);
    for (size_t d = 0; d < be.per_dev.size(); d++) {
        ZK_TRY(bind_device(*g.devs[d]));
        int st = ZK_ERR_INVALID_ARG;
        CURVE_SWITCH(c, st = CurveLaunch<C>::bases_precompute_run(be.per_dev[d], be.n, cw));
        ZK_TRY(st);
    }
    return ZK_OK;
}
// under g.mu.  Drops the copy's shift tables (the points changed, or the handle goes away)
static void shifts_drop(BasesCopy& bc) {
    if (bc.shift) {
        hipDeviceSynchronize();
        hipFree(bc.shift);
    }
    bc.shift = nullptr;
    bc.collapses = 0;
    bc.shift_failed = false;
}
API int zk_bases_precompute_shifts(zk_curve_t c, uint64_t handle) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    auto it = g.bases.find(handle);
    if (it == g.bases.end()) return ZK_ERR_BAD_HANDLE;
    BasesEntry& be = it->second;
    if (be.curve != (int)c) return ZK_ERR_INVALID_ARG;
    if (!ipa_shift_tables_enabled()) return ZK_OK;
    int st = ZK_OK;
    for (size_t d = 0; d < be.per_dev.size() && st == ZK_OK; d++) {
        st = bind_device(*g.devs[d]);
        if (st == ZK_OK && !be.per_dev[d].shift) CURVE_SWITCH(c, st = CurveLaunch<C>::bases_shifts_run(be.per_dev[d], be.n));
    }
    hipSetDevice(g.devs[0]->device);
    return st;
}
API int zk_bases_shift_tables(uint64_t handle, uint64_t* present) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    if (!present) return ZK_ERR_INVALID_ARG;
    auto it = g.bases.find(handle);
    if (it == g.bases.end()) return ZK_ERR_BAD_HANDLE;
    uint64_t all = 1;
    for (const BasesCopy& bc : it->second.per_dev) all &= bc.shift ? 1 : 0;
    *present = all;
    return ZK_OK;
}
API int zk_bases_refresh(uint64_t handle, uint64_t offset, uint64_t count, void* stream) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    auto it = g.bases.find(handle);
    if (it == g.bases.end()) return ZK_ERR_BAD_HANDLE;
    BasesEntry& be = it->second;
    if (offset > be.n || count > be.n - offset) return ZK_ERR_INVALID_ARG;
    size_t esz = 0;
    const zk_curve_t c = (zk_curve_t)be.curve;
    CURVE_SWITCH(c, esz = sizeof(Affine<C>));
    int src = -1;
    for (size_t d = 0; d < be.per_dev.size(); d++)
        if (!be.per_dev[d].owned) src = (int)d;          // the adopted copy is the one the caller rewrites
    if (src < 0) src = 0;
    for (size_t d = 0; d < be.per_dev.size(); d++) {
        DeviceCtx& dc = *g.devs[d];
        ZK_TRY(bind_device(dc));
        hipStream_t st = (hipStream_t)stream;
        if ((int)d != src) {      // a peer: wait for the caller's stream, copy the range over, convert on the library's stream
            HIP_TRY(hipSetDevice(g.devs[src]->device));
            HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
            HIP_TRY(hipSetDevice(dc.device));
#if defined(ZK_EMU)
            HIP_TRY(hipMemcpy((unsigned char*)be.per_dev[d].dev + offset * esz, (unsigned char*)be.per_dev[src].dev + offset * esz, count * esz, hipMemcpyDeviceToDevice));
#else
            HIP_TRY(hipMemcpyPeer((unsigned char*)be.per_dev[d].dev + offset * esz, dc.device, (unsigned char*)be.per_dev[src].dev + offset * esz,
                                  g.devs[src]->device, count * esz));
#endif
            st = nullptr;
        }
        shifts_drop(be.per_dev[d]);
        CURVE_SWITCH(c, ZK_TRY(CurveLaunch<C>::bases_refresh_run(be.per_dev[d], offset, count, st)));
        if ((int)d != src) HIP_TRY(hipStreamSynchronize(nullptr));
    }
    hipSetDevice(g.devs[0]->device);
    return ZK_OK;
}

}  // extern "C"
