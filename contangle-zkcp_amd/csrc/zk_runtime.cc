// The runtime of libzkcp_amd.so: the process context, the per-device contexts with their stream scratch, library streams and
// persistent workers, init and shutdown, and the entry points that need no more than that (status text, field and curve
// constants, host point arithmetic).  The entry points of the subsystems are in zk_api_*.cc.
#include "zk_api_common.h"

using namespace zk;

namespace zk {
Ctx g;
int msm_pick_c(uint64_t n, int requested, bool pre) {
    // digits are stored as u16 codes; the precomputed-table form (one bucket set, 32-bit codes) goes up to 2^19 buckets
    const int cmax = pre ? 20 : 16;
    if (requested > 0) return requested < 2 ? 2 : (requested > cmax ? cmax : requested);
    int l = 0;
    while ((1ull << l) < n) l++;
    // one bucket set over the table of window multiples: the windows no longer pay a bucket reduction each, so the window can
    // grow until the ONE reduction (2^(c-1) buckets) costs what the 16 x 2^15 of the plain form do -- 13 windows instead of 16
    // at 2^20 points (tools/r3_pre.sh: measured)
    if (pre && l >= 17) return l >= 20 ? 20 : l;
    // Measured on one MI355X (profiles/r02_g_msm_size_sweep_vesta.txt): below 2^20 points the fixed costs decide -- the bucket
    // reduction's dependent additions, the host Horner (c doublings per window), the sort launches -- not the additions per
    // point, so the rule "2^5 points per bucket" (c = log2 n - 4) of round 1 was 20 - 45 % slow from 2^15 to 2^19.
    if (l >= 16) return 16;
    if (l == 15) return 15;
    if (l == 14) return 10;
    return 8;
}

// the scratch set of a caller stream: found by stream, created on first use, least-recently-used one recycled (after its
// stream has drained) beyond ZK_MAX_STREAM_SCRATCH streams.  Called with dc.mu held.
int stream_scratch(DeviceCtx& dc, hipStream_t st, StreamScratch** out) {
    for (auto& s : dc.scratch)
        if (s->stream == st) {
            s->stamp = ++dc.scratch_stamp;
            *out = s.get();
            return ZK_OK;
        }
    if ((int)dc.scratch.size() < ZK_MAX_STREAM_SCRATCH) {
        dc.scratch.emplace_back(new StreamScratch());
        StreamScratch* s = dc.scratch.back().get();
        s->stream = st;
        s->stamp = ++dc.scratch_stamp;
        *out = s;
        return ZK_OK;
    }
    StreamScratch* victim = dc.scratch[0].get();
    for (auto& s : dc.scratch)
        if (s->stamp < victim->stamp) victim = s.get();
    HIP_TRY(hipStreamSynchronize(victim->stream));   // its last user may still be running
    victim->stream = st;
    victim->stamp = ++dc.scratch_stamp;
    *out = victim;
    return ZK_OK;
}
// ZK_IPA_SHIFT_TABLES=0: the generator collapse never builds or reads shift tables (A/B against the table-free path)
bool ipa_shift_tables_enabled() {
    static const bool on = [] {
        const char* e = getenv("ZK_IPA_SHIFT_TABLES");
        return !(e && e[0] == '0' && e[1] == 0);
    }();
    return on;
}

int point_add_host(zk_curve_t c, const void* ja, const void* jb, void* jout) {
    CURVE_SWITCH(c, {
        Jacobian<C> a, b, r;
        memcpy(&a, ja, 3 * 4 * coord_words<C>());
        memcpy(&b, jb, 3 * 4 * coord_words<C>());
        XYZZ<C> xa, xb;
        jac_to_xyzz(xa, a);
        jac_to_xyzz(xb, b);
        xyzz_add(xa, xb);
        xyzz_to_jacobian(r, xa);
        memcpy(jout, &r, 3 * 4 * coord_words<C>());
    });
    return ZK_OK;
}

// the device that owns a device pointer; the home device when the runtime cannot tell (or under the emulator)
DeviceCtx& device_of(const void* p) {
    if (g.devs.size() > 1 && p) {
#if !defined(ZK_EMU)
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, p) == hipSuccess) {
            for (auto& d : g.devs)
                if (d->device == attr.device) return *d;
        } else {
            (void)hipGetLastError();
        }
#endif
    }
    return *g.devs[0];
}

int ensure_lib_streams(DeviceCtx& dc) {
    if (!dc.side[0]) {
        for (auto& s : dc.side) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        for (auto& s : dc.submit_streams) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&dc.own, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&dc.fork_ev, hipEventDisableTiming));
        for (auto& e : dc.join_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return ZK_OK;
}

std::future<int> run_on_device(DeviceCtx& dc, std::function<int()> fn) {
    std::packaged_task<int()> task(std::move(fn));
    std::future<int> fut = task.get_future();
    if (!dc.worker) {      // single-device process: inline
        task();
        return fut;
    }
    {
        std::lock_guard<std::mutex> lk(dc.worker->mu);
        dc.worker->q.push_back(std::move(task));
    }
    dc.worker->cv.notify_one();
    return fut;
}
}  // namespace zk

namespace {
void free_job(MsmJob& j) {
    for (DevBuf* b : {&j.scalars_in, &j.hot, &j.counts, &j.digits, &j.blockcnt, &j.stage_idx, &j.stage_low, &j.queue, &j.seg_out, &j.subacc, &j.sorted,
                      &j.buckets, &j.part_a, &j.part_b, &j.part_std})
        ws_free(*b);
    if (j.host_partials) hipHostFree(j.host_partials);
    j.host_partials = nullptr;
    j.host_cap = 0;
    if (j.have_events) {
        for (auto& e : j.ev) hipEventDestroy(e);
        j.have_events = false;
    }
    for (auto& e : j.acc_ev) hipEventDestroy(e);
    j.acc_ev.clear();
    j.busy = false;
}

// ---- persistent per-device workers (multi-device processes)
void worker_loop(DeviceCtx* dc) {
    hipSetDevice(dc->device);
    DeviceWorker& w = *dc->worker;
    for (;;) {
        std::packaged_task<int()> task;
        {
            std::unique_lock<std::mutex> lk(w.mu);
            w.cv.wait(lk, [&] { return w.stop || !w.q.empty(); });
            if (w.q.empty()) return;     // stop requested and nothing left
            task = std::move(w.q.front());
            w.q.pop_front();
        }
        task();
    }
}
void stop_worker(DeviceCtx& dc) {
    if (!dc.worker) return;
    {
        std::lock_guard<std::mutex> lk(dc.worker->mu);
        dc.worker->stop = true;
    }
    dc.worker->cv.notify_one();
    if (dc.worker->th.joinable()) dc.worker->th.join();
    dc.worker.reset();
}

void free_device(DeviceCtx& dc) {
    stop_worker(dc);
    hipSetDevice(dc.device);
    ws_free(dc.batch_in);
    hipDeviceSynchronize();
    for (auto& kv : dc.tw) hipFree(kv.second.dev);
    dc.tw.clear();
    dc.tw_bytes = 0;
    ws_free(dc.pow_tbl);
    ws_free(dc.scratch_in);
    for (auto& s : dc.scratch) {
        ws_free(s->ntt_tmp);
        ws_free(s->fb_table);
        ws_free(s->fb_tmp);
        ws_free(s->poly_a);
        ws_free(s->poly_b);
        ws_free(s->poly_tot);
        ws_free(s->lk_keys);
        ws_free(s->lk_runs);
        ws_free(s->lk_meta);
        if (s->pinned) hipHostFree(s->pinned);
        if (s->pinned_ev) hipEventDestroy(s->pinned_ev);
        s->pinned = nullptr;
        s->pinned_ev = nullptr;
    }
    dc.scratch.clear();
    for (auto& j : dc.jobs) free_job(j);
    for (auto& e : dc.ntt_ev_pool) hipEventDestroy(e);
    dc.ntt_ev_pool.clear();
    dc.ntt_ev_used = 0;
    for (auto& s : dc.side)
        if (s) {
            hipStreamDestroy(s);
            s = nullptr;
        }
    for (auto& s : dc.submit_streams)
        if (s) {
            hipStreamDestroy(s);
            s = nullptr;
        }
    if (dc.own) hipStreamDestroy(dc.own);
    dc.own = nullptr;
    if (dc.fork_ev) hipEventDestroy(dc.fork_ev);
    dc.fork_ev = nullptr;
    for (auto& e : dc.join_ev)
        if (e) {
            hipEventDestroy(e);
            e = nullptr;
        }
}

int init_devices_locked(int n, const int* ids) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ZK_ERR_NO_DEVICE;
    if (n <= 0 || n > ndev || !ids) return ZK_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= ndev) return ZK_ERR_INVALID_ARG;
        for (int j = 0; j < i; j++)
            if (ids[j] == ids[i]) return ZK_ERR_INVALID_ARG;
    }
    if (g.inited) {
        if ((int)g.devs.size() != n) return ZK_ERR_INVALID_ARG;
        for (int i = 0; i < n; i++)
            if (g.devs[i]->device != ids[i]) return ZK_ERR_INVALID_ARG;
        return ZK_OK;
    }
    std::vector<std::unique_ptr<DeviceCtx>> devs;
    for (int i = 0; i < n; i++) {
        if (hipSetDevice(ids[i]) != hipSuccess) return ZK_ERR_NO_DEVICE;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ids[i]) != hipSuccess) return ZK_ERR_NO_DEVICE;
        std::unique_ptr<DeviceCtx> dc(new DeviceCtx());
        dc->device = ids[i];
        dc->index = i;
        dc->num_cus = prop.multiProcessorCount;
        if (i == 0) {
#if defined(ZK_EMU)
            snprintf(g.info, sizeof g.info, "emu %.200s x%d", prop.name, n);
#else
            snprintf(g.info, sizeof g.info, "hip %.60s %.120s cu=%d x%d", prop.gcnArchName, prop.name, prop.multiProcessorCount, n);
#endif
        }
        devs.push_back(std::move(dc));
    }
#if !defined(ZK_EMU)
    for (int i = 0; i < n; i++)   // peers copy scalars to each other over xGMI
        for (int j = 0; j < n; j++)
            if (i != j) {
                hipSetDevice(ids[i]);
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, ids[i], ids[j]) == hipSuccess && can) {
                    if (hipDeviceEnablePeerAccess(ids[j], 0) != hipSuccess) (void)hipGetLastError();   // already enabled is fine
                }
            }
#endif
    hipSetDevice(ids[0]);
    g.devs = std::move(devs);
    if (n > 1)
        for (auto& dc : g.devs) {
            dc->worker.reset(new DeviceWorker());
            dc->worker->th = std::thread(worker_loop, dc.get());
        }
    memset(&g.ntt_opts, 0, sizeof g.ntt_opts);
    memset(&g.totals, 0, sizeof g.totals);
    g.ntt_profile = false;
    g.inited = true;
    return ZK_OK;
}
}  // namespace

extern "C" {

API const char* zk_strerror(int s) {
    switch (s) {
        case ZK_OK: return "ok";
        case ZK_ERR_INVALID_ARG: return "invalid argument";
        case ZK_ERR_NOT_INITIALIZED: return "zk_init has not been called";
        case ZK_ERR_NO_DEVICE: return "no usable MI355X / HIP device (there is no CPU fallback)";
        case ZK_ERR_HIP: return "HIP runtime error";
        case ZK_ERR_OOM: return "out of device memory";
        case ZK_ERR_UNSUPPORTED: return "unsupported size or curve";
        case ZK_ERR_BAD_HANDLE: return "unknown bases handle or MSM ticket";
        case ZK_ERR_BUSY: return "too many MSMs in flight on this device: collect one first";
        case ZK_ERR_LOOKUP: return "a lookup input value is not in the table";
        default: return "unknown status";
    }
}

API int zk_init(int device_id) {
    std::lock_guard<std::mutex> lk(g.mu);
    return init_devices_locked(1, &device_id);
}
API int zk_init_devices(int n_devices, const int* device_ids) {
    std::lock_guard<std::mutex> lk(g.mu);
    return init_devices_locked(n_devices, device_ids);
}
API int zk_device_count(void) {
    std::lock_guard<std::mutex> lk(g.mu);
    return g.inited ? (int)g.devs.size() : 0;
}

API int zk_shutdown(void) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.inited) return ZK_OK;
    for (auto& kv : g.bases)
        for (size_t d = 0; d < kv.second.per_dev.size(); d++) {
            hipSetDevice(g.devs[d]->device);
            hipDeviceSynchronize();
            if (kv.second.per_dev[d].owned) hipFree(kv.second.per_dev[d].dev);
            if (kv.second.per_dev[d].dev29) hipFree(kv.second.per_dev[d].dev29);
            if (kv.second.per_dev[d].pre) hipFree(kv.second.per_dev[d].pre);
            if (kv.second.per_dev[d].shift) hipFree(kv.second.per_dev[d].shift);
        }
    g.bases.clear();
    g.tickets.clear();
    r1cs_release_all();
    poseidon_release_tables();
    for (auto& dc : g.devs) free_device(*dc);
    g.devs.clear();
    g.inited = false;
    return ZK_OK;
}

API int zk_backend_info(char* buf, uint64_t buflen) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    if (!buf || buflen == 0) return ZK_ERR_INVALID_ARG;
    snprintf(buf, (size_t)buflen, "%s", g.info);
    return ZK_OK;
}

API int zk_field_limbs64(zk_field_t f) {
    FIELD_SWITCH(f, return F::N / 2);
    return ZK_ERR_INVALID_ARG;
}
API int zk_curve_base_limbs64(zk_curve_t c) {
    CURVE_SWITCH(c, return coord_words<C>() / 2);
    return ZK_ERR_INVALID_ARG;
}
API int zk_curve_scalar_field(zk_curve_t c) {
    switch (c) {
        case ZK_PALLAS: return ZK_FQ_PALLAS;
        case ZK_VESTA: return ZK_FP_PALLAS;
        case ZK_BN254_G1: return ZK_FR_BN254;
        case ZK_BLS12_381_G1: return ZK_FR_BLS12_381;
        case ZK_BN254_G2: return ZK_FR_BN254;
        case ZK_BLS12_381_G2: return ZK_FR_BLS12_381;
        default: return ZK_ERR_INVALID_ARG;
    }
}

API int zk_field_modulus(zk_field_t f, void* out) {
    if (!out) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, memcpy(out, F::P, sizeof(uint32_t) * F::N));
    return ZK_OK;
}
API int zk_field_root_of_unity(zk_field_t f, uint32_t log_n, void* out) {
    if (!out) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (log_n > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
        Fe<F> w;
        for (int i = 0; i < F::N; i++) w.v[i] = F::ROOT[i];
        for (uint32_t i = log_n; i < (uint32_t)F::TWO_ADICITY; i++) fe_sqr(w, w);
        host_store(out, w);
    });
    return ZK_OK;
}
API int zk_field_multiplicative_generator(zk_field_t f, void* out) {
    if (!out) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        Fe<F> w;
        for (int i = 0; i < F::N; i++) w.v[i] = F::GEN[i];
        host_store(out, w);
    });
    return ZK_OK;
}
API int zk_field_inverse(zk_field_t f, const void* a, void* out) {
    if (!a || !out) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        Fe<F> x;
        host_load(x, a);
        fe_inv(x, x);
        host_store(out, x);
    });
    return ZK_OK;
}
API int zk_point_add(zk_curve_t c, const void* ja, const void* jb, void* jout) {
    if (!ja || !jb || !jout) return ZK_ERR_INVALID_ARG;
    return point_add_host(c, ja, jb, jout);
}
API int zk_point_to_affine(zk_curve_t c, const void* jac, void* aff) {
    if (!jac || !aff) return ZK_ERR_INVALID_ARG;
    CURVE_SWITCH(c, {
        Jacobian<C> a;
        memcpy(&a, jac, 3 * 4 * coord_words<C>());
        XYZZ<C> x;
        jac_to_xyzz(x, a);
        Affine<C> r;
        xyzz_to_affine(r, x);
        memcpy(aff, &r, 2 * 4 * coord_words<C>());
    });
    return ZK_OK;
}

}  // extern "C"
