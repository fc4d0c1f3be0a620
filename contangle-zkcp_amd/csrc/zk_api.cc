// C ABI implementation (include/zkcp_amd.h): argument checks, dispatch over curve / field / device, the MSM job pool
// (submit -> collect) and the host-side helpers.  The launch sequences live in zk_msm.inl / zk_ntt.inl (one TU per
// curve / field).  Compiled with `hipcc -x hip --offload-arch=gfx950` into libzkcp_amd.so.  (The CPU test tier
// compiles the same files against tests/emu/emu_hip.h; see zk_rt.h.)
#include "zk_internal.h"
#include "zk_msm_decl.h"
#include "zk_ntt_decl.h"
#include "zkcp_amd_prover.h"
#include "zk_poseidon_kernels.h"

#include <thread>

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
}  // namespace zk

namespace {
// R1CS matrices of the circuits in use (zk_r1cs_matrix_upload): fixed per circuit, resident on the home device
std::mutex g_mat_mu;
std::map<uint64_t, R1csMatrix> g_mats;
uint64_t g_next_mat = 1;
void free_matrix(R1csMatrix& m) {
    for (void* p : {m.row_ptr, m.col, m.val, m.long_rows, m.col_ptr, m.t_row, m.t_val, m.long_cols})
        if (p) hipFree(p);
    m = R1csMatrix();
}

// Poseidon parameter sets (zk_poseidon_create): the table [ark | mds | init] on the host, for the host twin and as the source of the
// one copy per device that the first *_device call there uploads.  Handles need no device and outlive zk_shutdown (their device
// copies do not).
struct PoseidonEntry {
    int field = 0;
    PoseidonShape shape;
    std::vector<uint64_t> tbl;            // 4 words per element
    std::map<int, void*> dev;             // device index -> table
};
std::mutex g_pos_mu;
std::map<uint64_t, std::shared_ptr<PoseidonEntry>> g_poseidon;
uint64_t g_next_poseidon = 1;
void free_poseidon_tables(PoseidonEntry& e) {   // (g.mu and g_pos_mu held)
    for (auto& kv : e.dev)
        if (kv.first < (int)g.devs.size()) {
            hipSetDevice(g.devs[kv.first]->device);
            hipDeviceSynchronize();
            hipFree(kv.second);
        }
    e.dev.clear();
}

bool spans_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}
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
int find_poseidon(uint64_t handle, std::shared_ptr<PoseidonEntry>* out) {
    std::lock_guard<std::mutex> lk(g_pos_mu);
    auto it = g_poseidon.find(handle);
    if (it == g_poseidon.end()) return ZK_ERR_BAD_HANDLE;
    *out = it->second;
    return ZK_OK;
}
// the handle's table on the calling device, uploaded at the first use there (dc.mu held)
int poseidon_table(PoseidonEntry& e, DeviceCtx& dc, const void** out) {
    std::lock_guard<std::mutex> lk(g_pos_mu);
    auto it = e.dev.find(dc.index);
    if (it == e.dev.end()) {
        void* p = nullptr;
        const size_t bytes = e.tbl.size() * sizeof(uint64_t);
        HIP_TRY(hipMalloc(&p, bytes));
        if (hipMemcpy(p, e.tbl.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(p);
            return ZK_ERR_HIP;
        }
        it = e.dev.emplace(dc.index, p).first;
    }
    *out = it->second;
    return ZK_OK;
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

MsmTuning tuning_from(const zk_msm_opts* o) {
    MsmTuning t;
    if (!o) return t;
    t.window_bits = o->window_bits;
    t.w0 = o->window_begin;
    t.w1 = o->window_end;
    t.limb_bits = o->limb_bits;
    t.split_log = o->split_log_plus1 > 0 ? o->split_log_plus1 - 1 : -1;
    t.slice_len = o->slice_len > 0 ? (uint32_t)o->slice_len : 0;
    t.big_thresh = o->big_threshold > 0 ? (uint32_t)o->big_threshold : 0;
    t.waves = o->waves_per_simd;
    t.no_hot_help = (o->flags & ZK_MSM_FLAG_NO_HOT_HELP) != 0;
    t.slice_reduce = (o->flags & ZK_MSM_FLAG_SLICE_REDUCE) != 0;
    t.precomputed = (o->flags & ZK_MSM_FLAG_PRECOMPUTED) != 0;
    t.device_partials = (o->flags & ZK_MSM_FLAG_DEVICE_PARTIALS) != 0;
    t.base_offset = o->base_offset > 0 ? (uint64_t)o->base_offset : 0;
    t.window_group = o->window_group > 0 ? o->window_group : 0;
    return t;
}

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

void stop_worker(DeviceCtx& dc);
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

// take a free job slot of the device (dc.mu held).  All busy -> ZK_ERR_BUSY: the caller must collect first.
int job_acquire(DeviceCtx& dc, MsmJob** out) {
    for (auto& j : dc.jobs)
        if (!j.busy) {
            j.dc = &dc;
            j.busy = true;
            *out = &j;
            return ZK_OK;
        }
    return ZK_ERR_BUSY;
}

// where the scalars of a submission are
enum ScalarSrc { SRC_LOCAL = 0, SRC_HOST = 1, SRC_PEER = 2 };

// enqueue one MSM on device dc / stream st (dc.mu held, thread bound to dc.device).  Scalars that are not already in this
// device's memory are staged into a buffer the JOB owns, so MSMs in flight never share a staging area.
int submit_on(DeviceCtx& dc, zk_curve_t c, const BasesEntry& be, const void* scalars, ScalarSrc kind, int peer_device, uint64_t n, int mont,
              const MsmTuning& tu, hipStream_t st, MsmJob** out) {
    MsmJob* job = nullptr;
    ZK_TRY(job_acquire(dc, &job));
    job->stream = st;
    job->curve = (int)c;
    int status = ZK_OK;
    const void* d_scalars = scalars;
    auto stage = [&]() -> int {
        if (kind == SRC_LOCAL || n == 0) return ZK_OK;
        ZK_TRY(ws_get(job->scalars_in, 32 * n));
        d_scalars = job->scalars_in.p;
        if (kind == SRC_HOST) {
            HIP_TRY(hipMemcpyAsync(job->scalars_in.p, scalars, 32 * n, hipMemcpyHostToDevice, st));
        } else {
#if defined(ZK_EMU)
            HIP_TRY(hipMemcpyAsync(job->scalars_in.p, scalars, 32 * n, hipMemcpyDeviceToDevice, st));
#else
            HIP_TRY(hipMemcpyPeerAsync(job->scalars_in.p, dc.device, scalars, peer_device, 32 * n, st));
#endif
        }
        return ZK_OK;
    };
    status = stage();
    (void)peer_device;
    const BasesCopy& bc = be.per_dev[dc.index];
    if (status == ZK_OK) {
        status = ZK_ERR_INVALID_ARG;
        switch (c) {
            case ZK_PALLAS: status = msm_enqueue<Pallas>(*job, bc, (const Fe<Pallas::Fr>*)d_scalars, n, mont, tu); break;
            case ZK_VESTA: status = msm_enqueue<Vesta>(*job, bc, (const Fe<Vesta::Fr>*)d_scalars, n, mont, tu); break;
            case ZK_BN254_G1: status = msm_enqueue<Bn254G1>(*job, bc, (const Fe<Bn254G1::Fr>*)d_scalars, n, mont, tu); break;
            case ZK_BLS12_381_G1: status = msm_enqueue<Bls381G1>(*job, bc, (const Fe<Bls381G1::Fr>*)d_scalars, n, mont, tu); break;
            case ZK_BN254_G2: status = msm_enqueue<Bn254G2>(*job, bc, (const Fe<Bn254G2::Fr>*)d_scalars, n, mont, tu); break;
            case ZK_BLS12_381_G2: status = msm_enqueue<Bls381G2>(*job, bc, (const Fe<Bls381G2::Fr>*)d_scalars, n, mont, tu); break;
            default: break;
        }
    }
    if (status != ZK_OK) {
        job->busy = false;
        return status;
    }
    *out = job;
    return ZK_OK;
}

int collect_job(MsmJob& job, void* out) {
    hipSetDevice(job.dc->device);
    const int status = job.finish(job, out);
    {
        std::lock_guard<std::mutex> lk(g.mu);
        g.prof = job.prof;
        if (!job.empty) {
            g.totals.msms += job.batch;
            g.totals.launches++;
            g.totals.accumulate_kernel_ms += job.prof.accumulate_kernel_ms;
            g.totals.accumulate_ms += job.prof.accumulate_ms;
            g.totals.sort_ms += job.prof.digits_ms + job.prof.hist_ms + job.prof.scatter_ms;
            g.totals.reduce_ms += job.prof.reduce_ms;
            g.totals.host_tail_ms += job.prof.host_tail_ms;
            g.totals.device_ms += job.prof.total_ms - job.prof.host_tail_ms;
            g.totals.algorithmic_bytes += job.alg_bytes;
        }
    }
    std::lock_guard<std::mutex> lk(job.dc->mu);
    job.busy = false;
    return status;
}

int find_bases(uint64_t handle, zk_curve_t c, uint64_t n, const BasesEntry** out, const zk_msm_opts* opts = nullptr) {
    std::lock_guard<std::mutex> lk(g.mu);
    ZK_TRY(require_init());
    auto it = g.bases.find(handle);
    if (it == g.bases.end()) return ZK_ERR_BAD_HANDLE;
    const uint64_t off = opts && opts->base_offset > 0 ? (uint64_t)opts->base_offset : 0;
    if (opts && opts->base_offset < 0) return ZK_ERR_INVALID_ARG;
    if (it->second.curve != (int)c || n > it->second.n || off > it->second.n - n) return ZK_ERR_INVALID_ARG;
    *out = &it->second;   // entries are only erased by zk_bases_free, which the caller must not race with a running MSM
    return ZK_OK;
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

size_t jac_bytes(zk_curve_t c) {
    size_t w = 0;
    switch (c) {
        case ZK_PALLAS: w = coord_words<Pallas>(); break;
        case ZK_VESTA: w = coord_words<Vesta>(); break;
        case ZK_BN254_G1: w = coord_words<Bn254G1>(); break;
        case ZK_BLS12_381_G1: w = coord_words<Bls381G1>(); break;
        case ZK_BN254_G2: w = coord_words<Bn254G2>(); break;
        default: w = coord_words<Bls381G2>(); break;
    }
    return (size_t)3 * 4 * w;
}

// One MSM over all devices of the process: device d sums windows [W d / G, W (d + 1) / G) from its own resident copy of
// the bases; the Jacobian partial sums are added on the host (EC addition is not an RCCL reduction; the partial is 96 -
// 288 bytes and is already on the host after the job's tail).  `src` is where the scalars are: a host pointer (src_dc ==
// nullptr; every device copies them over its own PCIe link) or a device pointer owned by src_dc (peers copy over xGMI).
// The shares run on the devices' persistent workers; the calling thread takes device 0's.
int msm_fanout(zk_curve_t c, const BasesEntry& be, const void* src, DeviceCtx* src_dc, hipStream_t src_stream, uint64_t n, int mont,
               const MsmTuning& tu_in, void* out) {
    const int G = (int)g.devs.size();
    int nwin = 0;
    CURVE_SWITCH(c, nwin = msm_windows<C>(msm_pick_c(n, tu_in.window_bits, tu_in.precomputed)));
    const size_t pbytes = jac_bytes(c);
    std::vector<std::vector<unsigned char>> parts(G, std::vector<unsigned char>(pbytes));
    hipEvent_t ready = nullptr;
    if (src_dc) {   // peers must not read the scalars before the caller's stream has produced them
        hipSetDevice(src_dc->device);
        std::lock_guard<std::mutex> lk(src_dc->mu);
        ZK_TRY(ensure_lib_streams(*src_dc));
        ready = src_dc->fork_ev;
        HIP_TRY(hipEventRecord(ready, src_stream));
    }
    auto work = [&](int d) -> int {
        DeviceCtx& dc = *g.devs[d];
        MsmTuning tu = tu_in;
        tu.w0 = nwin * d / G;
        tu.w1 = nwin * (d + 1) / G;
        MsmJob* job = nullptr;
        auto run = [&]() -> int {
            ZK_TRY(bind_device(dc));
            std::lock_guard<std::mutex> lk(dc.mu);
            if (tu.w0 == tu.w1) {   // more devices than windows: this one contributes the identity
                tu.w0 = tu.w1 = 0;
                return submit_on(dc, c, be, nullptr, SRC_LOCAL, 0, 0, mont, tu, nullptr, &job);
            }
            ZK_TRY(ensure_lib_streams(dc));
            if (!src_dc) return submit_on(dc, c, be, src, SRC_HOST, 0, n, mont, tu, dc.own, &job);
            if (&dc == src_dc) return submit_on(dc, c, be, src, SRC_LOCAL, 0, n, mont, tu, src_stream, &job);
            HIP_TRY(hipStreamWaitEvent(dc.own, ready, 0));
            return submit_on(dc, c, be, src, SRC_PEER, src_dc->device, n, mont, tu, dc.own, &job);
        };
        int st_ = run();
        if (st_ == ZK_OK) st_ = collect_job(*job, parts[d].data());
        return st_;
    };
    std::vector<std::future<int>> fut;
    for (int d = 1; d < G; d++) fut.push_back(run_on_device(*g.devs[d], [&, d] { return work(d); }));
    int status = work(0);
    for (auto& f : fut) {
        const int s2 = f.get();
        if (status == ZK_OK) status = s2;
    }
    ZK_TRY(status);
    memcpy(out, parts[0].data(), pbytes);
    for (int d = 1; d < G; d++) ZK_TRY(point_add_host(c, out, parts[d].data(), out));
    hipSetDevice(g.devs[0]->device);
    return ZK_OK;
}

bool whole_msm(const MsmTuning& tu) { return tu.w0 == 0 && tu.w1 == 0; }

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

// ====================================================================== exported C ABI
extern "C" {

#define API __attribute__((visibility("default")))

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
    {
        std::lock_guard<std::mutex> lkm(g_mat_mu);
        if (!g.devs.empty()) hipSetDevice(g.devs[0]->device);
        for (auto& kv : g_mats) free_matrix(kv.second);
        g_mats.clear();
    }
    {
        std::lock_guard<std::mutex> lkp(g_pos_mu);
        for (auto& kv : g_poseidon) free_poseidon_tables(*kv.second);
    }
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
API int zk_msm_window_bits(zk_curve_t c, uint64_t n, int requested) {
    CURVE_SWITCH(c, (void)sizeof(C); return msm_pick_c(n, requested));
    return ZK_ERR_INVALID_ARG;
}
API int zk_msm_window_count(zk_curve_t c, uint64_t n, int window_bits) {
    CURVE_SWITCH(c, return msm_windows<C>(msm_pick_c(n, window_bits)));
    return ZK_ERR_INVALID_ARG;
}

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
        if (st == ZK_OK) CURVE_SWITCH(c, st = bases_prepare_run<C>(bc, n));
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
        CURVE_SWITCH(c, st = bases_precompute_run<C>(be.per_dev[d], be.n, cw));
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
        if (st == ZK_OK && !be.per_dev[d].shift) CURVE_SWITCH(c, st = bases_shifts_run<C>(be.per_dev[d], be.n));
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
        CURVE_SWITCH(c, ZK_TRY(bases_refresh_run<C>(be.per_dev[d], offset, count, st)));
        if ((int)d != src) HIP_TRY(hipStreamSynchronize(nullptr));
    }
    hipSetDevice(g.devs[0]->device);
    return ZK_OK;
}

API int zk_msm_submit(zk_curve_t c, uint64_t handle, const void* d_scalars, uint64_t n, int mont, const zk_msm_opts* opts, void* stream,
                      uint64_t* ticket_out) {
    if (!ticket_out || (n && (!d_scalars || !aligned16(d_scalars)))) return ZK_ERR_INVALID_ARG;
    const BasesEntry* be = nullptr;
    ZK_TRY(find_bases(handle, c, n, &be, opts));
    DeviceCtx& dc = device_of(d_scalars);
    if (g.devs.size() > 1 && whole_msm(tuning_from(opts)) && n > 0) {
        // one process, several GPUs: one job per device (its window share), enqueued here without waiting; the peers copy the
        // scalars over xGMI into their job's own staging buffer behind an event on the caller's stream
        const int G = (int)g.devs.size();
        int nwin = 0;
        const MsmTuning tu_in = tuning_from(opts);
        CURVE_SWITCH(c, nwin = msm_windows<C>(msm_pick_c(n, tu_in.window_bits, tu_in.precomputed)));
        hipEvent_t ready = nullptr;
        {
            ZK_TRY(bind_device(dc));
            std::lock_guard<std::mutex> lk(dc.mu);
            ZK_TRY(ensure_lib_streams(dc));
            ready = dc.fork_ev;
            HIP_TRY(hipEventRecord(ready, (hipStream_t)stream));
        }
        std::vector<MsmJob*> jobs;
        int status = ZK_OK;
        for (int d = 0; d < G && status == ZK_OK; d++) {
            DeviceCtx& dd = *g.devs[d];
            MsmTuning tu = tu_in;
            tu.w0 = nwin * d / G;
            tu.w1 = nwin * (d + 1) / G;
            MsmJob* job = nullptr;
            status = bind_device(dd);
            if (status != ZK_OK) break;
            std::lock_guard<std::mutex> lk(dd.mu);
            if (tu.w0 == tu.w1) {
                tu.w0 = tu.w1 = 0;
                status = submit_on(dd, c, *be, nullptr, SRC_LOCAL, 0, 0, mont ? 1 : 0, tu, nullptr, &job);
            } else if (&dd == &dc) {
                status = submit_on(dd, c, *be, d_scalars, SRC_LOCAL, 0, n, mont ? 1 : 0, tu, (hipStream_t)stream, &job);
            } else {
                status = ensure_lib_streams(dd);
                if (status == ZK_OK && hipStreamWaitEvent(dd.own, ready, 0) != hipSuccess) status = ZK_ERR_HIP;
                if (status == ZK_OK) status = submit_on(dd, c, *be, d_scalars, SRC_PEER, dc.device, n, mont ? 1 : 0, tu, dd.own, &job);
            }
            if (status == ZK_OK) jobs.push_back(job);
        }
        hipSetDevice(g.devs[0]->device);
        if (status != ZK_OK) {      // release what was taken
            for (MsmJob* j : jobs) {
                std::vector<unsigned char> sink(jac_bytes(c));
                collect_job(*j, sink.data());
            }
            return status;
        }
        std::lock_guard<std::mutex> lk(g.mu);
        const uint64_t t = g.next_ticket++;
        for (MsmJob* j : jobs) j->ticket = t;
        g.tickets[t] = jobs;
        *ticket_out = t;
        return ZK_OK;
    }
    ZK_TRY(bind_device(dc));
    MsmJob* job = nullptr;
    {
        std::lock_guard<std::mutex> lk(dc.mu);
        hipStream_t run_on = (hipStream_t)stream;
        if (opts && (opts->flags & ZK_MSM_FLAG_OWN_STREAM)) {
            // the job runs on a library stream forked behind what `stream` holds now: the latency-bound phases of one MSM (the
            // oversized-bucket path and the bucket reduction: dependent additions at one wave per SIMD on the G2 types) then
            // run beside the next MSM's accumulate kernel instead of in front of it
            ZK_TRY(ensure_lib_streams(dc));
            HIP_TRY(hipEventRecord(dc.fork_ev, (hipStream_t)stream));
            run_on = dc.submit_streams[dc.submit_rr++ % ZK_MAX_JOBS];     // as many streams as job slots: every MSM in flight has its own
            HIP_TRY(hipStreamWaitEvent(run_on, dc.fork_ev, 0));
        }
        ZK_TRY(submit_on(dc, c, *be, d_scalars, SRC_LOCAL, 0, n, mont ? 1 : 0, tuning_from(opts), run_on, &job));
    }
    std::lock_guard<std::mutex> lk(g.mu);
    job->ticket = g.next_ticket++;
    g.tickets[job->ticket] = {job};
    *ticket_out = job->ticket;
    return ZK_OK;
}
API int zk_msm_collect(uint64_t ticket, void* out) {
    if (!out) return ZK_ERR_INVALID_ARG;
    std::vector<MsmJob*> jobs;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        ZK_TRY(require_init());
        auto it = g.tickets.find(ticket);
        if (it == g.tickets.end()) return ZK_ERR_BAD_HANDLE;
        jobs = it->second;
        g.tickets.erase(it);
    }
    if (jobs.size() == 1) return collect_job(*jobs[0], out);
    // a fanned-out submission: one window share per device; the tails run on the devices' workers, the partials are added here
    const zk_curve_t c = (zk_curve_t)jobs[0]->curve;
    const size_t pbytes = jac_bytes(c);
    std::vector<std::vector<unsigned char>> parts(jobs.size(), std::vector<unsigned char>(pbytes));
    std::vector<std::future<int>> fut;
    for (size_t d = 1; d < jobs.size(); d++) fut.push_back(run_on_device(*jobs[d]->dc, [&, d] { return collect_job(*jobs[d], parts[d].data()); }));
    int status = collect_job(*jobs[0], parts[0].data());
    for (auto& f : fut) {
        const int s2 = f.get();
        if (status == ZK_OK) status = s2;
    }
    ZK_TRY(status);
    memcpy(out, parts[0].data(), pbytes);
    for (size_t d = 1; d < jobs.size(); d++) ZK_TRY(point_add_host(c, out, parts[d].data(), out));
    hipSetDevice(g.devs[0]->device);
    return ZK_OK;
}

API int zk_msm_device(zk_curve_t c, uint64_t handle, const void* d_scalars, uint64_t n, int mont, const zk_msm_opts* opts,
                      void* out, void* stream) {
    if (!out || (n && (!d_scalars || !aligned16(d_scalars)))) return ZK_ERR_INVALID_ARG;
    const BasesEntry* be = nullptr;
    ZK_TRY(find_bases(handle, c, n, &be, opts));
    const MsmTuning tu = tuning_from(opts);
    DeviceCtx& dc = device_of(d_scalars);
    if (g.devs.size() > 1 && whole_msm(tu) && n > 0) return msm_fanout(c, *be, d_scalars, &dc, (hipStream_t)stream, n, mont ? 1 : 0, tu, out);
    ZK_TRY(bind_device(dc));
    MsmJob* job = nullptr;
    {
        std::lock_guard<std::mutex> lk(dc.mu);
        ZK_TRY(submit_on(dc, c, *be, d_scalars, SRC_LOCAL, 0, n, mont ? 1 : 0, tu, (hipStream_t)stream, &job));
    }
    return collect_job(*job, out);
}

API int zk_msm(zk_curve_t c, uint64_t handle, const void* scalars_host, uint64_t n, int mont, const zk_msm_opts* opts,
               void* out) {
    if (!out || (n && !scalars_host)) return ZK_ERR_INVALID_ARG;
    const BasesEntry* be = nullptr;
    ZK_TRY(find_bases(handle, c, n, &be, opts));
    const MsmTuning tu = tuning_from(opts);
    if (g.devs.size() > 1 && whole_msm(tu) && n > 0) return msm_fanout(c, *be, scalars_host, nullptr, nullptr, n, mont ? 1 : 0, tu, out);
    DeviceCtx& dc = *g.devs[0];
    ZK_TRY(bind_device(dc));
    MsmJob* job = nullptr;
    {
        std::lock_guard<std::mutex> lk(dc.mu);
        ZK_TRY(submit_on(dc, c, *be, scalars_host, SRC_HOST, 0, n, mont ? 1 : 0, tu, (hipStream_t)0, &job));
    }
    return collect_job(*job, out);
}

// `count` MSMs over one bases entry on ONE device (the scalars are in that device's memory): jobs of up to four vectors,
// alternating over the device's two library streams, forked from and joined back into `stream`
static int batch_on_device(DeviceCtx& dc, zk_curve_t c, const BasesEntry* be, const void* d_scalars, uint64_t n, uint32_t count, uint64_t stride_elems,
                           int mont, const MsmTuning& tu, void* out, void* stream) {
    ZK_TRY(bind_device(dc));
    size_t pbytes = 0;
    CURVE_SWITCH(c, pbytes = (size_t)3 * 4 * coord_words<C>());
    {
        std::lock_guard<std::mutex> lk(dc.mu);
        ZK_TRY(ensure_lib_streams(dc));
        HIP_TRY(hipEventRecord(dc.fork_ev, (hipStream_t)stream));
        for (auto& s : dc.side) HIP_TRY(hipStreamWaitEvent(s, dc.fork_ev, 0));
    }
    // Up to 4 scalar vectors go into ONE job: their windows are simply more windows of the same sort / accumulate / reduce
    // launches (one persistent accumulate launch without a drain per MSM, the latency-bound reduction steps once per job).
    // How many is the launch plan's answer (msm_plan_batch, zk_msm_plan.h).  Job k runs on side stream k mod 2; at most
    // ZK_MAX_JOBS - 1 in flight, collected in order.
    uint32_t per_job = 1;
    CURVE_SWITCH(c, per_job = msm_batch_size<C>(be->per_dev[dc.index], n, tu, dc.num_cus));
    struct Flight {
        MsmJob* job;
        uint32_t first, size;
    };
    std::vector<Flight> inflight;
    uint32_t submitted = 0, collected = 0, jobs = 0;
    int status = ZK_OK;
    while (collected < count && status == ZK_OK) {
        while (submitted < count && inflight.size() < (size_t)ZK_MAX_JOBS - 1 && status == ZK_OK) {
            MsmJob* job = nullptr;
            MsmTuning tj = tu;
            tj.batch = count - submitted < per_job ? count - submitted : per_job;
            tj.batch_stride = stride_elems;
            std::lock_guard<std::mutex> lk(dc.mu);
            status = submit_on(dc, c, *be, (const unsigned char*)d_scalars + (size_t)submitted * stride_elems * 32, SRC_LOCAL, 0, n, mont ? 1 : 0,
                               tj, dc.side[jobs & 1], &job);
            if (status == ZK_ERR_BUSY && !inflight.empty()) {   // other callers hold the remaining slots: drain ours first
                status = ZK_OK;
                break;
            }
            if (status == ZK_OK) {
                inflight.push_back({job, submitted, tj.batch});
                submitted += tj.batch;
                jobs++;
            }
        }
        if (status != ZK_OK || inflight.empty()) break;
        status = collect_job(*inflight.front().job, (unsigned char*)out + (size_t)inflight.front().first * pbytes);
        collected += inflight.front().size;
        inflight.erase(inflight.begin());
    }
    for (auto& fl : inflight) {   // error path: release what is still in flight
        std::vector<unsigned char> sink(pbytes * fl.size);
        collect_job(*fl.job, sink.data());
    }
    if (status == ZK_OK && collected < count) status = ZK_ERR_BUSY;
    {
        std::lock_guard<std::mutex> lk(dc.mu);
        for (int s = 0; s < 2; s++) {
            HIP_TRY(hipEventRecord(dc.join_ev[s], dc.side[s]));
            HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, dc.join_ev[s], 0));
        }
    }
    return status;
}

API int zk_msm_batch_device(zk_curve_t c, uint64_t handle, const void* d_scalars, uint64_t n, uint32_t count, uint64_t stride_elems,
                            int mont, const zk_msm_opts* opts, void* out, void* stream) {
    if (count == 0) return ZK_OK;
    if (!out || stride_elems < n || (n && (!d_scalars || !aligned16(d_scalars)))) return ZK_ERR_INVALID_ARG;
    const BasesEntry* be = nullptr;
    ZK_TRY(find_bases(handle, c, n, &be, opts));
    const MsmTuning tu = tuning_from(opts);
    DeviceCtx& owner = device_of(d_scalars);
    const int G = (int)g.devs.size();
    if (G == 1 || !whole_msm(tu) || n == 0) return batch_on_device(owner, c, be, d_scalars, n, count, stride_elems, mont, tu, out, stream);
    const size_t pbytes = jac_bytes(c);
    if (count < (uint32_t)G) {
        // fewer vectors than devices (the L / R pair of an IPA round): every vector window-sharded over ALL devices, one after another
        for (uint32_t v = 0; v < count; v++)
            ZK_TRY(msm_fanout(c, *be, (const unsigned char*)d_scalars + (size_t)v * stride_elems * 32, &owner, (hipStream_t)stream, n, mont ? 1 : 0, tu,
                              (unsigned char*)out + (size_t)v * pbytes));
        return ZK_OK;
    }
    // at least one vector per device (halo2's column commitments): device d takes the WHOLE MSMs of vectors [count d / G, count (d + 1) / G)
    // -- whole MSMs keep their fixed costs once per vector instead of once per vector and device -- and only those vectors
    // travel (over xGMI, into the device's staging buffer, behind an event on the caller's stream)
    hipEvent_t ready = nullptr;
    {
        ZK_TRY(bind_device(owner));
        std::lock_guard<std::mutex> lk(owner.mu);
        ZK_TRY(ensure_lib_streams(owner));
        ready = owner.fork_ev;
        HIP_TRY(hipEventRecord(ready, (hipStream_t)stream));
    }
    auto work = [&](int d) -> int {
        DeviceCtx& dc = *g.devs[d];
        const uint32_t first = (uint32_t)((uint64_t)count * d / G), last = (uint32_t)((uint64_t)count * (d + 1) / G);
        if (last == first) return ZK_OK;
        unsigned char* dst_out = (unsigned char*)out + (size_t)first * pbytes;
        if (&dc == &owner)
            return batch_on_device(dc, c, be, (const unsigned char*)d_scalars + (size_t)first * stride_elems * 32, n, last - first, stride_elems, mont, tu,
                                   dst_out, stream);
        ZK_TRY(bind_device(dc));
        std::lock_guard<std::mutex> stage_lk(dc.batch_mu);      // the staging buffer serves one fanned-out batch at a time
        {
            std::lock_guard<std::mutex> lk(dc.mu);
            ZK_TRY(ensure_lib_streams(dc));
            ZK_TRY(ws_get(dc.batch_in, (size_t)(last - first) * n * 32));
            HIP_TRY(hipStreamWaitEvent(dc.own, ready, 0));
            for (uint32_t v = first; v < last; v++) {
                const void* srcp = (const unsigned char*)d_scalars + (size_t)v * stride_elems * 32;
                void* dstp = (unsigned char*)dc.batch_in.p + (size_t)(v - first) * n * 32;
#if defined(ZK_EMU)
                HIP_TRY(hipMemcpyAsync(dstp, srcp, n * 32, hipMemcpyDeviceToDevice, dc.own));
#else
                HIP_TRY(hipMemcpyPeerAsync(dstp, dc.device, srcp, owner.device, n * 32, dc.own));
#endif
            }
        }
        return batch_on_device(dc, c, be, dc.batch_in.p, n, last - first, n, mont, tu, dst_out, dc.own);
    };
    std::vector<std::future<int>> fut;
    for (int d = 0; d < G; d++)
        if (g.devs[d].get() != &owner) fut.push_back(run_on_device(*g.devs[d], [&, d] { return work(d); }));
    int status = work(owner.index);
    for (auto& f : fut) {
        const int s2 = f.get();
        if (status == ZK_OK) status = s2;
    }
    hipSetDevice(g.devs[0]->device);
    return status;
}

API int zk_msm_last_profile(zk_msm_profile* out) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return ZK_ERR_INVALID_ARG;
    *out = g.prof;
    return ZK_OK;
}

API int zk_msm_profile_totals(zk_msm_totals* out, int reset) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (!out) return ZK_ERR_INVALID_ARG;
    *out = g.totals;
    if (reset) memset(&g.totals, 0, sizeof g.totals);
    return ZK_OK;
}

API int zk_ntt_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g.mu);
    g.ntt_profile = on != 0;
    return ZK_OK;
}
API int zk_ntt_profile_read(zk_ntt_totals* out) {
    if (!out) return ZK_ERR_INVALID_ARG;
    {
        std::lock_guard<std::mutex> lk0(g.mu);
        ZK_TRY(require_init());
    }
    memset(out, 0, sizeof *out);
    for (auto& dcp : g.devs) {
        DeviceCtx& dc = *dcp;
        ZK_TRY(bind_device(dc));
        std::lock_guard<std::mutex> lk(dc.mu);
        for (size_t i = 0; i + 1 < dc.ntt_ev_used; i += 2) {
            HIP_TRY(hipEventSynchronize(dc.ntt_ev_pool[i + 1]));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, dc.ntt_ev_pool[i], dc.ntt_ev_pool[i + 1]));
            out->kernel_ms += ms;
            out->launches++;
        }
        out->transforms += dc.ntt_transforms;
        out->algorithmic_bytes += dc.ntt_alg_bytes;
        dc.ntt_ev_used = 0;
        dc.ntt_transforms = 0;
        dc.ntt_alg_bytes = 0;
    }
    hipSetDevice(g.devs[0]->device);
    return ZK_OK;
}

API int zk_ntt_configure(const zk_ntt_opts* opts) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (opts)
        g.ntt_opts = *opts;
    else
        memset(&g.ntt_opts, 0, sizeof g.ntt_opts);
    return ZK_OK;
}

// entry points on device buffers: bind the calling thread to the owner of `a`, serialise the enqueue on that device
#define DEVICE_ENTRY(ptr)                       \
    {                                           \
        std::lock_guard<std::mutex> lk0(g.mu);  \
        ZK_TRY(require_init());                 \
    }                                           \
    DeviceCtx& dc = device_of(ptr);             \
    ZK_TRY(bind_device(dc));                    \
    std::lock_guard<std::mutex> lk(dc.mu)

API int zk_ntt_device(zk_field_t f, void* a, uint32_t log_n, const void* omega, int scale, void* stream) {
    if (!a || !omega || !aligned16(a)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> w;
        host_load(w, omega);
        return ntt_run<F>(dc, (int)f, (Fe<F>*)a, log_n, w, scale, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt(zk_field_t f, void* a_host, uint32_t log_n, const void* omega, int scale) {
    if (!a_host || !omega || log_n > 30) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    const size_t bytes = (size_t)32 << log_n;
    ZK_TRY(ws_get(dc.scratch_in, bytes));
    HIP_TRY(hipMemcpy(dc.scratch_in.p, a_host, bytes, hipMemcpyHostToDevice));
    FIELD_SWITCH(f, {
        Fe<F> w;
        host_load(w, omega);
        ZK_TRY(ntt_run<F>(dc, (int)f, (Fe<F>*)dc.scratch_in.p, log_n, w, scale, (hipStream_t)0));
    });
    HIP_TRY(hipStreamSynchronize((hipStream_t)0));
    HIP_TRY(hipMemcpy(a_host, dc.scratch_in.p, bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
}
API int zk_ntt_coset_device(zk_field_t f, void* a, uint32_t log_n, const void* omega, int scale, const void* g_pre,
                            const void* g_post, void* stream) {
    if (!a || !omega || !aligned16(a)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> w, gp, gq;
        host_load(w, omega);
        if (g_pre) host_load(gp, g_pre);
        if (g_post) host_load(gq, g_post);
        return ntt_run<F>(dc, (int)f, (Fe<F>*)a, log_n, w, scale, (hipStream_t)stream, g_pre ? &gp : nullptr, g_post ? &gq : nullptr);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt_extend_device(zk_field_t f, void* a, uint32_t log_n, uint32_t log_in, const void* omega, int scale, const void* g_pre,
                             const void* g_post, void* stream) {
    if (!a || !omega || !aligned16(a) || log_in > log_n || log_n > 30) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        if (log_n > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
        Fe<F> w, gp, gq;
        host_load(w, omega);
        if (g_pre) host_load(gp, g_pre);
        if (g_post) host_load(gq, g_post);
        if (log_n > 0 && log_in == 0) {   // a single coefficient: in_log = 0 means "all" to the pass kernel, so pad explicitly
            HIP_TRY(hipMemsetAsync((Fe<F>*)a + 1, 0, (((size_t)1 << log_n) - 1) * sizeof(Fe<F>), (hipStream_t)stream));
        }
        return ntt_run<F>(dc, (int)f, (Fe<F>*)a, log_n, w, scale, (hipStream_t)stream, g_pre ? &gp : nullptr, g_post ? &gq : nullptr, log_in);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt_oop_device(zk_field_t f, const void* src, void* dst, uint32_t log_n, uint32_t log_in, const void* omega, int scale, const void* g_pre,
                          const void* g_post, void* stream) {
    if (!src || !dst || !omega || !aligned16(src) || !aligned16(dst) || log_in > log_n || log_n > 30) return ZK_ERR_INVALID_ARG;
    if (src == dst) return zk_ntt_extend_device(f, dst, log_n, log_in, omega, scale, g_pre, g_post, stream);
    {   // the buffers must not overlap: the first pass reads src while later tiles of the same pass may already write dst
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + ((uintptr_t)32 << log_in), d0 = (uintptr_t)dst, d1 = d0 + ((uintptr_t)32 << log_n);
        if (s0 < d1 && d0 < s1) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(dst);
    FIELD_SWITCH(f, {
        if (log_n > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
        Fe<F> w, gp, gq;
        host_load(w, omega);
        if (g_pre) host_load(gp, g_pre);
        if (g_post) host_load(gq, g_post);
        if (log_n > 0 && log_in == 0) {   // a single coefficient (in_log = 0 means "all" to the pass kernel): pad explicitly, then in place
            HIP_TRY(hipMemcpyAsync(dst, src, sizeof(Fe<F>), hipMemcpyDeviceToDevice, (hipStream_t)stream));
            HIP_TRY(hipMemsetAsync((Fe<F>*)dst + 1, 0, (((size_t)1 << log_n) - 1) * sizeof(Fe<F>), (hipStream_t)stream));
            return ntt_run<F>(dc, (int)f, (Fe<F>*)dst, log_n, w, scale, (hipStream_t)stream, g_pre ? &gp : nullptr, g_post ? &gq : nullptr, log_in);
        }
        return ntt_run<F>(dc, (int)f, (Fe<F>*)dst, log_n, w, scale, (hipStream_t)stream, g_pre ? &gp : nullptr, g_post ? &gq : nullptr, log_in,
                          (const Fe<F>*)src);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_coset_mul_device(zk_field_t f, void* a, uint32_t log_n, const void* gm, void* stream) {
    if (!a || !gm || !aligned16(a)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> w;
        host_load(w, gm);
        return coset_run<F>(dc, (int)f, (Fe<F>*)a, log_n, w, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_coset_mul(zk_field_t f, void* a_host, uint32_t log_n, const void* gm) {
    if (!a_host || !gm || log_n > 30) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    const size_t bytes = (size_t)32 << log_n;
    ZK_TRY(ws_get(dc.scratch_in, bytes));
    HIP_TRY(hipMemcpy(dc.scratch_in.p, a_host, bytes, hipMemcpyHostToDevice));
    FIELD_SWITCH(f, {
        Fe<F> w;
        host_load(w, gm);
        ZK_TRY(coset_run<F>(dc, (int)f, (Fe<F>*)dc.scratch_in.p, log_n, w, (hipStream_t)0));
    });
    HIP_TRY(hipMemcpy(a_host, dc.scratch_in.p, bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
}

API int zk_vec_op_device(zk_field_t f, int op, void* a, const void* b, const void* c, uint64_t n, const void* scalar, void* stream) {
    if (op < 0 || op > 6 || (n && (!a || !aligned16(a)))) return ZK_ERR_INVALID_ARG;
    const bool needs_b = op == 0 || op == 1 || op == 2 || op == 6, needs_c = op == 6, needs_s = op == 3 || op == 6;
    if (n && ((needs_b && (!b || !aligned16(b))) || (needs_c && (!c || !aligned16(c))) || (needs_s && !scalar))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> s;
        fe_one(s);
        if (needs_s) host_load(s, scalar);
        return vec_op_run<F>((Fe<F>*)a, (const Fe<F>*)b, (const Fe<F>*)c, n, op, s, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_scale_periodic_device(zk_field_t f, void* a, uint64_t n, const void* table_host, uint32_t m, void* stream) {
    if ((n && (!a || !aligned16(a))) || !table_host) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, return scale_periodic_run<F>((Fe<F>*)a, n, (const Fe<F>*)table_host, m, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_groth16_witness_map_device(zk_field_t f, void* a, void* b, void* c, uint32_t log_m, void* stream) {
    if (!a || !b || !c || !aligned16(a) || !aligned16(b) || !aligned16(c)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, return witness_map_run<F>(dc, (int)f, (Fe<F>*)a, (Fe<F>*)b, (Fe<F>*)c, log_m, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

API int zk_r1cs_matrix_upload(zk_field_t f, const uint64_t* row_ptr, const uint32_t* col, const void* val, uint64_t n_rows, uint64_t n_cols,
                              uint64_t* handle_out) {
    if (!handle_out || !row_ptr || (int)f < 0 || (int)f > (int)ZK_FR_BLS12_381) return ZK_ERR_INVALID_ARG;
    const uint64_t nnz = row_ptr[n_rows];
    if (row_ptr[0] != 0 || (nnz && (!col || !val)) || n_cols >= (1ull << 32)) return ZK_ERR_INVALID_ARG;
    std::vector<uint64_t> long_rows;
    for (uint64_t i = 0; i < n_rows; i++) {
        if (row_ptr[i + 1] < row_ptr[i]) return ZK_ERR_INVALID_ARG;
        if (row_ptr[i + 1] - row_ptr[i] > R1CS_LONG_ROW) long_rows.push_back(i);
    }
    for (uint64_t k = 0; k < nnz; k++)
        if (col[k] >= n_cols) return ZK_ERR_INVALID_ARG;   // a mat-vec must never index past the assignment
    DEVICE_ENTRY(nullptr);
    R1csMatrix m;
    m.field = (int)f;
    m.n_rows = n_rows;
    m.n_cols = n_cols;
    m.nnz = nnz;
    m.n_long = long_rows.size();
    auto put = [&](void** dst, const void* src, size_t bytes) -> int {
        HIP_TRY(hipMalloc(dst, bytes ? bytes : 16));
        if (bytes) HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return ZK_OK;
    };
    int st = put(&m.row_ptr, row_ptr, (n_rows + 1) * 8);
    if (st == ZK_OK) st = put(&m.col, col, nnz * 4);
    if (st == ZK_OK) st = put(&m.val, val, nnz * 32);
    if (st == ZK_OK) st = put(&m.long_rows, long_rows.data(), long_rows.size() * 8);
    if (st != ZK_OK) {
        free_matrix(m);
        return st;
    }
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    const uint64_t h = g_next_mat++;
    g_mats[h] = m;
    *handle_out = h;
    return ZK_OK;
}
API int zk_r1cs_matrix_free(uint64_t handle) {
    DEVICE_ENTRY(nullptr);
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    auto it = g_mats.find(handle);
    if (it == g_mats.end()) return ZK_ERR_BAD_HANDLE;
    hipDeviceSynchronize();
    free_matrix(it->second);
    g_mats.erase(it);
    return ZK_OK;
}
static int find_matrix(uint64_t handle, R1csMatrix* out) {
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    auto it = g_mats.find(handle);
    if (it == g_mats.end()) return ZK_ERR_BAD_HANDLE;
    *out = it->second;
    return ZK_OK;
}
API int zk_r1cs_matvec_device(uint64_t matrix, const void* z, void* out, uint64_t out_len, void* stream) {
    if (!z || !out || !aligned16(z) || !aligned16(out)) return ZK_ERR_INVALID_ARG;
    R1csMatrix m;
    ZK_TRY(find_matrix(matrix, &m));
    DEVICE_ENTRY(nullptr);
    FIELD_SWITCH((zk_field_t)m.field, return r1cs_matvec_run<F>(m, (const Fe<F>*)z, (Fe<F>*)out, out_len, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_groth16_witness_map_r1cs_device(zk_field_t f, uint64_t ha, uint64_t hb, uint64_t hc, const void* z, uint64_t num_inputs,
                                           uint32_t log_m, void* a, void* b, void* c, void* stream) {
    if (!z || !a || !b || !c || !aligned16(z) || !aligned16(a) || !aligned16(b) || !aligned16(c) || log_m > 30) return ZK_ERR_INVALID_ARG;
    R1csMatrix ma, mb, mc;
    ZK_TRY(find_matrix(ha, &ma));
    ZK_TRY(find_matrix(hb, &mb));
    ZK_TRY(find_matrix(hc, &mc));
    const uint64_t m = 1ull << log_m, nc = ma.n_rows;
    if (ma.field != (int)f || mb.field != (int)f || mc.field != (int)f || mb.n_rows != nc || mc.n_rows != nc || nc + num_inputs > m ||
        num_inputs > ma.n_cols)
        return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    FIELD_SWITCH(f, {
        hipStream_t st = (hipStream_t)stream;
        ZK_TRY(r1cs_matvec_run<F>(ma, (const Fe<F>*)z, (Fe<F>*)a, m, st));
        ZK_TRY(r1cs_matvec_run<F>(mb, (const Fe<F>*)z, (Fe<F>*)b, m, st));
        ZK_TRY(r1cs_matvec_run<F>(mc, (const Fe<F>*)z, (Fe<F>*)c, m, st));
        // the input-consistency rows: a[num_constraints + j] = z[j]
        if (num_inputs) HIP_TRY(hipMemcpyAsync((Fe<F>*)a + nc, z, num_inputs * sizeof(Fe<F>), hipMemcpyDeviceToDevice, st));
        return witness_map_run<F>(dc, (int)f, (Fe<F>*)a, (Fe<F>*)b, (Fe<F>*)c, log_m, st);
    });
    return ZK_ERR_INVALID_ARG;
}

// ---- Groth16 key generation (ark-groth16 0.3 generator.rs generate_parameters)
// the matrix with its column-major companion, which is built on `st` at the handle's first transposed product
static int find_matrix_transposed(uint64_t handle, hipStream_t st, R1csMatrix* out) {
    std::lock_guard<std::mutex> lkm(g_mat_mu);
    auto it = g_mats.find(handle);
    if (it == g_mats.end()) return ZK_ERR_BAD_HANDLE;
    if (!it->second.t_ready) FIELD_SWITCH((zk_field_t)it->second.field, ZK_TRY(r1cs_transpose_run<F>(it->second, st)));
    *out = it->second;
    return ZK_OK;
}
API int zk_r1cs_matvec_transposed_device(uint64_t matrix, const void* x, uint64_t x_len, void* out, uint64_t out_len, void* stream) {
    if (!out || !aligned16(out) || (x_len && (!x || !aligned16(x)))) return ZK_ERR_INVALID_ARG;
    R1csMatrix m;
    ZK_TRY(find_matrix(matrix, &m));
    if (out_len < m.n_cols) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    ZK_TRY(find_matrix_transposed(matrix, (hipStream_t)stream, &m));
    FIELD_SWITCH((zk_field_t)m.field,
                 return r1cs_matvec_t_run<F>(m, (const Fe<F>*)x, x_len, (Fe<F>*)out, out_len, nullptr, 0, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_lagrange_coefficients_device(zk_field_t f, uint32_t log_m, const void* tau, void* out, void* zt_out, void* stream) {
    if (!tau || !out || !aligned16(out)) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        Fe<F> t, w, zt, s;
        host_load(t, tau);
        ZK_TRY(lagrange_consts<F>(log_m, t, &w, &zt, &s));   // tau in the domain is refused before the library is entered
    });
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> t, zt;
        host_load(t, tau);
        ZK_TRY(lagrange_run<F>(dc, (int)f, log_m, t, (Fe<F>*)out, &zt, (hipStream_t)stream));
        if (zt_out) host_store(zt_out, zt);
        return ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_groth16_qap_at_device(zk_field_t f, uint64_t ha, uint64_t hb, uint64_t hc, uint64_t num_inputs, uint32_t log_m, const void* tau, void* u,
                                 void* v, void* w, uint64_t n_vars, void* zt_out, void* stream) {
    if (!tau || !u || !v || !w || !aligned16(u) || !aligned16(v) || !aligned16(w) || log_m > 30) return ZK_ERR_INVALID_ARG;
    R1csMatrix ma, mb, mc;
    ZK_TRY(find_matrix(ha, &ma));
    ZK_TRY(find_matrix(hb, &mb));
    ZK_TRY(find_matrix(hc, &mc));
    const uint64_t m = 1ull << log_m, nc = ma.n_rows;
    if (ma.field != (int)f || mb.field != (int)f || mc.field != (int)f || mb.n_rows != nc || mc.n_rows != nc || nc + num_inputs > m ||
        num_inputs > n_vars || n_vars < ma.n_cols || n_vars < mb.n_cols || n_vars < mc.n_cols)
        return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        Fe<F> t, w0, zt, s;
        host_load(t, tau);
        ZK_TRY(lagrange_consts<F>(log_m, t, &w0, &zt, &s));
    });
    DEVICE_ENTRY(nullptr);
    hipStream_t st = (hipStream_t)stream;
    ZK_TRY(find_matrix_transposed(ha, st, &ma));
    ZK_TRY(find_matrix_transposed(hb, st, &mb));
    ZK_TRY(find_matrix_transposed(hc, st, &mc));
    FIELD_SWITCH(f, {
        Fe<F> t, zt;
        host_load(t, tau);
        ZK_TRY(groth16_qap_at_run<F>(dc, (int)f, ma, mb, mc, num_inputs, log_m, t, (Fe<F>*)u, (Fe<F>*)v, (Fe<F>*)w, n_vars, &zt, st));
        if (zt_out) host_store(zt_out, zt);
        return ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_groth16_key_scalars_device(zk_field_t f, const void* u, const void* v, const void* w, uint64_t n_vars, uint64_t num_inputs,
                                      uint32_t log_m, const void* alpha, const void* beta, const void* gamma, const void* delta, const void* tau,
                                      const void* zt, void* abc, void* h, void* stream) {
    if (!alpha || !beta || !gamma || !delta || !tau || !zt || log_m > 30 || num_inputs > n_vars) return ZK_ERR_INVALID_ARG;
    if (n_vars && (!u || !v || !w || !abc || !aligned16(u) || !aligned16(v) || !aligned16(w) || !aligned16(abc))) return ZK_ERR_INVALID_ARG;
    if (log_m && (!h || !aligned16(h))) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        Fe<F> g_, d, z;
        host_load(g_, gamma);
        host_load(d, delta);
        host_load(z, zt);
        if (log_m > (uint32_t)F::TWO_ADICITY || fe_is_zero(g_) || fe_is_zero(d) || fe_is_zero(z)) return ZK_ERR_INVALID_ARG;
    });
    DEVICE_ENTRY(abc);
    FIELD_SWITCH(f, {
        Fe<F> a, b, g_, d, t, z;
        host_load(a, alpha);
        host_load(b, beta);
        host_load(g_, gamma);
        host_load(d, delta);
        host_load(t, tau);
        host_load(z, zt);
        return groth16_key_scalars_run<F>(dc, (const Fe<F>*)u, (const Fe<F>*)v, (const Fe<F>*)w, n_vars, num_inputs, log_m, a, b, g_, d, t, z,
                                          (Fe<F>*)abc, (Fe<F>*)h, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}

// ---- halo2 prover steps beyond commit / FFT (include/zkcp_amd_prover.h)
API int zk_batch_invert_device(zk_field_t f, void* a, uint64_t n, void* stream) {
    if (n && (!a || !aligned16(a))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, return batch_invert_run<F>((Fe<F>*)a, n, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_prefix_product_device(zk_field_t f, const void* in, void* out, uint64_t n, const void* first, void* total_host, void* stream) {
    if (n && (!in || !out || !aligned16(in) || !aligned16(out))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> fst;
        fe_one(fst);
        if (first) host_load(fst, first);
        Fe<F>* total = nullptr;
        ZK_TRY(prefix_product_run<F>(dc, (const Fe<F>*)in, (Fe<F>*)out, n, fst, &total, (hipStream_t)stream));
        if (total_host) {
            HIP_TRY(hipMemcpyAsync(total_host, total, sizeof(Fe<F>), hipMemcpyDeviceToHost, (hipStream_t)stream));
            HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        }
        return ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_permutation_product_device(zk_field_t f, uint32_t ncols, const void* const* cols, const void* const* sigmas, uint32_t first_col,
                                            const void* beta, const void* gamma, const void* delta, uint32_t k, const void* z_first, void* z_out,
                                            void* z_last_host, void* stream) {
    if (!cols || !sigmas || !beta || !gamma || !delta || !z_out || !aligned16(z_out) || ncols == 0 || ncols > 8) return ZK_ERR_INVALID_ARG;
    for (uint32_t c = 0; c < ncols; c++)
        if (!cols[c] || !sigmas[c] || !aligned16(cols[c]) || !aligned16(sigmas[c])) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(z_out);
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY || k > 30) return ZK_ERR_INVALID_ARG;
        Fe<F> b, g_, d, fst, w;
        host_load(b, beta);
        host_load(g_, gamma);
        host_load(d, delta);
        fe_one(fst);
        if (z_first) host_load(fst, z_first);
        for (int i = 0; i < F::N; i++) w.v[i] = F::ROOT[i];
        for (uint32_t i = k; i < (uint32_t)F::TWO_ADICITY; i++) fe_sqr(w, w);
        return perm_product_run<F>(dc, (int)f, ncols, cols, sigmas, first_col, b, g_, d, k, w, fst, (Fe<F>*)z_out, z_last_host, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_lookup_product_device(zk_field_t f, const void* a, const void* s, const void* ap, const void* sp, const void* beta,
                                       const void* gamma, uint64_t n, void* z_out, void* z_last_host, void* stream) {
    if (!beta || !gamma || (n && (!a || !s || !ap || !sp || !z_out || !aligned16(a) || !aligned16(s) || !aligned16(ap) || !aligned16(sp) || !aligned16(z_out))))
        return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(z_out);
    FIELD_SWITCH(f, {
        Fe<F> b, g_, one;
        host_load(b, beta);
        host_load(g_, gamma);
        fe_one(one);
        return lookup_product_run<F>(dc, (const Fe<F>*)a, (const Fe<F>*)s, (const Fe<F>*)ap, (const Fe<F>*)sp, b, g_, n, one, (Fe<F>*)z_out,
                                     z_last_host, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
// [p, p + bytes) and [q, q + bytes) share an address
static bool ranges_overlap(const void* p, const void* q, uint64_t bytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + bytes && b < a + bytes;
}
API int zk_halo2_permute_expression_pair_device(zk_field_t f, const void* inputs_dev, const void* table_dev, uint64_t usable_rows, void* a_perm_dev,
                                                void* s_perm_dev, void* stream) {
    if (usable_rows >= (1ull << 31)) return ZK_ERR_INVALID_ARG;
    if (usable_rows) {
        const void* ptrs[4] = {inputs_dev, table_dev, a_perm_dev, s_perm_dev};
        for (const void* p : ptrs)
            if (!p || !aligned16(p)) return ZK_ERR_INVALID_ARG;
        const uint64_t bytes = usable_rows * 32;
        if (ranges_overlap(a_perm_dev, s_perm_dev, bytes) || ranges_overlap(a_perm_dev, inputs_dev, bytes) ||
            ranges_overlap(a_perm_dev, table_dev, bytes) || ranges_overlap(s_perm_dev, inputs_dev, bytes) ||
            ranges_overlap(s_perm_dev, table_dev, bytes))
            return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(a_perm_dev);
    FIELD_SWITCH(f, {
        int failed = 0;
        ZK_TRY(permute_expression_pair_run<F>(dc, (const Fe<F>*)inputs_dev, (const Fe<F>*)table_dev, (uint32_t)usable_rows, (Fe<F>*)a_perm_dev,
                                              (Fe<F>*)s_perm_dev, &failed, (hipStream_t)stream));
        return failed ? ZK_ERR_LOOKUP : ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
// ---- halo2 key generation: plonk/permutation/keygen.rs Assembly on the host (the walk of a cycle is sequential by definition),
// the permutation columns on the device (zk_keygen.inl)
namespace {
// Assembly { mapping, aux, sizes } over ncols x n cells, cell (c, r) at c * n + r.  mapping holds col << 32 | row, the form
// zk_halo2_assembly_mapping hands out; aux (the cycle's distinguished cell) and sizes are flat 32-bit cell indices / counts.
struct Halo2Assembly {
    uint64_t n = 0;
    uint32_t ncols = 0;
    std::vector<uint64_t> mapping;
    std::vector<uint32_t> aux, sizes;
    uint64_t flat(uint64_t packed) const { return (packed >> 32) * n + (packed & 0xffffffffull); }
    // Assembly::copy; false = Error::BoundsFailure (nothing changed)
    bool copy(uint32_t lc, uint32_t lr, uint32_t rc, uint32_t rr) {
        if (lc >= ncols || rc >= ncols || lr >= n || rr >= n) return false;
        uint64_t left = (uint64_t)lc * n + lr, right = (uint64_t)rc * n + rr;
        if (aux[left] == aux[right]) return true;                    // already in the same cycle
        if (sizes[aux[left]] < sizes[aux[right]]) std::swap(left, right);
        sizes[aux[left]] += sizes[aux[right]];                       // the left cycle absorbs the right one
        const uint32_t head = aux[left];
        uint64_t i = right;
        do {
            aux[i] = head;
            i = flat(mapping[i]);
        } while (i != right);
        std::swap(mapping[left], mapping[right]);
        return true;
    }
};
std::mutex g_asm_mu;
std::map<uint64_t, std::unique_ptr<Halo2Assembly>> g_asms;
uint64_t g_next_asm = 1;
}  // namespace

API int zk_halo2_assembly_new(uint64_t n, uint32_t ncols, uint64_t* handle_out) {
    if (!handle_out || n == 0 || ncols == 0 || n > (1ull << 32) || n * ncols >= (1ull << 32)) return ZK_ERR_INVALID_ARG;
    std::unique_ptr<Halo2Assembly> a;
    const uint64_t cells = n * ncols;
    try {
        a.reset(new Halo2Assembly());
        a->n = n;
        a->ncols = ncols;
        a->mapping.resize(cells);
        a->aux.resize(cells);
        a->sizes.assign(cells, 1u);
    } catch (const std::bad_alloc&) {
        return ZK_ERR_OOM;
    }
    for (uint32_t c = 0; c < ncols; c++)
        for (uint64_t r = 0; r < n; r++) {
            a->mapping[c * n + r] = ((uint64_t)c << 32) | r;
            a->aux[c * n + r] = (uint32_t)(c * n + r);
        }
    std::lock_guard<std::mutex> lk(g_asm_mu);
    const uint64_t h = g_next_asm++;
    g_asms[h] = std::move(a);
    *handle_out = h;
    return ZK_OK;
}
API int zk_halo2_assembly_copy(uint64_t handle, const uint32_t* quads, uint64_t count, uint64_t* applied_out) {
    if (applied_out) *applied_out = 0;
    if (count && !quads) return ZK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_asm_mu);
    auto it = g_asms.find(handle);
    if (it == g_asms.end()) return ZK_ERR_BAD_HANDLE;
    Halo2Assembly& a = *it->second;
    for (uint64_t q = 0; q < count; q++) {
        if (!a.copy(quads[4 * q], quads[4 * q + 1], quads[4 * q + 2], quads[4 * q + 3])) return ZK_ERR_INVALID_ARG;
        if (applied_out) *applied_out = q + 1;
    }
    return ZK_OK;
}
API int zk_halo2_assembly_mapping(uint64_t handle, void* mapping_out) {
    if (!mapping_out) return ZK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_asm_mu);
    auto it = g_asms.find(handle);
    if (it == g_asms.end()) return ZK_ERR_BAD_HANDLE;
    memcpy(mapping_out, it->second->mapping.data(), it->second->mapping.size() * sizeof(uint64_t));
    return ZK_OK;
}
API int zk_halo2_assembly_free(uint64_t handle) {
    std::lock_guard<std::mutex> lk(g_asm_mu);
    auto it = g_asms.find(handle);
    if (it == g_asms.end()) return ZK_ERR_BAD_HANDLE;
    g_asms.erase(it);
    return ZK_OK;
}
API int zk_halo2_permutation_sigmas_device(zk_field_t f, uint32_t k, uint32_t ncols, const void* mapping_dev, const void* delta,
                                           void* sigmas_dev, void* stream) {
    if (!mapping_dev || !delta || !sigmas_dev || !aligned16(mapping_dev) || !aligned16(sigmas_dev) || ncols == 0 || k > 30)
        return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
    });
    if (((uint64_t)ncols << k) >= (1ull << 32)) return ZK_ERR_INVALID_ARG;       // the assembly's own limit on the number of cells
    {   // 8 bytes per cell in, 32 out
        const uintptr_t m0 = (uintptr_t)mapping_dev, s0 = (uintptr_t)sigmas_dev, cells = (uintptr_t)ncols << k;
        if (m0 < s0 + cells * 32 && s0 < m0 + cells * 8) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(sigmas_dev);
    FIELD_SWITCH(f, {
        Fe<F> d, w;
        host_load(d, delta);
        for (int i = 0; i < F::N; i++) w.v[i] = F::ROOT[i];
        for (uint32_t i = k; i < (uint32_t)F::TWO_ADICITY; i++) fe_sqr(w, w);
        int bad = 0;
        ZK_TRY(perm_sigmas_run<F>(dc, (int)f, k, ncols, (const uint64_t*)mapping_dev, d, w, (Fe<F>*)sigmas_dev, &bad, (hipStream_t)stream));
        return bad ? ZK_ERR_INVALID_ARG : ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_inner_product_device(zk_field_t f, const void* a, const void* b, uint64_t n, void* out_host, void* stream) {
    if (!out_host || (n && (!a || !b || !aligned16(a) || !aligned16(b)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, return inner_product_run<F>(dc, (const Fe<F>*)a, (const Fe<F>*)b, n, out_host, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_muladd_device(zk_field_t f, void* a, const void* b, uint64_t n, const void* s, void* stream) {
    if (!s || (n && (!a || !b || !aligned16(a) || !aligned16(b)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> ss;
        host_load(ss, s);
        return vec_muladd_run<F>((Fe<F>*)a, (const Fe<F>*)a, (const Fe<F>*)b, n, ss, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_muladd_to_device(zk_field_t f, void* out, const void* a, const void* b, uint64_t n, const void* s, void* stream) {
    if (!s || (n && (!out || !a || !b || !aligned16(out) || !aligned16(a) || !aligned16(b)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> ss;
        host_load(ss, s);
        return vec_muladd_run<F>((Fe<F>*)out, (const Fe<F>*)a, (const Fe<F>*)b, n, ss, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_poly_eval_device(zk_field_t f, const void* c, uint64_t n, const void* x, void* out_host, void* stream) {
    return zk_poly_eval_batch_device(f, c, n, 1, n, x, out_host, stream);
}
API int zk_poly_eval_batch_device(zk_field_t f, const void* c, uint64_t n, uint32_t count, uint64_t stride_elems, const void* x, void* out_host,
                                  void* stream) {
    if (!out_host || !x || stride_elems < n || (n && count && (!c || !aligned16(c)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(c);
    FIELD_SWITCH(f, {
        Fe<F> xx;
        host_load(xx, x);
        return poly_eval_run<F>(dc, (const Fe<F>*)c, n, count, stride_elems, xx, (int)f, out_host, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_fold_many_device(zk_field_t f, void* out, const void* first, int64_t stride_elems, uint32_t count, uint64_t n, const void* s,
                                void* stream) {
    if (!s || count == 0 || (n && (!out || !first || !aligned16(out) || !aligned16(first)))) return ZK_ERR_INVALID_ARG;
    if (count > 1 && (stride_elems == 0 || (uint64_t)(stride_elems < 0 ? -stride_elems : stride_elems) < n)) return ZK_ERR_INVALID_ARG;
    {   // out may be one of the sources (every lane reads all of its inputs before it writes) or disjoint from all of them
        const intptr_t o = (intptr_t)out, len = (intptr_t)n * 32;
        for (uint32_t i = 0; i < count; i++) {
            const intptr_t a = (intptr_t)first + (intptr_t)i * stride_elems * 32;
            if (a != o && a < o + len && o < a + len) return ZK_ERR_INVALID_ARG;
        }
    }
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> ss;
        host_load(ss, s);
        return vec_fold_many_run<F>((Fe<F>*)out, (const Fe<F>*)first, stride_elems, count, n, ss, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ipa_fold_round_device(zk_field_t f, void* p, void* b, void* w, uint64_t half, uint64_t m0, const void* u, void* stream) {
    if (!u || (half && (!p || !b || !aligned16(p) || !aligned16(b))) || (w && !aligned16(w))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(p);
    FIELD_SWITCH(f, {
        Fe<F> uu;
        host_load(uu, u);
        if (fe_is_zero(uu)) return ZK_ERR_INVALID_ARG;
        return ipa_fold_round_run<F>((Fe<F>*)p, (Fe<F>*)b, (Fe<F>*)w, half, m0, uu, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_powers_device(zk_field_t f, void* out, uint64_t n, const void* x, void* stream) {
    if (!x || (n && (!out || !aligned16(out)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, {
        Fe<F> xx;
        host_load(xx, x);
        return vec_powers_run<F>(dc, (Fe<F>*)out, n, xx, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_kate_division_device(zk_field_t f, const void* a, void* q, uint64_t n, const void* x, void* stream) {
    if (!x || (n && (!a || !q || !aligned16(a) || !aligned16(q)))) return ZK_ERR_INVALID_ARG;
    if (a != q) {
        const uintptr_t a0 = (uintptr_t)a, q0 = (uintptr_t)q, len = (uintptr_t)n * 32;
        if (a0 < q0 + len && q0 < a0 + len) return ZK_ERR_INVALID_ARG;   // in place or disjoint
    }
    DEVICE_ENTRY(q);
    FIELD_SWITCH(f, {
        Fe<F> xx;
        host_load(xx, x);
        return kate_division_run<F>(dc, (const Fe<F>*)a, (Fe<F>*)q, n, xx, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_fold_device(zk_field_t f, void* a, uint64_t half, const void* c, void* stream) {
    if (!c || (half && (!a || !aligned16(a)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(a);
    FIELD_SWITCH(f, {
        Fe<F> cc;
        host_load(cc, c);
        return vec_fold_run<F>((Fe<F>*)a, half, cc, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ipa_fold_bases_device(zk_curve_t c, void* g_aff, uint64_t half, const void* u_mont, void* stream) {
    if (!u_mont || (half && (!g_aff || !aligned16(g_aff)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(g_aff);
    CURVE_SWITCH(c, {
        Fe<typename C::Fr> u;
        host_load(u, u_mont);
        fe_from_mont(u, u);
        return ipa_fold_bases_run<C>(dc, (Affine<C>*)g_aff, half, u, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt_points_device(zk_curve_t c, const void* src, void* dst, uint32_t log_n, const void* omega, int scale, void* stream) {
    if (!src || !dst || !omega || !aligned16(src) || !aligned16(dst) || log_n > ZK_NTT_POINTS_MAX_LOG_N) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(dst);
    CURVE_SWITCH(c, {
        Fe<typename C::Fr> w;
        host_load(w, omega);
        return ntt_points_run<C>(dc, (const Affine<C>*)src, (Affine<C>*)dst, log_n, w, scale ? 1 : 0, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt_points(zk_curve_t c, void* jac, uint32_t log_n, const void* omega, int scale) {
    if (!jac || !omega || log_n > ZK_NTT_POINTS_MAX_LOG_N) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    CURVE_SWITCH(c, {
        Fe<typename C::Fr> w;
        host_load(w, omega);
        return ntt_points_host_run<C>(dc, jac, log_n, w, scale ? 1 : 0);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ark_points_decode_checked_device(zk_curve_t c, const uint8_t* in_host, uint64_t n, int compressed, void* out_dev, uint64_t* first_bad_index,
                                            uint64_t* reason, void* stream) {
    if (first_bad_index) *first_bad_index = 0;
    if (reason) *reason = 0;
    if (c != ZK_BN254_G1 && c != ZK_BLS12_381_G1) return ZK_ERR_UNSUPPORTED;
    if (n == 0) return ZK_OK;
    if (!in_host || !out_dev || !aligned16(out_dev)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out_dev);
    CURVE_SWITCH(c, return points_decode_checked_run<C>(dc, in_host, n, compressed ? 1 : 0, (Affine<C>*)out_dev, first_bad_index, reason,
                                                       (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_ipa_collapse_device(zk_curve_t c, uint64_t handle, const void* w, uint64_t m0, uint64_t cur, void* g_out, void* stream) {
    return zk_ipa_collapse_range_device(c, handle, w, m0, cur, 0, cur, g_out, stream);
}
API int zk_ipa_collapse_range_device(zk_curve_t c, uint64_t handle, const void* w, uint64_t m0, uint64_t cur, uint64_t first, uint64_t count,
                                     void* g_out, void* stream) {
    if (!w || !g_out || !aligned16(w) || !aligned16(g_out)) return ZK_ERR_INVALID_ARG;
    const BasesCopy* bc = nullptr;
    uint64_t base_n = 0;
    DeviceCtx* dcp = nullptr;
    {
        std::lock_guard<std::mutex> lk0(g.mu);
        ZK_TRY(require_init());
        auto it = g.bases.find(handle);
        if (it == g.bases.end()) return ZK_ERR_BAD_HANDLE;
        if (it->second.curve != (int)c) return ZK_ERR_INVALID_ARG;
        dcp = &device_of(g_out);
        BasesCopy& mine = it->second.per_dev[dcp->index];
        base_n = it->second.n;
        // the second collapse over a large handle that was not rewritten in between builds its shift tables: a resident key pays once
        // (the first call runs the table-free path, so a handle that is collapsed once and dropped never pays); no memory, no tables
        if (mine.collapses++ >= 1 && !mine.shift && !mine.shift_failed && base_n >= ZK_SHIFT_AUTO_MIN && ipa_shift_tables_enabled() &&
            bind_device(*dcp) == ZK_OK) {
            int st = ZK_ERR_UNSUPPORTED;
            CURVE_SWITCH(c, st = bases_shifts_run<C>(mine, base_n));
            if (st != ZK_OK) {
                mine.shift_failed = true;
                (void)hipGetLastError();
            }
        }
        bc = &mine;
    }
    DeviceCtx& dc = *dcp;
    ZK_TRY(bind_device(dc));
    std::lock_guard<std::mutex> lk(dc.mu);
    CURVE_SWITCH(c, return ipa_collapse_run<C>(dc, *bc, base_n, (const Fe<typename C::Fr>*)w, m0, cur, first, count, (Affine<C>*)g_out,
                                               (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_ipa_virtual_scalars_device(zk_field_t f, const void* p, const void* w, uint64_t m0, uint64_t cur, void* sl, void* sr, void* stream) {
    if (!p || !w || !sl || !sr || !aligned16(p) || !aligned16(w) || !aligned16(sl) || !aligned16(sr)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(sl);
    FIELD_SWITCH(f, return ipa_virtual_scalars_run<F>((const Fe<F>*)p, (const Fe<F>*)w, (Fe<F>*)sl, (Fe<F>*)sr, m0, cur, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_ipa_round_device(zk_curve_t c, uint64_t handle, const void* p, const void* b, const void* w, uint64_t m0, uint64_t cur, void* s_dev,
                            void* lr_out, void* v_out, void* stream) {
    if (!p || !b || !w || !s_dev || !lr_out || !v_out || !aligned16(p) || !aligned16(b) || !aligned16(w) || !aligned16(s_dev))
        return ZK_ERR_INVALID_ARG;
    const int fi = zk_curve_scalar_field(c);
    if (fi < 0) return ZK_ERR_INVALID_ARG;
    const zk_field_t f = (zk_field_t)fi;
    size_t fbytes = 0;
    FIELD_SWITCH(f, fbytes = sizeof(Fe<F>));
    unsigned char* sl = (unsigned char*)s_dev;
    unsigned char* sr = sl + (size_t)m0 * fbytes;
    {
        DEVICE_ENTRY(s_dev);
        int st = ZK_ERR_INVALID_ARG;
        FIELD_SWITCH(f, st = ipa_round_begin_run<F>(dc, (const Fe<F>*)p, (const Fe<F>*)b, (const Fe<F>*)w, (Fe<F>*)sl, (Fe<F>*)sr, m0, cur,
                                                     (hipStream_t)stream));
        ZK_TRY(st);
    }
    // both MSMs over the resident generators (two library streams, forked behind the kernels above); dc.mu is not held here
    ZK_TRY(zk_msm_batch_device(c, handle, s_dev, m0, 2, m0, 1, nullptr, lr_out, stream));
    {
        DEVICE_ENTRY(s_dev);
        int st = ZK_ERR_INVALID_ARG;
        FIELD_SWITCH(f, st = ipa_round_end_run<F>(dc, (hipStream_t)stream, v_out, (unsigned char*)v_out + fbytes));
        return st;
    }
}
API int zk_ipa_update_weights_device(zk_field_t f, void* w, uint64_t m0, uint64_t bit, const void* u, void* stream) {
    if (!w || !u || !aligned16(w)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(w);
    FIELD_SWITCH(f, {
        Fe<F> uu;
        host_load(uu, u);
        return ipa_update_weights_run<F>((Fe<F>*)w, m0, bit, uu, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
// ---- halo2 opening verification: poly/commitment/verifier.rs compute_s on the device (zk_ipa_verify.inl), compute_b on host limbs
API int zk_halo2_ipa_s_device(zk_field_t f, uint32_t k, uint32_t count, const void* u_host, const void* init_host, void* s_dev, int accumulate,
                              void* stream) {
    if (!u_host || !init_host || !s_dev || !aligned16(u_host) || !aligned16(init_host) || !aligned16(s_dev) || count == 0 || k == 0)
        return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
    });
    DEVICE_ENTRY(s_dev);
    FIELD_SWITCH(f, return ipa_s_run<F>(dc, k, count, u_host, init_host, (Fe<F>*)s_dev, accumulate, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_ipa_compute_b(zk_field_t f, uint32_t k, const void* x, const void* u_host, void* out) {
    if (!x || !u_host || !out || k == 0) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
        Fe<F> cur, acc, one, t;
        host_load(cur, x);
        fe_one(one);
        acc = one;
        for (uint32_t j = k; j-- > 0;) {      // the last round's challenge goes with x^1: cur = x^(2^(k - 1 - j))
            host_load(t, (const unsigned char*)u_host + (size_t)j * sizeof(Fe<F>));
            fe_mul(t, t, cur);
            fe_add(t, t, one);
            fe_mul(acc, acc, t);
            fe_sqr(cur, cur);
        }
        host_store(out, acc);
    });
    return ZK_OK;
}
// ---- MockProver::verify on the device (zk_mock.inl) ----
API int zk_halo2_mock_eval_device(zk_field_t f, uint32_t k, const zk_expr_op* programs, const uint32_t* offsets, uint32_t n_programs,
                                  const void* const* cols, const uint64_t* poison_from, uint32_t n_cols, const void* consts, uint32_t n_consts,
                                  void* values_out, uint8_t* status_out, void* stream) {
    if (!programs || !offsets || !status_out || !aligned16(status_out) || (values_out && !aligned16(values_out)) || (n_cols && (!cols || !poison_from)) ||
        (n_consts && !consts) || k > 30 || n_programs == 0)
        return ZK_ERR_INVALID_ARG;
    if (values_out) {   // 32 bytes per entry in one output, 1 in the other
        const uintptr_t v0 = (uintptr_t)values_out, s0 = (uintptr_t)status_out, entries = (uintptr_t)n_programs << k;
        if (v0 < s0 + entries && s0 < v0 + entries * 32) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(status_out);
    FIELD_SWITCH(f, return mock_eval_run<F>(dc, k, programs, offsets, n_programs, cols, poison_from, n_cols, (const Fe<F>*)consts, n_consts,
                                            (Fe<F>*)values_out, status_out, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_mock_lookup_device(zk_field_t f, uint32_t k, const void* inputs_dev, const uint8_t* inputs_status, const void* table_dev,
                                    const uint8_t* table_status, uint64_t usable_rows, uint8_t* status_out, void* stream) {
    if (k > 30 || usable_rows > (1ull << k)) return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (k > (uint32_t)F::TWO_ADICITY) return ZK_ERR_INVALID_ARG;
    });
    if (usable_rows) {
        if (!inputs_dev || !table_dev || !status_out || !aligned16(inputs_dev) || !aligned16(table_dev)) return ZK_ERR_INVALID_ARG;
        const void* ins[4] = {inputs_dev, table_dev, inputs_status, table_status};
        const uint64_t bytes[4] = {usable_rows * 32, usable_rows * 32, usable_rows, usable_rows};
        for (int i = 0; i < 4; i++)
            if (ins[i]) {
                const uintptr_t a = (uintptr_t)ins[i], b = (uintptr_t)status_out;
                if (a < b + usable_rows && b < a + bytes[i]) return ZK_ERR_INVALID_ARG;
            }
    }
    DEVICE_ENTRY(status_out);
    FIELD_SWITCH(f, return mock_lookup_run<F>(dc, (const Fe<F>*)inputs_dev, inputs_status, (const Fe<F>*)table_dev, table_status, (uint32_t)usable_rows,
                                              status_out, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_mock_permutation_device(zk_field_t f, uint32_t k, uint32_t ncols, const void* const* cols, const uint64_t* poison_from,
                                         const void* mapping_dev, uint8_t* status_out, void* stream) {
    if (!cols || !poison_from || !mapping_dev || !status_out || !aligned16(mapping_dev) || ncols == 0 || k > 30) return ZK_ERR_INVALID_ARG;
    if (((uint64_t)ncols << k) >= (1ull << 32)) return ZK_ERR_INVALID_ARG;       // the assembly's own limit on the number of cells
    {
        const uintptr_t m0 = (uintptr_t)mapping_dev, s0 = (uintptr_t)status_out, cells = (uintptr_t)ncols << k;
        if (m0 < s0 + cells && s0 < m0 + cells * 8) return ZK_ERR_INVALID_ARG;
    }
    DEVICE_ENTRY(status_out);
    FIELD_SWITCH(f, {
        int bad = 0;
        ZK_TRY(mock_permutation_run<F>(dc, k, ncols, cols, poison_from, (const uint64_t*)mapping_dev, status_out, &bad, (hipStream_t)stream));
        return bad ? ZK_ERR_INVALID_ARG : ZK_OK;
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_halo2_mock_failures_device(const uint8_t* status_dev, uint64_t n_status, uint64_t cap, uint64_t* positions_out, uint8_t* kinds_out,
                                      uint64_t* total_out, void* stream) {
    if (!total_out || (n_status && (!status_dev || !aligned16(status_dev))) || (cap && n_status && (!positions_out || !kinds_out)))
        return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(status_dev);
    return mock_failures_run<PallasFp>(dc, status_dev, n_status, cap, positions_out, kinds_out, total_out, (hipStream_t)stream);   // (the bytes carry no field)
}
API int zk_expr_eval_device(zk_field_t f, const zk_expr_op* prog, uint32_t n_ops, const void* const* cols, uint32_t n_cols, const void* consts,
                            uint32_t n_consts, uint32_t log_n, uint32_t rot_scale, void* out, void* stream) {
    if (!prog || !out || !aligned16(out) || (n_cols && !cols) || (n_consts && !consts)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, return expr_eval_run<F>(dc, prog, n_ops, cols, n_cols, (const Fe<F>*)consts, n_consts, log_n, rot_scale, (Fe<F>*)out,
                                            (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

API int zk_expr_eval_lazy_device(zk_field_t f, const zk_expr_op* prog, uint32_t n_ops, const void* const* cols, uint32_t n_cols, const void* consts,
                                 uint32_t n_consts, uint32_t log_n, uint32_t rot_scale, void* out, void* stream) {
    if (!prog || !out || !aligned16(out) || (n_cols && !cols) || (n_consts && !consts)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(out);
    FIELD_SWITCH(f, return expr_eval_lazy_run<F>(dc, prog, n_ops, cols, n_cols, (const Fe<F>*)consts, n_consts, log_n, rot_scale, (Fe<F>*)out,
                                                 (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}

API int zk_expr_specialised_source(zk_field_t f, const zk_expr_op* prog, uint32_t n_ops, uint32_t n_cols, uint32_t n_consts, char* out, uint64_t cap,
                                   uint64_t* len_out) {
    if (!prog || !len_out) return ZK_ERR_INVALID_ARG;
    std::string src;
    int st = ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, st = expr_source_run<F>(prog, n_ops, n_cols, n_consts, src));
    ZK_TRY(st);
    *len_out = src.size();
    if (out && cap) {
        const size_t k = src.size() < cap - 1 ? src.size() : (size_t)cap - 1;
        memcpy(out, src.data(), k);
        out[k] = 0;
    }
    return ZK_OK;
}

API int zk_expr_configure(int jit_mode) {
    if (jit_mode < 0 || jit_mode > 2) return ZK_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g.mu);
    g.expr_jit = jit_mode;
    return ZK_OK;
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

API int zk_groth16_prepare_inputs(zk_curve_t g1, uint64_t gamma_abc_tail_bases, const void* gamma_abc0_affine, uint64_t gamma_abc_len,
                                  const void* inputs_mont_dev, uint64_t n_inputs, void* g_ic_affine_out, void* stream) {
    if (!gamma_abc0_affine || !g_ic_affine_out || (g1 != ZK_BN254_G1 && g1 != ZK_BLS12_381_G1)) return ZK_ERR_INVALID_ARG;
    if (n_inputs + 1 != gamma_abc_len) return ZK_ERR_INVALID_ARG;   // upstream: SynthesisError::MalformedVerifyingKey; nothing is launched
    CURVE_SWITCH(g1, {
        Jacobian<C> sum;
        XYZZ<C> acc;
        xyzz_set_inf(acc);
        if (n_inputs) {
            ZK_TRY(zk_msm_device(g1, gamma_abc_tail_bases, inputs_mont_dev, n_inputs, 1, nullptr, &sum, stream));
            jac_to_xyzz(acc, sum);
        }
        Affine<C> first, r;
        memcpy(&first, gamma_abc0_affine, 2 * 4 * coord_words<C>());
        xyzz_add_mixed(acc, first);
        xyzz_to_affine(r, acc);
        memcpy(g_ic_affine_out, &r, 2 * 4 * coord_words<C>());
    });
    return ZK_OK;
}

API int zk_fixed_base_mul_device(zk_curve_t c, const void* d_scalars, uint64_t n, void* d_out, void* stream) {
    if (n == 0) return ZK_OK;
    if (!d_scalars || !d_out || !aligned16(d_scalars) || !aligned16(d_out) || n >= (1ull << 31)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(d_out);
    CURVE_SWITCH(c, return fixed_base_run<C>((const Fe<typename C::Fr>*)d_scalars, n, (Affine<C>*)d_out, (hipStream_t)stream));
    return ZK_OK;
}

API int zk_fixed_base_msm_device(zk_curve_t c, const void* base_affine_mont, const void* d_scalars, uint64_t n, int scalars_are_montgomery,
                                 void* d_out, void* stream) {
    if (n == 0) return ZK_OK;
    if (!d_scalars || !d_out || !aligned16(d_scalars) || !aligned16(d_out) || n >= (1ull << 31)) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(d_out);
    CURVE_SWITCH(c, {
        Affine<C> base;
        if (base_affine_mont)
            memcpy(&base, base_affine_mont, 2 * 4 * coord_words<C>());
        else
            curve_generator(base);
        return fixed_base_msm_run<C>(dc, base, (const Fe<typename C::Fr>*)d_scalars, n, scalars_are_montgomery ? 1 : 0, (Affine<C>*)d_out,
                                     (hipStream_t)stream);
    });
    return ZK_OK;
}

// ---- Poseidon, the Merkle tree over it, the ElGamal stream (zk_poseidon.inl) ----
API int zk_poseidon_create(zk_field_t f, uint32_t width, uint32_t rate, uint32_t rate_offset, uint32_t full_rounds, uint32_t partial_rounds,
                           uint64_t alpha, const void* ark_mont_host, const void* mds_mont_host, const void* init_mont_host, uint64_t* handle_out) {
    if (!ark_mont_host || !mds_mont_host || !handle_out || width < POSEIDON_MIN_WIDTH || width > POSEIDON_MAX_WIDTH || rate == 0 || rate > width ||
        rate_offset > width - rate || (full_rounds & 1) || full_rounds > POSEIDON_MAX_ROUNDS || partial_rounds > POSEIDON_MAX_ROUNDS ||
        full_rounds + partial_rounds == 0 || full_rounds + partial_rounds > POSEIDON_MAX_ROUNDS || alpha == 0)
        return ZK_ERR_INVALID_ARG;
    const size_t n_ark = (size_t)(full_rounds + partial_rounds) * width, n_mds = (size_t)width * width;
    FIELD_SWITCH(f, {
        if (!canonical_elems<F>(ark_mont_host, n_ark) || !canonical_elems<F>(mds_mont_host, n_mds) ||
            (init_mont_host && !canonical_elems<F>(init_mont_host, width)))
            return ZK_ERR_INVALID_ARG;
    });
    auto e = std::make_shared<PoseidonEntry>();
    e->field = (int)f;
    e->shape = PoseidonShape{width, rate, rate_offset, full_rounds, partial_rounds, (uint32_t)(63 - __builtin_clzll(alpha)), alpha};
    e->tbl.assign((n_ark + n_mds + width) * 4, 0);
    memcpy(e->tbl.data(), ark_mont_host, n_ark * 32);
    memcpy(e->tbl.data() + n_ark * 4, mds_mont_host, n_mds * 32);
    if (init_mont_host) memcpy(e->tbl.data() + (n_ark + n_mds) * 4, init_mont_host, (size_t)width * 32);
    std::lock_guard<std::mutex> lk(g_pos_mu);
    *handle_out = g_next_poseidon;
    g_poseidon[g_next_poseidon++] = e;
    return ZK_OK;
}
API int zk_poseidon_free(uint64_t handle) {
    std::lock_guard<std::mutex> lk0(g.mu);
    std::lock_guard<std::mutex> lk(g_pos_mu);
    auto it = g_poseidon.find(handle);
    if (it == g_poseidon.end()) return ZK_ERR_BAD_HANDLE;
    free_poseidon_tables(*it->second);
    g_poseidon.erase(it);
    return ZK_OK;
}
API int zk_poseidon_permute_host(uint64_t handle, void* states_mont_host, uint64_t count) {
    if (!states_mont_host) return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    FIELD_SWITCH((zk_field_t)e->field, return poseidon_permute_host_run<F>(e->shape, (const Fe<F>*)e->tbl.data(), (Fe<F>*)states_mont_host, count));
    return ZK_ERR_INVALID_ARG;
}
API int zk_poseidon_hash_host(uint64_t handle, const void* in_mont_host, uint32_t arity, uint64_t count, void* out_mont_host) {
    if (!in_mont_host || !out_mont_host || arity == 0 || arity > POSEIDON_MAX_ARITY || count > (1ull << 48) ||
        spans_overlap(in_mont_host, count * arity * 32, out_mont_host, count * 32))
        return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    FIELD_SWITCH((zk_field_t)e->field, return poseidon_hash_host_run<F>(e->shape, (const Fe<F>*)e->tbl.data(), (const Fe<F>*)in_mont_host, arity, count,
                                                                        (Fe<F>*)out_mont_host));
    return ZK_ERR_INVALID_ARG;
}
API int zk_poseidon_permute_device(uint64_t handle, void* states_dev, uint64_t count, void* stream) {
    if (!states_dev || !aligned16(states_dev) || count > (1ull << 48)) return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    DEVICE_ENTRY(states_dev);
    const void* tbl = nullptr;
    ZK_TRY(poseidon_table(*e, dc, &tbl));
    FIELD_SWITCH((zk_field_t)e->field, return poseidon_permute_run<F>(e->shape, (const Fe<F>*)tbl, (Fe<F>*)states_dev, count, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_poseidon_hash_device(uint64_t handle, const void* in_dev, uint32_t arity, uint64_t count, void* out_dev, void* stream) {
    if (!in_dev || !out_dev || !aligned16(in_dev) || !aligned16(out_dev) || arity == 0 || arity > POSEIDON_MAX_ARITY || count > (1ull << 48) ||
        spans_overlap(in_dev, count * arity * 32, out_dev, count * 32))
        return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    DEVICE_ENTRY(out_dev);
    const void* tbl = nullptr;
    ZK_TRY(poseidon_table(*e, dc, &tbl));
    FIELD_SWITCH((zk_field_t)e->field,
                 return poseidon_hash_run<F>(e->shape, (const Fe<F>*)tbl, (const Fe<F>*)in_dev, arity, count, (Fe<F>*)out_dev, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_poseidon_merkle_tree_device(uint64_t handle, const void* leaves_dev, uint32_t leaf_arity, uint32_t log_n, void* nodes_dev, void* stream) {
    if (!leaves_dev || !nodes_dev || !aligned16(leaves_dev) || !aligned16(nodes_dev) || leaf_arity == 0 || leaf_arity > POSEIDON_MAX_ARITY || log_n == 0 ||
        log_n > MERKLE_MAX_LOG_N || spans_overlap(leaves_dev, ((uint64_t)leaf_arity << log_n) * 32, nodes_dev, ((2ull << log_n) - 1) * 32))
        return ZK_ERR_INVALID_ARG;
    std::shared_ptr<PoseidonEntry> e;
    ZK_TRY(find_poseidon(handle, &e));
    DEVICE_ENTRY(nodes_dev);
    const void* tbl = nullptr;
    ZK_TRY(poseidon_table(*e, dc, &tbl));
    FIELD_SWITCH((zk_field_t)e->field,
                 return poseidon_tree_run<F>(e->shape, (const Fe<F>*)tbl, (const Fe<F>*)leaves_dev, leaf_arity, log_n, (Fe<F>*)nodes_dev, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_merkle_paths_device(zk_field_t f, const void* nodes_dev, uint32_t log_n, const uint64_t* indices_host, uint64_t count, void* out_dev,
                               void* stream) {
    if (!nodes_dev || !indices_host || !out_dev || !aligned16(nodes_dev) || !aligned16(out_dev) || log_n == 0 || log_n > MERKLE_MAX_LOG_N ||
        count > (1ull << 32) || spans_overlap(nodes_dev, ((2ull << log_n) - 1) * 32, out_dev, count * log_n * 32) || (int)f < 0 ||
        (int)f > (int)ZK_FR_BLS12_381)
        return ZK_ERR_INVALID_ARG;
    for (uint64_t c = 0; c < count; c++)
        if (indices_host[c] >> log_n) return ZK_ERR_INVALID_ARG;       // a lane must never read past the tree
    DEVICE_ENTRY(nodes_dev);
    FIELD_SWITCH(f, return merkle_paths_run<F>((const Fe<F>*)nodes_dev, log_n, indices_host, count, (Fe<F>*)out_dev, (hipStream_t)stream));
    return ZK_ERR_INVALID_ARG;
}
API int zk_vec_add_scalar_device(zk_field_t f, void* out_dev, const void* a_dev, uint64_t n, const void* scalar_mont_host, void* stream) {
    if (!out_dev || !a_dev || !scalar_mont_host || !aligned16(out_dev) || !aligned16(a_dev) || n > (1ull << 48) ||
        (out_dev != a_dev && spans_overlap(out_dev, n * 32, a_dev, n * 32)))
        return ZK_ERR_INVALID_ARG;
    FIELD_SWITCH(f, {
        if (!canonical_elems<F>(scalar_mont_host, 1)) return ZK_ERR_INVALID_ARG;
    });
    DEVICE_ENTRY(out_dev);
    FIELD_SWITCH(f, {
        Fe<F> s;
        host_load(s, scalar_mont_host);
        return vec_add_scalar_run<F>((Fe<F>*)out_dev, (const Fe<F>*)a_dev, n, s, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}

}  // extern "C"
