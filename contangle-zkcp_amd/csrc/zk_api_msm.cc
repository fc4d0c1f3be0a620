// C ABI, curve side: the MSM job pool (submit -> collect), the fan-out of one MSM or one batch over the devices of the
// process, and the entry points over curve points (fixed-base, IPA generator folding, point DFT, checked decode).
#include "zk_api_common.h"
#include "zk_msm_decl.h"
#include "zk_ntt_decl.h"

using namespace zk;

namespace {
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
    if (status == ZK_OK)
        status = [&]() -> int {   // (the lambda takes the macro's `default: return`: the slot is released below)
            CURVE_SWITCH(c, return CurveLaunch<C>::msm_enqueue(*job, bc, (const Fe<typename C::Fr>*)d_scalars, n, mont, tu));
            return ZK_ERR_INVALID_ARG;
        }();
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

size_t jac_bytes(zk_curve_t c) {
    CURVE_SWITCH(c, return (size_t)3 * 4 * coord_words<C>());   // (only reached with a curve that find_bases or a job has validated)
    return 0;
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
}  // namespace

extern "C" {

API int zk_msm_window_bits(zk_curve_t c, uint64_t n, int requested) {
    CURVE_SWITCH(c, (void)sizeof(C); return msm_pick_c(n, requested));
    return ZK_ERR_INVALID_ARG;
}
API int zk_msm_window_count(zk_curve_t c, uint64_t n, int window_bits) {
    CURVE_SWITCH(c, return msm_windows<C>(msm_pick_c(n, window_bits)));
    return ZK_ERR_INVALID_ARG;
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
    CURVE_SWITCH(c, per_job = CurveLaunch<C>::msm_batch_size(be->per_dev[dc.index], n, tu, dc.num_cus));
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

API int zk_ipa_fold_bases_device(zk_curve_t c, void* g_aff, uint64_t half, const void* u_mont, void* stream) {
    if (!u_mont || (half && (!g_aff || !aligned16(g_aff)))) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(g_aff);
    CURVE_SWITCH(c, {
        Fe<typename C::Fr> u;
        host_load(u, u_mont);
        fe_from_mont(u, u);
        return CurveLaunch<C>::ipa_fold_bases_run(dc, (Affine<C>*)g_aff, half, u, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt_points_device(zk_curve_t c, const void* src, void* dst, uint32_t log_n, const void* omega, int scale, void* stream) {
    if (!src || !dst || !omega || !aligned16(src) || !aligned16(dst) || log_n > ZK_NTT_POINTS_MAX_LOG_N) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(dst);
    CURVE_SWITCH(c, {
        Fe<typename C::Fr> w;
        host_load(w, omega);
        return CurveLaunch<C>::ntt_points_run(dc, (const Affine<C>*)src, (Affine<C>*)dst, log_n, w, scale ? 1 : 0, (hipStream_t)stream);
    });
    return ZK_ERR_INVALID_ARG;
}
API int zk_ntt_points(zk_curve_t c, void* jac, uint32_t log_n, const void* omega, int scale) {
    if (!jac || !omega || log_n > ZK_NTT_POINTS_MAX_LOG_N) return ZK_ERR_INVALID_ARG;
    DEVICE_ENTRY(nullptr);
    CURVE_SWITCH(c, {
        Fe<typename C::Fr> w;
        host_load(w, omega);
        return CurveLaunch<C>::ntt_points_host_run(dc, jac, log_n, w, scale ? 1 : 0);
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
    CURVE_SWITCH(c, return CurveLaunch<C>::points_decode_checked_run(dc, in_host, n, compressed ? 1 : 0, (Affine<C>*)out_dev, first_bad_index, reason,
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
            CURVE_SWITCH(c, st = CurveLaunch<C>::bases_shifts_run(mine, base_n));
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
    CURVE_SWITCH(c, return CurveLaunch<C>::ipa_collapse_run(dc, *bc, base_n, (const Fe<typename C::Fr>*)w, m0, cur, first, count, (Affine<C>*)g_out,
                                               (hipStream_t)stream));
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
        FIELD_SWITCH(f, st = FieldLaunch<F>::ipa_round_begin_run(dc, (const Fe<F>*)p, (const Fe<F>*)b, (const Fe<F>*)w, (Fe<F>*)sl, (Fe<F>*)sr, m0, cur,
                                                     (hipStream_t)stream));
        ZK_TRY(st);
    }
    // both MSMs over the resident generators (two library streams, forked behind the kernels above); dc.mu is not held here
    ZK_TRY(zk_msm_batch_device(c, handle, s_dev, m0, 2, m0, 1, nullptr, lr_out, stream));
    {
        DEVICE_ENTRY(s_dev);
        int st = ZK_ERR_INVALID_ARG;
        FIELD_SWITCH(f, st = FieldLaunch<F>::ipa_round_end_run(dc, (hipStream_t)stream, v_out, (unsigned char*)v_out + fbytes));
        return st;
    }
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
    CURVE_SWITCH(c, return CurveLaunch<C>::fixed_base_run((const Fe<typename C::Fr>*)d_scalars, n, (Affine<C>*)d_out, (hipStream_t)stream));
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
        return CurveLaunch<C>::fixed_base_msm_run(dc, base, (const Fe<typename C::Fr>*)d_scalars, n, scalars_are_montgomery ? 1 : 0, (Affine<C>*)d_out,
                                     (hipStream_t)stream);
    });
    return ZK_OK;
}

}  // extern "C"
