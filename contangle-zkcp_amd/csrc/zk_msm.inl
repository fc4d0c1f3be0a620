// MSM launch sequence and host tail: members of CurveLaunch<C> (zk_msm_decl.h).  Included by zk_msm_inst.cc, once per curve.
#pragma once
#include "zk_internal.h"
#include "zk_msm_decl.h"
#include "zk_host64.h"
#include "zk_msm_kernels.h"
namespace zk {
// ------------------------------------------------------------------ MSM
inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Host tail of one MSM (per curve): Horner over the job's windows, high to low, then the shift by 2^(c*w0) -- on 64-bit
// host limbs, from the per-window partial sums the job copied to pinned memory.  Runs in zk_msm_collect, i.e. after the
// caller has had the chance to enqueue the next MSM: the GPU never waits for it.
// Partial sums leave the device in the kernels' view CK of the curve (C itself, or its F29 view) and are brought back to the
// caller's limb form here: r = partial i of scalar vector bt.
// ZK_MSM_FLAG_DEVICE_PARTIALS: the reduction's last kernel also wrote every partial in the caller's limb form (and the
// stages of that conversion); the result is built from those, and each is checked against the host's conversion of
// the raw partial -- prof.reserved = mismatching partials | first differing stage << 24 | its component << 28
template <class C, class CK>
void msm_load_partial(MsmJob& job, uint32_t bt, size_t i, HostXYZZ<C>& r) {
    const size_t nparts = (size_t)job.batch * job.nw * job.per, gi = (size_t)bt * job.nw * job.per + i;
    const XYZZ<CK>* host = (const XYZZ<CK>*)job.host_partials;
    XYZZ<C> ps;
    partial_to_std<C>(ps, host[gi]);
    if (job.dev_std) {
        const XYZZ<C>* host_std = (const XYZZ<C>*)(host + nparts);
        const uint32_t* host_dbg = (const uint32_t*)(host_std + nparts);
        if (memcmp(&ps, &host_std[gi], sizeof ps) != 0) {
            if ((job.prof.reserved & 0xffffff) == 0) {
                constexpr uint32_t DW = partial_dbg_words<CK>();
                int stage = 5, comp = 0;
                if constexpr (DW != 0) {
                    std::vector<uint32_t> mine(DW);
                    partial_std_stages<CK>(host[gi], mine.data());
                    const uint32_t* dev = host_dbg + gi * DW;
                    using F = typename CK::Fq;
                    constexpr uint32_t L = F29<F>::L, N = F::N, PER = 3 * L + N;
                    for (uint32_t k = 0; k < DW && stage == 5; k++)
                        if (mine[k] != dev[k]) {
                            comp = (int)(k / PER);
                            const uint32_t o = k % PER;
                            stage = o < L ? 1 : o < 2 * L ? 2 : o < 3 * L ? 3 : 4;
                            fprintf(stderr, "zk: device partial %zu differs: component %d, stage %d (1 norm, 2 product, 3 canonical, 4 packed), word %u\n",
                                    gi, comp, stage, o);
                            const uint32_t b0 = (uint32_t)comp * PER;
                            for (uint32_t q = 0; q < PER; q++)
                                fprintf(stderr, "   [%2u] host %08x dev %08x%s\n", q, mine[b0 + q], dev[b0 + q], mine[b0 + q] != dev[b0 + q] ? "  <--" : "");
                        }
                }
                job.prof.reserved |= (stage << 24) | (comp << 28);
            }
            job.prof.reserved++;
        }
        ps = host_std[gi];
    }
    to_host<C>(r, ps);
}

// row / column form: one axis of a window is nb blocks x (W, S) starting at partial b0; axis total = sum_u W_u + TL sum_u u S_u
template <class C, class CK>
void msm_axis_sum(MsmJob& job, uint32_t bt, size_t b0, uint32_t nb, HostXYZZ<C>& tot) {
    HostXYZZ<C> run, acc, hp;
    msm_load_partial<C, CK>(job, bt, b0, tot);
    if (nb <= 1) return;
    XYZZ<C> inf;
    xyzz_set_inf(inf);
    to_host<C>(run, inf);
    to_host<C>(acc, inf);
    for (uint32_t u = nb - 1; u >= 1; u--) {
        msm_load_partial<C, CK>(job, bt, b0 + 2 * (size_t)u + 1, hp);
        xyzz_add(run, hp);
        xyzz_add(acc, run);        // sum_u u S_u
        msm_load_partial<C, CK>(job, bt, b0 + 2 * (size_t)u, hp);
        xyzz_add(tot, hp);
    }
    for (uint32_t k = 0; k < job.log_tl; k++) xyzz_dbl(acc);
    xyzz_add(tot, acc);
}

// the job's events -> its profile (t0: when the host tail began)
inline void msm_read_profile(MsmJob& job, double t0) {
    job.prof.host_tail_ms = (float)(now_ms() - t0);
    hipEventElapsedTime(&job.prof.digits_ms, job.ev[0], job.ev[1]);
    hipEventElapsedTime(&job.prof.hist_ms, job.ev[1], job.ev[2]);
    hipEventElapsedTime(&job.prof.scatter_ms, job.ev[2], job.ev[3]);
    hipEventElapsedTime(&job.prof.accumulate_ms, job.ev[3], job.ev[4]);
    job.prof.accumulate_kernel_ms = 0;          // the accumulate kernel of every window group
    for (int gi = 0; gi < job.groups; gi++) {
        float ms = 0;
        hipEventElapsedTime(&ms, job.acc_ev[2 * gi], job.acc_ev[2 * gi + 1]);
        job.prof.accumulate_kernel_ms += ms;
    }
    hipEventElapsedTime(&job.prof.reduce_ms, job.ev[4], job.ev[5]);
    hipEventElapsedTime(&job.prof.total_ms, job.ev[0], job.ev[5]);
    job.prof.total_ms += job.prof.host_tail_ms;
    job.prof.groups = job.groups;
}

template <class C, class CK>
int msm_finish_impl(MsmJob& job, void* out_jac) {
    const size_t out_bytes = 3 * sizeof(uint32_t) * coord_words<C>();
    double t0 = 0;
    if (!job.empty) {
        HIP_TRY(hipEventSynchronize(job.ev[6]));
        t0 = now_ms();
    }
    for (uint32_t bt = 0; bt < job.batch; bt++) {      // one result per scalar vector of the job
        Jacobian<C> result;
        XYZZ<C> total;
        xyzz_set_inf(total);
        if (!job.empty) {
            HostXYZZ<C> htotal, hp;
            to_host<C>(htotal, total);
            for (int w = job.nw - 1; w >= 0; w--) {
                const size_t base = (size_t)w * job.per;
                // axes form: acc 2^c + (2^lc rows + columns) = (acc 2^(c - lc) + rows) 2^lc + columns -- no extra doublings
                for (int k = 0; k < (job.axes ? job.c - (int)job.log_cols : job.c); k++) xyzz_dbl(htotal);
                if (!job.axes) {
                    for (uint32_t i = 0; i < job.per; i++) {
                        msm_load_partial<C, CK>(job, bt, base + i, hp);
                        xyzz_add(htotal, hp);
                    }
                    continue;
                }
                // per window [row blocks | column blocks] x (W, S); window total = 2^lc rows + columns
                msm_axis_sum<C, CK>(job, bt, base, job.row_blocks, hp);
                xyzz_add(htotal, hp);
                for (uint32_t k = 0; k < job.log_cols; k++) xyzz_dbl(htotal);
                msm_axis_sum<C, CK>(job, bt, base + 2 * (size_t)job.row_blocks, job.col_blocks, hp);
                xyzz_add(htotal, hp);
            }
            for (int k = 0; k < job.c * job.w0; k++) xyzz_dbl(htotal);
            from_host<C>(total, htotal);
        }
        xyzz_to_jacobian(result, total);
        memcpy((unsigned char*)out_jac + (size_t)bt * out_bytes, &result, out_bytes);
    }
    if (!job.empty) msm_read_profile(job, t0);
    return ZK_OK;
}

// ---- enqueue: plan (zk_msm_plan.h), allocate, launch
template <class C, class CK>
constexpr MsmView msm_view() {
    return {(uint32_t)sizeof(XYZZ<CK>), (uint32_t)sizeof(XYZZ<C>), tree_lanes<CK>(), (uint32_t)msm_acc_waves<CK>(), partial_dbg_words<CK>(),
            ViewBase<CK>::LAZY};
}
template <class T>
T* ws_at(const DevBuf& b, size_t at = 0) {
    return (T*)((unsigned char*)b.p + at);
}
#define MSM_LAUNCH(kernel, l, ...) ZK_LAUNCH(kernel, (l).grid, (l).block, (l).lds, st, __VA_ARGS__)

// grow the job's workspaces to what one window group asks for (ws_get never shrinks: groups share them)
inline int msm_reserve(MsmJob& job, const MsmPlan& p) {
    ZK_TRY(ws_get(job.counts, p.counts_bytes));
    ZK_TRY(ws_get(job.blockcnt, p.blockcnt_bytes));
    ZK_TRY(ws_get(job.stage_idx, p.stage_idx_bytes));
    ZK_TRY(ws_get(job.stage_low, p.stage_low_bytes));
    ZK_TRY(ws_get(job.digits, p.digits_bytes));
    ZK_TRY(ws_get(job.sorted, p.sorted_bytes));
    ZK_TRY(ws_get(job.buckets, p.buckets_bytes));
    if (p.subacc_bytes) ZK_TRY(ws_get(job.subacc, p.subacc_bytes));
    ZK_TRY(ws_get(job.queue, p.queue_bytes));
    ZK_TRY(ws_get(job.seg_out, p.seg_out_bytes));
    if (p.hot_bytes) ZK_TRY(ws_get(job.hot, p.hot_bytes));
    ZK_TRY(ws_get(job.part_a, p.part_a_bytes));
    ZK_TRY(ws_get(job.part_b, p.part_b_bytes));
    if (p.part_std_bytes) ZK_TRY(ws_get(job.part_std, p.part_std_bytes));
    return ZK_OK;
}

// bucket reduction of one window group: buckets -> p.per partial sums per window; *out = where they are
template <class C, class CK>
int msm_launch_reduce(MsmJob& job, const MsmPlan& p, const XYZZ<CK>* buckets, XYZZ<CK>** out) {
    hipStream_t st = job.stream;
    if (p.axes) {
        // row / column sums (zk_msm_kernels.h, MsmAxes)
        const MsmAxes& A = p.A;
        XYZZ<CK>* part = ws_at<XYZZ<CK>>(job.part_a);
        XYZZ<CK>* elem = ws_at<XYZZ<CK>>(job.part_b);
        MSM_LAUNCH((msm_axis_partials_kernel<CK>), p.axis_partials, buckets, part, A);
        MSM_LAUNCH((msm_axis_fold_kernel<CK>), p.axis_fold, (const XYZZ<CK>*)part, elem, A, p.fold_rows);
        using Std = XYZZ<typename ViewBase<CK>::type>;
        if (p.dev_std) {
            // [raw partials | converted partials | conversion stages], copied to the host as one block
            *out = ws_at<XYZZ<CK>>(job.part_std);
            MSM_LAUNCH((msm_axis_weighted_kernel<CK, true>), p.axis_weighted, (const XYZZ<CK>*)elem, *out, A, p.row_blocks, p.col_blocks,
                       ws_at<Std>(job.part_std, p.std_at), ws_at<uint32_t>(job.part_std, p.dbg_at));
        } else {
            *out = ws_at<XYZZ<CK>>(job.part_b, p.part_b_out_at);
            MSM_LAUNCH((msm_axis_weighted_kernel<CK>), p.axis_weighted, (const XYZZ<CK>*)elem, *out, A, p.row_blocks, p.col_blocks, (Std*)nullptr,
                       (uint32_t*)nullptr);
        }
        return ZK_OK;
    }
    // slice form (ZK_MSM_FLAG_SLICE_REDUCE): running sums + windowed multiplier per slice, then the tree sums, ping-pong
    XYZZ<CK>* cur = ws_at<XYZZ<CK>>(job.part_a);
    XYZZ<CK>* nxt = ws_at<XYZZ<CK>>(job.part_b);
    MSM_LAUNCH((msm_reduce_kernel<CK>), p.slices, buckets, cur, p.sh.nbk, p.L, p.spw, p.nslices);
    for (int k = 0; k < p.nsum; k++) {
        MSM_LAUNCH((msm_sum_kernel<CK>), p.sum[k].launch, (const XYZZ<CK>*)cur, nxt, p.sum[k].per, p.sum[k].per_out, p.sum[k].E);
        std::swap(cur, nxt);
    }
    *out = cur;
    return ZK_OK;
}

// C: the curve of the ABI call.  CK: the view the kernels compute in.  bases: device array of StoredAffine<CK>.
// One window group of the job, planned and with its workspaces reserved: group `gi`, whose windows start `woff` windows into
// the job's range -- the whole pipeline of DESIGN section 5 (sort, accumulate, reduction, copy of the partial sums) on
// job.stream; no host synchronisation.
template <class C, class CK>
int msm_launch_group(MsmJob& job, const MsmPlan& p, const StoredAffine<CK>* bases, const Fe<typename C::Fr>* d_scalars, int mont, int gi, int woff) {
    hipStream_t st = job.stream;
    MsmShape sh = p.sh;
    sh.mont = mont;
    uint32_t* counts = ws_at<uint32_t>(job.counts);
    uint32_t* offs = ws_at<uint32_t>(job.counts, p.offs_at);
    uint32_t* order = ws_at<uint32_t>(job.counts, p.order_at);
    uint32_t* wg_total = ws_at<uint32_t>(job.counts, p.wg_total_at);
    uint32_t* region_base = ws_at<uint32_t>(job.counts, p.region_base_at);
    uint32_t* blockcnt = ws_at<uint32_t>(job.blockcnt);
    uint32_t* stage_idx = ws_at<uint32_t>(job.stage_idx);
    uint16_t* stage_low = ws_at<uint16_t>(job.stage_low);
    uint32_t* sorted = ws_at<uint32_t>(job.sorted);
    XYZZ<CK>* buckets = ws_at<XYZZ<CK>>(job.buckets);
    XYZZ<CK>* acc_out = sh.split_log > 0 ? ws_at<XYZZ<CK>>(job.subacc) : buckets;
    MsmQueue* q = ws_at<MsmQueue>(job.queue);
    MsmSeg* seg_list = ws_at<MsmSeg>(job.queue, p.seg_list_at);
    uint32_t* big_list = ws_at<uint32_t>(job.queue, p.big_list_at);
    XYZZ<CK>* seg_out = ws_at<XYZZ<CK>>(job.seg_out);
    uint32_t* hot_flag = p.hot_help ? ws_at<uint32_t>(job.hot) : nullptr;
    uint32_t* hot_list = p.hot_help ? ws_at<uint32_t>(job.hot, p.hot_list_at) : nullptr;
    uint32_t* gcur = p.hot_help ? ws_at<uint32_t>(job.hot, p.gcur_at) : nullptr;
    hipEvent_t* ev = job.ev;   // [0] begin, [1] counted, [2] staged, [3] sorted, [4] accumulated, [5] reduced, [6] partials on the host
    if (gi == 0) HIP_TRY(hipEventRecord(ev[0], st));

    // ---- sort: partition the digits by (window, bucket range), then counting-sort every region in LDS
    if (p.pre)
        MSM_LAUNCH((msm_digits_pre_kernel<C>), p.digits, d_scalars, sh, ws_at<uint32_t>(job.digits), blockcnt);
    else
        MSM_LAUNCH((msm_digits_kernel<C>), p.digits, d_scalars, sh, ws_at<uint16_t>(job.digits), blockcnt);
    MSM_LAUNCH((msm_region_scan_kernel<void>), p.region_scan, blockcnt, p.nblocks, wg_total);
    MSM_LAUNCH((msm_region_base_kernel<void>), p.region_base, (const uint32_t*)wg_total, p.nreg, region_base);
    HIP_TRY(hipEventRecord(ev[1], st));
    if (p.pre)
        MSM_LAUNCH((msm_stage_kernel<uint32_t>), p.stage, (const uint32_t*)job.digits.p, sh, (const uint32_t*)blockcnt, (const uint32_t*)wg_total,
                   (const uint32_t*)region_base, p.nblocks, stage_idx, stage_low);
    else
        MSM_LAUNCH((msm_stage_kernel<uint16_t>), p.stage, (const uint16_t*)job.digits.p, sh, (const uint32_t*)blockcnt, (const uint32_t*)wg_total,
                   (const uint32_t*)region_base, p.nblocks, stage_idx, stage_low);
    HIP_TRY(hipEventRecord(ev[2], st));
    // hot regions are histogrammed (pass 0) and scattered (pass 1) by p.hot_slices workgroups each, around the sort kernel
    if (p.hot_help) {
        HIP_TRY(hipMemsetAsync(counts, 0, (size_t)p.nbuckets * 4, st));
        MSM_LAUNCH((msm_hot_list_kernel<void>), p.hot_list, (const uint32_t*)wg_total, p.nreg, p.chunk_limit, hot_flag, hot_list);
        MSM_LAUNCH((msm_hot_kernel<void>), p.hot, (const uint32_t*)stage_idx, (const uint16_t*)stage_low, sh, (const uint32_t*)region_base,
                   (const uint32_t*)wg_total, (const uint32_t*)hot_list, counts, gcur, sorted, 0, p.hot_slices);
    }
    MSM_LAUNCH((msm_sort_kernel<void>), p.sort, (const uint32_t*)stage_idx, (const uint16_t*)stage_low, sh, (const uint32_t*)region_base,
               (const uint32_t*)wg_total, counts, offs, order, sorted, p.cap, p.chunk_limit, (const uint32_t*)hot_flag, gcur);
    if (p.hot_help)
        MSM_LAUNCH((msm_hot_kernel<void>), p.hot, (const uint32_t*)stage_idx, (const uint16_t*)stage_low, sh, (const uint32_t*)region_base,
                   (const uint32_t*)wg_total, (const uint32_t*)hot_list, counts, gcur, sorted, 1, p.hot_slices);
    HIP_TRY(hipMemsetAsync(q, 0, sizeof(MsmQueue), st));
    HIP_TRY(hipEventRecord(ev[3], st));   // [3] -> [7] brackets the accumulate kernel alone (per group: acc_ev)
    HIP_TRY(hipEventRecord(job.acc_ev[2 * gi], st));

    // ---- persistent accumulate: lanes stream buckets, largest first; oversized buckets go to the cooperative segment
    // kernels (fixed grids over device-side lists, no host round trip)
    MSM_LAUNCH((msm_accumulate_kernel<CK>), p.accumulate, bases, (const uint32_t*)sorted, (const uint32_t*)offs, (const uint32_t*)counts,
               (const uint32_t*)order, acc_out, sh, q, seg_list, big_list);
    HIP_TRY(hipEventRecord(ev[7], st));
    HIP_TRY(hipEventRecord(job.acc_ev[2 * gi + 1], st));
    if (sh.split_log > 0) MSM_LAUNCH((msm_combine_sub_kernel<CK>), p.combine_sub, (const XYZZ<CK>*)acc_out, buckets, p.nbuckets, sh.split_log);
    MSM_LAUNCH((msm_accumulate_big_kernel<CK>), p.accumulate_big, bases, (const uint32_t*)sorted, (const MsmQueue*)q, (const MsmSeg*)seg_list, seg_out);
    MSM_LAUNCH((msm_combine_big_kernel<CK>), p.combine_big, (const MsmQueue*)q, (const uint32_t*)big_list, (const uint32_t*)counts,
               (const XYZZ<CK>*)seg_out, buckets, sh.seg);
    HIP_TRY(hipEventRecord(ev[4], st));

    // ---- bucket reduction, then the per-window partial sums go to the host
    XYZZ<CK>* cur = nullptr;
    ZK_TRY((msm_launch_reduce<C, CK>(job, p, buckets, &cur)));
    HIP_TRY(hipEventRecord(ev[5], st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync((unsigned char*)job.host_partials + (size_t)woff * p.per * p.pbytes1, cur, p.hbytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev[6], st));
    return ZK_OK;
}

// Enqueues every kernel of the MSM and the copy of the per-window partial sums on job.stream and returns; no host
// synchronisation (workspace growth aside).  Every window group is planned first: a shape the kernels cannot index is refused
// before a workspace grows, an event is created or anything is enqueued; then the workspaces of all groups are reserved, then
// the groups are launched (window groups: msm_plan_groups).
template <class C, class CK>
int msm_enqueue_impl(MsmJob& job, const StoredAffine<CK>* bases, const Fe<typename C::Fr>* d_scalars, uint64_t n, int mont, const MsmTuning& tu) {
    memset(&job.prof, 0, sizeof job.prof);
    job.dev_std = false;
    job.finish = &msm_finish_impl<C, CK>;
    job.empty = true;
    job.alg_bytes = 0;
    const int c = msm_pick_c(n, tu.window_bits, tu.precomputed);
    const int nwin = msm_windows<C>(c);
    int w0 = 0, w1 = nwin;
    if (!(tu.w0 == 0 && tu.w1 == 0)) {
        w0 = tu.w0;
        w1 = tu.w1;
        if (w0 < 0 || w1 > nwin || w0 > w1) return ZK_ERR_INVALID_ARG;
    }
    job.c = c;
    job.w0 = w0;
    job.nw = w1 - w0;
    job.batch = tu.batch ? tu.batch : 1;
    job.prof.window_bits = c;
    job.prof.windows_total = nwin;
    job.prof.windows_done = w1 - w0;
    job.prof.limb_bits = CK::EXT >= 29 ? 29 : 32;
    job.groups = 1;
    if (n == 0 || w1 <= w0) return ZK_OK;
    const MsmGroups groups = msm_plan_groups(w1 - w0, tu);
    const int ng = groups.ng, gw = groups.gw;
    job.groups = ng;
    std::vector<MsmPlan> plans(ng);
    auto group_begin = [&](int gi) { return w0 + gi * gw; };
    auto group_end = [&](int gi) { return group_begin(gi) + gw < w1 ? group_begin(gi) + gw : w1; };
    for (int gi = 0; gi < ng; gi++)
        ZK_TRY(msm_plan(plans[gi], n, c, nwin, group_begin(gi), group_end(gi), tu, job.dc->num_cus, msm_view<C, CK>()));
    const double bytes_per_window = (double)job.batch * (double)n * (sizeof(Fe<typename C::Fr>) + sizeof(Affine<C>));
    const MsmPlan& p0 = plans[0];
    for (const MsmPlan& p : plans) ZK_TRY(msm_reserve(job, p));
    // one host buffer for the partial sums of all groups (groups: batch == 1, no diagnostic form)
    const size_t hbytes_job = ng > 1 ? (size_t)(w1 - w0) * p0.per * p0.pbytes1 : p0.hbytes;
    if (job.host_cap < hbytes_job) {
        if (job.host_partials) hipHostFree(job.host_partials);
        job.host_partials = nullptr;
        job.host_cap = 0;
        HIP_TRY(hipHostMalloc(&job.host_partials, hbytes_job + 4096, 0));
        job.host_cap = hbytes_job + 4096;
    }
    if (!job.have_events) {
        for (auto& e : job.ev) HIP_TRY(hipEventCreate(&e));
        job.have_events = true;
    }
    while (job.acc_ev.size() < 2 * (size_t)ng) {      // one bracket of the accumulate kernel per window group
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        job.acc_ev.push_back(e);
    }
    for (int gi = 0; gi < ng; gi++) {
        ZK_TRY((msm_launch_group<C, CK>(job, plans[gi], bases, d_scalars, mont, gi, gi * gw)));
        job.alg_bytes += bytes_per_window * (double)(group_end(gi) - group_begin(gi)) / (double)nwin;
    }
    // what the host tail reads: the reduction form is the same in every group, `per` the last group's
    const MsmPlan& pl = plans[ng - 1];
    if (p0.pre) job.nw = 1;
    job.axes = pl.axes;
    job.dev_std = pl.dev_std;
    job.row_blocks = pl.row_blocks;
    job.col_blocks = pl.col_blocks;
    job.log_cols = pl.A.log_cols;
    job.log_tl = pl.log_tl;
    job.per = pl.per;
    job.empty = false;
    return ZK_OK;
}

// every curve runs its bucket arithmetic in the lazy-limb view (Pallas, Vesta, BN254: 9 x 29-bit limbs; BLS12-381: 14 x 28;
// G2 as pairs of those); zk_msm_opts.limb_bits = 32 forces the saturated 32-bit path
template <class C>
constexpr bool has_f29() {
    return C::EXT == 1 || C::EXT == 2;
}
template <class C>
int CurveLaunch<C>::bases_prepare_run(BasesCopy& bc, uint64_t n) {
    bc.dev29 = nullptr;
    if constexpr (has_f29<C>()) {
        if (n == 0) return ZK_OK;
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(StoredAffine<F29View<C>>) * n));
        ZK_LAUNCH((bases_to29_kernel<C>), (unsigned)((n + 255) / 256), 256, 0, (hipStream_t)0, (const Affine<C>*)bc.dev,
                  (StoredAffine<F29View<C>>*)d, n);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize((hipStream_t)0) != hipSuccess) {
            hipFree(d);
            return ZK_ERR_HIP;
        }
        bc.dev29 = d;
    }
    return ZK_OK;
}

// rows x n packed lazy-limb points [2^(bits w)] P_i, w < rows, built over the resident copy and stored into *slot (whose old
// table is freed first)
template <class C>
int bases_multiples_run(BasesCopy& bc, uint64_t n, uint32_t bits, uint32_t rows, void** slot) {
    if constexpr (has_f29<C>()) {
        if (n == 0 || n * (uint64_t)rows >= (1ull << 31)) return ZK_ERR_UNSUPPORTED;
        if (*slot) hipFree(*slot);
        *slot = nullptr;
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(StoredAffine<F29View<C>>) * n * rows));
        ZK_LAUNCH((bases_precompute_kernel<C>), (unsigned)((n + 63) / 64), 64, 0, (hipStream_t)0, (const Affine<C>*)bc.dev,
                  (StoredAffine<F29View<C>>*)d, (uint32_t)n, bits, rows);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize((hipStream_t)0) != hipSuccess) {
            hipFree(d);
            return ZK_ERR_HIP;
        }
        *slot = d;
        return ZK_OK;
    }
    return ZK_ERR_UNSUPPORTED;
}

// the table of window multiples for the one-bucket-set form (zk_bases_precompute): nwin * n points
template <class C>
int CurveLaunch<C>::bases_precompute_run(BasesCopy& bc, uint64_t n, int c) {
    const int nwin = msm_windows<C>(c);
    ZK_TRY(bases_multiples_run<C>(bc, n, (uint32_t)c, (uint32_t)nwin, &bc.pre));
    bc.pre_c = c;
    bc.pre_w = nwin;
    return ZK_OK;
}

// the shift tables of the generator collapse (zk_bases_precompute_shifts): the same kernel with 64-bit "windows", [4][n] points
template <class C>
int CurveLaunch<C>::bases_shifts_run(BasesCopy& bc, uint64_t n) {
    return bases_multiples_run<C>(bc, n, 64u, (uint32_t)ZK_SHIFT_TABLES, &bc.shift);
}

template <class C>
int CurveLaunch<C>::bases_refresh_run(const BasesCopy& bc, uint64_t offset, uint64_t count, hipStream_t st) {
    if constexpr (has_f29<C>()) {
        if (!bc.dev29 || count == 0) return ZK_OK;
        ZK_LAUNCH((bases_to29_kernel<C>), (unsigned)((count + 255) / 256), 256, 0, st, (const Affine<C>*)bc.dev + offset,
                  (StoredAffine<F29View<C>>*)bc.dev29 + offset, count);
        HIP_TRY(hipGetLastError());
    }
    return ZK_OK;
}

// every curve runs its bucket arithmetic in the lazy-limb view unless opts.limb_bits = 32 asks for the saturated words
template <class C>
int CurveLaunch<C>::msm_enqueue(MsmJob& job, const BasesCopy& bc, const Fe<typename C::Fr>* d_scalars, uint64_t n, int mont, const MsmTuning& tu) {
    if constexpr (has_f29<C>()) {
        if (tu.precomputed) {
            if (!bc.pre || tu.base_offset != 0 || bc.pre_c != msm_pick_c(n, tu.window_bits, true) || bc.pre_w != msm_windows<C>(bc.pre_c))
                return ZK_ERR_INVALID_ARG;
            return msm_enqueue_impl<C, F29View<C>>(job, (const StoredAffine<F29View<C>>*)bc.pre, d_scalars, n, mont, tu);
        }
        if (bc.dev29 && tu.limb_bits != 32)
            return msm_enqueue_impl<C, F29View<C>>(job, (const StoredAffine<F29View<C>>*)bc.dev29 + tu.base_offset, d_scalars, n, mont, tu);
    }
    return msm_enqueue_impl<C, C>(job, (const Affine<C>*)bc.dev + tu.base_offset, d_scalars, n, mont, tu);
}

template <class C>
uint32_t CurveLaunch<C>::msm_batch_size(const BasesCopy& bc, uint64_t n, const MsmTuning& tu, int num_cus) {
    const int c = msm_pick_c(n, tu.window_bits, tu.precomputed), nwin = msm_windows<C>(c);
    const bool whole = tu.w0 == 0 && tu.w1 == 0;
    // (an empty window range makes an empty job whatever its batch: sized as one window)
    const int w0 = whole ? 0 : tu.w0, w1 = whole ? nwin : tu.w1 > tu.w0 ? tu.w1 : tu.w0 + 1;
    MsmView v = msm_view<C, C>();
    if constexpr (has_f29<C>())
        if (tu.precomputed || (bc.dev29 && tu.limb_bits != 32)) v = msm_view<C, F29View<C>>();
    return msm_plan_batch(n, c, nwin, w0, w1, tu, num_cus, v);
}

template <class C>
int CurveLaunch<C>::fixed_base_run(const Fe<typename C::Fr>* d_scalars, uint64_t n, Affine<C>* d_out, hipStream_t st) {
    ZK_LAUNCH((fixed_base_mul_kernel<C>), (unsigned)((n + 63) / 64), 64, 0, st, d_scalars, d_out, (uint32_t)n);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}
// ark-ec 0.3 FixedBaseMSM (window table + multi_scalar_mul) + batch_normalization_into_affine for one base
template <class C>
int CurveLaunch<C>::fixed_base_msm_run(DeviceCtx& dc, const Affine<C>& base, const Fe<typename C::Fr>* d_scalars, uint64_t n, int mont, Affine<C>* d_out,
                                       hipStream_t st) {
    const uint32_t entries = (uint32_t)fb_windows<C>() * FB_ROW;
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));   // table and temporaries belong to the caller's stream
    ZK_TRY(ws_get(ss->fb_table, (size_t)entries * sizeof(Affine<C>)));
    ZK_TRY(ws_get(ss->fb_tmp, (size_t)n * sizeof(XYZZ<C>)));
    Affine<C>* table = (Affine<C>*)ss->fb_table.p;
    XYZZ<C>* tmp = (XYZZ<C>*)ss->fb_tmp.p;
    ZK_LAUNCH((fixed_base_table_kernel<C>), (entries + 63) / 64, 64, 0, st, base, table, entries);
    ZK_LAUNCH((fixed_base_msm_kernel<C>), (unsigned)((n + 63) / 64), 64, 0, st, (const Affine<C>*)table, d_scalars, tmp, (uint32_t)n, mont);
    const uint64_t lanes = (n + FB_K - 1) / FB_K;
    ZK_LAUNCH((xyzz_batch_to_affine_kernel<C>), (unsigned)((lanes + 63) / 64), 64, 0, st, (const XYZZ<C>*)tmp, d_out, (uint32_t)n);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}
// ---- GLV decomposition of a scalar (64-bit limbs; constants from tools/gen_glv.py): on the host for the fold's shared scalar, in
// ecfft_twiddle_kernel for the twiddles of the point FFT ----
namespace glv {
ZK_HD void mul_lo256(uint64_t* r, const uint64_t* a, const uint64_t* b) {   // (a * b) mod 2^256
    uint64_t t[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        unsigned __int128 c = 0;
        for (int j = 0; i + j < 4; j++) {
            c += (unsigned __int128)a[i] * b[j] + t[i + j];
            t[i + j] = (uint64_t)c;
            c >>= 64;
        }
    }
    for (int i = 0; i < 4; i++) r[i] = t[i];
}
ZK_HD void sub256(uint64_t* r, const uint64_t* a, const uint64_t* b) {
    unsigned __int128 br = 0;
    for (int i = 0; i < 4; i++) {
        unsigned __int128 x = (unsigned __int128)a[i] - b[i] - (uint64_t)br;
        r[i] = (uint64_t)x;
        br = (x >> 64) & 1;
    }
}
ZK_HD void neg256(uint64_t* r, const uint64_t* a) {
    const uint64_t z[4] = {0, 0, 0, 0};
    sub256(r, z, a);
}
// c = (k * g) >> 384 for k < 2^256, g < 2^320
ZK_HD void mulhi384(uint64_t* c, const uint64_t* k, const uint64_t* g5) {
    uint64_t t[9] = {0};
    for (int i = 0; i < 4; i++) {
        unsigned __int128 cy = 0;
        for (int j = 0; j < 5; j++) {
            cy += (unsigned __int128)k[i] * g5[j] + t[i + j];
            t[i + j] = (uint64_t)cy;
            cy >>= 64;
        }
        t[i + 5] = (uint64_t)cy;
    }
    c[0] = t[6];
    c[1] = t[7];
    c[2] = t[8];
    c[3] = 0;
}
}  // namespace glv

template <class C>
ZK_HD bool glv_decompose(const Fe<typename C::Fr>& u_canonical, FoldScalar& out) {
    if constexpr (Glv<C>::HAS) {
        using G = Glv<C>;
        uint64_t k[4], c1[4], c2[4], t[4], k1[4], k2[4];
        for (int i = 0; i < 4; i++) k[i] = (uint64_t)u_canonical.v[2 * i] | ((uint64_t)u_canonical.v[2 * i + 1] << 32);
        glv::mulhi384(c1, k, G::G1);
        glv::mulhi384(c2, k, G::G2);
        if (G::G1_NEG) glv::neg256(c1, c1);
        if (G::G2_NEG) glv::neg256(c2, c2);
        // k1 = k - c1 a1 - c2 a2 ; k2 = -c1 b1 - c2 b2      (mod 2^256, two's complement; the results are ~129-bit)
        glv::mul_lo256(t, c1, G::A1);
        glv::sub256(k1, k, t);
        glv::mul_lo256(t, c2, G::A2);
        glv::sub256(k1, k1, t);
        glv::mul_lo256(k2, c1, G::B1);
        glv::mul_lo256(t, c2, G::B2);
        {
            unsigned __int128 cy = 0;
            for (int i = 0; i < 4; i++) {
                cy += (unsigned __int128)k2[i] + t[i];
                k2[i] = (uint64_t)cy;
                cy >>= 64;
            }
        }
        glv::neg256(k2, k2);
        out.neg1 = (int)(k1[3] >> 63);
        out.neg2 = (int)(k2[3] >> 63);
        if (out.neg1) glv::neg256(k1, k1);
        if (out.neg2) glv::neg256(k2, k2);
        if (k1[3] | k2[3] | (k1[2] >> 2) | (k2[2] >> 2)) return false;   // not short: fall back to the plain chain
        for (int i = 0; i < 4; i++) {
            out.k1[2 * i] = (uint32_t)k1[i];
            out.k1[2 * i + 1] = (uint32_t)(k1[i] >> 32);
            out.k2[2 * i] = (uint32_t)k2[i];
            out.k2[2 * i + 1] = (uint32_t)(k2[i] >> 32);
        }
        out.glv = 1;
        return true;
    }
    return false;
}

// g[i] <- affine(g[i] + [u] g[i + half]) for i < half (u canonical)
template <class C>
int CurveLaunch<C>::ipa_fold_bases_run(DeviceCtx& dc, Affine<C>* gens, uint64_t half, const Fe<typename C::Fr>& u_canonical, hipStream_t st) {
    if (half == 0) return ZK_OK;
    if (half >= (1ull << 31)) return ZK_ERR_UNSUPPORTED;
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    ZK_TRY(ws_get(ss->fb_tmp, (size_t)half * sizeof(XYZZ<C>)));
    XYZZ<C>* tmp = (XYZZ<C>*)ss->fb_tmp.p;
    FoldScalar ks;
    memset(&ks, 0, sizeof ks);
    if (!glv_decompose<C>(u_canonical, ks)) {
        memset(&ks, 0, sizeof ks);
        for (int i = 0; i < C::Fr::N && i < 8; i++) ks.k1[i] = u_canonical.v[i];
    }
    ks.top_bit = -1;
    for (int b = 255; b >= 0; b--)
        if (((ks.k1[b >> 5] | ks.k2[b >> 5]) >> (b & 31)) & 1) {
            ks.top_bit = b;
            break;
        }
    ZK_LAUNCH((ipa_fold_bases_kernel<C>), (unsigned)((half + 63) / 64), 64, 0, st, (const Affine<C>*)gens, tmp, (uint32_t)half, ks);
    const uint64_t lanes = (half + FB_K - 1) / FB_K;
    ZK_LAUNCH((xyzz_batch_to_affine_kernel<C>), (unsigned)((lanes + 63) / 64), 64, 0, st, (const XYZZ<C>*)tmp, gens, (uint32_t)half);
    HIP_TRY(hipGetLastError());
    return ZK_OK;
}
// G'[i] = sum_{t < T} W_t G0[t cur + i] for first <= i < first + count <= cur (T = m0 / cur): what r = log2 T literal folds would
// have left in generators [first, first + count) (a rank's share of the survivors, or all of them) (zk_msm_kernels.h, "Several IPA rounds of generator folding at once").  w_dev: the weight vector of
// the fold-free rounds; only W[t cur] is read (the weights do not depend on i).
template <class C>
int CurveLaunch<C>::ipa_collapse_run(DeviceCtx& dc, const BasesCopy& bc, uint64_t base_n, const Fe<typename C::Fr>* w_dev, uint64_t m0, uint64_t cur,
                                     uint64_t first, uint64_t count, Affine<C>* g_out, hipStream_t st) {
    using Fr = typename C::Fr;
    using CK = F29View<C>;
    if (cur == 0 || m0 == 0 || (m0 & (m0 - 1)) || (cur & (cur - 1)) || cur > m0 || m0 > base_n) return ZK_ERR_INVALID_ARG;
    if (m0 >= (1ull << 31) || m0 / cur > 4096 || !bc.dev29) return ZK_ERR_UNSUPPORTED;
    if (first > cur || count > cur - first) return ZK_ERR_INVALID_ARG;
    if (count == 0) return ZK_OK;
    const uint32_t T = (uint32_t)(m0 / cur), m = (uint32_t)cur, i0 = (uint32_t)first, cnt = (uint32_t)count;
    if (T == 1) {
        HIP_TRY(hipMemcpyAsync(g_out, (const Affine<C>*)bc.dev + i0, (size_t)cnt * sizeof(Affine<C>), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ZK_OK;
    }
    // K = 4 over the handle's shift tables ([2^(64 k)] P in row k: every 255-bit weight is four 64-bit scalars over four points),
    // K = 1 over the points alone.  Per output and window: K T additions into the buckets + 2 per bucket to reduce them; every
    // chunk has ceil(chunk bits / c) windows, the top one narrower (K = 1: one chunk, the whole scalar plus the carry bit).
    static_assert(Fr::BITS < 64 * ZK_SHIFT_TABLES, "the top chunk must absorb the last carry");
    const uint32_t K = bc.shift && ipa_shift_tables_enabled() ? (uint32_t)ZK_SHIFT_TABLES : 1u;
    const uint32_t chunk_bits = K > 1 ? 64u : (uint32_t)Fr::BITS + 1;
    int c = 2;
    {
        uint64_t best = ~0ull;
        for (int cc = 2; cc <= 8; cc++) {
            const uint64_t cost = ((uint64_t)K * T + (1ull << cc)) * (uint64_t)((chunk_bits + cc - 1) / cc);
            if (cost < best) {
                best = cost;
                c = cc;
            }
        }
    }
    const uint32_t nbk = 1u << (c - 1);
    const uint32_t nwin = (chunk_bits + c - 1) / c;
    const uint32_t E = K * T;            // entries per window at most
    StreamScratch* ss = nullptr;
    ZK_TRY(stream_scratch(dc, st, &ss));
    const size_t list_words = (size_t)nwin * nbk + 1 + (size_t)nwin * E;
    ZK_TRY(ws_get(ss->poly_a, (size_t)T * sizeof(Fe<Fr>) + list_words * 4 + 64));
    ZK_TRY(ws_get(ss->poly_b, (size_t)nwin * cnt * sizeof(XYZZ<CK>)));
    ZK_TRY(ws_get(ss->fb_tmp, (size_t)cnt * sizeof(XYZZ<C>)));
    Fe<Fr>* d_w = (Fe<Fr>*)ss->poly_a.p;
    uint32_t* d_off = (uint32_t*)(d_w + T);
    uint32_t* d_ent = d_off + (size_t)nwin * nbk + 1;
    XYZZ<CK>* part = (XYZZ<CK>*)ss->poly_b.p;
    XYZZ<C>* tmp = (XYZZ<C>*)ss->fb_tmp.p;
    ZK_LAUNCH((ipa_gather_weights_kernel<C>), (T + 255) / 256, 256, 0, st, w_dev, (uint64_t)m, T, d_w);
    std::vector<Fe<Fr>> wt(T);
    HIP_TRY(hipMemcpyAsync(wt.data(), d_w, (size_t)T * sizeof(Fe<Fr>), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // signed digits of every weight (the carry method of msm_digits_kernel; the carry runs on across the chunk boundaries, and the
    // last chunk cannot carry out: the weights are below the modulus), then the bucket lists of every window
    auto bits = [&](const Fe<Fr>& x, uint32_t start, uint32_t width) -> uint32_t {
        uint64_t v = 0;
        const uint32_t idx = start >> 5, sh = start & 31;
        if (idx < (uint32_t)Fr::N) v = x.v[idx];
        if (idx + 1 < (uint32_t)Fr::N) v |= (uint64_t)x.v[idx + 1] << 32;
        return (uint32_t)(v >> sh) & ((1u << width) - 1);
    };
    std::vector<int32_t> dig((size_t)nwin * E);      // [window][chunk][t]
    std::vector<uint32_t> off((size_t)nwin * nbk + 1, 0), ent((size_t)nwin * E);
    for (uint32_t t = 0; t < T; t++) {
        uint32_t carry = 0;
        for (uint32_t k = 0; k < K; k++)
            for (uint32_t w = 0; w < nwin; w++) {
                const uint32_t width = (w + 1) * c <= chunk_bits ? (uint32_t)c : chunk_bits - w * c;
                const uint32_t raw = bits(wt[t], k * chunk_bits + w * c, width) + carry;
                const bool neg = raw > (1u << (width - 1));
                const uint32_t mag = neg ? (1u << width) - raw : raw;
                carry = neg ? 1u : 0u;
                dig[((size_t)w * K + k) * T + t] = neg ? -(int32_t)mag : (int32_t)mag;
                if (mag) off[(size_t)w * nbk + (mag - 1) + 1]++;
            }
    }
    for (size_t k = 1; k < off.size(); k++) off[k] += off[k - 1];
    {
        std::vector<uint32_t> pos(off.begin(), off.end() - 1);
        for (uint32_t w = 0; w < nwin; w++)
            for (uint32_t k = 0; k < K; k++)
                for (uint32_t t = 0; t < T; t++) {
                    const int32_t d = dig[((size_t)w * K + k) * T + t];
                    if (d == 0) continue;
                    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
                    ent[pos[(size_t)w * nbk + (mag - 1)]++] = t | (k << 28) | (d < 0 ? 0x80000000u : 0u);
                }
    }
    HIP_TRY(hipMemcpyAsync(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ent, ent.data(), ent.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors go out of scope below
    const uint64_t lanes = (uint64_t)nwin * cnt;
    ZK_LAUNCH((ipa_collapse_window_kernel<CK>), (unsigned)((lanes + 63) / 64), 64, 0, st, (const StoredAffine<CK>*)(K > 1 ? bc.shift : bc.dev29),
              (const uint32_t*)d_off, (const uint32_t*)d_ent, part, m, i0, cnt, nbk, nwin, (uint32_t)(K > 1 ? base_n : 0));
    ZK_LAUNCH((ipa_collapse_horner_kernel<C>), (cnt + 63) / 64, 64, 0, st, (const XYZZ<CK>*)part, tmp, cnt, (uint32_t)c, nwin);
    const uint64_t nl = ((uint64_t)cnt + FB_K - 1) / FB_K;
    ZK_LAUNCH((xyzz_batch_to_affine_kernel<C>), (unsigned)((nl + 63) / 64), 64, 0, st, (const XYZZ<C>*)tmp, g_out, cnt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // g_out is complete on return: the caller adopts it as a bases handle next (any stream)
    return ZK_OK;
}
}  // namespace zk
#include "zk_ecfft.inl"
#include "zk_decode.inl"
