// TEST INFRASTRUCTURE: prints the MSM launch plan (contangle-zkcp_amd/csrc/zk_msm_plan.h, the only header included) of shapes
// read from stdin, so that tests/test_msm_plan.py can hold it against the rules DESIGN.md states, in Python integers.
// Line format (one job per line, all integers):
//   n c nwin w0 w1  batch pre slice_reduce device_partials window_group num_cus  xyzz_ck xyzz_c tree_lanes acc_waves dbg_words lazy
// ->  one line of key=value fields: the job's groups (ng, gw, the status and the window count of every group's plan), the batch
//     zk_msm_batch_device would choose (per_job), and the plan of group 0 (status != 0: its fields are not meaningful).
#include <stdio.h>

#include "zk_msm_plan.h"
using namespace zk;

static void launch(const char* name, const MsmLaunch& l) { printf(" %s=%u,%u,%zu", name, l.grid, l.block, l.lds); }

int main() {
    unsigned long long n;
    int c, nwin, w0, w1, pre, slice, devp, wgroup, num_cus, lazy;
    unsigned batch;
    MsmView v;
    while (scanf("%llu %d %d %d %d %u %d %d %d %d %d %u %u %u %u %u %d", &n, &c, &nwin, &w0, &w1, &batch, &pre, &slice, &devp, &wgroup, &num_cus,
                 &v.xyzz_ck, &v.xyzz_c, &v.tree_lanes, &v.acc_waves, &v.dbg_words, &lazy) == 17) {
        v.lazy = lazy != 0;
        MsmTuning tu;
        tu.batch = batch;
        tu.precomputed = pre != 0;
        tu.slice_reduce = slice != 0;
        tu.device_partials = devp != 0;
        tu.window_group = wgroup;
        if (w1 <= w0) {      // an empty job: nothing is planned
            printf("empty\n");
            continue;
        }
        const MsmGroups g = msm_plan_groups(w1 - w0, tu);
        MsmPlan p, p0;
        int st0 = ZK_OK;
        printf("ng=%d gw=%d groups=", g.ng, g.gw);
        for (int gi = 0; gi < g.ng; gi++) {
            const int a = w0 + gi * g.gw, b = a + g.gw < w1 ? a + g.gw : w1;
            const int st = msm_plan(p, n, c, nwin, a, b, tu, num_cus, v);
            printf("%s%d:%d", gi ? "," : "", st, b - a);
            if (gi == 0) {
                p0 = p;
                st0 = st;
            }
        }
        printf(" per_job=%u status=%d", msm_plan_batch(n, c, nwin, w0, w1, tu, num_cus, v), st0);
        const MsmPlan& q = p0;
        const MsmShape& s = q.sh;
        printf(" n=%u c=%d w0=%d nw=%d nwb=%d batch=%u nbk=%u rb=%u nranges=%u big_thresh=%u split_log=%d sblk=%u seg=%u pre_n=%u pre_w=%u", s.n, s.c, s.w0, s.nw,
               s.nwb, s.batch, s.nbk, s.rb, s.nranges, s.big_thresh, s.split_log, s.sblk, s.seg, s.pre_n, s.pre_w);
        printf(" nbuckets=%u nreg=%u nblocks_real=%u nblocks=%u", q.nbuckets, q.nreg, q.nblocks_real, q.nblocks);
        printf(" counts_bytes=%zu offs_at=%zu order_at=%zu wg_total_at=%zu region_base_at=%zu", q.counts_bytes, q.offs_at, q.order_at, q.wg_total_at,
               q.region_base_at);
        printf(" blockcnt_bytes=%zu stage_idx_bytes=%zu stage_low_bytes=%zu digits_bytes=%zu sorted_bytes=%zu buckets_bytes=%zu subacc_bytes=%zu", q.blockcnt_bytes,
               q.stage_idx_bytes, q.stage_low_bytes, q.digits_bytes, q.sorted_bytes, q.buckets_bytes, q.subacc_bytes);
        printf(" max_seg=%zu max_big=%zu queue_bytes=%zu seg_list_at=%zu big_list_at=%zu seg_out_bytes=%zu", q.max_seg, q.max_big, q.queue_bytes, q.seg_list_at,
               q.big_list_at, q.seg_out_bytes);
        printf(" cap=%u chunk_limit=%u hot_help=%d hot_slices=%u hot_bytes=%zu hot_list_at=%zu gcur_at=%zu ntasks=%u", q.cap, q.chunk_limit, (int)q.hot_help,
               q.hot_slices, q.hot_bytes, q.hot_list_at, q.gcur_at, q.ntasks);
        launch("digits", q.digits);
        launch("region_scan", q.region_scan);
        launch("region_base", q.region_base);
        launch("stage", q.stage);
        launch("hot_list", q.hot_list);
        launch("hot", q.hot);
        launch("sort", q.sort);
        launch("accumulate", q.accumulate);
        launch("combine_sub", q.combine_sub);
        launch("accumulate_big", q.accumulate_big);
        launch("combine_big", q.combine_big);
        printf(" axes=%d dev_std=%d", (int)q.axes, (int)q.dev_std);
        if (q.axes) {
            const MsmAxes& A = q.A;
            printf(" log_cols=%u rows=%u cols=%u k_row=%u k_col=%u p_row=%u p_col=%u row_lanes=%u col_lanes=%u fold_rows=%u row_blocks=%u col_blocks=%u log_tl=%u",
                   A.log_cols, A.rows, A.cols, A.k_row, A.k_col, A.p_row, A.p_col, A.row_lanes, A.col_lanes, q.fold_rows, q.row_blocks, q.col_blocks, q.log_tl);
            launch("axis_partials", q.axis_partials);
            launch("axis_fold", q.axis_fold);
            launch("axis_weighted", q.axis_weighted);
        } else {
            printf(" L=%u spw=%u pbw=%u nslices=%u nsum=%d", q.L, q.spw, q.pbw, q.nslices, q.nsum);
            launch("slices", q.slices);
            for (int k = 0; k < q.nsum; k++) printf(" sum%d=%u,%u,%u,%u,%u", k, q.sum[k].per, q.sum[k].per_out, q.sum[k].E, q.sum[k].launch.grid, q.sum[k].launch.block);
        }
        printf(" part_a_bytes=%zu part_b_bytes=%zu part_b_out_at=%zu part_std_bytes=%zu std_at=%zu dbg_at=%zu per=%u pbytes1=%zu hbytes=%zu\n",
               q.part_a_bytes, q.part_b_bytes, q.part_b_out_at, q.part_std_bytes, q.std_at, q.dbg_at, q.per, q.pbytes1, q.hbytes);
    }
    return 0;
}
