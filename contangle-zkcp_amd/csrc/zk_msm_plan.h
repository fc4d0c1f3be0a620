// The launch plan of an MSM: everything the host decides before it enqueues a window group -- the shape the kernels read,
// bucket splitting, block sizes, sort capacities, the byte size of every workspace and where its sub-arrays start, every grid,
// workgroup and dynamic-LDS size, and every refusal.  Plain data computed by plain C++: no HIP type, no template parameter, no
// allocation, so a host compiler builds it alone (tests/emu/msm_plan_check.cc) and its arithmetic is checked without a kernel.
// msm_enqueue_impl (zk_msm.inl) plans every group of a job first, then allocates, then launches; zk_msm_batch_device sizes its
// jobs with msm_plan_batch.  Also here: the plain structs and constants the plan shares with the kernels (zk_msm_kernels.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zkcp_amd.h"

namespace zk {

struct MsmShape {
    uint32_t n;
    int c;            // window bits (<= 16)
    int w0, nw;       // this call accumulates windows [w0, w0 + nw) of the scalar (window-range sharding)
    uint32_t nbk;     // buckets per window = 2^(c-1)
    uint32_t rb;      // buckets per range (power of two, <= 512: a region of the sorted array should fit the LDS of its sort workgroup)
    uint32_t nranges; // ranges per window = nbk / rb
    int mont;         // scalars arrive in Montgomery form (halo2) rather than canonical (ark BigInt)
    uint32_t big_thresh;  // buckets longer than this take the cooperative path
    int split_log;        // every bucket's entry list is cut into 2^split_log pieces summed by different lanes (msm_combine_sub_kernel adds them)
    uint32_t sblk;        // scalars per workgroup of the digit / stage kernels: MSM_SBLK, less for small inputs (>= 64 workgroups)
    uint32_t batch;       // scalar vectors summed over the same bases by this job; nw = batch * nwb windows in all, window-major per vector
    int nwb;              // windows per scalar vector
    uint64_t batch_stride;   // elements between the scalar vectors
    uint32_t seg;         // entries per cooperative segment of an oversized bucket (power of two in [128, MSM_SEG_MAX], from n: msm_seg_len)
    uint32_t pre_n;       // precomputed-table form (ZK_MSM_FLAG_PRECOMPUTED): the real point count; n = pre_w * pre_n table entries,
    uint32_t pre_w;       // ONE bucket set (nwb = 1): entry w * pre_n + i = the digit of scalar i in window w, point [2^(c w)] P_i
};

constexpr uint32_t MSM_RANGE = 512;   // buckets per (window, range) region of the sort
constexpr uint32_t MSM_SBLK = 4096;   // scalars per workgroup of the digit / stage kernels (1024 lanes x 4) at full size: MsmShape::sblk
constexpr uint32_t MSM_MAX_REGIONS = 4096;   // (window, range) regions of a job: the LDS tables of the scan / hot-list kernels

// ---- hot regions (far above the mean: a skewed witness) are histogrammed and scattered by many workgroups ----
constexpr uint32_t MSM_HOT_MAX = 8;       // hot regions served this way (the rest stay with their own sort workgroup)
constexpr uint32_t MSM_HOT_SLICES = 32;   // workgroups per hot region at most (n / 65536 of them for smaller inputs)

// Entries per cooperative segment (one wave: len / 64 additions per lane + a 6-level tree).  The worst oversized bucket of a
// Groth16 assignment holds the unit scalars, a quarter of all entries: with 2048-entry segments a 2^20-point MSM cuts it into
// 128 segments -- 128 waves on 1024 SIMDs, each doing 38 dependent additions (1.35 ms per G2 launch in round 2).  The length
// now follows n so that such a bucket yields ~1024 segments: n / 4096, at least 128 (below that the tree dominates).
constexpr uint32_t MSM_SEG_MAX = 2048;
inline uint32_t msm_seg_len(uint64_t n) {
    uint32_t s = 128;
    while (s < MSM_SEG_MAX && (uint64_t)s * 4096 < n) s <<= 1;
    return s;
}

struct MsmQueue {          // device-side control words, zeroed before every MSM
    uint32_t head;         // next task
    uint32_t nseg;         // segments appended
    uint32_t nbig;         // big buckets appended
    uint32_t pad;
};
struct MsmSeg {
    uint32_t bucket, start, len, big_index;
};

constexpr uint32_t MSM_BATCH = 64;
// Visiting order: rank-major over the per-range size-sorted bucket lists, MSM_RANKW buckets of a range at a time.  The
// narrower the rank, the closer the order is to globally largest-first (512-bucket ranges: 32 ranks).
constexpr uint32_t MSM_RANKW = 16;

struct MsmAxes {
    uint32_t nbk;        // buckets per window = rows * cols
    uint32_t nw;         // windows
    uint32_t log_cols;   // C = 2^log_cols, R = nbk / C  (R <= C)
    uint32_t k_row, k_col;   // buckets per lane in the partials kernel (powers of two, k_row <= C, k_col <= R)
    // derived
    uint32_t rows, cols, p_row, p_col;   // partials per row = C / k_row, per column = R / k_col
    uint32_t row_lanes, col_lanes;       // nw * rows * p_row, nw * cols * p_col
};

// resolved MSM plan knobs (zk_msm_opts; 0 / negative = choose automatically)
struct MsmTuning {
    int window_bits = 0, w0 = 0, w1 = 0;
    int split_log = -1;
    uint32_t slice_len = 0;
    uint32_t big_thresh = 0;
    int limb_bits = 0;        // 32 forces the saturated path
    int waves = 0;
    int window_group = 0;     // windows per group of a large single MSM (0 = automatic)
    bool no_hot_help = false;
    bool slice_reduce = false;   // the round-1 bucket reduction (slices + multiplier) instead of row / column sums
    bool device_partials = false;   // ZK_MSM_FLAG_DEVICE_PARTIALS: partial sums converted on the device, checked against the host's conversion
    bool precomputed = false;    // ONE bucket set over the handle's precomputed window multiples (ZK_MSM_FLAG_PRECOMPUTED)
    uint64_t base_offset = 0;
    uint32_t batch = 1;          // internal (zk_msm_batch_device): scalar vectors summed by ONE job
    uint64_t batch_stride = 0;   // elements between them
};

// What the plan's arithmetic uses of the curve C and the view CK its kernels compute in (msm_view<C, CK>() in zk_msm.inl)
struct MsmView {
    uint32_t xyzz_ck, xyzz_c;   // sizeof(XYZZ<CK>), sizeof(XYZZ<C>)
    uint32_t tree_lanes;        // tree_lanes<CK>()
    uint32_t acc_waves;         // msm_acc_waves<CK>()
    uint32_t dbg_words;         // partial_dbg_words<CK>()
    bool lazy;                  // ViewBase<CK>::LAZY
};

struct MsmLaunch {
    unsigned grid, block;
    size_t lds;       // dynamic LDS bytes
};

// One window group [w0, w1) of a job.  Sizes are the bytes requested of ws_get (0: the workspace is not used), `*_at` the byte
// offsets of the sub-arrays inside their workspace.
struct MsmPlan {
    MsmShape sh;      // (sh.mont is the caller's: set at enqueue)
    bool pre;
    uint32_t nbuckets, nreg;          // nw * nbk; (window, bucket range) regions = nw * nranges
    uint32_t nblocks_real, nblocks;   // scalar blocks of a vector; blocks the stage kernel partitions (x pre_w in the precomputed form)
    // counts = [counts | offs | order] per bucket, [wg_total | region_base] per region
    size_t counts_bytes, offs_at, order_at, wg_total_at, region_base_at;
    size_t blockcnt_bytes, stage_idx_bytes, stage_low_bytes, digits_bytes, sorted_bytes, buckets_bytes, subacc_bytes;
    // queue = [MsmQueue | seg_list[max_seg] | big_list]; a bucket above big_thresh yields ceil(cnt / sh.seg) segments
    size_t max_seg, max_big, queue_bytes, seg_list_at, big_list_at, seg_out_bytes;
    uint32_t cap, chunk_limit;        // LDS permutation capacity of a sort workgroup; regions above chunk_limit entries are hot
    bool hot_help;
    uint32_t hot_slices;
    size_t hot_bytes, hot_list_at, gcur_at;   // hot = [hot_flag per region | hot_list | gcur per bucket]
    MsmLaunch digits, region_scan, region_base, stage, hot_list, hot, sort, accumulate, combine_sub, accumulate_big, combine_big;
    uint32_t ntasks;                  // batches in the accumulate queue
    // reduction: row / column sums (axes) or slices
    bool axes, dev_std;
    MsmAxes A;
    uint32_t fold_rows, row_blocks, col_blocks, log_tl;   // fold workgroups of the row side; blocks of tree_lanes rows / columns per window
    MsmLaunch axis_partials, axis_fold, axis_weighted;
    uint32_t L, spw, pbw, nslices;    // slice length, slices per window, points per window of the second ping-pong buffer
    MsmLaunch slices;
    struct Sum {
        uint32_t per, per_out, E;
        MsmLaunch launch;
    } sum[4];                         // tree schedule: per -> per_out until <= 8 remain (2^19 slices shrink >= 128-fold a step: <= 3 steps)
    int nsum;
    size_t part_a_bytes, part_b_bytes, part_b_out_at, part_std_bytes, std_at, dbg_at;
    uint32_t per;                     // partial sums per window that go to the host
    size_t pbytes1, hbytes;           // host bytes per partial sum and of this group
};

// workgroup size for a scan over `items` values: a power of two in [64, 1024]
inline unsigned msm_scan_lanes(uint32_t items) {
    unsigned b = 64;
    while (b < items && b < 1024) b <<= 1;
    return b;
}

// The plan of windows [w0, w1) of an MSM over n points with c-bit windows (nwin in the whole scalar).  ZK_ERR_UNSUPPORTED for
// a shape the kernels cannot index; nothing is allocated, created or enqueued before every group of a job has passed here.
inline int msm_plan(MsmPlan& p, uint64_t n, int c, int nwin, int w0, int w1, const MsmTuning& tu, int num_cus, const MsmView& v) {
    p = MsmPlan();
    if (n >= (1ull << 31)) return ZK_ERR_UNSUPPORTED;
    if (num_cus <= 0) num_cus = 256;
    MsmShape& sh = p.sh;
    sh.n = (uint32_t)n;
    sh.c = c;
    sh.w0 = w0;
    sh.nwb = w1 - w0;
    sh.batch = tu.batch ? tu.batch : 1;
    sh.batch_stride = tu.batch_stride;
    sh.nw = sh.nwb * (int)sh.batch;          // the job's windows: those of vector 0, then of vector 1, ...
    sh.nbk = 1u << (c - 1);
    sh.rb = sh.nbk < MSM_RANGE ? sh.nbk : MSM_RANGE;
    sh.nranges = sh.nbk / sh.rb;
    const bool pre = p.pre = tu.precomputed;
    const uint64_t n_real = n;
    if (pre) {
        // ONE bucket set over the table [2^(c w)] P_i: the job is an MSM over nwin * n table entries with c-bit "scalars" and a
        // single window; finer ranges keep a region at the size the LDS sort handles (nwin * n / nranges entries)
        if (w0 != 0 || w1 != nwin || n * (uint64_t)nwin >= (1ull << 31)) return ZK_ERR_UNSUPPORTED;
        sh.pre_n = (uint32_t)n;
        sh.pre_w = (uint32_t)nwin;
        n = n * (uint64_t)nwin;
        sh.n = (uint32_t)n;
        sh.w0 = 0;
        sh.nwb = 1;
        sh.nw = (int)sh.batch;
        uint32_t rb = sh.nbk < MSM_RANGE ? sh.nbk : MSM_RANGE;
        while (rb > 8 && sh.nbk / rb < 1024 && (n / (sh.nbk / rb)) > 20000) rb >>= 1;
        sh.rb = rb;
        sh.nranges = sh.nbk / sh.rb;
    }
    // oversize threshold: 2x the mean bucket length + 64 (uniform 2^20 / c=16: mean 32, max ~70 -> none)
    sh.big_thresh = tu.big_thresh ? tu.big_thresh : (uint32_t)(2 * (n / sh.nbk) + 64);
    sh.seg = msm_seg_len(n);
    const int nw = sh.nw;
    // Bucket splitting: with fewer than ~4 work items per resident lane the accumulate kernel ends in a long drain (every
    // lane finishing one partly summed bucket) -- 2.7 buckets per lane for a full 2^20 MSM, less than one for the window
    // share of a rank of a sharded MSM.  Cut every bucket into 2^split_log pieces (one extra point addition per piece).
    // Measured at 2^20 / c = 16 (tools/shard_model.py, accumulate ms for split 0/1/2/3):
    //   16 windows 1.49/1.32/1.36/1.59   8 windows 0.71/0.65/0.70/0.84   4 windows 0.55/0.42/0.39/0.49   2: 0.44/0.33/0.25/0.28
    // i.e. halves while there are fewer than 8 buckets per lane, quarters below one bucket per lane, pieces never
    // shorter than 8 entries on average.
    {
        const uint64_t lanes = (uint64_t)num_cus * 4 * 3 * 64;
        const uint64_t items = (uint64_t)nw * sh.nbk;
        int sl = 0;
        if (items < 8 * lanes && (n >> 1) / sh.nbk >= 8) sl = 1;
        if (items < lanes && (n >> 2) / sh.nbk >= 8) sl = 2;
        if (pre) {                 // ~nwin * n / nbk entries per bucket: pieces of ~32; halves while a lane would get < 8 buckets
            sl = 0;
            while (sl < 4 && ((n >> (sl + 1)) / sh.nbk) >= 24) sl++;
            if (sl == 0 && items < 8 * lanes && (n >> 1) / sh.nbk >= 8) sl = 1;
        }
        if (tu.split_log >= 0) sl = tu.split_log > 4 ? 4 : tu.split_log;
        sh.split_log = sl;
    }
    const uint32_t nbuckets = p.nbuckets = (uint32_t)nw * sh.nbk;
    const uint32_t nreg = p.nreg = (uint32_t)nw * sh.nranges;
    // scalar blocks of the count / stage kernels: 4096 scalars each at full size; a small input (the later IPA rounds, small
    // keys) would leave all of its digit extraction to a handful of workgroups (72 us for 2^12 scalars in one), so it gets
    // blocks as small as 256 scalars, enough for >= 64 workgroups
    sh.sblk = MSM_SBLK;
    while (sh.sblk > 256 && (n_real + sh.sblk - 1) / sh.sblk < 64) sh.sblk >>= 1;
    // precomputed form: the stage kernel's blocks are the (window, scalar block) pairs: the table must tile into whole blocks
    if (pre && n_real % sh.sblk != 0) return ZK_ERR_UNSUPPORTED;
    p.nblocks_real = (uint32_t)((n_real + sh.sblk - 1) / sh.sblk);
    const uint32_t nblocks = p.nblocks = pre ? p.nblocks_real * sh.pre_w : p.nblocks_real;
    if (nreg > MSM_MAX_REGIONS || sh.nranges > (pre ? 1024u : 64u)) return ZK_ERR_UNSUPPORTED;   // LDS tables of those kernels (<= 1024 / 64 ranges per window)
    if ((uint64_t)n * (uint64_t)nw >= (1ull << 32)) return ZK_ERR_UNSUPPORTED;   // entry positions are u32 (2^27 points x 16 windows fit)

    // ---- workspaces
    p.counts_bytes = ((size_t)nbuckets * 3 + 2 * (size_t)nreg) * 4;
    p.offs_at = (size_t)nbuckets * 4;
    p.order_at = 2 * p.offs_at;
    p.wg_total_at = 3 * p.offs_at;
    p.region_base_at = p.wg_total_at + (size_t)nreg * 4;
    p.blockcnt_bytes = (size_t)nreg * nblocks * 4;
    p.stage_idx_bytes = (size_t)n * nw * 4;
    p.stage_low_bytes = (size_t)n * nw * 2;
    p.digits_bytes = (size_t)n * nw * (pre ? 4 : 2);   // (the one-bucket-set form: 32-bit codes, up to 2^19 buckets)
    p.sorted_bytes = (size_t)n * nw * 4;
    p.buckets_bytes = (size_t)nbuckets * v.xyzz_ck;
    p.subacc_bytes = sh.split_log > 0 ? ((size_t)nbuckets << sh.split_log) * v.xyzz_ck : 0;
    p.max_seg = ((size_t)n / sh.seg + (size_t)n / sh.big_thresh + 2) * nw;
    p.queue_bytes = sizeof(MsmQueue) + p.max_seg * (sizeof(MsmSeg) + 8) + 64;
    p.seg_list_at = sizeof(MsmQueue);
    p.big_list_at = p.seg_list_at + p.max_seg * sizeof(MsmSeg);
    p.seg_out_bytes = p.max_seg * v.xyzz_ck;

    // ---- sort: partition the digits by (window, bucket range), then counting-sort every region in LDS
    // small problems: fewer lanes, cheaper barriers -- but the stage kernel sets up one lane per range (up to 1024 in the
    // one-bucket-set form: a wide window over few points)
    const unsigned dblk = (sh.sblk >= 4096 || sh.nranges > 256) ? 1024u : 256u;
    p.digits = pre ? MsmLaunch{p.nblocks_real * sh.batch, dblk, (size_t)sh.nranges * 4} : MsmLaunch{nblocks * sh.batch, dblk, (size_t)sh.nwb * sh.nranges * 4};
    p.region_scan = {nreg, msm_scan_lanes(nblocks), 0};
    p.region_base = {1, msm_scan_lanes(nreg), 0};
    p.stage = {nblocks * (unsigned)nw, dblk, (size_t)sh.sblk * 8 + (size_t)(3 * sh.nranges + 1) * 4};
    // LDS permutation capacity of a sort workgroup: 1.5x the mean region, at most 24576 entries (61 KB of LDS in all,
    // two workgroups per CU); larger regions are sorted in chunks of half that
    uint32_t cap = (uint32_t)((n / sh.nranges) * 3 / 2 + 64);
    if (cap > 24576) cap = 24576;
    p.cap = cap = (cap + 1) & ~1u;
    // regions up to 4x the mean (large n) are sorted in LDS chunks; anything beyond is a skewed witness's hot region
    const uint64_t cl64 = 4 * (n / sh.nranges) + 4 * (uint64_t)cap;
    p.chunk_limit = cl64 < 0xffffffffull ? (uint32_t)cl64 : 0xffffffffu;
    // hot regions (skewed witnesses) are histogrammed and scattered by MSM_HOT_SLICES workgroups each, around the sort kernel
    p.hot_help = nreg <= 1024 && !tu.no_hot_help && n >= 32768;   // a small input's hot region is one sort workgroup's work anyway
    p.hot_slices = (uint32_t)(n >> 16);
    if (p.hot_slices < 1) p.hot_slices = 1;
    if (p.hot_slices > MSM_HOT_SLICES) p.hot_slices = MSM_HOT_SLICES;
    p.hot_bytes = p.hot_help ? ((size_t)nreg + 1 + MSM_HOT_MAX + nbuckets) * 4 : 0;
    p.hot_list_at = (size_t)nreg * 4;
    p.gcur_at = p.hot_list_at + (1 + MSM_HOT_MAX) * 4;
    p.hot_list = {1, 1024, 0};
    p.hot = {MSM_HOT_MAX * p.hot_slices, 1024, (size_t)2 * sh.rb * 4};
    p.sort = {nreg, n >= 8192 ? 1024u : 256u, (size_t)(4 * sh.rb + 1024 + 258) * 4 + (size_t)cap * 2};

    // ---- persistent accumulate: lanes stream buckets, largest first; oversized buckets go to the cooperative segment
    // kernels (fixed grids over device-side lists, no host round trip)
    // resident waves per SIMD = what the kernel was compiled for (msm_acc_waves); opts.waves_per_simd launches fewer
    unsigned waves_per_simd = v.acc_waves;
    if (tu.waves >= 1 && tu.waves <= 8) waves_per_simd = (unsigned)tu.waves;
    p.ntasks = (((nreg * ((sh.rb + MSM_RANKW - 1) / MSM_RANKW) * MSM_RANKW) << sh.split_log) + MSM_BATCH - 1) / MSM_BATCH;
    unsigned acc_grid = (unsigned)num_cus * 4u * waves_per_simd;
    if (acc_grid > p.ntasks) acc_grid = p.ntasks;
    p.accumulate = {acc_grid, 64, 0};
    p.combine_sub = {(nbuckets + 63) / 64, 64, 0};
    p.accumulate_big = {p.max_seg < 4096 ? (unsigned)p.max_seg : 4096u, 64, 0};
    // (an oversized bucket holds more than big_thresh entries: at most n nw / big_thresh of them exist)
    p.max_big = (size_t)n * nw / sh.big_thresh + 1;
    p.combine_big = {(unsigned)(p.max_big < 2048 ? p.max_big : 2048), v.tree_lanes, 0};

    const uint32_t TL = v.tree_lanes;
    p.axes = !tu.slice_reduce;
    if (p.axes) {
        // ---- bucket reduction by row / column sums (zk_msm_kernels.h, MsmAxes)
        MsmAxes& A = p.A;
        A.nbk = sh.nbk;
        A.nw = (uint32_t)nw;
        A.log_cols = (uint32_t)c / 2;                               // ceil((c - 1) / 2)
        A.cols = 1u << A.log_cols;
        A.rows = sh.nbk >> A.log_cols;
        uint32_t K = 2;                                             // buckets per lane: <= ~2 waves per SIMD of lanes, at most 8
        while (K < 8 && 2ull * A.nw * A.nbk / K > 131072) K <<= 1;
        A.k_row = K < A.cols ? K : A.cols;
        A.k_col = K < A.rows ? K : A.rows;
        A.p_row = A.cols / A.k_row;
        A.p_col = A.rows / A.k_col;
        A.row_lanes = A.nw * A.rows * A.p_row;
        A.col_lanes = A.nw * A.cols * A.p_col;
        auto fold_blocks = [&](uint32_t nelem, uint32_t P) {
            const uint32_t tw = P < 16 ? P : 16;
            const uint32_t per_wg = TL / tw;
            return (nelem + per_wg - 1) / per_wg;
        };
        const uint32_t fr = p.fold_rows = fold_blocks(A.nw * A.rows, A.p_row), fc = fold_blocks(A.nw * A.cols, A.p_col);
        const uint32_t rb = p.row_blocks = (A.rows + TL - 1) / TL, cb = p.col_blocks = (A.cols + TL - 1) / TL;
        p.log_tl = TL == 256 ? 8u : 7u;
        p.per = 2 * (rb + cb);
        p.part_a_bytes = ((size_t)A.row_lanes + A.col_lanes) * v.xyzz_ck;
        p.part_b_bytes = ((size_t)A.nw * (A.rows + A.cols) + (size_t)A.nw * p.per) * v.xyzz_ck;
        p.part_b_out_at = (size_t)A.nw * (A.rows + A.cols) * v.xyzz_ck;
        p.axis_partials = {(A.row_lanes + A.col_lanes + 63) / 64, 64, 0};
        p.axis_fold = {fr + fc, TL, 0};
        p.axis_weighted = {A.nw * (rb + cb), TL, 0};
        p.dev_std = tu.device_partials && v.lazy;
        if (p.dev_std) {
            // [raw partials | converted partials | conversion stages], copied to the host as one block
            const size_t np = (size_t)A.nw * p.per;
            p.part_std_bytes = np * (v.xyzz_ck + v.xyzz_c + 4 * (size_t)v.dbg_words);
            p.std_at = np * v.xyzz_ck;
            p.dbg_at = p.std_at + np * v.xyzz_c;
        }
    } else {
        // ---- slice form (ZK_MSM_FLAG_SLICE_REDUCE): running sums + windowed multiplier per slice, then tree-sum the
        // slices of each window until <= 8 remain.  Slice length: 64K lanes = one wave on every SIMD; a rank of a
        // window-sharded MSM owns few windows and gets shorter slices
        uint32_t L = (uint32_t)(((uint64_t)nw * sh.nbk) >> 16);
        if (L < 1) L = 1;
        if (L > 8) L = 8;
        if (tu.slice_len >= 1 && tu.slice_len <= 1024) L = tu.slice_len;
        if (L > sh.nbk) L = sh.nbk;
        p.L = L;
        p.spw = (sh.nbk + L - 1) / L;                  // slices per window
        p.pbw = p.spw / 128 + 2;                        // second ping-pong buffer, points per window
        p.part_a_bytes = (size_t)p.spw * nw * v.xyzz_ck;
        p.part_b_bytes = (size_t)p.pbw * nw * v.xyzz_ck;
        p.nslices = p.spw * (uint32_t)nw;
        p.slices = {(p.nslices + 63) / 64, 64, 0};
        p.per = p.spw;
        while (p.per > 8) {
            const uint32_t E = p.per >= 1024 ? 4 : 1;
            const uint32_t chunk = TL * E;
            const uint32_t per_out = (p.per + chunk - 1) / chunk;
            p.sum[p.nsum++] = {p.per, per_out, E, {(unsigned)nw * per_out, TL, 0}};
            p.per = per_out;
        }
    }
    p.pbytes1 = v.xyzz_ck + (p.dev_std ? v.xyzz_c + 4 * (size_t)v.dbg_words : 0);
    p.hbytes = (size_t)nw * p.per * p.pbytes1;
    return ZK_OK;
}

// Window groups (zk_msm_opts.window_group, OFF by default): the windows of a single MSM processed a few at a time, each group
// running the whole pipeline over workspaces sized for a group, all partial sums landing in one host buffer.  The idea (round-2
// shard model: 4 windows of a 2^22-point MSM in 1.82 ms against 8.68 / 4 = 2.17 ms) was that 16 windows keep 268 MB of sorted
// entries + 256 MB of bases live, past the 256 MiB Infinity Cache.  Measured inside one job (profiles/r03_e_window_group_sweep.txt,
// BN254 G1 2^22, ms: all 16 windows 8.20 | 2 groups 8.81 | 4 groups 8.81 | 8 groups 11.35): the accumulate kernels do get faster
// (5.96 -> 5.62 in 4 groups) but every group pays its own sort launches and its own latency-bound bucket reduction, which costs
// more than the cache gives back; with a 0/1-heavy witness it is 2.90 -> 3.95.  So the default is one group; the knob stays.
// A job of nwj >= 1 windows runs as `ng` groups of `gw` windows (the last may hold fewer).
struct MsmGroups {
    int ng, gw;
};
inline MsmGroups msm_plan_groups(int nwj, const MsmTuning& tu) {
    int gw = nwj;
    if ((tu.batch ? tu.batch : 1) == 1 && !tu.precomputed && !tu.device_partials) {
        if (tu.window_group > 0) gw = tu.window_group;
        if (gw < 1) gw = 1;
        if (gw > nwj) gw = nwj;
    }
    const int ng = (nwj + gw - 1) / gw;
    return {ng, (nwj + ng - 1) / ng};                  // even groups
}

// zk_msm_batch_device: scalar vectors per job = the largest batch <= 4 the plan accepts.  What limits it is the (window, range)
// region count the sort kernels index.  A batch whose regions fit but which is refused all the same -- four vectors pass the
// u32 entry positions (2^26 points x 16 windows), or the shape is refused at any batch -- gets one vector per job, not 2 or 3:
// the rule from before the plan existed, kept.
inline uint32_t msm_plan_batch(uint64_t n, int c, int nwin, int w0, int w1, MsmTuning tu, int num_cus, const MsmView& v) {
    MsmPlan p;
    for (tu.batch = 4; tu.batch > 1; tu.batch--) {
        if (msm_plan(p, n, c, nwin, w0, w1, tu, num_cus, v) == ZK_OK) return tu.batch;
        if (p.nreg <= MSM_MAX_REGIONS) break;
    }
    return 1;
}
}  // namespace zk
