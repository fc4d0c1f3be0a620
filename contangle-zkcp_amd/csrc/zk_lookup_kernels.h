// Kernels of the lookup argument's permute_expression_pair (halo2_proofs 0.2 plonk/lookup/prover.rs) on the device:
//   lk_keys_kernel       A and S (Montgomery) -> one merged array of 2u canonical keys, key = value << 1 | tag (0 = input,
//                        1 = table), plus the histogram of all 32 8-bit digits of every key (LDS, then global atomics)
//   lk_plan_kernel       per digit: live (no bucket holds every key) and the digit's bucket bases (exclusive scan); which
//                        of the two key buffers holds the data before each pass (dead digits are skipped on the device)
//   lk_count_kernel      one LSD pass, reduce: per-workgroup digit counts of its chunk, counts[bucket * nblocks + block]
//   lk_offsets_kernel    one LSD pass, scan: one workgroup per bucket turns the counts into global write offsets
//                        (lk_offsets_small_kernel: one workgroup for all buckets when there are at most 8 chunks)
//   lk_scatter_kernel    one LSD pass, stable scatter: ranks within a tile of 256 keys from 8 ballots per wave
//   lk_runs_reduce / lk_runs_totals / lk_runs_apply   reduce-then-scan over the sorted keys: at every run head (a new value)
//                        its key position, its first A' row and its first leftover / repeated-row ordinals; the status
//                        word is set where a run ends on an input key (an input value with no table key)
//   lk_emit_kernel       row by row: the run of A'[row] by binary search, A' and S' converted back to Montgomery
// Every scalar field modulus is below 2^255, so value << 1 | tag fits the 256-bit key and sorting keys sorts values with
// the inputs of a value ahead of its table entries.  No inter-workgroup waits: every cross-workgroup step is a launch.
#pragma once
#include "zk_rt.h"
#include "zk_field.h"

namespace zk {

constexpr uint32_t LK_WG = 256;                       // lanes per workgroup (4 waves of 64)
constexpr uint32_t LK_TILES = 16;                     // tiles of LK_WG keys per workgroup chunk of an LSD pass
constexpr uint32_t LK_CHUNK = LK_WG * LK_TILES;       // 4096 keys per workgroup chunk (LSD passes and the run scan)
constexpr uint32_t LK_DIGITS = 32;                    // 8-bit digits of a 256-bit key
// meta words after the 32 x 256 digit histogram
constexpr uint32_t LK_M_LIVE = 0;                     // [32] digit d is live
constexpr uint32_t LK_M_SEL = 32;                     // [33] key buffer (0 / 1) that holds the keys before pass d; [32] after the sort
constexpr uint32_t LK_M_RUNS = 65;                    // number of runs (distinct values)
constexpr uint32_t LK_M_INRUNS = 66;                  // runs holding an input (= distinct input values)
constexpr uint32_t LK_M_STATUS = 67;                  // 1: an input value is not in the table
constexpr uint32_t LK_META = 68;

struct alignas(16) LkKey {
    uint32_t w[8];
};

#ifdef ZK_EMU
#define LK_READLANE(v, l) __shfl((v), (l))
#else
#define LK_READLANE(v, l) ((uint32_t)__builtin_amdgcn_readlane((int)(v), (l)))
#endif

__device__ __forceinline__ uint32_t lk_digit(const LkKey& k, uint32_t d) { return (k.w[d >> 2] >> (8 * (d & 3))) & 255u; }
__device__ __forceinline__ bool lk_same_value(const LkKey& a, const LkKey& b) {
    uint32_t o = (a.w[0] ^ b.w[0]) & ~1u;
    for (int i = 1; i < 8; i++) o |= a.w[i] ^ b.w[i];
    return o == 0;
}

// hist[v] += 1 for every valid lane; the lanes of the wave that share the first valid lane's value are served by one atomic
// (the range-check shape puts nearly every key in bucket 0 of most digits).  Every lane of the wave must call it.
__device__ __forceinline__ void lk_hist_add(uint32_t* hist, uint32_t v, bool valid) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t vm = __ballot(valid);
    if (vm == 0) return;
    const int leader = __ffsll((unsigned long long)vm) - 1;
    const uint32_t hot = LK_READLANE(v, leader);
    const bool match = valid && v == hot;
    const uint64_t mm = __ballot(match);
    if (lane == (uint32_t)leader) atomicAdd(&hist[hot], (uint32_t)__popcll((unsigned long long)mm));
    if (valid && !match) atomicAdd(&hist[v], 1u);
}

// exclusive sum over the LK_WG lanes of the workgroup (Hillis-Steele in LDS); *total gets the sum of all lanes
__device__ __forceinline__ uint32_t lk_block_excl(uint32_t v, uint32_t* s, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < LK_WG; off <<= 1) {
        const uint32_t add = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const uint32_t incl = s[t];
    *total = s[LK_WG - 1];
    __syncthreads();
    return incl - v;
}

// keys[i] = canonical(A[i]) << 1 for i < u, canonical(S[i - u]) << 1 | 1 after; hist[d * 256 + b] += keys with digit d == b
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_keys_kernel(const Fe<F>* A, const Fe<F>* S, uint32_t u, LkKey* __restrict__ keys,
                                                         uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[LK_DIGITS * 256];
    for (uint32_t j = threadIdx.x; j < LK_DIGITS * 256; j += LK_WG) h[j] = 0;
    __syncthreads();
    const uint64_t total = 2ull * u;
    for (uint64_t base = (uint64_t)blockIdx.x * LK_WG; base < total; base += (uint64_t)gridDim.x * LK_WG) {
        const uint64_t i = base + threadIdx.x;
        const bool valid = i < total;
        LkKey k;
        for (int w = 0; w < 8; w++) k.w[w] = 0;
        if (valid) {
            const uint32_t tag = i < u ? 0u : 1u;
            Fe<F> c;
            fe_from_mont(c, tag ? S[i - u] : A[i]);
            k.w[0] = c.v[0] << 1 | tag;
            for (int w = 1; w < 8; w++) k.w[w] = c.v[w] << 1 | c.v[w - 1] >> 31;
            keys[i] = k;
        }
        for (uint32_t d = 0; d < LK_DIGITS; d++) lk_hist_add(&h[d * 256], lk_digit(k, d), valid);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < LK_DIGITS * 256; j += LK_WG)
        if (h[j]) atomicAdd(&hist[j], h[j]);
}

// one workgroup of 64 lanes: lane d < 32 decides digit d and turns its histogram row into exclusive bucket bases
template <class F>
__global__ void __launch_bounds__(64) lk_plan_kernel(uint32_t* hist, uint32_t* meta, uint64_t total) {
    const uint32_t d = threadIdx.x;
    if (d < LK_DIGITS) {
        uint32_t* row = hist + d * 256;
        uint32_t run = 0, live = 1;
        for (uint32_t b = 0; b < 256; b++) {
            const uint32_t c = row[b];
            if ((uint64_t)c == total) live = 0;
            row[b] = run;
            run += c;
        }
        meta[LK_M_LIVE + d] = live;
    }
    __syncthreads();
    if (d == 0) {
        uint32_t sel = 0;
        for (uint32_t j = 0; j < LK_DIGITS; j++) {
            meta[LK_M_SEL + j] = sel;
            sel ^= meta[LK_M_LIVE + j];
        }
        meta[LK_M_SEL + LK_DIGITS] = sel;
    }
}

// LSD pass over digit d, reduce: counts[b * nblocks + block] = keys of the block's chunk whose digit d is b
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_count_kernel(const LkKey* k0, const LkKey* k1, const uint32_t* meta, uint32_t d, uint64_t total,
                                                          uint32_t* counts, uint32_t nblocks) {
    if (!meta[LK_M_LIVE + d]) return;
    const LkKey* src = meta[LK_M_SEL + d] ? k1 : k0;
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * LK_CHUNK;
    for (uint32_t t = 0; t < LK_TILES && base + (uint64_t)t * LK_WG < total; t++) {   // (the last chunk may be short)
        const uint64_t i = base + (uint64_t)t * LK_WG + threadIdx.x;
        const bool valid = i < total;
        lk_hist_add(h, valid ? lk_digit(src[i], d) : 0u, valid);
    }
    __syncthreads();
    counts[(uint64_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// LSD pass over digit d, scan: workgroup b turns counts[b * nblocks + j] into bases[d][b] + sum_{j' < j} counts[b][j']
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_offsets_kernel(const uint32_t* meta, uint32_t d, const uint32_t* bases, uint32_t* counts,
                                                            uint32_t nblocks) {
    if (!meta[LK_M_LIVE + d]) return;
    __shared__ uint32_t s[LK_WG];
    uint32_t* row = counts + (uint64_t)blockIdx.x * nblocks;
    uint32_t carry = bases[d * 256 + blockIdx.x];
    for (uint32_t j0 = 0; j0 < nblocks; j0 += LK_WG) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t v = j < nblocks ? row[j] : 0u;
        uint32_t tot;
        const uint32_t ex = lk_block_excl(v, s, &tot);
        if (j < nblocks) row[j] = carry + ex;
        carry += tot;
    }
}

// ... the same for at most LK_SMALL_SCAN chunks: one workgroup, lane b walks bucket b's counts
constexpr uint32_t LK_SMALL_SCAN = 8;
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_offsets_small_kernel(const uint32_t* meta, uint32_t d, const uint32_t* bases, uint32_t* counts,
                                                                  uint32_t nblocks) {
    if (!meta[LK_M_LIVE + d]) return;
    uint32_t* row = counts + (uint64_t)threadIdx.x * nblocks;
    uint32_t carry = bases[d * 256 + threadIdx.x];
    for (uint32_t j = 0; j < nblocks; j++) {
        const uint32_t c = row[j];
        row[j] = carry;
        carry += c;
    }
}

// LSD pass over digit d, stable scatter of the block's chunk, one tile of LK_WG keys at a time: a lane's rank among the
// equal digits of its wave comes from 8 ballots; the waves ahead of it in the tile and the tiles ahead of it in the chunk
// are added from LDS counters
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_scatter_kernel(LkKey* k0, LkKey* k1, const uint32_t* meta, uint32_t d, uint64_t total,
                                                            const uint32_t* offsets, uint32_t nblocks) {
    if (!meta[LK_M_LIVE + d]) return;
    const bool from1 = meta[LK_M_SEL + d] != 0;
    const LkKey* src = from1 ? k1 : k0;
    LkKey* dst = from1 ? k0 : k1;
    __shared__ uint32_t run[256];
    __shared__ uint32_t wcnt[LK_WG / 64][256];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    run[t] = offsets[(uint64_t)t * nblocks + blockIdx.x];
    for (uint32_t w = 0; w < LK_WG / 64; w++) wcnt[w][t] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * LK_CHUNK;
    for (uint32_t tile = 0; tile < LK_TILES && base + (uint64_t)tile * LK_WG < total; tile++) {
        const uint64_t i = base + (uint64_t)tile * LK_WG + t;
        const bool valid = i < total;
        LkKey k;
        uint32_t dig = 0;
        if (valid) {
            k = src[i];
            dig = lk_digit(k, d);
        }
        uint64_t m = __ballot(valid);
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (dig >> b) & 1u;
            const uint64_t bb = __ballot(bit);
            m &= bit ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll((unsigned long long)(m & ((1ull << lane) - 1ull)));
        if (valid && rank == 0) wcnt[wv][dig] = (uint32_t)__popcll((unsigned long long)m);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[dig] + rank;
            for (uint32_t w = 0; w < wv; w++) pos += wcnt[w][dig];
            dst[pos] = k;
        }
        __syncthreads();
        uint32_t add = 0;
        for (uint32_t w = 0; w < LK_WG / 64; w++) {
            add += wcnt[w][t];
            wcnt[w][t] = 0;
        }
        run[t] += add;
        __syncthreads();
    }
}

// the per-key flags the run scan sums: a run head, an input key (tag 0), an input run head
struct LkFlags {
    uint32_t head, input, in_head;
};
__device__ __forceinline__ LkFlags lk_flags(const LkKey* keys, uint64_t i) {
    const LkKey k = keys[i];
    LkFlags f;
    f.head = i == 0 || !lk_same_value(k, keys[i - 1]);
    f.input = (k.w[0] & 1u) == 0;
    f.in_head = f.head & f.input;
    return f;
}

// run scan, reduce: tot[block] = flag sums of the block's chunk (lane t owns LK_TILES consecutive keys)
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_runs_reduce_kernel(const LkKey* k0, const LkKey* k1, const uint32_t* meta, uint64_t total,
                                                                uint32_t* tot) {
    const LkKey* keys = meta[LK_M_SEL + LK_DIGITS] ? k1 : k0;
    __shared__ uint32_t s[LK_WG];
    const uint64_t lo = (uint64_t)blockIdx.x * LK_CHUNK + (uint64_t)threadIdx.x * LK_TILES;
    uint32_t h = 0, in = 0, ih = 0;
    for (uint32_t j = 0; j < LK_TILES; j++)
        if (lo + j < total) {
            const LkFlags f = lk_flags(keys, lo + j);
            h += f.head;
            in += f.input;
            ih += f.in_head;
        }
    uint32_t th, tin, tih;
    lk_block_excl(h, s, &th);
    lk_block_excl(in, s, &tin);
    lk_block_excl(ih, s, &tih);
    if (threadIdx.x == 0) {
        tot[3 * blockIdx.x + 0] = th;
        tot[3 * blockIdx.x + 1] = tin;
        tot[3 * blockIdx.x + 2] = tih;
    }
}

// run scan, one workgroup: exclusive scan of the block sums in place; the run counts go to meta
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_runs_totals_kernel(uint32_t* tot, uint32_t nblocks, uint32_t* meta) {
    __shared__ uint32_t s[LK_WG];
    uint32_t carry[3] = {0, 0, 0};
    for (uint32_t j0 = 0; j0 < nblocks; j0 += LK_WG) {
        const uint32_t j = j0 + threadIdx.x;
        for (uint32_t c = 0; c < 3; c++) {
            const uint32_t v = j < nblocks ? tot[3 * j + c] : 0u;
            uint32_t all;
            const uint32_t ex = lk_block_excl(v, s, &all);
            if (j < nblocks) tot[3 * j + c] = carry[c] + ex;
            carry[c] += all;
        }
    }
    if (threadIdx.x == 0) {
        meta[LK_M_RUNS] = carry[0];
        meta[LK_M_INRUNS] = carry[2];
    }
}

// run scan, apply: at the head key i of run r (with `in` input keys and `ih` input runs ahead of it)
//   rpos[r] = i                         the run's value is keys[i] >> 1
//   astart[r] = in                      its first row in A' (inputs before it)
//   lstart[r] = (i - in) - ih           its first leftover ordinal (table keys before it, less one per input run)
//   rstart[r] = in - ih                 the repeated-row ordinal of its second A' row
// and a run that ends on an input key has no table key: status word set
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_runs_apply_kernel(const LkKey* k0, const LkKey* k1, uint32_t* meta, uint64_t total,
                                                               const uint32_t* tot, uint32_t* __restrict__ rpos, uint32_t* __restrict__ astart,
                                                               uint32_t* __restrict__ lstart, uint32_t* __restrict__ rstart) {
    const LkKey* keys = meta[LK_M_SEL + LK_DIGITS] ? k1 : k0;
    __shared__ uint32_t s[LK_WG];
    const uint64_t lo = (uint64_t)blockIdx.x * LK_CHUNK + (uint64_t)threadIdx.x * LK_TILES;
    uint32_t h = 0, in = 0, ih = 0;
    for (uint32_t j = 0; j < LK_TILES; j++)
        if (lo + j < total) {
            const LkFlags f = lk_flags(keys, lo + j);
            h += f.head;
            in += f.input;
            ih += f.in_head;
        }
    uint32_t all;
    h = tot[3 * blockIdx.x + 0] + lk_block_excl(h, s, &all);
    in = tot[3 * blockIdx.x + 1] + lk_block_excl(in, s, &all);
    ih = tot[3 * blockIdx.x + 2] + lk_block_excl(ih, s, &all);
    bool missing = false;
    for (uint32_t j = 0; j < LK_TILES; j++) {
        const uint64_t i = lo + j;
        if (i >= total) break;
        const LkFlags f = lk_flags(keys, i);
        if (f.head) {
            rpos[h] = (uint32_t)i;
            astart[h] = in;
            lstart[h] = (uint32_t)(i - in) - ih;
            rstart[h] = in - ih;
        }
        if (f.input && (i + 1 == total || !lk_same_value(keys[i], keys[i + 1]))) missing = true;
        h += f.head;
        in += f.input;
        ih += f.in_head;
    }
    if (missing) meta[LK_M_STATUS] = 1;
}

// largest r in [0, n) with a[r] <= x (a[0] == 0 <= x, a non-decreasing)
__device__ __forceinline__ uint32_t lk_find(const uint32_t* a, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;   // a[lo] <= x, answer in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <class F>
__device__ __forceinline__ void lk_store_mont(Fe<F>* out, const LkKey& k) {
    Fe<F> c, m;
    for (int w = 0; w < 7; w++) c.v[w] = k.w[w] >> 1 | k.w[w + 1] << 31;
    c.v[7] = k.w[7] >> 1;
    fe_to_mont(m, c);
    *out = m;
}

// rows [0, u): A'[row] = the value of its run; S'[row] = that value at the run's first row, else leftover T - 1 - q for the
// row's repeated-row ordinal q (T = u - input runs leftovers, filled from the last repeated row up)
template <class F>
__global__ void __launch_bounds__(LK_WG) lk_emit_kernel(const LkKey* k0, const LkKey* k1, const uint32_t* meta, uint32_t u,
                                                         const uint32_t* rpos, const uint32_t* astart, const uint32_t* lstart,
                                                         const uint32_t* rstart, Fe<F>* __restrict__ a_out, Fe<F>* __restrict__ s_out) {
    const LkKey* keys = meta[LK_M_SEL + LK_DIGITS] ? k1 : k0;
    const uint32_t nruns = meta[LK_M_RUNS];
    const uint32_t T = u - meta[LK_M_INRUNS];
    for (uint64_t row = (uint64_t)blockIdx.x * LK_WG + threadIdx.x; row < u; row += (uint64_t)gridDim.x * LK_WG) {
        const uint32_t r = lk_find(astart, nruns, (uint32_t)row);
        const LkKey v = keys[rpos[r]];
        lk_store_mont<F>(a_out + row, v);
        if (row == astart[r]) {
            lk_store_mont<F>(s_out + row, v);
        } else {
            const uint32_t q = rstart[r] + (uint32_t)(row - astart[r] - 1);
            const uint32_t r2 = lk_find(lstart, nruns, T - 1 - q);
            lk_store_mont<F>(s_out + row, keys[rpos[r2]]);
        }
    }
}

}  // namespace zk
