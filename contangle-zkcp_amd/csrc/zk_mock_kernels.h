// Kernels of MockProver::verify on the device (halo2_proofs 0.2 dev.rs, restated in DESIGN.md §5 "MockProver"): does an assignment satisfy a
// circuit -- gates, lookups, copy constraints -- with upstream's poisoned cells (the blinding rows of the advice columns).
//   mock_eval_kernel         P stack programs (the zk_expr_op set) at every row of the 2^k-row domain in ONE launch, three-valued:
//                            a value is Real(v) or Poison.  Per program and row one status byte (0 Real zero, 1 Real non-zero,
//                            2 Poison) and, when asked for, the value (0 at Poison entries).
//   flags_count / flags_scan / flags_emit
//                            the positions of the first `cap` non-zero bytes of a status array, ascending, with their bytes and
//                            the total: reduce per workgroup, one workgroup scans the block totals, the emit pass writes in
//                            order.  No atomics pick a position, so the output is the same on every run.
//   mock_permutation_kernel  one lane per cell of the permutation's columns: the partner cell through the Assembly mapping, a
//                            status byte [ncols][n]
//   mock_lookup_keys_kernel / mock_lookup_find_kernel
//                            a one-expression lookup, exact: the usable table rows as canonical 256-bit keys (a Poison entry is
//                            the all-ones key, which no field element has: equal to Poison, above every value -- upstream's
//                            derived order), sorted by the LSD passes of zk_lookup_kernels.h; then one lane per usable input
//                            row searches the sorted keys and writes a status byte.
// House rules of zk_lookup_kernels.h: no inter-workgroup waits, every cross-workgroup step is a launch, every table index is
// clamped in the kernel although the host validates it.
//
// Limits of mock_eval_kernel.  Per program those of expr_eval_kernel: <= 512 ops, stack depth <= 8, <= 64 columns, <= 32
// constants.  Per call <= MOCK_MAX_PROGRAMS = 1024 programs.  The grid is one-dimensional, program-major: MOCK_GRID_X = 512
// workgroups of 128 rows per program (2^16 rows a trip of the grid-stride loop), times the number of programs.
//
// Arithmetic: the saturated Fe<F> routines of zk_field.h.  fe_add / fe_sub / fe_neg / fe_mul return the canonical residue in
// [0, p) when their operands are below p (each ends in one conditional subtraction or addition of p; fe_sub of equal operands and
// fe_neg of 0 borrow nothing and give 0), so Real(v) is zero exactly when all limbs are zero -- PROVIDED the operands are
// canonical.  Constants come from the host in canonical Montgomery form; a cell is reduced once as it is loaded (a stored word in
// [p, 2p) is taken for its residue), which makes a + (p - a), a - a, (p - 1) + 1 and every product with a zero operand exact.
#pragma once
#include "zk_rt.h"
#include "zk_field.h"
#include "zk_poly_kernels.h"
#include "zk_lookup_kernels.h"

namespace zk {

constexpr uint32_t MOCK_MAX_PROGRAMS = 1024;
constexpr uint32_t MOCK_GRID_X = 512;          // workgroups of EXPR_WG rows per program
constexpr uint32_t MOCK_ST_ZERO = 0, MOCK_ST_NONZERO = 1, MOCK_ST_POISON = 2;

// prog: the programs back to back, one 64-bit word per op (op | rot << 16 | arg << 32); offs: n_programs + 1 word offsets;
// poison_from[c]: the cells of column c at rows >= poison_from[c] are Poison.  Stack as in expr_eval_kernel (top in registers,
// the rest limb-major in LDS) plus `pm`, one Poison bit per stack slot; the value of a Poison slot is never used.
template <class F>
__global__ void __launch_bounds__(EXPR_WG) mock_eval_kernel(const uint64_t* __restrict__ prog, const uint32_t* __restrict__ offs, uint32_t n_programs,
                                                            uint32_t bx, const Fe<F>* const* __restrict__ cols, const uint32_t* __restrict__ poison_from,
                                                            uint32_t n_cols, const Fe<F>* __restrict__ consts, uint32_t n_consts, uint32_t log_n,
                                                            Fe<F>* __restrict__ vals, uint8_t* __restrict__ status) {
    __shared__ uint32_t stack[EXPR_STACK * F::N * EXPR_WG];
    const uint32_t lane = threadIdx.x;
    const uint32_t p = blockIdx.x / bx, xb = blockIdx.x % bx;
    if (p >= n_programs) return;
    const uint32_t k0 = offs[p], k1 = offs[p + 1];
    const uint64_t n = 1ull << log_n, mask = n - 1;
    for (uint64_t i = (uint64_t)xb * EXPR_WG + lane; i < n; i += (uint64_t)bx * EXPR_WG) {
        uint32_t sp = 0, pm = 0;
        Fe<F> tos;
        fe_zero(tos);
        for (uint32_t k = k0; k < k1; k++) {
            const uint64_t w = prog[k];
            const uint32_t op = (uint32_t)(w & 0xff), arg = (uint32_t)(w >> 32);
            const int32_t rot = (int32_t)(int16_t)(uint16_t)(w >> 16);
            if (op <= 1) {
                if (sp >= EXPR_STACK) break;
                if (sp >= 1) {
                    ZK_UNROLL
                    for (int l = 0; l < F::N; l++) stack[((sp - 1) * F::N + l) * EXPR_WG + lane] = tos.v[l];
                }
                if (op == 0) {
                    const uint32_t c = arg < n_cols ? arg : 0;
                    const uint64_t j = (i + (uint64_t)(int64_t)rot) & mask;
                    tos = cols[c][j];
                    fe_reduce_once<F>(tos.v);
                    if (j >= poison_from[c]) pm |= 1u << sp;
                } else {
                    tos = consts[arg < n_consts ? arg : 0];
                }
                sp++;
            } else if (op == 5 || op == 6) {
                if (sp < 1) break;
                const uint32_t bit = 1u << (sp - 1);
                if (op == 5) {
                    fe_neg(tos, tos);                                   // keeps the kind
                } else {
                    const Fe<F> y = consts[arg < n_consts ? arg : 0];
                    if (pm & bit) {                                     // Poison scaled by 0 is Real(0), by anything else Poison
                        if (fe_is_zero(y)) {
                            pm &= ~bit;
                            fe_zero(tos);
                        }
                    } else {
                        fe_mul(tos, tos, y);
                    }
                }
            } else {
                if (sp < 2) break;
                Fe<F> x;
                ZK_UNROLL
                for (int l = 0; l < F::N; l++) x.v[l] = stack[((sp - 2) * F::N + l) * EXPR_WG + lane];
                const uint32_t bt = 1u << (sp - 1), bx_ = 1u << (sp - 2);
                const bool pt = (pm & bt) != 0, px = (pm & bx_) != 0;
                bool pr;                                                // the result is Poison
                if (op == 4) {
                    // Real(0) x Poison = Real(0) in either order; Real(non-zero) x Poison and Poison x Poison are Poison
                    const bool zero_side = (!px && fe_is_zero(x)) || (!pt && fe_is_zero(tos));
                    pr = (px || pt) && !zero_side;
                    if (px || pt)
                        fe_zero(x);
                    else
                        fe_mul(x, x, tos);
                } else {
                    pr = px || pt;                                      // x - x of a poisoned cell is Poison, not 0
                    if (op == 2)
                        fe_add(x, x, tos);
                    else
                        fe_sub(x, x, tos);
                }
                pm = (pm & ~(bt | bx_)) | (pr ? bx_ : 0u);
                tos = x;
                sp--;
            }
        }
        const bool poison = (pm & 1u) != 0;
        const uint64_t o = (uint64_t)p * n + i;
        status[o] = (uint8_t)(poison ? MOCK_ST_POISON : fe_is_zero(tos) ? MOCK_ST_ZERO : MOCK_ST_NONZERO);
        if (vals) {
            if (poison) fe_zero(tos);
            vals[o] = tos;
        }
    }
}

// ---- compaction of a status array ----
constexpr uint32_t FLAGS_WG = 256;                       // lanes per workgroup
constexpr uint32_t FLAGS_CHUNK = FLAGS_WG * 16;          // bytes per workgroup: one 16-byte load per lane

// bit j of the result: byte 16 g + j of the array is non-zero (bytes past N count as zero); words[] gets the 16 bytes.  The array
// is 16-byte aligned, so a whole group is one wide load; the last, partial group is read byte by byte.
// (The three kernels are templates like the lk_ kernels, so that every field unit owns its copy; the bytes carry no field.)
__device__ __forceinline__ uint32_t flags_load(const uint8_t* st, uint64_t N, uint64_t g, uint32_t* words) {
    const uint64_t lo = g * 16;
    words[0] = words[1] = words[2] = words[3] = 0;
    if (lo + 16 <= N) {
        const uint4 q = *reinterpret_cast<const uint4*>(st + lo);
        words[0] = q.x;
        words[1] = q.y;
        words[2] = q.z;
        words[3] = q.w;
    } else {
        for (uint32_t j = 0; lo + j < N; j++) words[j >> 2] |= (uint32_t)st[lo + j] << (8 * (j & 3));
    }
    uint32_t m = 0;
    for (uint32_t j = 0; j < 16; j++)
        if ((words[j >> 2] >> (8 * (j & 3))) & 255u) m |= 1u << j;
    return m;
}

// tot[block] = non-zero bytes of the block's chunk: 16 ballots and popcounts per wave, the four waves meet in LDS
template <class F>
__global__ void __launch_bounds__(FLAGS_WG) flags_count_kernel(const uint8_t* __restrict__ st, uint64_t N, uint32_t* __restrict__ tot) {
    __shared__ uint32_t wsum[FLAGS_WG / 64];
    uint32_t words[4];
    const uint32_t m = flags_load(st, N, (uint64_t)blockIdx.x * FLAGS_WG + threadIdx.x, words);
    uint32_t c = 0;
    for (uint32_t j = 0; j < 16; j++) c += (uint32_t)__popcll((unsigned long long)__ballot((m >> j) & 1u));
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < FLAGS_WG / 64; w++) s += wsum[w];
        tot[blockIdx.x] = s;
    }
}

// one workgroup: tot[] -> exclusive offsets (64-bit: N may exceed 2^32 flags), *total = the sum
template <class F>
__global__ void __launch_bounds__(FLAGS_WG) flags_scan_kernel(const uint32_t* __restrict__ tot, uint64_t* __restrict__ offs, uint32_t nblocks,
                                                              uint64_t* __restrict__ total) {
    __shared__ uint32_t s[FLAGS_WG];
    uint64_t carry = 0;
    for (uint32_t j0 = 0; j0 < nblocks; j0 += FLAGS_WG) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t v = j < nblocks ? tot[j] : 0u;
        uint32_t all;
        const uint32_t ex = lk_block_excl(v, s, &all);      // (a tile of 256 chunks holds at most 2^20 flags)
        if (j < nblocks) offs[j] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

// the flag at array position i with q non-zero bytes ahead of it goes to pos[q], kind[q] when q < cap
template <class F>
__global__ void __launch_bounds__(FLAGS_WG) flags_emit_kernel(const uint8_t* __restrict__ st, uint64_t N, const uint64_t* __restrict__ offs, uint64_t cap,
                                                              uint64_t* __restrict__ pos, uint8_t* __restrict__ kind) {
    __shared__ uint32_t s[FLAGS_WG];
    uint32_t words[4];
    const uint64_t g = (uint64_t)blockIdx.x * FLAGS_WG + threadIdx.x;
    const uint32_t m = flags_load(st, N, g, words);
    uint32_t all;
    uint64_t q = offs[blockIdx.x] + lk_block_excl((uint32_t)__popc(m), s, &all);
    for (uint32_t j = 0; j < 16; j++)
        if ((m >> j) & 1u) {
            if (q < cap) {
                pos[q] = g * 16 + j;
                kind[q] = (uint8_t)((words[j >> 2] >> (8 * (j & 3))) & 255u);
            }
            q++;
        }
}

// ---- copy constraints ----
constexpr uint32_t MOCK_PERM_GRID = 1024;      // workgroups of 256 cells: 2^18 cells a trip of the grid-stride loop

// status[c n + r] = 1 iff mapping[c][r] != (c, r) and (either end is Poison or the two stored values differ).  A mapping word
// outside the ncols x n grid is never used as an index: the cell gets 0 and *bad is raised.
template <class F>
__global__ void __launch_bounds__(256) mock_permutation_kernel(const uint64_t* __restrict__ mapping, const Fe<F>* const* __restrict__ cols,
                                                               const uint32_t* __restrict__ poison_from, uint64_t cells, uint64_t n, uint32_t ncols,
                                                               uint8_t* __restrict__ status, uint32_t* __restrict__ bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t m = mapping[i];
        const uint64_t row = m & 0xffffffffull, col = m >> 32;
        const uint64_t c = i / n, r = i % n;
        uint8_t s = 0;
        if (row >= n || col >= ncols) {
            *bad = 1;
        } else if (col != c || row != r) {
            if (r >= poison_from[c] || row >= poison_from[col])
                s = 1;
            else
                s = fe_eq(cols[c][r], cols[col][row]) ? 0 : 1;
        }
        status[i] = s;
    }
}

// ---- lookup membership, one expression wide ----
// key of a value: its canonical integer (below 2^255); of a Poison entry: all ones
template <class F>
__device__ __forceinline__ void mock_lookup_key(LkKey& k, const Fe<F>* vals, const uint8_t* st, uint64_t i) {
    if (st && st[i] == MOCK_ST_POISON) {
        for (int w = 0; w < 8; w++) k.w[w] = 0xffffffffu;
    } else {
        Fe<F> c;
        fe_from_mont(c, vals[i]);
        for (int w = 0; w < 8; w++) k.w[w] = c.v[w];
    }
}

// keys[i] = key of table row i < u, and the digit histogram the sort plans from (lk_keys_kernel's)
template <class F>
__global__ void __launch_bounds__(LK_WG) mock_lookup_keys_kernel(const Fe<F>* __restrict__ S, const uint8_t* __restrict__ s_status, uint32_t u,
                                                                  LkKey* __restrict__ keys, uint32_t* __restrict__ hist) {
    static_assert(F::N == 8, "256-bit keys");
    __shared__ uint32_t h[LK_DIGITS * 256];
    for (uint32_t j = threadIdx.x; j < LK_DIGITS * 256; j += LK_WG) h[j] = 0;
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * LK_WG; base < u; base += (uint64_t)gridDim.x * LK_WG) {
        const uint64_t i = base + threadIdx.x;
        const bool valid = i < u;
        LkKey k;
        for (int w = 0; w < 8; w++) k.w[w] = 0;
        if (valid) {
            mock_lookup_key<F>(k, S, s_status, i);
            keys[i] = k;
        }
        for (uint32_t d = 0; d < LK_DIGITS; d++) lk_hist_add(&h[d * 256], lk_digit(k, d), valid);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < LK_DIGITS * 256; j += LK_WG)
        if (h[j]) atomicAdd(&hist[j], h[j]);
}

__device__ __forceinline__ int mock_key_cmp(const LkKey& a, const LkKey& b) {      // -1, 0, 1: a < b, a == b, a > b
    int r = 0;
    for (int w = 0; w < 8; w++)      // from the least significant word up: a more significant difference overrides
        if (a.w[w] != b.w[w]) r = a.w[w] < b.w[w] ? -1 : 1;
    return r;
}

// status[r] = 0 when the key of input row r is among the u sorted keys, 1 when it is not
template <class F>
__global__ void __launch_bounds__(LK_WG) mock_lookup_find_kernel(const Fe<F>* __restrict__ A, const uint8_t* __restrict__ a_status, uint32_t u,
                                                                  const LkKey* k0, const LkKey* k1, const uint32_t* __restrict__ meta,
                                                                  uint8_t* __restrict__ status) {
    const LkKey* keys = meta[LK_M_SEL + LK_DIGITS] ? k1 : k0;
    for (uint64_t r = (uint64_t)blockIdx.x * LK_WG + threadIdx.x; r < u; r += (uint64_t)gridDim.x * LK_WG) {
        LkKey x;
        mock_lookup_key<F>(x, A, a_status, r);
        uint32_t lo = 0, hi = u;                 // the first key >= x lies in [lo, hi]
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (mock_key_cmp(keys[mid], x) < 0) lo = mid + 1;
            else hi = mid;
        }
        status[r] = (uint8_t)((lo < u && mock_key_cmp(keys[lo], x) == 0) ? 0 : 1);
    }
}

}  // namespace zk
