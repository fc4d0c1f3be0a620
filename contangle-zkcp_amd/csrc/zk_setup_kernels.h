// Groth16 key generation (ark-groth16 0.3 generator.rs generate_parameters, reached from the reference's `compile` at
// lib/src/zk/encryption.rs:169): everything between the R1CS matrices and the scalars of the fixed-base multiplications.
//   upstream: domain.evaluate_all_lagrange_coefficients(t)                    (ark-poly 0.3 domain/radix2/mod.rs)
//             LibsnarkReduction::instance_map_with_evaluation                 (r1cs_to_qap.rs: u, v, w from the matrices ROW by row,
//                                                                             u[index] += coeff * L_i -- a scatter)
//             cfg_iter!(..).map(|..| (beta a + alpha b + c) * gamma_inverse / delta_inverse), the powers of tau times zt / delta
//   here:     r1cs_col_count / u32_scan_* / r1cs_col_finish / r1cs_col_scatter   the column-major companion of a resident CSR
//                                      matrix (histogram of col_idx, scan, scatter), built once per handle on the device:
//                                      there are no 256-bit field atomics, so the scatter above becomes a gather per column
//             r1cs_matvec_t_kernel       out[j] = sum_i M[i][j] x[i], one lane per column (a variable appears in a few rows)
//             r1cs_matvec_t_long_kernel  one workgroup per column longer than R1CS_LONG_ROW terms (variable 0, the packed inputs)
//             lagrange_den / lagrange_scale   L_i(tau) = (tau^m - 1)/m * w^i / (tau - w^i) around the batch inversion
//             groth16_abc_kernel         (beta u + alpha v + w) / gamma for the inputs, / delta for the rest, one pass
//             groth16_h_scalars_kernel   tau^i * zt / delta
// All of them stream HBM with at most a handful of Montgomery products per element; powers come from the two small tables
// of zk_ntt_kernels.h (PowTables), never from an m-entry table.
#pragma once
#include "zk_rt.h"
#include "zk_field.h"
#include "zk_ntt_kernels.h"
#include "zk_r1cs_kernels.h"

namespace zk {

constexpr uint32_t TSCAN_WG = 256;   // lanes of a scan workgroup
constexpr uint32_t TSCAN_K = 16;     // counters per lane: 4096 per workgroup

// cnt[c] = number of terms in column c  (cnt zeroed by the caller; col[k] < n_cols was checked at upload)
template <class F>
__global__ void __launch_bounds__(256) r1cs_col_count_kernel(const uint32_t* __restrict__ col, uint64_t nnz, uint32_t* __restrict__ cnt) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (uint64_t)gridDim.x * blockDim.x) atomicAdd(&cnt[col[k]], 1u);
}

// inclusive Hillis-Steele over one value per lane of a 256-lane workgroup; returns the inclusive sum of the calling lane
__device__ __forceinline__ uint32_t u32_scan_wg(uint32_t* part, uint32_t v) {
    const uint32_t tid = threadIdx.x;
    part[tid] = v;
    __syncthreads();
    uint32_t acc = v;
    for (uint32_t d = 1; d < TSCAN_WG; d <<= 1) {
        const uint32_t o = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        acc += o;
        part[tid] = acc;
        __syncthreads();
    }
    return acc;
}

// exclusive sum scan, phase 1: out[i] = sum of in[.. i) INSIDE the workgroup's 4096 counters, tot[b] = the workgroup's total
template <class F>
__global__ void __launch_bounds__(TSCAN_WG) u32_scan_block_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                  uint32_t* __restrict__ tot, uint64_t n) {
    __shared__ uint32_t part[TSCAN_WG];
    const uint64_t lo = ((uint64_t)blockIdx.x * TSCAN_WG + threadIdx.x) * TSCAN_K;
    uint32_t v[TSCAN_K], run = 0;
    for (uint32_t k = 0; k < TSCAN_K; k++) {
        v[k] = lo + k < n ? in[lo + k] : 0u;
        run += v[k];
    }
    const uint32_t incl = u32_scan_wg(part, run);
    uint32_t excl = incl - run;
    for (uint32_t k = 0; k < TSCAN_K; k++) {
        if (lo + k < n) out[lo + k] = excl;
        excl += v[k];
    }
    if (threadIdx.x == TSCAN_WG - 1) tot[blockIdx.x] = incl;
}

// phase 2, one workgroup: tot[b] <- sum of tot[.. b), 256 totals at a time with a running carry
template <class F>
__global__ void __launch_bounds__(TSCAN_WG) u32_scan_totals_kernel(uint32_t* __restrict__ tot, uint32_t nblocks) {
    __shared__ uint32_t part[TSCAN_WG];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += TSCAN_WG) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? tot[i] : 0u;
        const uint32_t incl = u32_scan_wg(part, v);
        const uint32_t carry = carry_s;
        if (i < nblocks) tot[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == TSCAN_WG - 1) carry_s = carry + incl;
        __syncthreads();
    }
}

// phase 3 and the bookkeeping of the transposition: col_ptr[j] gets its workgroup's offset; cnt[j] becomes the scatter cursor of
// column j (= col_ptr[j]); columns longer than R1CS_LONG_ROW are appended to long_cols (in no particular order)
template <class F>
__global__ void __launch_bounds__(256) r1cs_col_finish_kernel(uint32_t* __restrict__ col_ptr, uint32_t* __restrict__ cnt,
                                                              const uint32_t* __restrict__ tot, uint64_t n_cols, uint32_t* __restrict__ long_cols,
                                                              uint32_t* __restrict__ n_long) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= n_cols; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = col_ptr[j] + tot[j / (TSCAN_WG * TSCAN_K)];
        const uint32_t c = cnt[j];
        col_ptr[j] = p;
        cnt[j] = p;
        if (j < n_cols && c > R1CS_LONG_ROW) long_cols[atomicAdd(n_long, 1u)] = (uint32_t)j;
    }
}

// term k of the CSR matrix -> its slot in column col[k]: the row index (found by bisection in row_ptr: the rows of one wave's
// 64 consecutive terms share their path) and a copy of the coefficient, so that a column's terms are contiguous for the gather
template <class F>
__global__ void __launch_bounds__(256) r1cs_col_scatter_kernel(const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
                                                               const Fe<F>* __restrict__ val, uint64_t n_rows, uint64_t nnz,
                                                               uint32_t* __restrict__ cursor, uint32_t* __restrict__ t_row, Fe<F>* __restrict__ t_val) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = n_rows - 1;        // the first row i with row_ptr[i + 1] > k; nnz > 0 implies n_rows > 0
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (row_ptr[mid + 1] <= k) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t pos = atomicAdd(&cursor[col[k]], 1u);
        t_row[pos] = (uint32_t)lo;
        t_val[pos] = val[k];
    }
}

// out[j] = sum_i M[i][j] x[i] over the rows i < x_len (+ extra[j] for j < n_extra) for j < n_cols, columns longer than
// R1CS_LONG_ROW are left to the long kernel; extra[j] alone for n_cols <= j < out_len (0 beyond n_extra)
template <class F>
__global__ void __launch_bounds__(256) r1cs_matvec_t_kernel(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ t_row,
                                                            const Fe<F>* __restrict__ t_val, const Fe<F>* __restrict__ x, uint64_t x_len,
                                                            Fe<F>* __restrict__ out, uint64_t n_cols, uint64_t out_len,
                                                            const Fe<F>* __restrict__ extra, uint64_t n_extra) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < out_len; j += (uint64_t)gridDim.x * blockDim.x) {
        Fe<F> acc;
        fe_zero(acc);
        if (j < n_cols) {
            const uint32_t k0 = col_ptr[j], k1 = col_ptr[j + 1];
            if (k1 - k0 > R1CS_LONG_ROW) continue;
            for (uint32_t k = k0; k < k1; k++) {
                const uint32_t r = t_row[k];
                if (r >= x_len) continue;
                Fe<F> c = t_val[k], xv = x[r];
                r1cs_term(acc, c, xv);
            }
        }
        if (j < n_extra) {
            Fe<F> e = extra[j];
            fe_add(acc, acc, e);
        }
        out[j] = acc;
    }
}

// grid = number of long columns; one workgroup of 256 lanes strides over the column's terms and tree-sums in LDS
template <class F>
__global__ void __launch_bounds__(256) r1cs_matvec_t_long_kernel(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ t_row,
                                                                 const Fe<F>* __restrict__ t_val, const Fe<F>* __restrict__ x, uint64_t x_len,
                                                                 Fe<F>* __restrict__ out, const uint32_t* __restrict__ long_cols,
                                                                 const Fe<F>* __restrict__ extra, uint64_t n_extra) {
    __shared__ Fe<F> part[256];
    const uint32_t j = long_cols[blockIdx.x];
    const uint32_t k0 = col_ptr[j], k1 = col_ptr[j + 1];
    Fe<F> acc;
    fe_zero(acc);
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += blockDim.x) {
        const uint32_t r = t_row[k];
        if (r >= x_len) continue;
        Fe<F> c = t_val[k], xv = x[r];
        r1cs_term(acc, c, xv);
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            Fe<F> o = part[threadIdx.x + d];
            fe_add(acc, acc, o);
            part[threadIdx.x] = acc;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (j < n_extra) {
            Fe<F> e = extra[j];
            fe_add(acc, acc, e);
        }
        out[j] = acc;
    }
}

// out[i] = tau - w^i: the denominators of the Lagrange coefficients (tau is outside the domain: none of them is zero)
template <class F>
__global__ void __launch_bounds__(256) lagrange_den_kernel(Fe<F>* __restrict__ out, uint64_t m, Fe<F> tau, PowTables<F> pw) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        Fe<F> x, d;
        fe_one(x);
        mul_pow(x, pw, i);
        fe_sub(d, tau, x);
        out[i] = d;
    }
}

// a[i] <- a[i] * w^i * s with a[i] = 1 / (tau - w^i) and s = (tau^m - 1) / m: L_i(tau)
template <class F>
__global__ void __launch_bounds__(256) lagrange_scale_kernel(Fe<F>* __restrict__ a, uint64_t m, Fe<F> s, PowTables<F> pw) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        Fe<F> x = a[i];
        fe_mul(x, x, s);
        mul_pow(x, pw, i);
        a[i] = x;
    }
}

// out[j] = (beta u[j] + alpha v[j] + w[j]) * (j < num_inputs ? 1 / gamma : 1 / delta): the scalars of gamma_abc_g1 followed by
// those of l_query, one pass over u, v, w.  out may be one of the inputs.
template <class F>
__global__ void __launch_bounds__(256) groth16_abc_kernel(const Fe<F>* u, const Fe<F>* v, const Fe<F>* w, Fe<F>* out, uint64_t n_vars,
                                                          uint64_t num_inputs, Fe<F> alpha, Fe<F> beta, Fe<F> gamma_inv, Fe<F> delta_inv) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_vars; j += (uint64_t)gridDim.x * blockDim.x) {
        Fe<F> a = u[j], b = v[j], c = w[j];
        fe_mul(a, a, beta);
        fe_mul(b, b, alpha);
        fe_add(a, a, b);
        fe_add(a, a, c);
        if (j < num_inputs) fe_mul(a, a, gamma_inv);
        else fe_mul(a, a, delta_inv);
        out[j] = a;
    }
}

// out[i] = tau^i * s, s = zt / delta: the scalars of h_query
template <class F>
__global__ void __launch_bounds__(256) groth16_h_scalars_kernel(Fe<F>* __restrict__ out, uint64_t n, Fe<F> s, PowTables<F> pw) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        Fe<F> x = s;
        mul_pow(x, pw, i);
        out[i] = x;
    }
}

}  // namespace zk
