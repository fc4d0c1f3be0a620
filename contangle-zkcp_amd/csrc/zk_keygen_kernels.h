// halo2 key generation (halo2_proofs 0.2 plonk/keygen.rs keygen_vk / keygen_pk, plonk/permutation/keygen.rs
// Assembly::build_vk / build_pk): the one step between the copy constraints and the key that is not a transform or a commitment.
//   upstream: for every column i and row j (on CPU threads)   permutations[i][j] = deltaomega[permuted_i][permuted_j]
//             with (permuted_i, permuted_j) = mapping[i][j] and deltaomega[c][r] = delta^c omega^r, a ncols x n table
//   here:     perm_sigma_kernel    out[c n + j] = delta^col omega^row for mapping[c n + j] = col << 32 | row
// The table upstream gathers from is ncols x n elements (512 MB for 16 columns of 2^20 rows), and even one column of it, omega^row,
// is a random 32-byte read into 32 MB per cell.  omega^row comes instead from the two small tables of zk_ntt_kernels.h
// (PowTables: omega^j for j < 1024 and omega^(1024 j), 64 KB together at k = 20 -- they stay in every XCD's 4 MiB L2 however the
// mapping scatters the rows, and they are the tables the permutation product of the same domain already keeps cached) and
// delta^col from a ncols-entry table: two Montgomery products, one coalesced 8-byte read and one coalesced 32-byte store per cell.
// The mapping is data the library did not produce: a cell that names a row >= n or a column >= ncols is never used as an index;
// it gets 0 in its own slot and raises the status word, which the host reads once at the end of the call.
#pragma once
#include "zk_rt.h"
#include "zk_field.h"
#include "zk_ntt_kernels.h"

namespace zk {

template <class F>
__global__ void __launch_bounds__(256) perm_sigma_kernel(const uint64_t* __restrict__ mapping, Fe<F>* __restrict__ out, uint64_t cells, uint64_t n,
                                                         uint32_t ncols, const Fe<F>* __restrict__ dpow, PowTables<F> wpow,
                                                         uint32_t* __restrict__ status) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t m = mapping[i];
        const uint64_t row = m & 0xffffffffull, col = m >> 32;
        Fe<F> x;
        if (row >= n || col >= ncols) {      // (row < n keeps both table indices of mul_pow in range: lo has min(n, 1024) entries)
            *status = 1;
            fe_zero(x);
        } else {
            x = dpow[col];
            mul_pow(x, wpow, row);
        }
        out[i] = x;
    }
}

}  // namespace zk
