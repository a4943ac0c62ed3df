// row_mask.hpp — the 0 / 1 mask of the largest cluster (cluster.hip) applied to a per-particle table between a unit's walk and its sums
// kernel, written once (coordination.hip: g'(n_i), one double per particle; tetrahedral.hip: the adjoint row, twelve).  The variable
// restricted to the largest cluster is (1 / N_type) sum_i w_i v_i with w piecewise constant, so the mask enters linearly: the table
// entry of a particle that is not a member becomes zero, and the unit's force pass then runs unchanged on the masked table.  k_row_mask,
// launched through row_mask; not on a hot path: one load of w_i and of v_i per particle, stores for the non-members only.  The read and
// write pattern is that of k_qll_cluster_apply (steinhardt_local.hip).  The kernel is static: a unit that includes this has its own
// copy, and the linker has nothing to merge.
#pragma once

#include "row_walk.hpp"

namespace mtd
{

constexpr int ROW_MASK_THREADS = 256;
constexpr int ROW_MASK_G = 8;                                       // lanes per particle: lane q takes the doubles q, q + 8, ... of its row
constexpr int ROW_MASK_PPB = ROW_MASK_THREADS / ROW_MASK_G;         // particles per block and round

// Every particle i < N with w[i] == 0: the row_doubles contiguous doubles at table + row_doubles i are set to ZERO — stored, not
// multiplied: a row that holds a non-finite number comes out 0 all the same.  A member's row stays as it is.  part[blockIdx.x] = this
// block's share of sum_i w_i v_i (v_i selected, not multiplied): lane 0 of a group adds its particles chunk by chunk, block_sum adds
// the lanes — the order of the walk kernels, no atomics, the same bits at every call.  v itself is not written: it is what the clusters
// were built from.  Every block of the launch writes its column, so with the block count of the walk no column of the row is stale.
static __global__ __launch_bounds__(ROW_MASK_THREADS) void k_row_mask(const unsigned int N, const unsigned int row_doubles,
                                                                      const double *__restrict__ w, const double *__restrict__ v,
                                                                      double *__restrict__ table, double *__restrict__ part)
    {
    __shared__ double s_red[16];
    const unsigned int tid = threadIdx.x, g = tid / ROW_MASK_G, q = tid % ROW_MASK_G;
    const unsigned int n_chunks = (N + ROW_MASK_PPB - 1) / ROW_MASK_PPB;
    double v_sum = 0.0;                                             // lane 0 of a group: sum w_i v_i over its chunks
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const unsigned int i = chunk * ROW_MASK_PPB + g;
        if (i >= N) continue;
        const bool member = w[i] != 0.0;                            // w is 0 or 1
        if (!member)
            for (unsigned int k = q; k < row_doubles; k += ROW_MASK_G) table[(size_t)row_doubles * i + k] = 0.0;
        if (q == 0 && member) v_sum += v[i];
        }
    const double sum = block_sum(v_sum, s_red);
    if (tid == 0) part[blockIdx.x] = sum;
    }

// k_row_mask in `blocks` blocks — the block count of the unit's walk, row_blocks(N, PPB, ROW_MAX_BLOCKS), whose columns of slot 0 it
// overwrites; the launch is grid-stride, so any count >= 1 covers every particle.  n_particles == 0 launches too: column 0 becomes 0.
inline void row_mask(const unsigned int n_particles, const unsigned int blocks, const unsigned int row_doubles, const double *w, const double *v,
                     double *table, double *part, hipStream_t s)
    {
    k_row_mask<<<blocks, ROW_MASK_THREADS, 0, s>>>(n_particles, row_doubles, w, v, table, part);
    }

}
