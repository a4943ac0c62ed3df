// cluster.hip — connected components of the solid particles over a neighbour list, and the mask of the largest one, on gfx950.
//
// No reference counterpart.  What nucleation studies bias is not the number of solid particles but the size of the LARGEST CONNECTED
// CLUSTER of them (ten Wolde, Ruiz-Montero and Frenkel; PLUMED's DFSCLUSTERING + CLUSTER_NATOMS / CLUSTER_PROPERTIES).  This unit labels the
// clusters and hands back the 0 / 1 mask of the largest; it knows nothing of what made the per-particle value v, so any variable that has
// one per particle can use it (steinhardt_local.hip, coordination.hip and tetrahedral.hip do).  Definition of nodes, edges and outputs:
// include/mtd_abi.h, "Clusters".
//
// Lock-free union-find with hooking by the smaller index: a root is only ever hooked under a SMALLER index, so the root of a component
// is its smallest member when the link pass is done, whatever order the edges arrived in.
//
//   INVARIANT   parent[x] <= x at all times, and parent[x] only ever DECREASES.  Init writes parent[x] = x; a hook is
//               atomicCAS(&parent[hi], hi, lo) with lo < hi, which succeeds only while hi is still a root; path halving is
//               atomicMin(&parent[x], grandparent), and a grandparent is never above the parent.  Two consequences:
//                 - every `find` walks a strictly decreasing chain of indices and ends after at most N steps, even on values that are
//                   stale (an old parent of x is still an ancestor of x: it is only a longer way to the same root);
//                 - every retry of a failed hook starts from the value the CAS returned, which is below hi: at most N retries.
//   NO WAITING  no wave ever waits for another wave's progress: no flag is spun on, no lock is taken.  A lane loops only on what it
//               read itself, and each trip lowers an index.
//   BITS        only integer atomics (compare-and-swap, min, add, max): every output is a function of the input alone, two calls give
//               the same bits whatever the arrival order.
//
// Five launches, stream-ordered, nothing read back:
//   k_cluster_init     parent[i] = i for a node, NONE else; size, the summary and the key of the pick zeroed
//   k_cluster_link     the rows walked by the walk of row_walk.hpp (four lanes per row, local entries only: a ghost entry j >= N is
//                      skipped, its position is not even loaded), the pair test with r_link as the cut-off; an entry whose other end is a
//                      node unites the two.  The list need not be symmetric, so EVERY entry that passes unites — the hook itself always
//                      goes from the larger root to the smaller; the second sight of an edge of a symmetric list costs two finds
//   k_cluster_flatten  label[i] = find(i) (reads only); members counted at the root: the lanes of a wave that share a label add once
//                      (in a crystal consecutive indices mostly do: a 100 000-member cluster is 1 600 adds on its root, not 100 000)
//   k_cluster_pick     64-bit max of (size << 32) | ~root over the roots — most members, a tie to the smaller root — reduced per block
//                      first: one atomic per block; and the number of clusters
//   k_cluster_mask     w[i] = 1.0 for label[i] == the root picked, 0.0 else; the summary
// Cost at 256 000 particles (profiles/r21): 17.5 us with nothing solid, 42 us for a nucleus of 1 263, 91 us for one of 10 255, 583 us when
// the whole box is one cluster — there the link pass is bound by its atomics (2.9 million single-lane requests per call).
// The parents are read with agent-scope relaxed loads in the link pass (they are written by other compute dies while it runs); a stale
// value is harmless (above).  After a launch everything is visible: flatten, pick and mask read plainly.
#include "mtd_device.hpp"
#include "row_walk.hpp"
#include "dispatch.hpp"
#include "cluster_host.hpp"

#include <cstring>

namespace
{

using namespace mtd;

constexpr int CL_THREADS = 256;
constexpr int CL_G = 4;                                    // lanes per row, as the Steinhardt passes: rows of 40 - 60 entries
constexpr int CL_PPB = CL_THREADS / CL_G;
constexpr unsigned int CL_MAX_BLOCKS = 1024;
constexpr unsigned int CL_NONE = MTD_CLUSTER_NONE;

// the scratch: every segment starts on a multiple of 16 bytes
struct ClScratch
    {
    unsigned int *parent, *label, *size, *summary;         // summary: 4 words, then the 64-bit key of the pick behind them
    unsigned long long *best;
    double *w;
    size_t total;                                          // bytes
    };

ClScratch cl_scratch(void *scratch, const size_t n)
    {
    const size_t words = (n + 3) & ~(size_t)3;             // n unsigned ints, rounded up to 16 bytes
    size_t at = 0;
    const auto take = [&](const size_t bytes)
        {
        char *p = scratch ? (char *)scratch + at : nullptr;
        at += bytes;
        return p;
        };
    ClScratch s;
    s.summary = (unsigned int *)take(16);
    s.best = (unsigned long long *)take(16);
    s.parent = (unsigned int *)take(4 * words);
    s.label = (unsigned int *)take(4 * words);
    s.size = (unsigned int *)take(4 * words);
    s.w = (double *)take(8 * ((n + 1) & ~(size_t)1));
    s.total = at;
    return s;
    }

__device__ __forceinline__ unsigned int cl_load(const unsigned int *p)
    {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

// the root of x, halving the path on the way: x -> parent -> grandparent, parent[x] lowered to the grandparent.  x is a node.
__device__ __forceinline__ unsigned int cl_find_halving(unsigned int *parent, unsigned int x)
    {
    unsigned int p = cl_load(parent + x);
    while (p != x)
        {
        const unsigned int g = cl_load(parent + p);
        if (g != p) atomicMin(parent + x, g);                // never raises parent[x]: the invariant
        x = p;
        p = g;
        }
    return x;
    }

// the root of x, reading only
__device__ __forceinline__ unsigned int cl_find(const unsigned int *parent, unsigned int x)
    {
    unsigned int p = parent[x];
    while (p != x)
        {
        x = p;
        p = parent[x];
        }
    return x;
    }

// unites the sets of a and b; returns the root of the union as far as this lane knows it (an ancestor of both: a good place to start the
// next find from).  b hanging directly under a's root is seen with one load: the common case once the trees are flat.
__device__ __forceinline__ unsigned int cl_unite(unsigned int *parent, unsigned int a, unsigned int b)
    {
    for (;;)
        {
        a = cl_find_halving(parent, a);
        if (cl_load(parent + b) == a) return a;
        b = cl_find_halving(parent, b);
        if (a == b) return a;
        const unsigned int hi = a > b ? a : b, lo = a > b ? b : a;
        const unsigned int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;                            // hi was a root and now hangs under lo
        a = old;                                             // hi had been hooked meanwhile: old < hi, go on from there
        b = lo;
        }
    }

template<typename S4>
__global__ __launch_bounds__(CL_THREADS) void k_cluster_init(const unsigned int N, const unsigned int type, const double v_min,
                                                             const S4 *__restrict__ postype, const double *__restrict__ v,
                                                             unsigned int *__restrict__ parent, unsigned int *__restrict__ size,
                                                             unsigned int *__restrict__ summary, unsigned long long *__restrict__ best)
    {
    const unsigned int stride = gridDim.x * blockDim.x;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride)
        {
        const Particle p = scalar4_traits<S4>::load(postype, i);
        const bool node = (unsigned int)p.type == type && v[i] >= v_min;          // NaN fails the comparison: not a node
        parent[i] = node ? i : CL_NONE;
        size[i] = 0;
        }
    if (blockIdx.x == 0 && threadIdx.x < 4) summary[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 4) *best = 0ull;
    }

template<typename S4>
__global__ __launch_bounds__(CL_THREADS) void k_cluster_link(const QlArgs<4> a, const S4 *__restrict__ postype,
                                                             const unsigned int *__restrict__ head_list,
                                                             const unsigned int *__restrict__ n_neigh,
                                                             const unsigned int *__restrict__ nlist, unsigned int *parent)
    {
    const unsigned int tid = threadIdx.x, p = tid / CL_G, q = tid % CL_G;
    const unsigned int n_chunks = (a.N + CL_PPB - 1) / CL_PPB;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * CL_PPB + p);
        if (c.i < a.N && cl_load(parent + c.i) == CL_NONE) c.cnt = 0;            // not a node: its row is not walked
        unsigned int up = c.i;                                                     // the lowest ancestor of i this lane has seen: finds start there
        row_walk_entries<CL_G, true, false>(a, postype, nlist, nullptr, c, q,
            [&](const double *, const unsigned int j, double, double, double, double)
                {
                if (cl_load(parent + j) != CL_NONE) up = cl_unite(parent, up, j);
                });
        }
    }

__global__ __launch_bounds__(CL_THREADS) void k_cluster_flatten(const unsigned int N, const unsigned int *__restrict__ parent,
                                                                unsigned int *__restrict__ label, unsigned int *size,
                                                                unsigned int *summary)
    {
    const unsigned int stride = gridDim.x * blockDim.x;
    const unsigned int rounds = (N + stride - 1) / stride;                        // every lane of a wave takes every round: ballots below
    unsigned int nodes = 0;
    for (unsigned int r = 0; r < rounds; ++r)
        {
        const unsigned int i = r * stride + blockIdx.x * blockDim.x + threadIdx.x;
        unsigned int l = CL_NONE;
        if (i < N && parent[i] != CL_NONE) l = cl_find(parent, i);
        if (i < N) label[i] = l;
        // the lanes of the wave that share a label add their count once
        bool todo = l != CL_NONE;
        nodes += todo ? 1u : 0u;
        unsigned long long left = __ballot(todo);
        while (left != 0ull)
            {
            const unsigned int lead = __builtin_amdgcn_readlane(l, __builtin_ctzll(left));
            const unsigned long long same = __ballot(todo && l == lead);
            if (todo && l == lead)
                {
                if ((unsigned int)__builtin_ctzll(same) == (threadIdx.x & 63u)) atomicAdd(size + lead, (unsigned int)__popcll(same));
                todo = false;
                }
            left &= ~same;
            }
        }
    // the number of nodes: one add per wave
    const unsigned int lane = threadIdx.x & 63u;
    unsigned int wave_nodes = nodes;
#pragma unroll
    for (int off = 1; off < MTD_WAVE; off <<= 1) wave_nodes += __shfl_xor(wave_nodes, off, MTD_WAVE);
    if (lane == 0 && wave_nodes) atomicAdd(summary + 3, wave_nodes);
    }

__global__ __launch_bounds__(CL_THREADS) void k_cluster_pick(const unsigned int N, const unsigned int *__restrict__ label,
                                                             const unsigned int *__restrict__ size, unsigned int *summary,
                                                             unsigned long long *best)
    {
    __shared__ unsigned long long s_key[CL_THREADS / MTD_WAVE];
    __shared__ unsigned int s_roots[CL_THREADS / MTD_WAVE];
    const unsigned int stride = gridDim.x * blockDim.x;
    unsigned long long key = 0ull;
    unsigned int roots = 0;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride)
        if (label[i] == i)
            {
            const unsigned long long k = ((unsigned long long)size[i] << 32) | (unsigned long long)(~i);
            key = k > key ? k : key;
            ++roots;
            }
#pragma unroll
    for (int off = 1; off < MTD_WAVE; off <<= 1)
        {
        const unsigned long long other = __shfl_xor(key, off, MTD_WAVE);
        key = other > key ? other : key;
        roots += __shfl_xor(roots, off, MTD_WAVE);
        }
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0)
        {
        s_key[wave] = key;
        s_roots[wave] = roots;
        }
    __syncthreads();
    if (threadIdx.x == 0)
        {
        for (unsigned int w = 1; w < CL_THREADS / MTD_WAVE; ++w)
            {
            key = s_key[w] > key ? s_key[w] : key;
            roots += s_roots[w];
            }
        if (key != 0ull) atomicMax(best, key);
        if (roots) atomicAdd(summary + 2, roots);
        }
    }

__global__ __launch_bounds__(CL_THREADS) void k_cluster_mask(const unsigned int N, const unsigned int *__restrict__ label,
                                                             const unsigned long long *__restrict__ best, double *__restrict__ w,
                                                             unsigned int *__restrict__ summary)
    {
    const unsigned long long key = *best;
    const unsigned int members = (unsigned int)(key >> 32);
    const unsigned int root = members ? ~(unsigned int)key : CL_NONE;             // no node at all: key == 0
    const unsigned int stride = gridDim.x * blockDim.x;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) w[i] = members && label[i] == root ? 1.0 : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        {
        summary[0] = root;
        summary[1] = members;
        }
    }

template<typename S4>
int cl_largest_impl(const unsigned int N, const void *d_postype, const mtd_box *box, const unsigned int *head, const unsigned int *nneigh,
                    const unsigned int *nlist, const unsigned int type, const double *d_v, const mtd_cluster_params &p, const ClScratch &sc,
                    hipStream_t s)
    {
    const double one = 1.0;
    QlArgs<4> a;                                           // the box, N, the type and r_link as the cut-off: what the walk reads
    const int rc = fill_args<4>(a, N, box, p.r_link, 0.0, 0, type, &one, 1, 0);
    if (rc) return rc;
    const S4 *postype = (const S4 *)d_postype;
    const unsigned int flat = row_blocks(N, CL_THREADS, CL_MAX_BLOCKS), rows = row_blocks(N, CL_PPB, 4 * CL_MAX_BLOCKS);
    const unsigned int few = row_blocks(N, CL_THREADS, 256);                      // pick: one atomic per block on one word
    k_cluster_init<S4><<<flat, CL_THREADS, 0, s>>>(N, type, p.v_min, postype, d_v, sc.parent, sc.size, sc.summary, sc.best);
    MTD_LAUNCH_CHECK();
    k_cluster_link<S4><<<rows, CL_THREADS, 0, s>>>(a, postype, head, nneigh, nlist, sc.parent);
    MTD_LAUNCH_CHECK();
    k_cluster_flatten<<<flat, CL_THREADS, 0, s>>>(N, sc.parent, sc.label, sc.size, sc.summary);
    MTD_LAUNCH_CHECK();
    k_cluster_pick<<<few, CL_THREADS, 0, s>>>(N, sc.label, sc.size, sc.summary, sc.best);
    MTD_LAUNCH_CHECK();
    k_cluster_mask<<<flat, CL_THREADS, 0, s>>>(N, sc.label, sc.best, sc.w, sc.summary);
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // namespace

extern "C" {

size_t mtd_cluster_scratch_bytes(unsigned int n_particles) { return cl_scratch(nullptr, n_particles).total; }

int mtd_cluster_largest(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                        const unsigned int *d_n_neigh, const unsigned int *d_nlist, unsigned int type, const double *d_v,
                        const mtd_cluster_params *p, void *d_scratch, const unsigned int **d_label, const unsigned int **d_size,
                        const double **d_w, const unsigned int **d_summary, mtd_stream_t stream)
    {
    if (!box || !d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    int rc = refuse_row_arrays(n_particles, d_postype && d_head_list && d_n_neigh && d_nlist && d_v, dtype, d_scratch, nullptr, 0);
    if (rc) return rc;
    rc = cluster_refuse(p);
    if (rc) return rc;
    const ClScratch sc = cl_scratch(d_scratch, n_particles);
    rc = dispatch_s4(dtype, [&](auto t)
        {
        return cl_largest_impl<typename decltype(t)::type>(n_particles, d_postype, box, d_head_list, d_n_neigh, d_nlist, type, d_v, *p, sc,
                                                           (hipStream_t)stream);
        });
    if (rc) return rc;
    if (d_label) *d_label = sc.label;
    if (d_size) *d_size = sc.size;
    if (d_w) *d_w = sc.w;
    if (d_summary) *d_summary = sc.summary;
    return MTD_SUCCESS;
    }

} // extern "C"
