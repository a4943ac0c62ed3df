// nlist.hip — cell-list neighbour build on the device (mtd_nlist_*), in HOOMD's array layout: the neighbours of particle i are
// nlist[head_list[i] .. head_list[i] + n_neigh[i]).  HOOMD's NeighborList is not part of the reference plugin; this serves the
// stand-alone path (cv.nlist_cell(device=True)), specified by its result: the set of pairs with |minimum_image(r_i - r_j)|^2 <=
// r_list^2 in fp64 under the minimum-image convention of mtd_box (steinhardt.hip::min_image, HOOMD BoxDim::minImage).
//
// One rebuild, all on the stream:
//   a. BIN     k_nl_cell_count   cell of every particle (locals and ghosts) from its fractional coordinates, one non-returning
//                                integer atomic per particle on its cell's counter (counters spread over ~N/4 words: no word is hot)
//              scan              exclusive scan of the cell counters -> cell_start
//              k_nl_scatter      particle index into its cell's segment, slot from a returning atomic (arrival order)
//              k_nl_order        one thread per slot: rank of its index inside the segment = number of smaller indices there, record
//                                (x, y, z, index, type) written to cell_start + rank.  The cell-ordered copy therefore does NOT depend
//                                on the arrival order of the atomics, and neither does anything below.
//   b. COUNT   k_nl_pairs<false> one thread per record of a local particle: walks the (at most 3 x 3 x 3, each cell at most once)
//                                neighbouring cells, counts the partners within r_list -> n_neigh[i]
//              scan              exclusive scan over the particles -> head_list; the total goes to the host (pinned word): the ONE
//                                synchronisation of a rebuild, needed to size nlist
//   c. FILL    k_nl_pairs<true>  the same walk, partners stored at head_list[i] + k: sizes are exact, no row capacity, no overflow path
//   d. CHECK   k_nl_check        per step: one thread per record, |minimum_image(r_now - r_at_build)|^2 > (r_buff / 2)^2 -> stamps the
//                                flag word (pinned host memory, written only when a particle did move that far)
//
// The pair walks read the cell-ordered records (32 B each, contiguous inside a cell) straight from global memory: a cell holds a
// handful of particles (about rho r_list^3), the lanes of a wave are consecutive records, i.e. the same or adjacent cells, so
// they ask for the same few lines at the same time, and the whole copy (8 MB at 256 000 particles) stays in the L2s.  Staging
// through LDS would need the union of the neighbourhoods of a block's cells, which for blocks that are runs of the x-fastest cell
// order is nine separate runs per block, with a barrier each: more instructions for loads that already hit.  DESIGN.md 4.10.
#include "mtd_device.hpp"

#include <cmath>
#include <cstring>
#include <new>

namespace
{

using namespace mtd;

constexpr int NL_THREADS = 256;
constexpr unsigned int NL_SCAN_TILE = 1024;      // elements per block of the scan: 256 threads x 4

struct NlBox
    {
    double B[3][3];          // reciprocal rows without 2 pi: fractional coordinate f_k = B_k . r + off_k
    double off[3];
    double L[3], Linv[3];    // Linv[k] = 0 in a non-periodic direction: no image is ever taken there
    double xy, xz, yz;
    unsigned int dim[3];     // cells per direction
    unsigned int periodic[3];
    };

// one record of the cell-ordered copy: position widened to fp64, original index and type id
struct __attribute__((aligned(32))) NlRecord
    {
    double x, y, z;
    unsigned int idx;
    int type;
    };

__device__ __forceinline__ void nl_min_image(const NlBox &b, double &x, double &y, double &z)
    {
    // HOOMD BoxDim::minImage (as steinhardt.hip::min_image), periodic directions only
    double img = rint(z * b.Linv[2]);
    z -= b.L[2] * img;
    y -= b.L[2] * b.yz * img;
    x -= b.L[2] * b.xz * img;
    img = rint(y * b.Linv[1]);
    y -= b.L[1] * img;
    x -= b.L[1] * b.xy * img;
    x -= b.L[0] * rint(x * b.Linv[0]);
    }

// cell coordinate along k of fractional coordinate f: wrapped into the box when periodic, clamped to the outermost cells when not
// (monotonic, so two particles closer than a cell width stay in the same or in adjacent cells)
__device__ __forceinline__ unsigned int nl_cell_coord(const NlBox &b, const int k, double f)
    {
    const unsigned int n = b.dim[k];
    if (b.periodic[k]) f -= floor(f);
    if (!(f > 0.0)) return 0;                   // also NaN
    const double c = floor(f * (double)n);
    return c >= (double)n ? n - 1 : (unsigned int)c;
    }

__device__ __forceinline__ unsigned int nl_cell_of(const NlBox &b, const Particle &p)
    {
    const double f0 = b.B[0][0] * p.x + b.B[0][1] * p.y + b.B[0][2] * p.z + b.off[0];
    const double f1 = b.B[1][0] * p.x + b.B[1][1] * p.y + b.B[1][2] * p.z + b.off[1];
    const double f2 = b.B[2][0] * p.x + b.B[2][1] * p.y + b.B[2][2] * p.z + b.off[2];
    return (nl_cell_coord(b, 2, f2) * b.dim[1] + nl_cell_coord(b, 1, f1)) * b.dim[0] + nl_cell_coord(b, 0, f0);
    }

// ---- a. bin ----------------------------------------------------------------------------------------------------------------------

template<typename S4>
__global__ void __launch_bounds__(NL_THREADS) k_nl_cell_count(const NlBox b, const unsigned int n, const S4 *__restrict__ pos,
                                                              unsigned int *__restrict__ cell_of, unsigned int *__restrict__ cell_count)
    {
    const unsigned int i = blockIdx.x * NL_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned int c = nl_cell_of(b, scalar4_traits<S4>::load(pos, i));
    cell_of[i] = c;
    atomicAdd(&cell_count[c], 1u);
    }

__global__ void __launch_bounds__(NL_THREADS) k_nl_scatter(const unsigned int n, const unsigned int *__restrict__ cell_of,
                                                           const unsigned int *__restrict__ cell_start, unsigned int *__restrict__ cell_fill,
                                                           unsigned int *__restrict__ slot_idx)
    {
    const unsigned int i = blockIdx.x * NL_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned int c = cell_of[i];
    slot_idx[cell_start[c] + atomicAdd(&cell_fill[c], 1u)] = i;
    }

template<typename S4>
__global__ void __launch_bounds__(NL_THREADS) k_nl_order(const unsigned int n, const S4 *__restrict__ pos, const unsigned int *__restrict__ cell_of,
                                                         const unsigned int *__restrict__ cell_start, const unsigned int *__restrict__ cell_count,
                                                         const unsigned int *__restrict__ slot_idx, NlRecord *__restrict__ rec)
    {
    const unsigned int s = blockIdx.x * NL_THREADS + threadIdx.x;
    if (s >= n) return;
    const unsigned int i = slot_idx[s];
    const unsigned int c = cell_of[i];
    const unsigned int first = cell_start[c], cnt = cell_count[c];
    unsigned int rank = 0;
    for (unsigned int q = 0; q < cnt; ++q) rank += slot_idx[first + q] < i ? 1u : 0u;
    const Particle p = scalar4_traits<S4>::load(pos, i);
    NlRecord r;
    r.x = p.x; r.y = p.y; r.z = p.z;
    r.idx = i;
    r.type = p.type;
    rec[first + rank] = r;
    }

// ---- exclusive scan of unsigned ints (three launches; sums in 64 bits so that a total beyond 2^32 is seen, not wrapped) -----------

__device__ __forceinline__ unsigned int nl_block_exclusive(const unsigned int v, unsigned int *s_wave, unsigned int &block_total)
    {
    // inclusive scan inside the wave (ascending offsets), then over the wave sums
    const unsigned int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int incl = v;
#pragma unroll
    for (int off = 1; off < MTD_WAVE; off <<= 1)
        {
        const unsigned int up = __shfl_up(incl, off, MTD_WAVE);
        if (lane >= (unsigned int)off) incl += up;
        }
    __syncthreads();
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned int before = 0, total = 0;
    for (unsigned int w = 0; w < NL_THREADS / MTD_WAVE; ++w)
        {
        const unsigned int t = s_wave[w];
        if (w < wave) before += t;
        total += t;
        }
    block_total = total;
    return before + incl - v;
    }

__device__ __forceinline__ uint4 nl_load4(const unsigned int *__restrict__ in, const unsigned int n, const unsigned int base)
    {
    // (the arrays are allocated in whole tiles, and base is a multiple of 4: the vector load stays inside the allocation)
    uint4 v = *reinterpret_cast<const uint4 *>(in + base);
    if (base + 0 >= n) v.x = 0;
    if (base + 1 >= n) v.y = 0;
    if (base + 2 >= n) v.z = 0;
    if (base + 3 >= n) v.w = 0;
    return v;
    }

__global__ void __launch_bounds__(NL_THREADS) k_nl_scan_sums(const unsigned int n, const unsigned int *__restrict__ in,
                                                             unsigned long long *__restrict__ tile_sum)
    {
    __shared__ unsigned int s_wave[NL_THREADS / MTD_WAVE];
    const uint4 v = nl_load4(in, n, blockIdx.x * NL_SCAN_TILE + threadIdx.x * 4);
    unsigned int total;
    (void)nl_block_exclusive(v.x + v.y + v.z + v.w, s_wave, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
    }

// one block: tile sums -> exclusive tile offsets, in place; the grand total to *h_total (pinned host memory, optional)
__global__ void __launch_bounds__(NL_THREADS) k_nl_scan_top(const unsigned int n_tiles, unsigned long long *__restrict__ tile_sum,
                                                            unsigned long long *__restrict__ h_total)
    {
    __shared__ unsigned long long s_part[NL_THREADS];
    // thread t owns the contiguous chunk [t * per, (t + 1) * per)
    const unsigned int per = (n_tiles + NL_THREADS - 1) / NL_THREADS;
    const unsigned int lo = min(threadIdx.x * per, n_tiles), hi = min(lo + per, n_tiles);
    unsigned long long sum = 0;
    for (unsigned int q = lo; q < hi; ++q) sum += tile_sum[q];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (unsigned int t = 0; t < NL_THREADS; ++t)
        {
        const unsigned long long x = s_part[t];
        if (t < threadIdx.x) before += x;
        total += x;
        }
    for (unsigned int q = lo; q < hi; ++q)
        {
        const unsigned long long x = tile_sum[q];
        tile_sum[q] = before;
        before += x;
        }
    if (threadIdx.x == 0 && h_total) *h_total = total;
    }

__global__ void __launch_bounds__(NL_THREADS) k_nl_scan_apply(const unsigned int n, const unsigned int *__restrict__ in,
                                                              const unsigned long long *__restrict__ tile_off, unsigned int *__restrict__ out)
    {
    __shared__ unsigned int s_wave[NL_THREADS / MTD_WAVE];
    const unsigned int base = blockIdx.x * NL_SCAN_TILE + threadIdx.x * 4;
    const uint4 v = nl_load4(in, n, base);
    unsigned int total;
    const unsigned int e = nl_block_exclusive(v.x + v.y + v.z + v.w, s_wave, total) + (unsigned int)tile_off[blockIdx.x];
    uint4 o;
    o.x = e;
    o.y = o.x + v.x;
    o.z = o.y + v.y;
    o.w = o.z + v.z;
    *reinterpret_cast<uint4 *>(out + base) = o;      // (whole tiles are allocated: the tail of the last one is scratch)
    }

// ---- b. / c. count and fill ---------------------------------------------------------------------------------------------------------

// the distinct cells along k that can hold a partner of a particle in cell coordinate c
__device__ __forceinline__ int nl_stencil(const NlBox &b, const int k, const unsigned int c, unsigned int out[3])
    {
    const unsigned int n = b.dim[k];
    out[0] = out[1] = out[2] = 0;
    if (n == 1) return 1;
    if (b.periodic[k])
        {
        if (n == 2)
            {
            out[0] = c;
            out[1] = 1 - c;
            return 2;
            }
        out[0] = c == 0 ? n - 1 : c - 1;
        out[1] = c;
        out[2] = c + 1 == n ? 0 : c + 1;
        return 3;
        }
    int m = 0;
    if (c > 0) out[m++] = c - 1;
    out[m++] = c;
    if (c + 1 < n) out[m++] = c + 1;
    return m;
    }

template<bool FILL>
__global__ void __launch_bounds__(NL_THREADS) k_nl_pairs(const NlBox b, const unsigned int n_total, const unsigned int n_local, const double rlistsq,
                                                         const int half, const int type, const NlRecord *__restrict__ rec,
                                                         const unsigned int *__restrict__ cell_of, const unsigned int *__restrict__ cell_start,
                                                         const unsigned int *__restrict__ cell_count, unsigned int *__restrict__ n_neigh,
                                                         const unsigned int *__restrict__ head, unsigned int *__restrict__ nlist)
    {
    const unsigned int s = blockIdx.x * NL_THREADS + threadIdx.x;
    if (s >= n_total) return;
    const NlRecord me = rec[s];
    if (me.idx >= n_local) return;                         // ghosts are partners only, they own no row
    unsigned int k = 0;
    if (type < 0 || me.type == type)
        {
        const unsigned int c = cell_of[me.idx];
        const unsigned int cx = c % b.dim[0], cy = (c / b.dim[0]) % b.dim[1], cz = c / (b.dim[0] * b.dim[1]);
        unsigned int sx[3], sy[3], sz[3];
        const int nx = nl_stencil(b, 0, cx, sx), ny = nl_stencil(b, 1, cy, sy), nz = nl_stencil(b, 2, cz, sz);
        unsigned int *row = nullptr;
        if (FILL) row = nlist + head[me.idx];
        for (int iz = 0; iz < nz; ++iz)
            for (int iy = 0; iy < ny; ++iy)
                for (int ix = 0; ix < nx; ++ix)
                    {
                    const unsigned int cc = (sz[iz] * b.dim[1] + sy[iy]) * b.dim[0] + sx[ix];
                    const unsigned int first = cell_start[cc], cnt = cell_count[cc];
                    for (unsigned int q = 0; q < cnt; ++q)
                        {
                        const NlRecord o = rec[first + q];
                        double dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
                        nl_min_image(b, dx, dy, dz);
                        const double rsq = dx * dx + dy * dy + dz * dz;
                        bool take = rsq <= rlistsq && o.idx != me.idx;
                        if (half) take = take && o.idx > me.idx;
                        if (type >= 0) take = take && o.type == type;
                        if (take)
                            {
                            if (FILL) row[k] = o.idx;
                            ++k;
                            }
                        }
                    }
        }
    if (!FILL) n_neigh[me.idx] = k;
    }

// ---- d. displacement check --------------------------------------------------------------------------------------------------------

template<typename S4>
__global__ void __launch_bounds__(NL_THREADS) k_nl_check(const NlBox b, const unsigned int n_total, const double maxsq, const S4 *__restrict__ pos,
                                                         const NlRecord *__restrict__ rec, const unsigned int stamp, unsigned int *__restrict__ flag)
    {
    const unsigned int s = blockIdx.x * NL_THREADS + threadIdx.x;
    if (s >= n_total) return;
    const NlRecord o = rec[s];
    const Particle p = scalar4_traits<S4>::load(pos, o.idx);
    double dx = p.x - o.x, dy = p.y - o.y, dz = p.z - o.z;
    nl_min_image(b, dx, dy, dz);
    // (every writer stores the same stamp: the order of the stores does not matter; !(<=) also catches NaN)
    if (!(dx * dx + dy * dy + dz * dz <= maxsq)) *flag = stamp;
    }

// ---- host ---------------------------------------------------------------------------------------------------------------------------

template<typename T> struct NlBuf
    {
    T *p = nullptr;
    size_t cap = 0;
    // at least n elements, grown geometrically; the contents are NOT kept
    int reserve(size_t n)
        {
        if (n <= cap) return 0;
        size_t want = cap + cap / 2;
        if (want < n) want = n;
        if (p) MTD_HIP_TRY(hipFree(p));
        p = nullptr;
        cap = 0;
        MTD_HIP_TRY(hipMalloc((void **)&p, want * sizeof(T)));
        cap = want;
        return 0;
        }
    void release()
        {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        }
    };

inline size_t nl_tiles(size_t n) { return (n + NL_SCAN_TILE - 1) / NL_SCAN_TILE; }
inline size_t nl_padded(size_t n) { return (nl_tiles(n) ? nl_tiles(n) : 1) * NL_SCAN_TILE; }

// geometry of a build; MTD_ERR_INVALID_ARGUMENT when the box is degenerate or r_list exceeds half a periodic face distance
int nl_geometry(const mtd_box &box, const double r_list, const size_t n_total, NlBox &g)
    {
    for (int k = 0; k < 3; ++k)
        if (!(box.L[k] > 0.0) || !std::isfinite(box.L[k])) return MTD_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(box.xy) || !std::isfinite(box.xz) || !std::isfinite(box.yz)) return MTD_ERR_INVALID_ARGUMENT;
    std::memset(&g, 0, sizeof(g));
    reciprocal_rows(box, g.B);
    // no more cells than about two per particle (a dilute gas in a huge box): fewer, larger cells are always correct
    double cap = std::cbrt(2.0 * (double)(n_total ? n_total : 1));
    if (cap < 3.0) cap = 3.0;
    if (cap > 1024.0) cap = 1024.0;
    for (int k = 0; k < 3; ++k)
        {
        const double d = 1.0 / std::sqrt(g.B[k][0] * g.B[k][0] + g.B[k][1] * g.B[k][1] + g.B[k][2] * g.B[k][2]);   // distance of the k-th pair of faces
        g.periodic[k] = box.periodic[k] ? 1 : 0;
        if (g.periodic[k] && r_list > 0.5 * d) return MTD_ERR_INVALID_ARGUMENT;
        double n = std::floor(d / r_list);
        if (n < 1.0) n = 1.0;
        if (n > cap) n = std::floor(cap);
        g.dim[k] = (unsigned int)n;
        g.off[k] = -box.lo[k] / box.L[k];
        g.L[k] = box.L[k];
        g.Linv[k] = g.periodic[k] ? 1.0 / box.L[k] : 0.0;
        }
    g.xy = box.xy; g.xz = box.xz; g.yz = box.yz;
    return MTD_SUCCESS;
    }

int nl_scan(const unsigned int n, const unsigned int *in, unsigned int *out, unsigned long long *tile_sum, unsigned long long *h_total,
            hipStream_t s)
    {
    const unsigned int tiles = (unsigned int)nl_tiles(n);
    hipLaunchKernelGGL(k_nl_scan_sums, dim3(tiles), dim3(NL_THREADS), 0, s, n, in, tile_sum);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nl_scan_top, dim3(1), dim3(NL_THREADS), 0, s, tiles, tile_sum, h_total);
    MTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nl_scan_apply, dim3(tiles), dim3(NL_THREADS), 0, s, n, in, (const unsigned long long *)tile_sum, out);
    MTD_LAUNCH_CHECK();
    return 0;
    }

} // namespace

struct mtd_nlist
    {
    NlBuf<unsigned int> cell_of, slot_idx, cell_count, cell_start, n_neigh, head, nlist;
    NlBuf<unsigned long long> tile_sum;
    NlBuf<NlRecord> rec;
    unsigned long long *h_total = nullptr;     // pinned, device-visible: entry count of a build
    unsigned int *h_flag = nullptr;            // pinned, device-visible: stamp of the last check that saw a particle beyond r_buff / 2
    unsigned long long *d_total = nullptr;     // the two words as the device addresses them
    unsigned int *d_flag = nullptr;
    unsigned int stamp = 0;
    bool built = false;
    unsigned int n_total = 0;
    int dtype = -1;
    mtd_box box;
    NlBox geom;
    };

extern "C" int mtd_nlist_create(mtd_nlist **out)
    {
    if (!out) return MTD_ERR_INVALID_ARGUMENT;
    *out = new (std::nothrow) mtd_nlist();        // no device call: buffers come with the first build
    return *out ? MTD_SUCCESS : (int)hipErrorOutOfMemory;
    }

extern "C" int mtd_nlist_destroy(mtd_nlist *h)
    {
    if (!h) return MTD_ERR_INVALID_ARGUMENT;
    h->cell_of.release(); h->slot_idx.release(); h->cell_count.release(); h->cell_start.release();
    h->n_neigh.release(); h->head.release(); h->nlist.release(); h->tile_sum.release(); h->rec.release();
    if (h->h_total) (void)hipHostFree(h->h_total);
    if (h->h_flag) (void)hipHostFree(h->h_flag);
    delete h;
    return MTD_SUCCESS;
    }

extern "C" int mtd_nlist_build(mtd_nlist *h, unsigned int n_local, unsigned int n_ghost, const void *d_postype, int dtype, const mtd_box *box,
                               double r_list, int half_nlist, int type, const unsigned int **d_head_list, const unsigned int **d_n_neigh,
                               const unsigned int **d_nlist, size_t *n_entries, mtd_stream_t stream)
    {
    if (!h || !box || !(r_list > 0.0) || !std::isfinite(r_list)) return MTD_ERR_INVALID_ARGUMENT;
    if (dtype != MTD_F32 && dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    if (!d_head_list || !d_n_neigh || !d_nlist || !n_entries) return MTD_ERR_INVALID_ARGUMENT;
    const size_t n_total_z = (size_t)n_local + n_ghost;
    if (n_total_z > 0x7fffffffu) return MTD_ERR_INVALID_ARGUMENT;
    NlBox g;
    const int rc = nl_geometry(*box, r_list, n_total_z, g);
    if (rc != MTD_SUCCESS) return rc;
    if (half_nlist && n_ghost) return MTD_ERR_UNSUPPORTED;     // the pair of a local and a ghost particle has no row on the ghost's side
    if (n_total_z && !d_postype) return MTD_ERR_INVALID_ARGUMENT;

    hipStream_t s = (hipStream_t)stream;
    const unsigned int n_total = (unsigned int)n_total_z;
    const unsigned int n_cells = g.dim[0] * g.dim[1] * g.dim[2];
    h->built = false;
    if (!h->h_total)
        {
        MTD_HIP_TRY(hipHostMalloc((void **)&h->h_total, sizeof(unsigned long long), hipHostMallocDefault));
        MTD_HIP_TRY(hipHostMalloc((void **)&h->h_flag, sizeof(unsigned int), hipHostMallocDefault));
        *h->h_flag = 0;
        MTD_HIP_TRY(hipHostGetDevicePointer((void **)&h->d_total, h->h_total, 0));
        MTD_HIP_TRY(hipHostGetDevicePointer((void **)&h->d_flag, h->h_flag, 0));
        }
    // (scanned arrays are allocated in whole tiles of the scan: its vector loads and stores never leave them)
    int e = 0;
    if ((e = h->cell_of.reserve(n_total ? n_total : 1))) return e;
    if ((e = h->slot_idx.reserve(n_total ? n_total : 1))) return e;
    if ((e = h->rec.reserve(n_total ? n_total : 1))) return e;
    if ((e = h->cell_count.reserve(2 * nl_padded(n_cells)))) return e;          // counters, then the scatter's fill cursors
    if ((e = h->cell_start.reserve(nl_padded(n_cells)))) return e;
    if ((e = h->n_neigh.reserve(nl_padded(n_local)))) return e;
    if ((e = h->head.reserve(nl_padded(n_local)))) return e;
    const size_t max_tiles = nl_tiles(n_cells) > nl_tiles(n_local) ? nl_tiles(n_cells) : nl_tiles(n_local);
    if ((e = h->tile_sum.reserve(max_tiles ? max_tiles : 1))) return e;
    if ((e = h->nlist.reserve(1))) return e;

    size_t total = 0;
    if (n_total)
        {
        const unsigned int blocks = (n_total + NL_THREADS - 1) / NL_THREADS;
        unsigned int *cell_fill = h->cell_count.p + nl_padded(n_cells);
        MTD_HIP_TRY(hipMemsetAsync(h->cell_count.p, 0, sizeof(unsigned int) * 2 * nl_padded(n_cells), s));
        if (dtype == MTD_F32)
            hipLaunchKernelGGL(k_nl_cell_count<float4>, dim3(blocks), dim3(NL_THREADS), 0, s, g, n_total, (const float4 *)d_postype, h->cell_of.p,
                               h->cell_count.p);
        else
            hipLaunchKernelGGL(k_nl_cell_count<double4>, dim3(blocks), dim3(NL_THREADS), 0, s, g, n_total, (const double4 *)d_postype, h->cell_of.p,
                               h->cell_count.p);
        MTD_LAUNCH_CHECK();
        if ((e = nl_scan(n_cells, h->cell_count.p, h->cell_start.p, h->tile_sum.p, nullptr, s))) return e;
        hipLaunchKernelGGL(k_nl_scatter, dim3(blocks), dim3(NL_THREADS), 0, s, n_total, (const unsigned int *)h->cell_of.p,
                           (const unsigned int *)h->cell_start.p, cell_fill, h->slot_idx.p);
        MTD_LAUNCH_CHECK();
        if (dtype == MTD_F32)
            hipLaunchKernelGGL(k_nl_order<float4>, dim3(blocks), dim3(NL_THREADS), 0, s, n_total, (const float4 *)d_postype,
                               (const unsigned int *)h->cell_of.p, (const unsigned int *)h->cell_start.p, (const unsigned int *)h->cell_count.p,
                               (const unsigned int *)h->slot_idx.p, h->rec.p);
        else
            hipLaunchKernelGGL(k_nl_order<double4>, dim3(blocks), dim3(NL_THREADS), 0, s, n_total, (const double4 *)d_postype,
                               (const unsigned int *)h->cell_of.p, (const unsigned int *)h->cell_start.p, (const unsigned int *)h->cell_count.p,
                               (const unsigned int *)h->slot_idx.p, h->rec.p);
        MTD_LAUNCH_CHECK();
        if (n_local)
            {
            hipLaunchKernelGGL(k_nl_pairs<false>, dim3(blocks), dim3(NL_THREADS), 0, s, g, n_total, n_local, r_list * r_list, half_nlist ? 1 : 0,
                               type, (const NlRecord *)h->rec.p, (const unsigned int *)h->cell_of.p, (const unsigned int *)h->cell_start.p,
                               (const unsigned int *)h->cell_count.p, h->n_neigh.p, (const unsigned int *)nullptr, (unsigned int *)nullptr);
            MTD_LAUNCH_CHECK();
            if ((e = nl_scan(n_local, h->n_neigh.p, h->head.p, h->tile_sum.p, h->d_total, s))) return e;
            MTD_HIP_TRY(hipStreamSynchronize(s));          // the one synchronisation of a rebuild: the entry count sizes nlist
            const unsigned long long t = *(volatile unsigned long long *)h->h_total;
            if (t > 0xffffffffull) return MTD_ERR_UNSUPPORTED;            // head_list is 32 bits wide
            total = (size_t)t;
            if ((e = h->nlist.reserve(total ? total : 1))) return e;
            if (total)
                {
                hipLaunchKernelGGL(k_nl_pairs<true>, dim3(blocks), dim3(NL_THREADS), 0, s, g, n_total, n_local, r_list * r_list,
                                   half_nlist ? 1 : 0, type, (const NlRecord *)h->rec.p, (const unsigned int *)h->cell_of.p,
                                   (const unsigned int *)h->cell_start.p, (const unsigned int *)h->cell_count.p, (unsigned int *)nullptr,
                                   (const unsigned int *)h->head.p, h->nlist.p);
                MTD_LAUNCH_CHECK();
                }
            }
        }
    h->built = true;
    h->n_total = n_total;
    h->dtype = dtype;
    h->box = *box;
    h->geom = g;
    *d_head_list = h->head.p;
    *d_n_neigh = h->n_neigh.p;
    *d_nlist = h->nlist.p;
    *n_entries = total;
    return MTD_SUCCESS;
    }

extern "C" int mtd_nlist_check(mtd_nlist *h, const void *d_postype, int dtype, const mtd_box *box, double r_buff, int *needs_rebuild,
                               mtd_stream_t stream)
    {
    if (!h || !box || !needs_rebuild || !(r_buff >= 0.0)) return MTD_ERR_INVALID_ARGUMENT;
    if (dtype != MTD_F32 && dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    *needs_rebuild = 1;
    if (!h->built || dtype != h->dtype) return MTD_SUCCESS;
    for (int k = 0; k < 3; ++k)
        if (box->L[k] != h->box.L[k] || box->lo[k] != h->box.lo[k] || (box->periodic[k] != 0) != (h->box.periodic[k] != 0)) return MTD_SUCCESS;
    if (box->xy != h->box.xy || box->xz != h->box.xz || box->yz != h->box.yz) return MTD_SUCCESS;
    *needs_rebuild = 0;
    if (!h->n_total) return MTD_SUCCESS;
    if (!d_postype) return MTD_ERR_INVALID_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    if (++h->stamp == 0) ++h->stamp;               // never 0, the word's initial value
    const unsigned int stamp = h->stamp;
    const unsigned int blocks = (h->n_total + NL_THREADS - 1) / NL_THREADS;
    const double maxsq = 0.25 * r_buff * r_buff;
    if (dtype == MTD_F32)
        hipLaunchKernelGGL(k_nl_check<float4>, dim3(blocks), dim3(NL_THREADS), 0, s, h->geom, h->n_total, maxsq, (const float4 *)d_postype,
                           (const NlRecord *)h->rec.p, stamp, h->d_flag);
    else
        hipLaunchKernelGGL(k_nl_check<double4>, dim3(blocks), dim3(NL_THREADS), 0, s, h->geom, h->n_total, maxsq, (const double4 *)d_postype,
                           (const NlRecord *)h->rec.p, stamp, h->d_flag);
    MTD_LAUNCH_CHECK();
    MTD_HIP_TRY(hipStreamSynchronize(s));
    *needs_rebuild = *(volatile unsigned int *)h->h_flag == stamp ? 1 : 0;
    return MTD_SUCCESS;
    }

extern "C" int mtd_nlist_cells(const mtd_nlist *h, unsigned int dim[3])
    {
    if (!h || !dim || !h->built) return MTD_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 3; ++k) dim[k] = h->geom.dim[k];
    return MTD_SUCCESS;
    }
