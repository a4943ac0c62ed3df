// row_walk.hpp — the lane-group walk over one row of a full neighbour list, written once (device; steinhardt_local.hip, cluster.hip,
// pair_entropy.hip, pair_entropy_local.hip, env_similarity.hip, debye.hip, coordination.hip; the scaling of stored gradient sums, which
// three of them share, is in row_scale.hpp; the mask of the largest cluster on a per-particle table, which two of them share, in row_mask.hpp).
//
// G lanes (a DPP quad, or half a DPP row) share one central particle; lane q takes entries q, q + G, ... of its row.  Here: the centre of
// a group (RowCentre / row_centre), the walk itself with its look-ahead (row_walk), the group's sum (group_sum), the zero that keeps the
// smoothing table's loads inside a loop (loop_table), the moves of wave-uniform constants into vector registers (in_vgpr), the store of a
// particle's virial by lane 0 of its group (row_store_virial), the block count of a launch (row_blocks) with the width of a table of
// block sums (ROW_MAX_BLOCKS), the kernel that adds such a table up (k_row_sums) and the pitch of per-particle rows in a scratch
// (row_pitch).  Everything a walk kernel calls is __forceinline__ and holds no state of its own: a kernel that uses a piece has the
// instruction stream of the kernel that wrote it out (profiles/r20/README.md and profiles/r26/README.md compare them kernel by kernel).
//
// The walk lives in FOUR forms, and a change to the look-ahead, the list format or the skip rule is made in all of them:
//   row_walk                   here: both passes of pair_entropy.hip and of env_similarity.hip, the walk and the spectrum of debye.hip; as
//                              row_walk_entries<.., GHOSTS = false> the passes of pair_entropy_local.hip and the link pass of cluster.hip
//                              (local entries only: the rule of QllWalker, switched at compile time)
//   QllWalker                  steinhardt_local.hip: its four gather passes, through qll_entries
//   three loops written out    k_qll_accumulate, k_qll_forces and k_qll_forces_tile of steinhardt_local.hip (through a walker their bits
//                              or their speed did not stay the parent's: profiles/r10/README.md)
//   row_walk_pairs             here, at the end: coordination.hip.  The walk of row_walk with TWO types: the centre (row_centre_pairs) is
//                              of type A or B, and an entry takes part as (A centre, B partner), as (B centre, A partner) or as both when
//                              A = B; the body is told which.  Ghosts are walked, as in row_walk.  A function of its own, so that the
//                              kernels on row_walk keep their instruction streams
// They differ in ONE rule on purpose.  QllWalker::position and the three loops load a neighbour's position for j < N only: the Steinhardt
// passes read per-particle table rows of their neighbours, which ghosts do not have, so an entry j >= N is skipped.  row_walk loads it for
// every j != ROW_NONE: the rows of these two variables may address ghost particles stored behind the N local ones
// (include/mtd_abi.h, "Pair entropy" and mtd_es_accumulate's n_ghost), and those entries count.  Neither test is a slip of the other.
#pragma once

#include "mtd_device.hpp"
#include "steinhardt_device.hpp"

namespace mtd
{

constexpr unsigned int ROW_NONE = 0xffffffffu;             // no entry: past the end of the row

template<typename S4> __device__ __forceinline__ S4 row_zero();
template<> __device__ __forceinline__ float4 row_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template<> __device__ __forceinline__ double4 row_zero<double4>() { return make_double4(0.0, 0.0, 0.0, 0.0); }

// A wave-uniform constant moved into a vector register.  The pair passes of pair_entropy.hip and env_similarity.hip hold the box, the
// window, their own constants, nine pointers, the literals of two exponentials and the masks of four nested branches — more than the 102
// scalar registers of a wave, and the surplus was spilled.  Vector registers are not short there; what the inner loops multiply with
// lives in them.
__device__ __forceinline__ double in_vgpr(double v)
    {
    asm volatile("" : "+v"(v));
    return v;
    }

// the box of the argument block (what min_image reads) ...
__device__ __forceinline__ QlArgs<4> in_vgpr(QlArgs<4> a)
    {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.L[k] = in_vgpr(a.L[k]), a.Linv[k] = in_vgpr(a.Linv[k]);
    a.xy = in_vgpr(a.xy), a.xz = in_vgpr(a.xz), a.yz = in_vgpr(a.yz);
    return a;
    }

// ... and the smoothing window with it (env_similarity.hip; pair_entropy.hip keeps the window in scalar registers)
__device__ __forceinline__ QlArgs<4> in_vgpr_window(QlArgs<4> a)
    {
    a = in_vgpr(a);
    a.rcutsq = in_vgpr(a.rcutsq), a.ronsq = in_vgpr(a.ronsq), a.r_on = in_vgpr(a.r_on), a.inv_width = in_vgpr(a.inv_width);
    return a;
    }

// sum over the G lanes of a particle, the same bits in all of them: (q0 + q1) + (q2 + q3) in a quad, then the other half of the half row
template<int G> __device__ __forceinline__ double group_sum(double v)
    {
    static_assert(G == 4 || G == 8, "a DPP quad or half a DPP row");
    v += dpp_move<MTD_DPP_QUAD_XOR1>(v);
    v += dpp_move<MTD_DPP_QUAD_XOR2>(v);
    if constexpr (G == 8) v += dpp_move<MTD_DPP_ROW_HALF_MIRROR>(v);
    return v;
    }

// the central particle of a lane group: particle i of the chunk, its row of the list (empty for i >= N and for a particle of another type)
struct RowCentre
    {
    unsigned int i;
    Particle p;
    unsigned int start, cnt;
    __device__ __forceinline__ unsigned int row(const unsigned int N) const { return i < N ? i : 0; }   // a table row that is safe to address
    __device__ __forceinline__ double own(const unsigned int N, const double *of) const { return i < N ? of[i] : 0.0; }   // its per-particle value
    };

template<typename S4, int LMAX>
__device__ __forceinline__ RowCentre row_centre(const QlArgs<LMAX> &a, const S4 *postype, const unsigned int *head_list, const unsigned int *n_neigh,
                                                const unsigned int i)
    {
    Particle p = {0.0, 0.0, 0.0, -1};
    unsigned int start = 0, cnt = 0;
    if (i < a.N)
        {
        p = scalar4_traits<S4>::load(postype, i);
        if ((unsigned int)p.type == a.type)
            {
            start = head_list[i];
            cnt = n_neigh[i];
            }
        }
    return {i, p, start, cnt};
    }

// the table with a zero added that the compiler cannot see through: called inside a loop, it keeps the table's loads in the loop (its
// twenty coefficients are then loaded where the window is evaluated and not held in scalar registers across the walk: they spilled)
__device__ __forceinline__ const double *loop_table(const double *tab)
    {
    unsigned int tab_shift = 0;
    asm volatile("" : "+s"(tab_shift));
    return tab + tab_shift;
    }

// The walk over one row: calls body(tab_k, j, dx, dy, dz, rsq) for every entry of lane q that takes part — j is not the particle itself,
// has the type and lies within the cut-off.  The list entry is asked for two trips, the neighbour's position one trip ahead of the
// arithmetic.  j is NOT compared with N (header: ghosts are walked).  FROM_CENTRE says which way d points, d = minImage(r_i - r_j) (true:
// pair_entropy.hip) or minImage(r_j - r_i) (false: env_similarity.hip); each unit's subtraction is the one it always made, nothing is
// negated afterwards.
// GHOSTS = false (cluster.hip, whose per-particle arrays end at N like the Steinhardt tables): an entry j >= a.N is skipped and its
// position is not loaded, the rule of QllWalker.  It is a compile-time switch: row_walk, below, is the walk with ghosts, as it always was.
template<int G, bool FROM_CENTRE, bool GHOSTS, typename S4, typename F>
__device__ __forceinline__ void row_walk_entries(const QlArgs<4> &a, const S4 *__restrict__ postype, const unsigned int *__restrict__ nlist,
                                                 const double *__restrict__ tab, const RowCentre &c, const unsigned int q, F &&body)
    {
    const auto held = [&](const unsigned int j) { return GHOSTS ? j != ROW_NONE : j < a.N; };      // its position may be loaded
    unsigned int e = q;
    unsigned int j0 = e < c.cnt ? nlist[c.start + e] : ROW_NONE;
    unsigned int j1 = e + G < c.cnt ? nlist[c.start + e + G] : ROW_NONE;
    S4 pos0 = row_zero<S4>();
    if (held(j0)) pos0 = postype[j0];
#pragma unroll 1
    for (; e < c.cnt; e += G)
        {
        const double *__restrict__ tab_k = loop_table(tab);
        const unsigned int j2 = e + 2 * G < c.cnt ? nlist[c.start + e + 2 * G] : ROW_NONE;
        S4 pos1 = row_zero<S4>();
        if (held(j1)) pos1 = postype[j1];
        if (GHOSTS ? j0 != c.i : j0 != c.i && j0 < a.N)
            {
            const Particle pj = scalar4_traits<S4>::unpack(pos0);
            double dx, dy, dz;
            if constexpr (FROM_CENTRE)
                dx = c.p.x - pj.x, dy = c.p.y - pj.y, dz = c.p.z - pj.z;
            else
                dx = pj.x - c.p.x, dy = pj.y - c.p.y, dz = pj.z - c.p.z;
            min_image(a, dx, dy, dz);
            const double rsq = dx * dx + dy * dy + dz * dz;
            if ((unsigned int)pj.type == a.type && rsq <= a.rcutsq) body(tab_k, j0, dx, dy, dz, rsq);
            }
        j0 = j1;
        j1 = j2;
        pos0 = pos1;
        }
    }

template<int G, bool FROM_CENTRE, typename S4, typename F>
__device__ __forceinline__ void row_walk(const QlArgs<4> &a, const S4 *__restrict__ postype, const unsigned int *__restrict__ nlist,
                                         const double *__restrict__ tab, const RowCentre &c, const unsigned int q, F &&body)
    {
    row_walk_entries<G, FROM_CENTRE, true>(a, postype, nlist, tab, c, q, body);
    }

// The virial of a force pass, stored by lane 0 of the group of a particle i < N (the caller's test): the six sums times `h`, the diagonal
// ones plus `diag` where DIAG (the explicit volume term of the pair entropy), at v = virial + i, component-major with `virial_pitch`
// between components, non-temporally.
// NOT shared, on purpose: the group's sums, the test `q == 0 && c.i < a.N` and the ONE statement that stores the force stay written out
// in k_pe_forces and k_es_forces.  With any of them in here (the test inside or handed in, the force store as a function of (i, F,
// scale, force) or of the offset pointer) the 16 force kernels did not keep the instruction streams of their parents, and
// k_es_forces<.., false, false, false> measured 0.3 % slower, outside the bound for a refactor (profiles/r20/README.md, "what was tried").
template<bool DIAG, typename scalar>
__device__ __forceinline__ void row_store_virial(scalar *v, const unsigned int virial_pitch, const double vxx, const double vxy, const double vxz,
                                                 const double vyy, const double vyz, const double vzz, const double h, const double diag)
    {
    nt_store((scalar)(DIAG ? vxx * h + diag : vxx * h), v);
    nt_store((scalar)(vxy * h), v + virial_pitch);
    nt_store((scalar)(vxz * h), v + 2 * (size_t)virial_pitch);
    nt_store((scalar)(DIAG ? vyy * h + diag : vyy * h), v + 3 * (size_t)virial_pitch);
    nt_store((scalar)(vyz * h), v + 4 * (size_t)virial_pitch);
    nt_store((scalar)(DIAG ? vzz * h + diag : vzz * h), v + 5 * (size_t)virial_pitch);
    }

// The two-type forms of row_centre and row_walk (coordination.hip).  The centre owns a row when it is of type A or of type B.  The walk
// calls body(j, as_centre, as_partner, dx, dy, dz, rsq), d = minImage(r_i - r_j), for every entry of lane q with j != i and
// rsq <= a.rcutsq that plays a role: as_centre = (type_i == A and type_j == B), the entry counts in n_i; as_partner = (type_i == B and
// type_j == A), the mirror entry counts in n_j and its gradient falls on i.  With A = B both hold.  Look-ahead and ghost rule of row_walk.
template<typename S4, int LMAX>
__device__ __forceinline__ RowCentre row_centre_pairs(const QlArgs<LMAX> &a, const unsigned int type_a, const unsigned int type_b,
                                                      const S4 *postype, const unsigned int *head_list, const unsigned int *n_neigh,
                                                      const unsigned int i)
    {
    Particle p = {0.0, 0.0, 0.0, -1};
    unsigned int start = 0, cnt = 0;
    if (i < a.N)
        {
        p = scalar4_traits<S4>::load(postype, i);
        if ((unsigned int)p.type == type_a || (unsigned int)p.type == type_b)
            {
            start = head_list[i];
            cnt = n_neigh[i];
            }
        }
    return {i, p, start, cnt};
    }

template<int G, typename S4, typename F>
__device__ __forceinline__ void row_walk_pairs(const QlArgs<4> &a, const unsigned int type_a, const unsigned int type_b,
                                               const S4 *__restrict__ postype, const unsigned int *__restrict__ nlist, const RowCentre &c,
                                               const unsigned int q, F &&body)
    {
    const bool centre_a = (unsigned int)c.p.type == type_a, centre_b = (unsigned int)c.p.type == type_b;
    unsigned int e = q;
    unsigned int j0 = e < c.cnt ? nlist[c.start + e] : ROW_NONE;
    unsigned int j1 = e + G < c.cnt ? nlist[c.start + e + G] : ROW_NONE;
    S4 pos0 = row_zero<S4>();
    if (j0 != ROW_NONE) pos0 = postype[j0];
#pragma unroll 1
    for (; e < c.cnt; e += G)
        {
        const unsigned int j2 = e + 2 * G < c.cnt ? nlist[c.start + e + 2 * G] : ROW_NONE;
        S4 pos1 = row_zero<S4>();
        if (j1 != ROW_NONE) pos1 = postype[j1];
        if (j0 != c.i)
            {
            const Particle pj = scalar4_traits<S4>::unpack(pos0);
            double dx = c.p.x - pj.x, dy = c.p.y - pj.y, dz = c.p.z - pj.z;
            min_image(a, dx, dy, dz);
            const double rsq = dx * dx + dy * dy + dz * dz;
            const bool as_centre = centre_a && (unsigned int)pj.type == type_b, as_partner = centre_b && (unsigned int)pj.type == type_a;
            if ((as_centre || as_partner) && rsq <= a.rcutsq) body(j0, as_centre, as_partner, dx, dy, dz, rsq);
            }
        j0 = j1;
        j1 = j2;
        pos0 = pos1;
        }
    }

// columns of a unit's table of block sums [row][ROW_MAX_BLOCKS] in its scratch; each unit's own name for it stays, as an alias, in the
// bodies of its walk kernels
constexpr unsigned int ROW_MAX_BLOCKS = 1024;

// One wave per slot adds the blocks' doubles of such a table in the fixed order of wave_sum: lane k takes the columns k, k + 64, ...
// The slots [0, n_live) are rows [0, n_live) of the table; a slot from n_live on is the count, kept in row `count_row` (debye.hip: behind
// the rows of the COMPILED peak count).  With n_live = gridDim.x slot b is row b (pair_entropy.hip, coordination.hip).  MAX_BLOCKS is the
// unit's alias of ROW_MAX_BLOCKS; a template, so that only a unit that launches it holds a copy.
template<unsigned int MAX_BLOCKS>
static __global__ __launch_bounds__(MTD_WAVE) void k_row_sums(const unsigned int n_blocks, const unsigned int n_live, const unsigned int count_row,
                                                              const double *__restrict__ part, double *__restrict__ sums)
    {
    const unsigned int src = blockIdx.x < n_live ? blockIdx.x : count_row;
    const double *row = part + (size_t)src * MAX_BLOCKS;
    double v = 0.0;
    for (unsigned int k = threadIdx.x; k < n_blocks; k += MTD_WAVE) v += row[k];
    v = wave_sum(v);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
    }

// pitch, in doubles, of the per-particle rows in a scratch: n_particles rounded up to even, so that every row is 16-byte aligned
__host__ __device__ inline size_t row_pitch(const unsigned int n) { return ((size_t)n + 1) & ~(size_t)1; }

// blocks of a launch that walks `ppb` central particles per block and round: one per chunk, at least one, at most `max_blocks` (the
// columns of block sums a unit's scratch holds)
inline unsigned int row_blocks(const unsigned int N, const unsigned int ppb, const unsigned int max_blocks)
    {
    unsigned int b = (N + ppb - 1) / ppb;
    if (b < 1) b = 1;
    return b > max_blocks ? max_blocks : b;
    }

}
