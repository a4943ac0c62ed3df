// steinhardt_local.hip — per-particle Steinhardt bond order (cv.steinhardt_local) on gfx950.
//
// No reference counterpart: the reference's variable (SteinhardtQl.cc, steinhardt.hip here) squares ONE sum over the whole box.
// This one squares per particle and averages — the order parameter nucleation is biased with.  Conventions are those of
// mtd_ql_accumulate in every respect (smoothing f of SteinhardtQl.cc:36-48, Condon-Shortley phase, d = minImage(r_i - r_j)):
//
//   for a particle i of `type`, over the entries j of row i of a FULL neighbour list with type(j) == type and r_ij^2 <= r_cut^2
//     n_i      = sum_j f(r_ij)
//     A_lm(i)  = sum_j f(r_ij) Y_lm(d_ij / r_ij)                         l = 0..lmax
//     q_l^2(i) = 4 pi / (2l + 1) sum_{m = -l..l} |A_lm(i)|^2 / n_i^2      (0 when n_i == 0)
//     c_i      = sum_l Ql_ref[l] q_l^2(i)                                (0 for particles of another type)
//     s        = (1 / N_global) sum_i c_i
//     F_k      = -bias ds/dr_k                                           (w component 0)
//
// Not square-rooted (the root is not differentiable at 0), divided by N_global like the global variable.  A perfect fcc crystal
// gives every particle q_4^2 = 7/192 and q_6^2 = 169/512 whatever the size of the box.
//
// The gradient as a gather: with g_l(i) = Ql_ref[l] 4 pi / (2l + 1) 2 / n_i^2, W_lm(i) = g_l(i) conj(A_lm(i)) and
// Y_lm(-d) = (-1)^l Y_lm(d), row k of a symmetric full list yields the whole derivative with respect to r_k:
//
//   N_global ds/dr_k = sum_{j in row k} [ sum_lm Re{ (W_lm(k) + (-1)^l W_lm(j)) grad_d (f Y_lm)(d_kj) } - 2 (c_k / n_k + c_j / n_j) grad_d f(d_kj) ]
//
// One evaluation of grad(f Y_lm) per list entry serves the term where k is the centre and the term where k is j's neighbour: no
// reaction force is scattered, no floating-point atomic, no dependence on any arrival order.  grad f = sqrt(4 pi) grad(f Y_00), so
// the last term rides in the (0, 0) slot of the table.
//
// Preconditions: the list is full and symmetric for same-type pairs within r_cut (what HOOMD and nlist.hip build), holds no
// duplicate and indexes no ghost particle (entries j >= N and self entries are skipped).  A pair on the z axis of the box (a column of a cubic
// crystal: dx = dy = 0 exactly) has a finite force, here and in mtd_ql_forces: ql_pair_force forms the gradient without 1 / rho
// (tests/test_gpu_ql_axis.py, every entry point, on and next to the axis).  Known limit: c_i jumps from 0 to the one-neighbour value
// when a first neighbour enters an empty shell (inherent in the normalised definition; irrelevant at liquid or solid density).
//
// MI355X design.  Two launches per step, both walk chunks of 64 consecutive central particles per block and round:
//   lanes            FOUR lanes (a quad) per central particle; lane q takes entries q, q + 4, ... of the particle's row, so the
//                    per-particle sums stay in registers: no LDS atomics.  The quad's sums are added with two DPP quad_perm moves
//                    ((q0 + q1) + (q2 + q3), the same bits in all four lanes)
//   memory trips     list entry two iterations ahead, neighbour position one iteration ahead of the arithmetic
//   one walk         the centre of a quad (RowCentre / row_centre), the quad's sum (group_sum<4>) and the zero that keeps the table loads
//                    in the loop (loop_table) come from row_walk.hpp, which pair_entropy.hip and env_similarity.hip share, and serve all
//                    seven kernels; the look-ahead and the pair test are written once (QllWalker) for the
//                    four gather passes of the options, which share their whole frame (below).  accumulate, forces (per lane) and
//                    forces_tile (per wave) keep the walk written out: see the note above QllWalker
//   one gather frame k_qll_average, k_qll_backprop, k_qll_bonds and k_qll_bonds_backprop are one frame with four bodies: the window of a
//                    row and its slots (QllWindow), the loop over the entries of a row that yields (f, j, counts) per entry
//                    (qll_entries), the hand-round of the quad's four entries (quad_all, qll_add_rows), the quad's sum that only the
//                    entry's own lane keeps (quad_keep), the per-entry scratch summed over the windows (qll_park) and the chunk's sum
//                    into the block's (qll_chunk_sum, also in k_qll_accumulate).  A change to the window size, the look-ahead, the skip
//                    rule or the row format of the gather passes is made there, once
//   k_qll_accumulate monic sums S_lm = sum f p_m,l-m(cos theta) h^m (QlTab, as k_ql_accumulate) for every (l, m >= 0) of the compiled
//                    LMAX; then per particle n_i, c_i and the table row
//                        R_lm(i) = nrm(l, m)^2 (m > 0 ? 2 : 1) g_l(i) conj(S_lm(i))        degrees in use only, m >= 0
//                        R_00(i) = [the same for l = 0] - 2 c_i / n_i
//                    (already in the form ql_pair_force contracts: normalisation and the weight of the m < 0 partner folded in);
//                    per-block sums of c_i: chunk sums by one wave in the fixed order of wave_sum, chunks in the order walked
//   k_qll_forces_tile  the pair gradient of steinhardt.hip (ql_pair_force) with q_lm = R_lm(k) + (-1)^l R_lm(j); the rows R(j) of the
//                    64 entries a wave visits in one iteration are fetched by the wave together (four lanes per 64 bytes of a row)
//                    into an LDS tile of its own, R(k) of its 16 particles once per chunk; times bias / N_global at the end
//   k_qll_forces     the same with R(k) and R(j) read per lane and (l, m) straight from memory: rows longer than 256 bytes (more
//                    than 16 complex slots) whose tiles would not fit
//   virial           both force kernels carry a compile-time switch VIR (mtd_ql_local_forces_virial, for constant-pressure runs): the
//                    entry's pair force fp and pair vector d are in hand, so virial_k[ab] = 1/2 sum_j d_a fp_b is six more sums per
//                    lane beside the force (QllVirial), quad-summed and stored by lane 0; VIR = false is the kernel without it
// Double precision throughout.  Host side: the compiled LMAX, the array type, AVG and the mode of pass 1 are chosen through dispatch.hpp.
//
// Options (mtd_ql_local_options; definition and gradient in include/mtd_abi.h): per-particle transforms of the quantities above.
//   switch, gate     v_i = g(n_i) h(c_i) in place of c_i.  Still two launches: the epilogue of k_qll_accumulate<QLL_TRANSFORM> forms c_i
//                    first, scales the row with g h'(c_i), adds g'(n_i) h(c_i) to its (0, 0) slot and sums v_i; the force kernels are
//                    the plain ones.  The plain instantiations sit behind template switches and keep their instruction streams.
//   average          qbar_lm(i) = [q_lm(i) + sum_j f_ij q_lm(j)] / (1 + n_i): the value of i depends on its neighbours' rows and its
//                    gradient on its second neighbours.  Four launches: k_qll_accumulate<QLL_AVERAGE> (n_i, the rows q(i)),
//                    k_qll_average (gathers q(j): qbar, c_i, v_i, the rows B(i)), k_qll_backprop (gathers B(j) and q(j): the table row
//                    C(k) / n_k with a_k folded in, and one double E_kj per list entry), then the force pass, which streams E beside
//                    the list and adds it to the (0, 0) weight of the pair.  The two gather kernels are bodies in the gather frame: see
//                    the block above QllWindow for the frame and the one above k_qll_average for the sums.
//   bonds            (mtd_ql_local_bonds) the solid-bond count: d_ij = the normalised scalar product of q(i) and q(j), b_i = sum_j f_ij sigma(d_ij),
//                    v_i = g(n_i) h(b_i).  Four launches, the two in the middle in the gather frame: k_qll_accumulate<QLL_BONDS> (n_i, c_i, the rows
//                    q(i) / sqrt(c_i)), k_qll_bonds (gathers u(j): d per list entry, b_i, v_i, beta_i), k_qll_bonds_backprop (gathers u(j)
//                    and beta_j: the table row and E_kj = (beta_k + beta_j) sigma(d_kj) per list entry), then the AVG force pass as it is.
//                    See the block above k_qll_bonds.
//   cluster          (mtd_cluster_params, mtd_ql_local_accumulate_cluster) the sum restricted to the largest connected cluster of particles with
//                    v_i >= v_min: s = (1 / N) sum_i w_i v_i with the 0 / 1 mask w of cluster.hip.  The mask enters linearly, so it is applied
//                    BETWEEN the launches above by k_qll_cluster_apply (rows, or beta_i and a0_i, of the non-members zeroed; the block sums
//                    replaced by those of w_i v_i); the force kernels and the virial run unchanged on the masked table.  Not with the
//                    average.  See the block above k_qll_cluster_apply.
#include "mtd_device.hpp"
#include "row_walk.hpp"
#include "dispatch.hpp"
#include "cluster_host.hpp"

namespace
{

using namespace mtd;

constexpr int QLL_THREADS = 256;
constexpr int QLL_G = 4;                                   // lanes per central particle
constexpr int QLL_PPB = QLL_THREADS / QLL_G;               // central particles per block and round
constexpr unsigned int QLL_MAX_BLOCKS = 1024;              // rows of block sums in the scratch
constexpr unsigned int QLL_NONE = 0xffffffffu;
static_assert(QLL_PPB == MTD_WAVE, "one wave sums the c_i of a chunk");

// where the degrees in use sit in a table row: complex slot off[l] + m; slot 0 is (0, 0) and always there
struct QllLayout
    {
    unsigned int act;                                      // bit l: Ql_ref[l] != 0 and l <= lmax
    unsigned int row_doubles;                              // 2 * slots, even: rows stay 16-byte aligned
    unsigned int off[13];
    };

// The chunk's sum of a per-particle value, added to the block's running sum: every lane brings the value of its quad's particle (0
// past the end), wave 0 adds the 64 in the fixed order of wave_sum.  Every lane of the block is here: the chunk loop is uniform.
__device__ __forceinline__ void qll_chunk_sum(double (&s_c)[QLL_PPB], const unsigned int tid, const double v, double &block_sum)
    {
    __syncthreads();
    if (tid % QLL_G == 0) s_c[tid / QLL_G] = v;
    __syncthreads();
    if (tid < MTD_WAVE) block_sum += wave_sum(s_c[tid]);
    }

// value of lane u of the quad in all four of its lanes
template<int U> __device__ __forceinline__ double quad_bcast(const double v) { return dpp_move<U * 0x55>(v); }
template<int U> __device__ __forceinline__ unsigned int quad_bcast(const unsigned int v)
    {
    return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, U * 0x55, 0xf, 0xf, false);
    }

// ---- the walk over a row: its lane's share of the row (the quad's central particle, all seven kernels: RowCentre of row_walk.hpp) ------
// Lane q of the quad takes entries q, q + 4, ... of the row.  The walker owns the look-ahead: the list entry is asked for two
// iterations, the neighbour's position one iteration ahead of the arithmetic on (j0, pos0).  A loop is
//     w.begin(..); while (its own condition on w.e) { w.ahead(..); w.pair(.., what to do with the pair); w.step(); }
// Used by the four gather passes, through qll_entries.  k_qll_accumulate, k_qll_forces and k_qll_forces_tile keep the same walk written out:
// through the walker their bits or their speed did not stay the parent's (profiles/r10/README.md).  The walk therefore lives in these
// places, and a change to the look-ahead, the list format or the skip rule is made in ALL of them:
//     QllWalker (here)                                       the four gather passes
//     the loops of k_qll_accumulate, k_qll_forces and k_qll_forces_tile, written out below
//     row_walk of row_walk.hpp                               both passes of pair_entropy.hip and of env_similarity.hip
// The walks of this unit skip an entry j >= N (position, listed: a ghost has no table row); row_walk walks ghosts and tests j against
// "no entry" alone.  That difference is meant (row_walk.hpp).  The walker holds the look-ahead only; what it reads from is handed to
// begin and ahead.
template<typename S4> struct QllWalker
    {
    unsigned int e, j0, j1, j2;                            // the entry in hand and its index; the indices one and two entries on
    S4 pos0, pos1;                                         // the positions of j0 and j1

    static __device__ __forceinline__ unsigned int entry(const unsigned int *nlist, const RowCentre &c, const unsigned int k)
        {
        return k < c.cnt ? nlist[c.start + k] : QLL_NONE;
        }
    static __device__ __forceinline__ S4 position(const unsigned int N, const S4 *postype, const unsigned int j)
        {
        S4 pos = row_zero<S4>();
        if (j < N) pos = postype[j];
        return pos;
        }
    __device__ __forceinline__ void begin(const unsigned int N, const S4 *postype, const unsigned int *nlist, const RowCentre &c, const unsigned int q)
        {
        e = q;
        j0 = entry(nlist, c, e);
        j1 = entry(nlist, c, e + QLL_G);
        pos0 = position(N, postype, j0);
        }
    __device__ __forceinline__ void ahead(const unsigned int N, const S4 *postype, const unsigned int *nlist, const RowCentre &c)
        {
        j2 = entry(nlist, c, e + 2 * QLL_G);
        pos1 = position(N, postype, j1);
        }
    __device__ __forceinline__ void step()
        {
        j0 = j1;
        j1 = j2;
        pos0 = pos1;
        e += QLL_G;
        }
    // The pair test, in two halves.  listed: the entry in hand is a neighbour at all — an index >= N (a ghost, or QLL_NONE past the end
    // of the row) and the particle itself are skipped.  near: d = minImage(r_c - r_j0), and whether j0 has the type and lies within the
    // cut-off.  pair: calls f(dx, dy, dz, rsq) for an entry that passes both, the geometry formed for listed entries only.  The pair's
    // arithmetic is handed in, not a flag handed out: d then lives where the hand-written loops declared it.
    __device__ __forceinline__ bool listed(const unsigned int N, const RowCentre &c) const { return j0 < N && j0 != c.i; }
    template<int LMAX>
    __device__ __forceinline__ bool near(const QlArgs<LMAX> &a, const RowCentre &c, double &dx, double &dy, double &dz, double &rsq) const
        {
        const Particle pj = scalar4_traits<S4>::unpack(pos0);
        dx = c.p.x - pj.x, dy = c.p.y - pj.y, dz = c.p.z - pj.z;
        min_image(a, dx, dy, dz);
        rsq = dx * dx + dy * dy + dz * dz;
        return (unsigned int)pj.type == a.type && rsq <= a.rcutsq;
        }
    template<int LMAX, typename F> __device__ __forceinline__ void pair(const QlArgs<LMAX> &a, const RowCentre &c, F &&f) const
        {
        if (listed(a.N, c))
            {
            double dx, dy, dz, rsq;
            if (near(a, c, dx, dy, dz, rsq)) f(dx, dy, dz, rsq);
            }
        }
    };

// ---- the per-particle transforms of the options: v_i = g(n_i) h(c_i) ------------------------------------------------------------
struct QllOpt
    {
    int sw, gate;
    unsigned int p;
    double inv_c0, n_lo, inv_dn;                           // 1 / c0, n_lo, 1 / (n_hi - n_lo)
    };

enum { QLL_PLAIN = 0, QLL_TRANSFORM = 1, QLL_AVERAGE = 2, QLL_BONDS = 3 };

// the ramp of the solid-bond count: sigma = 3 t^2 - 2 t^3, t = clip((d - d_lo) / (d_hi - d_lo), 0, 1), and d sigma / dd
struct QllRamp
    {
    double d_lo, inv_dd;                                   // d_lo, 1 / (d_hi - d_lo)
    __device__ __forceinline__ void operator()(const double d, double &sg, double &dsg) const
        {
        const double t = fmin(fmax((d - d_lo) * inv_dd, 0.0), 1.0);
        sg = t * t * (3.0 - 2.0 * t);
        dsg = 6.0 * t * (1.0 - t) * inv_dd;
        }
    };

// h = x^p / (1 + x^p), x = max(c, 0) / c0 (h = c without a switch); g = 3 t^2 - 2 t^3, t = clip((n - n_lo) / (n_hi - n_lo), 0, 1)
// (g = 1 without a gate); and their derivatives.  x^(p - 1) by squaring: p is uniform, the loop is a scalar one.
__device__ __forceinline__ void qll_transform(const QllOpt &o, const double c, const double n, double &h, double &dh, double &g, double &dg)
    {
    h = c;
    dh = 1.0;
    if (o.sw)
        {
        const double x = fmax(c, 0.0) * o.inv_c0;
        double xp1 = 1.0, b = x;
        for (unsigned int k = o.p - 1; k != 0; k >>= 1)
            {
            if (k & 1u) xp1 *= b;
            b *= b;
            }
        const double xp = xp1 * x, den = 1.0 / (1.0 + xp);
        h = xp * den;
        dh = c >= 0.0 ? (double)o.p * xp1 * (den * den) * o.inv_c0 : 0.0;
        if (!(xp < HUGE_VAL))                                // x^p beyond the range of a double: the limit, not inf * 0
            {
            h = 1.0;
            dh = 0.0;
            }
        }
    g = 1.0;
    dg = 0.0;
    if (o.gate)
        {
        const double t = fmin(fmax((n - o.n_lo) * o.inv_dn, 0.0), 1.0);
        g = t * t * (3.0 - 2.0 * t);
        dg = 6.0 * t * (1.0 - t) * o.inv_dn;
        }
    }

// ---- pass 1: n_i, A_lm(i) -> c_i, table row, block sums of c_i ------------------------------------------------------------
// MODE  QLL_PLAIN      the variable without options, as described above
//       QLL_TRANSFORM  switch and/or gate, no average: c_i is formed before the row is scaled; the row is g h'(c_i) times the plain one
//                      with g'(n_i) h(c_i) added to its (0, 0) slot, v_i = g h is written and block-summed in place of c_i
//       QLL_AVERAGE    writes n_i and the monic row S_lm(i) / n_i (q_lm = nrm(l, m) times it) for the two gather passes below, and
//                      (block 0) the weight of every slot, wtab[off[l] + m] = Ql_ref[l] 4 pi / (2l + 1) (m > 0 ? 2 : 1) nrm(l, m)^2
//       QLL_BONDS      the sums of QLL_AVERAGE and the slot weights; writes n_i, the plain c_i = sum_c w_c |qm_c(i)|^2 and the monic row
//                      NORMALISED, u_c(i) = qm_c(i) / sqrt(c_i) (0 when c_i == 0), for the two gather passes of the bond count
template<typename S4, int LMAX, int MODE>
__global__ __launch_bounds__(QLL_THREADS) void k_qll_accumulate(const QlArgs<LMAX> a, const QllLayout lay, const QllOpt o, const S4 *__restrict__ postype,
                                                                const unsigned int *__restrict__ head_list,
                                                                const unsigned int *__restrict__ n_neigh,
                                                                const unsigned int *__restrict__ nlist, double *__restrict__ n_out,
                                                                double *__restrict__ c_out, double *__restrict__ v_out, double *__restrict__ rows,
                                                                double *__restrict__ wtab, double *__restrict__ partials,
                                                                const double *__restrict__ tab)
    {
    typedef QlTab<LMAX> T;
    __shared__ double s_c[QLL_PPB];
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    double block_c = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre ci = row_centre(a, postype, head_list, n_neigh, chunk * QLL_PPB + p);
        const unsigned int i = ci.i, start = ci.start, cnt = ci.cnt;
        const Particle pi = ci.p;
        cplx S[LMAX + 1][LMAX + 1];                                                // [m][l], l >= m
#pragma unroll
        for (int m = 0; m <= LMAX; ++m)
#pragma unroll
            for (int l = 0; l <= LMAX; ++l) S[m][l] = {0.0, 0.0};
        double nsum = 0.0;
        unsigned int e = q;
        unsigned int j0 = e < cnt ? nlist[start + e] : QLL_NONE;
        unsigned int j1 = e + QLL_G < cnt ? nlist[start + e + QLL_G] : QLL_NONE;
        S4 pos0 = row_zero<S4>();
        if (j0 < a.N) pos0 = postype[j0];
#pragma unroll 1
        for (; e < cnt; e += QLL_G)
            {
            const double *__restrict__ tab_k = loop_table(tab);
            const unsigned int j2 = e + 2 * QLL_G < cnt ? nlist[start + e + 2 * QLL_G] : QLL_NONE;
            S4 pos1 = row_zero<S4>();
            if (j1 < a.N) pos1 = postype[j1];
            if (j0 < a.N && j0 != i)
                {
                const Particle pj = scalar4_traits<S4>::unpack(pos0);
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(a, dx, dy, dz);
                const double rsq = dx * dx + dy * dy + dz * dz;
                if ((unsigned int)pj.type == a.type && rsq <= a.rcutsq)
                    {
                    const double inv_r = rsqrt(rsq);
                    const double ct = dz * inv_r, ex = dx * inv_r, ey = dy * inv_r;
                    double f, fprime_divr;
                    smoothing_tab<LMAX>(a, tab_k, rsq, inv_r, f, fprime_divr);
                    nsum += f;
                    cplx fh = {f, 0.0};                                              // f h^m
#pragma unroll
                    for (int m = 0; m <= LMAX; ++m)
                        {
                        double pm2 = 1.0, pm1 = ct;                                  // p_m,n-2 and p_m,n-1
#pragma unroll
                        for (int nn = 0; m + nn <= LMAX; ++nn)
                            {
                            const int l = m + nn;
                            if (nn == 0)
                                {
                                S[m][l].re += fh.re;
                                if (m > 0) S[m][l].im += fh.im;
                                }
                            else
                                {
                                double pn = ct;
                                if (nn >= 2)
                                    {
                                    pn = ct * pm1 - tab_k[T::beta(m, nn)] * pm2;
                                    pm2 = pm1;
                                    pm1 = pn;
                                    }
                                S[m][l].re += pn * fh.re;
                                if (m > 0) S[m][l].im += pn * fh.im;
                                }
                            }
                        if (m < LMAX) fh = m == 0 ? cplx{f * ex, f * ey} : cmul(fh, {ex, ey});
                        }
                    }
                }
            j0 = j1;
            j1 = j2;
            pos0 = pos1;
            }
        // the quad's sums (every lane of the wave is here: the chunk loop is uniform), then the particle's value and table row
        nsum = group_sum<QLL_G>(nsum);
        const double inv_n = nsum > 0.0 ? 1.0 / nsum : 0.0;
        const double inv_n2 = inv_n * inv_n;
        const bool write = q == 0 && i < a.N;
        double *__restrict__ row = rows + (size_t)ci.row(a.N) * lay.row_doubles;
        double c = 0.0, r00 = 0.0;
        if constexpr (MODE == QLL_PLAIN)
            {
#pragma unroll
            for (int l = 0; l <= LMAX; ++l)
                {
#pragma unroll
                for (int m = 0; m <= l; ++m)
                    {
                    S[m][l].re = group_sum<QLL_G>(S[m][l].re);
                    if (m > 0) S[m][l].im = group_sum<QLL_G>(S[m][l].im);
                    }
                if (lay.act & (1u << l))
                    {
                    const double gl = a.ql_ref[l] * (4.0 * M_PI / (2 * l + 1)) * inv_n2;
                    double sq = 0.0;
#pragma unroll
                    for (int m = 0; m <= l; ++m)
                        {
                        const double nr = tab[T::nrm(l, m)];
                        const double w = (m > 0 ? 2.0 : 1.0) * (nr * nr);
                        sq += w * (S[m][l].re * S[m][l].re + S[m][l].im * S[m][l].im);
                        const double rr = 2.0 * gl * w;
                        if (l == 0)
                            r00 = rr * S[m][l].re;
                        else if (write)
                            {
                            row[2 * (lay.off[l] + m)] = rr * S[m][l].re;
                            row[2 * (lay.off[l] + m) + 1] = -(rr * S[m][l].im);
                            }
                        }
                    c += gl * sq;
                    }
                }
            if (write)
                {
                row[0] = r00 - 2.0 * c * inv_n;
                row[1] = 0.0;
                n_out[i] = nsum;
                c_out[i] = c;
                }
            }
        else if constexpr (MODE == QLL_TRANSFORM)
            {
            // c_i first: the row is scaled with g(n_i) h'(c_i)
#pragma unroll
            for (int l = 0; l <= LMAX; ++l)
                if (lay.act & (1u << l))
                    {
                    const double gl = a.ql_ref[l] * (4.0 * M_PI / (2 * l + 1)) * inv_n2;
                    double sq = 0.0;
#pragma unroll
                    for (int m = 0; m <= l; ++m)
                        {
                        S[m][l].re = group_sum<QLL_G>(S[m][l].re);
                        if (m > 0) S[m][l].im = group_sum<QLL_G>(S[m][l].im);
                        const double nr = tab[T::nrm(l, m)];
                        sq += ((m > 0 ? 2.0 : 1.0) * (nr * nr)) * (S[m][l].re * S[m][l].re + S[m][l].im * S[m][l].im);
                        }
                    c += gl * sq;
                    }
            double h, dh, g, dg;
            qll_transform(o, c, nsum, h, dh, g, dg);
            const double gh = g * dh;
#pragma unroll
            for (int l = 0; l <= LMAX; ++l)
                if (lay.act & (1u << l))
                    {
                    const double gl = a.ql_ref[l] * (4.0 * M_PI / (2 * l + 1)) * inv_n2;
#pragma unroll
                    for (int m = 0; m <= l; ++m)
                        {
                        const double nr = tab[T::nrm(l, m)];
                        const double rr = gh * (2.0 * gl * ((m > 0 ? 2.0 : 1.0) * (nr * nr)));
                        if (l == 0)
                            r00 = rr * S[m][l].re;
                        else if (write)
                            {
                            row[2 * (lay.off[l] + m)] = rr * S[m][l].re;
                            row[2 * (lay.off[l] + m) + 1] = -(rr * S[m][l].im);
                            }
                        }
                    }
            if (write)
                {
                row[0] = r00 - gh * (2.0 * c * inv_n) + dg * h;
                row[1] = 0.0;
                n_out[i] = nsum;
                c_out[i] = c;
                v_out[i] = g * h;
                }
            c = g * h;                                                              // what the blocks sum
            }
        else if constexpr (MODE == QLL_BONDS)
            {
            // c_i first: the row is scaled with 1 / sqrt(c_i).  Up to LMAX = 6 the sums wait in registers for it.  Above, that costs a wave
            // per SIMD (LMAX = 8: 256 + 9 registers against 243) or does not fit at all (LMAX = 12: spills), so there the row is written
            // monic as QLL_AVERAGE writes it and the lane scales what it wrote itself
            constexpr bool KEEP = LMAX <= 6;
            if (write)
                {
                row[0] = 0.0;
                row[1] = 0.0;
                n_out[i] = nsum;
                }
#pragma unroll
            for (int l = 0; l <= LMAX; ++l)
                if (lay.act & (1u << l))
                    {
                    const double gl = a.ql_ref[l] * (4.0 * M_PI / (2 * l + 1));
                    double sq = 0.0;
#pragma unroll
                    for (int m = 0; m <= l; ++m)
                        {
                        S[m][l].re = group_sum<QLL_G>(S[m][l].re);
                        if (m > 0) S[m][l].im = group_sum<QLL_G>(S[m][l].im);
                        const double nr = tab[T::nrm(l, m)];
                        const double w = (m > 0 ? 2.0 : 1.0) * (nr * nr);
                        sq += w * (S[m][l].re * S[m][l].re + S[m][l].im * S[m][l].im);
                        if (!KEEP && write)
                            {
                            row[2 * (lay.off[l] + m)] = S[m][l].re * inv_n;
                            row[2 * (lay.off[l] + m) + 1] = m > 0 ? S[m][l].im * inv_n : 0.0;
                            }
                        if (chunk == 0 && tid == 0) wtab[lay.off[l] + m] = gl * w;
                        }
                    c += (gl * inv_n2) * sq;
                    }
            if (chunk == 0 && tid == 0 && !(lay.act & 1u)) wtab[0] = 0.0;
            const double inv_rc = c > 0.0 ? 1.0 / sqrt(c) : 0.0;
            if (write) c_out[i] = c;
            if constexpr (KEEP)
                {
                const double un = inv_n * inv_rc;
#pragma unroll
                for (int l = 0; l <= LMAX; ++l)
                    if (lay.act & (1u << l))
                        {
#pragma unroll
                        for (int m = 0; m <= l; ++m)
                            if (write)
                                {
                                row[2 * (lay.off[l] + m)] = S[m][l].re * un;
                                row[2 * (lay.off[l] + m) + 1] = m > 0 ? S[m][l].im * un : 0.0;
                                }
                        }
                }
            else if (write)
                {
                double2 *row2 = reinterpret_cast<double2 *>(row);
                const unsigned int rs16 = lay.row_doubles / 2;
#pragma unroll 1
                for (unsigned int cc = 0; cc < rs16; cc += 4)                        // four loads in flight, then their stores
                    {
                    double2 r[4];
#pragma unroll
                    for (unsigned int v = 0; v < 4; ++v) r[v] = row2[cc + v < rs16 ? cc + v : rs16 - 1];
#pragma unroll
                    for (unsigned int v = 0; v < 4; ++v)
                        if (cc + v < rs16) row2[cc + v] = make_double2(r[v].x * inv_rc, r[v].y * inv_rc);
                    }
                }
            }
        else
            {
            if (write)
                {
                row[0] = 0.0;
                row[1] = 0.0;
                n_out[i] = nsum;
                }
#pragma unroll
            for (int l = 0; l <= LMAX; ++l)
                if (lay.act & (1u << l))
                    {
#pragma unroll
                    for (int m = 0; m <= l; ++m)
                        {
                        S[m][l].re = group_sum<QLL_G>(S[m][l].re);
                        if (m > 0) S[m][l].im = group_sum<QLL_G>(S[m][l].im);
                        if (write)
                            {
                            row[2 * (lay.off[l] + m)] = S[m][l].re * inv_n;
                            row[2 * (lay.off[l] + m) + 1] = m > 0 ? S[m][l].im * inv_n : 0.0;
                            }
                        if (chunk == 0 && tid == 0)
                            {
                            const double nr = tab[T::nrm(l, m)];
                            wtab[lay.off[l] + m] = a.ql_ref[l] * (4.0 * M_PI / (2 * l + 1)) * ((m > 0 ? 2.0 : 1.0) * (nr * nr));
                            }
                        }
                    }
            if (chunk == 0 && tid == 0 && !(lay.act & 1u)) wtab[0] = 0.0;
            }
        if constexpr (MODE == QLL_PLAIN || MODE == QLL_TRANSFORM)
            {
            qll_chunk_sum(s_c, tid, i < a.N ? c : 0.0, block_c);                  // c_i; v_i with a switch or a gate
            }
        }
    if constexpr (MODE == QLL_AVERAGE || MODE == QLL_BONDS) return;                 // k_qll_average / k_qll_bonds sum the v_i
    if (tid == 0) partials[blockIdx.x] = block_c;
    }

// ---- pass 2: forces, gathered --------------------------------------------------------------------------------------------
// The weight q_lm = R_lm(k) + (-1)^l R_lm(j) ql_pair_force contracts, from the two table rows: ROW is const double * (memory, a slot
// read as one double2) or const double2 * (the LDS tiles).  AVG: the pair's own scalar E_kj (k_qll_backprop) joins the (0, 0) weight,
// the coefficient of grad f
__device__ __forceinline__ double2 qll_slot(const double *row, const unsigned int s) { return *reinterpret_cast<const double2 *>(row + 2 * s); }
__device__ __forceinline__ double2 qll_slot(const double2 *row, const unsigned int s) { return row[s]; }

template<bool AVG, typename ROW> struct QllWeights
    {
    ROW rk, rj;                                            // the rows of this lane's particle and of its neighbour
    const QllLayout &lay;
    double e;
    __device__ __forceinline__ cplx operator()(const int l, const int m, const int) const
        {
        const unsigned int s = lay.off[l] + m;
        const double2 wk = qll_slot(rk, s), wj = qll_slot(rj, s);
        if (l & 1) return {wk.x - wj.x, wk.y - wj.y};
        if (AVG && l == 0) return {wk.x + wj.x + e, wk.y + wj.y};
        return {wk.x + wj.x, wk.y + wj.y};
        }
    };

template<int LMAX> constexpr int qll_force_waves() { return LMAX <= 4 ? 3 : (LMAX <= 6 ? 2 : 1); }

// VIR: the virial of the bias force beside it (definition: include/mtd_abi.h).  fp is the complete force of the pair {k, j} on k and d
// its pair vector, so the entry gives 1/2 d_a fp_b to k — the other half is formed in row j, from -d and -fp.  Six more sums per lane,
// added over the quad in the order of the force and stored by lane 0, component c at virial[c * pitch + k]: no atomics, no LDS.  The
// VIR = false instantiations are the kernels without the switch, instruction for instruction (profiles/r12).
struct QllVirial
    {
    double xx, xy, xz, yy, yz, zz;
    __device__ __forceinline__ void add(const double dx, const double dy, const double dz, const double fx, const double fy, const double fz)
        {
        xx += dx * fx, xy += dx * fy, xz += dx * fz;
        yy += dy * fy, yz += dy * fz, zz += dz * fz;
        }
    template<typename scalar> __device__ __forceinline__ void store(scalar *virial, const unsigned int pitch, const unsigned int k, const unsigned int q,
                                                                     const unsigned int N, const double scale)
        {
        xx = group_sum<QLL_G>(xx), xy = group_sum<QLL_G>(xy), xz = group_sum<QLL_G>(xz);
        yy = group_sum<QLL_G>(yy), yz = group_sum<QLL_G>(yz), zz = group_sum<QLL_G>(zz);
        if (q == 0 && k < N)
            {
            const double h = 0.5 * scale;
            scalar *v = virial + k;
            nt_store((scalar)(xx * h), v);
            nt_store((scalar)(xy * h), v + pitch);
            nt_store((scalar)(xz * h), v + 2 * (size_t)pitch);
            nt_store((scalar)(yy * h), v + 3 * (size_t)pitch);
            nt_store((scalar)(yz * h), v + 4 * (size_t)pitch);
            nt_store((scalar)(zz * h), v + 5 * (size_t)pitch);
            }
        }
    };

template<typename S4, int LMAX, bool AVG, bool VIR>
__global__ __launch_bounds__(QLL_THREADS, (qll_force_waves<LMAX>())) void k_qll_forces(const QlArgs<LMAX> a, const QllLayout lay, const S4 *__restrict__ postype,
                                                            const unsigned int *__restrict__ head_list,
                                                            const unsigned int *__restrict__ n_neigh,
                                                            const unsigned int *__restrict__ nlist, const double *__restrict__ rows,
                                                            S4 *__restrict__ force, const double *__restrict__ d_bias, const double bias_host,
                                                            const double *__restrict__ tab, const double *__restrict__ epair,
                                                            typename scalar4_traits<S4>::scalar *__restrict__ virial, const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    const double scale = (d_bias ? *d_bias : bias_host) / (double)a.n_global;
    const unsigned int act = __builtin_amdgcn_readfirstlane(lay.act | 1u);         // slot (0, 0) carries the -2 (c_k/n_k + c_j/n_j) grad f term
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre ck = row_centre(a, postype, head_list, n_neigh, chunk * QLL_PPB + p);
        const unsigned int k = ck.i, start = ck.start, cnt = ck.cnt;
        const Particle pk = ck.p;
        const double *__restrict__ rk = rows + (size_t)ck.row(a.N) * lay.row_doubles;
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        QllVirial W = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        unsigned int e = q;
        unsigned int j0 = e < cnt ? nlist[start + e] : QLL_NONE;
        unsigned int j1 = e + QLL_G < cnt ? nlist[start + e + QLL_G] : QLL_NONE;
        S4 pos0 = row_zero<S4>();
        if (j0 < a.N) pos0 = postype[j0];
        double e0 = 0.0;                                     // E of the entry in hand; the next one travels with the next position
        if (AVG && e < cnt) e0 = epair[start + e];
#pragma unroll 1
        for (; e < cnt; e += QLL_G)
            {
            const double *__restrict__ tab_k = loop_table(tab);
            const unsigned int j2 = e + 2 * QLL_G < cnt ? nlist[start + e + 2 * QLL_G] : QLL_NONE;
            S4 pos1 = row_zero<S4>();
            if (j1 < a.N) pos1 = postype[j1];
            double e1 = 0.0;
            if (AVG && e + QLL_G < cnt) e1 = epair[start + e + QLL_G];
            if (j0 < a.N && j0 != k)
                {
                const Particle pj = scalar4_traits<S4>::unpack(pos0);
                double dx = pk.x - pj.x, dy = pk.y - pj.y, dz = pk.z - pj.z;
                min_image(a, dx, dy, dz);
                const double rsq = dx * dx + dy * dy + dz * dz;
                if ((unsigned int)pj.type == a.type && rsq <= a.rcutsq)
                    {
                    double fpx, fpy, fpz;
                    ql_pair_force<LMAX>(a, tab_k, QllWeights<AVG, const double *>{rk, rows + (size_t)j0 * lay.row_doubles, lay, e0}, act, dx, dy, dz, rsq, fpx, fpy, fpz);
                    Fx += fpx;
                    Fy += fpy;
                    Fz += fpz;
                    if constexpr (VIR) W.add(dx, dy, dz, fpx, fpy, fpz);
                    }
                }
            j0 = j1;
            j1 = j2;
            pos0 = pos1;
            if (AVG) e0 = e1;
            }
        Fx = group_sum<QLL_G>(Fx);
        Fy = group_sum<QLL_G>(Fy);
        Fz = group_sum<QLL_G>(Fz);
        if (q == 0 && k < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + k);
        if constexpr (VIR) W.store(virial, virial_pitch, k, q, a.N, scale);
        }
    }

// ---- pass 2 through LDS tiles: rows of at most QLL_TILE_MAX16 x 16 bytes ------------------------------------------------------
// The direct form above reads a table row with one 16-byte load per lane and (l, m): 64 different cache lines per wave instruction,
// 26 such instructions per entry — it runs at the rate the L1 looks lines up (measured at config 5: 203 us, three times the global
// pass with the same pair arithmetic).  Here the wave fetches the 64 neighbour rows of an iteration TOGETHER: four lanes take 64
// consecutive bytes of one row (16 rows per instruction), the rows land in the wave's own LDS tile and every lane reads its row
// back from there; the 16 own rows of the wave's particles are fetched the same way once per chunk.  Entries beyond the cut-off or
// of another type are dropped before their row is asked for.  Tiles are private to a wave: wave barriers only.
constexpr unsigned int QLL_TILE_MAX16 = 16;
constexpr unsigned int QLL_TILE_ROWS = QLL_THREADS + QLL_PPB;            // 64 neighbour rows per wave + 16 own rows per wave

__device__ __forceinline__ void qll_wave_sync()
    {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

template<typename S4, int LMAX, bool AVG, bool VIR>
__global__ __launch_bounds__(QLL_THREADS, (qll_force_waves<LMAX>())) void k_qll_forces_tile(const QlArgs<LMAX> a, const QllLayout lay, const S4 *__restrict__ postype,
                                                            const unsigned int *__restrict__ head_list,
                                                            const unsigned int *__restrict__ n_neigh,
                                                            const unsigned int *__restrict__ nlist, const double *__restrict__ rows,
                                                            S4 *__restrict__ force, const double *__restrict__ d_bias, const double bias_host,
                                                            const double *__restrict__ tab, const unsigned int ts /* tile row stride, 16-byte units */,
                                                            const double *__restrict__ epair,
                                                            typename scalar4_traits<S4>::scalar *__restrict__ virial, const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    extern __shared__ double2 s_tiles[];
    __shared__ unsigned int s_j[QLL_THREADS];
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G, lane = tid & 63u, wave = tid >> 6;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    const unsigned int rs16 = lay.row_doubles / 2;
    const double2 *__restrict__ rows16 = reinterpret_cast<const double2 *>(rows);
    double2 *tile_j = s_tiles + (size_t)wave * MTD_WAVE * ts;
    double2 *tile_k = s_tiles + (size_t)QLL_THREADS * ts + (size_t)wave * (MTD_WAVE / QLL_G) * ts;
    unsigned int *sj = s_j + wave * MTD_WAVE;
    const double scale = (d_bias ? *d_bias : bias_host) / (double)a.n_global;
    const unsigned int act = __builtin_amdgcn_readfirstlane(lay.act | 1u);
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre ck = row_centre(a, postype, head_list, n_neigh, chunk * QLL_PPB + p);
        const unsigned int k = ck.i, start = ck.start, cnt = ck.cnt;
        const Particle pk = ck.p;
        qll_wave_sync();                                    // the last chunk's reads of the tiles are done
        if (cnt > 0)
            {
#pragma unroll
            for (unsigned int v = 0; v < QLL_TILE_MAX16 / QLL_G; ++v)
                {
                const unsigned int c = QLL_G * v + q;
                if (c < rs16) tile_k[(lane / QLL_G) * ts + c] = rows16[(size_t)k * rs16 + c];
                }
            }
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        QllVirial W = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        unsigned int e = q;
        unsigned int j0 = e < cnt ? nlist[start + e] : QLL_NONE;
        unsigned int j1 = e + QLL_G < cnt ? nlist[start + e + QLL_G] : QLL_NONE;
        S4 pos0 = row_zero<S4>();
        if (j0 < a.N) pos0 = postype[j0];
        double e0 = 0.0;                                     // E of the entry in hand; the next one travels with the next position
        if (AVG && e < cnt) e0 = epair[start + e];
#pragma unroll 1
        while (__ballot(e < cnt) != 0ull)
            {
            const double *__restrict__ tab_k = loop_table(tab);
            const unsigned int j2 = e + 2 * QLL_G < cnt ? nlist[start + e + 2 * QLL_G] : QLL_NONE;
            S4 pos1 = row_zero<S4>();
            if (j1 < a.N) pos1 = postype[j1];
            double e1 = 0.0;
            if (AVG && e + QLL_G < cnt) e1 = epair[start + e + QLL_G];
            const Particle pj = scalar4_traits<S4>::unpack(pos0);
            double dx = pk.x - pj.x, dy = pk.y - pj.y, dz = pk.z - pj.z;
            min_image(a, dx, dy, dz);
            const double rsq = dx * dx + dy * dy + dz * dz;
            const bool visit = e < cnt && j0 < a.N && j0 != k && (unsigned int)pj.type == a.type && rsq <= a.rcutsq;
            if (__ballot(visit) != 0ull)
                {
                // the rows of this iteration's neighbours -> the wave's tile
                sj[lane] = visit ? j0 : QLL_NONE;
                qll_wave_sync();
                double2 w[MTD_WAVE / 16][QLL_TILE_MAX16 / QLL_G];
#pragma unroll
                for (unsigned int u = 0; u < MTD_WAVE / 16; ++u)
                    {
                    const unsigned int jr = sj[16 * u + lane / QLL_G];
#pragma unroll
                    for (unsigned int v = 0; v < QLL_TILE_MAX16 / QLL_G; ++v)
                        {
                        const unsigned int c = QLL_G * v + q;
                        w[u][v] = make_double2(0.0, 0.0);
                        if (jr != QLL_NONE && c < rs16) w[u][v] = rows16[(size_t)jr * rs16 + c];
                        }
                    }
#pragma unroll
                for (unsigned int u = 0; u < MTD_WAVE / 16; ++u)
#pragma unroll
                    for (unsigned int v = 0; v < QLL_TILE_MAX16 / QLL_G; ++v)
                        {
                        const unsigned int c = QLL_G * v + q;
                        if (c < rs16) tile_j[(16 * u + lane / QLL_G) * ts + c] = w[u][v];
                        }
                qll_wave_sync();
                if (visit)
                    {
                    double fpx, fpy, fpz;
                    ql_pair_force<LMAX>(a, tab_k, QllWeights<AVG, const double2 *>{tile_k + (lane / QLL_G) * ts, tile_j + lane * ts, lay, e0}, act, dx, dy, dz, rsq, fpx, fpy, fpz);
                    Fx += fpx;
                    Fy += fpy;
                    Fz += fpz;
                    if constexpr (VIR) W.add(dx, dy, dz, fpx, fpy, fpz);
                    }
                qll_wave_sync();                            // the tile is free for the next iteration
                }
            j0 = j1;
            j1 = j2;
            pos0 = pos1;
            if (AVG) e0 = e1;
            e += QLL_G;
            }
        Fx = group_sum<QLL_G>(Fx);
        Fy = group_sum<QLL_G>(Fy);
        Fz = group_sum<QLL_G>(Fz);
        if (q == 0 && k < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + k);
        if constexpr (VIR) W.store(virial, virial_pitch, k, q, a.N, scale);
        }
    }

// ---- the gather passes: the averaged variable and the solid-bond count, two passes each between pass 1 and the force pass --------
// Gather pattern: a quad still owns one central particle and its lanes still take entries q, q + 4, ... of the row for
// the pair geometry (same look-ahead), but the ROWS are split by slot: lane q holds slots q, q + 4, ... of its particle.  Each of the
// quad's four entries is handed round with a DPP quad broadcast (index and a scalar), and the four lanes read 64 consecutive bytes of
// that neighbour's row: sixteen rows per wave instruction, whole 64-byte segments, no LDS, and the sums stay in registers in list order.
// Rows longer than QLL_GV x 64 bytes are taken in windows of QLL_GV x 4 slots, the list walked once per window.  Entries that do not
// count (beyond r_cut, other type, self, j >= N) read the particle's own row with f = 0: the loads need no branch.
// The frame of all four kernels is written once, below: the window and its slots (QllWindow), the walk over the entries of a row
// (qll_entries, on QllWalker), the hand-round of the quad's four entries (quad_all; with the rows added up, qll_add_rows), the quad's
// sum for an entry that only the entry's own lane keeps (quad_keep) and the per-entry scratch that is summed over the windows
// (qll_park).  What is left in a kernel is its sums.
constexpr unsigned int QLL_GV = 4;                                  // 16-byte slots per lane and window: one window up to 256-byte rows

// one window of a row of rs16 slots: lane q of the quad holds slots w0 + q, w0 + 4 + q, ... (QLL_GV of them)
struct QllWindow
    {
    unsigned int w0;
    const unsigned int rs16, q;
    __device__ __forceinline__ QllWindow(const unsigned int rs16_, const unsigned int q_) : w0(0), rs16(rs16_), q(q_) {}
    __device__ __forceinline__ bool more() const { return w0 < rs16; }
    __device__ __forceinline__ void next() { w0 += QLL_G * QLL_GV; }
    __device__ __forceinline__ bool first() const { return w0 == 0; }
    __device__ __forceinline__ bool last() const { return w0 + QLL_G * QLL_GV >= rs16; }
    __device__ __forceinline__ unsigned int slot(const unsigned int v) const { return w0 + QLL_G * v + q; }
    __device__ __forceinline__ bool inside(const unsigned int v) const { return slot(v) < rs16; }        // a slot past the row adds nothing
    __device__ __forceinline__ unsigned int clamped(const unsigned int v) const { return inside(v) ? slot(v) : rs16 - 1; }   // safe to load
    };

// what the walk hands to a gather pass for the entry a lane has in hand
struct QllEntry
    {
    double f;                                              // the smoothing function; 0 for an entry that does not count
    unsigned int j;                                        // the neighbour; the central particle's own (safe) row for one that does not count
    bool counts;
    unsigned int e, start, cnt;                            // entry e of the row that starts at `start` and has cnt entries
    __device__ __forceinline__ bool mine() const { return e < cnt; }               // the lane has an entry at all: the quad walks its row together
    __device__ __forceinline__ unsigned int at() const { return start + e; }       // where it sits in the list, and in the per-entry scratch
    };

// the entries of the quad's row, four per round: body(QllEntry) for the entry of this lane, every lane of the quad in every round
template<typename S4, typename F>
__device__ __forceinline__ void qll_entries(const QlArgs<12> &a, const S4 *postype, const unsigned int *nlist, const RowCentre &c,
                                            const unsigned int q, const double *tab, F &&body)
    {
    QllWalker<S4> w;
    w.begin(a.N, postype, nlist, c, q);
#pragma unroll 1
    for (unsigned int eb = 0; eb < c.cnt; eb += QLL_G, w.step())                    // cnt is the quad's: its four lanes stay together
        {
        const double *__restrict__ tab_k = loop_table(tab);
        w.ahead(a.N, postype, nlist, c);
        QllEntry en = {0.0, c.row(a.N), false, w.e, c.start, c.cnt};
        w.pair(a, c, [&](double, double, double, const double rsq)
            {
            double fprime_divr;
            smoothing_tab<12>(a, tab_k, rsq, rsqrt(rsq), en.f, fprime_divr);
            en.j = w.j0;
            en.counts = true;
            });
        body(en);
        }
    }

// the quad's four values of v, lane by lane, in all four of its lanes
template<typename T> __device__ __forceinline__ void quad_all(const T v, T (&of)[QLL_G])
    {
    of[0] = quad_bcast<0>(v), of[1] = quad_bcast<1>(v), of[2] = quad_bcast<2>(v), of[3] = quad_bcast<3>(v);
    }

// acc_c += sum over the quad's four entries (neighbour j, scalar s, lane by lane: list order) of s row_c(j), for this lane's slots cs
__device__ __forceinline__ void qll_add_rows(double2 (&acc)[QLL_GV], const double2 *rows, const unsigned int rs16, const unsigned int (&cs)[QLL_GV],
                                             const unsigned int j, const double s)
    {
    unsigned int ju[QLL_G];
    double su[QLL_G];
    quad_all(j, ju);
    quad_all(s, su);
#pragma unroll
    for (unsigned int u = 0; u < QLL_G; ++u)
#pragma unroll
        for (unsigned int v = 0; v < QLL_GV; ++v)
            {
            const double2 r = rows[(size_t)ju[u] * rs16 + cs[v]];
            acc[v].x += su[u] * r.x;
            acc[v].y += su[u] * r.y;
            }
    }

// share(u) is this lane's share of a sum that belongs to the entry of lane u: the quad's sums, of which every lane keeps its own
template<typename F> __device__ __forceinline__ double quad_keep(const unsigned int q, F &&share)
    {
    double mine = 0.0;
#pragma unroll
    for (unsigned int u = 0; u < QLL_G; ++u)
        {
        const double sum = group_sum<QLL_G>(share(u));
        if (q == u) mine = sum;
        }
    return mine;
    }

// a per-entry value that is summed over the windows: the lane adds to what it wrote in the last window; returns the sum so far
__device__ __forceinline__ double qll_park(double *epair, const QllEntry &en, const QllWindow &win, double val)
    {
    if (!win.first()) val += epair[en.at()];
    epair[en.at()] = val;
    return val;
    }

// ---- the averaged variable ----------------------------------------------------------------------------------------------------
// Rows here are the MONIC ones of pass 1, qm_c(i) = S_lm(i) / n_i per slot c = off[l] + m (q_lm = nrm(l, m) qm), and the slot weights
// w_c = Ql_ref[l] 4 pi / (2l + 1) (m > 0 ? 2 : 1) nrm(l, m)^2 carry everything that depends on (l, m):
//   k_qll_average   qbar_c(i) = [qm_c(i) + sum_j f_ij qm_c(j)] / (1 + n_i),  c_i = sum_c w_c |qbar_c(i)|^2,  v_i = g(n_i) h(c_i),
//                   Bm_c(i) = g h'(c_i) 2 w_c conj(qbar_c(i)) / (1 + n_i)    (sum_c Re Bm_c qm_c = Re sum_lm B_lm q_lm of the header),
//                   a0_i = g'(n_i) h(c_i) - g h' 2 c_i / (1 + n_i),  block sums of v_i
//   k_qll_backprop  Cm_c(k) = Bm_c(k) + sum_i f_ik Bm_c(i);  the table row of the force pass R_c(k) = Cm_c(k) / n_k with
//                   a_k = a0_k - sum_c Re Cm_c(k) qm_c(k) / n_k added to slot 0;  per list entry E_kj = sum_c Re[Bm_c(k) qm_c(j) + Bm_c(j) qm_c(k)]
template<typename S4>
__global__ __launch_bounds__(QLL_THREADS) void k_qll_average(const QlArgs<12> a, const QllOpt o, const unsigned int rs16, const S4 *__restrict__ postype,
                                                             const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                             const unsigned int *__restrict__ nlist, const double *__restrict__ n_in,
                                                             const double2 *__restrict__ qrows, const double *__restrict__ wtab,
                                                             double2 *brows, double *__restrict__ c_out, double *__restrict__ v_out,
                                                             double *__restrict__ a0_out, double *__restrict__ partials, const double *__restrict__ tab)
    {
    __shared__ double s_c[QLL_PPB];
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    double block_v = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre ci = row_centre(a, postype, head_list, n_neigh, chunk * QLL_PPB + p);
        const unsigned int i = ci.i, ii = ci.row(a.N);
        const double ni = ci.own(a.N, n_in);
        const double inv_1n = 1.0 / (1.0 + ni);
        double csum = 0.0;
        for (QllWindow win(rs16, q); win.more(); win.next())
            {
            unsigned int cs[QLL_GV];                                                 // this lane's slots, clamped into the row
            double2 acc[QLL_GV];
#pragma unroll
            for (unsigned int v = 0; v < QLL_GV; ++v)
                {
                cs[v] = win.clamped(v);
                acc[v] = qrows[(size_t)ii * rs16 + cs[v]];
                }
            qll_entries(a, postype, nlist, ci, q, tab, [&](const QllEntry &en)
                {
                qll_add_rows(acc, qrows, rs16, cs, en.j, en.f);
                });
            // this window of qbar: its share of c_i, and 2 w conj(qbar) / (1 + n) parked in the B row until h'(c_i) is known
#pragma unroll
            for (unsigned int v = 0; v < QLL_GV; ++v)
                if (win.inside(v))
                    {
                    const unsigned int c = win.slot(v);
                    const double w = wtab[c];
                    const double qx = acc[v].x * inv_1n, qy = acc[v].y * inv_1n;
                    csum += w * (qx * qx + qy * qy);
                    if (i < a.N) brows[(size_t)i * rs16 + c] = make_double2(2.0 * w * inv_1n * qx, -(2.0 * w * inv_1n * qy));
                    }
            }
        const double c = group_sum<QLL_G>(csum);
        double h, dh, g, dg;
        qll_transform(o, c, ni, h, dh, g, dg);
        const double gh = g * dh;
        for (unsigned int cc = q; cc < rs16; cc += QLL_G)                           // the lane scales what it wrote itself
            if (i < a.N)
                {
                const double2 b = brows[(size_t)i * rs16 + cc];
                brows[(size_t)i * rs16 + cc] = make_double2(gh * b.x, gh * b.y);
                }
        if (q == 0 && i < a.N)
            {
            c_out[i] = c;
            v_out[i] = g * h;
            a0_out[i] = dg * h - gh * (2.0 * c * inv_1n);
            }
        qll_chunk_sum(s_c, tid, i < a.N ? g * h : 0.0, block_v);
        }
    if (tid == 0) partials[blockIdx.x] = block_v;
    }

template<typename S4>
__global__ __launch_bounds__(QLL_THREADS) void k_qll_backprop(const QlArgs<12> a, const unsigned int rs16, const S4 *__restrict__ postype,
                                                              const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                              const unsigned int *__restrict__ nlist, const double *__restrict__ n_in,
                                                              const double *__restrict__ a0_in, const double2 *__restrict__ qrows,
                                                              const double2 *__restrict__ brows, double2 *__restrict__ rows, double *epair,
                                                              const double *__restrict__ tab)
    {
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre ck = row_centre(a, postype, head_list, n_neigh, chunk * QLL_PPB + p);
        const unsigned int k = ck.i, kk = ck.row(a.N);
        const double nk = ck.own(a.N, n_in), a0 = ck.own(a.N, a0_in);
        const double inv_n = nk > 0.0 ? 1.0 / nk : 0.0;
        double cq = 0.0, r00 = 0.0;
        for (QllWindow win(rs16, q); win.more(); win.next())
            {
            unsigned int cs[QLL_GV];
            double2 acc[QLL_GV], bk[QLL_GV], qk[QLL_GV];
#pragma unroll
            for (unsigned int v = 0; v < QLL_GV; ++v)
                {
                cs[v] = win.clamped(v);
                bk[v] = brows[(size_t)kk * rs16 + cs[v]];
                qk[v] = qrows[(size_t)kk * rs16 + cs[v]];
                if (!win.inside(v)) bk[v] = qk[v] = make_double2(0.0, 0.0);         // a slot past the row adds nothing to E
                acc[v] = bk[v];
                }
            qll_entries(a, postype, nlist, ck, q, tab, [&](const QllEntry &en)
                {
                unsigned int ju[QLL_G];
                double fu[QLL_G];
                quad_all(en.j, ju);
                quad_all(en.f, fu);
                const double e_kj = quad_keep(q, [&](const unsigned int u)
                    {
                    double ee = 0.0;
#pragma unroll
                    for (unsigned int v = 0; v < QLL_GV; ++v)
                        {
                        const double2 bj = brows[(size_t)ju[u] * rs16 + cs[v]], qj = qrows[(size_t)ju[u] * rs16 + cs[v]];
                        acc[v].x += fu[u] * bj.x;
                        acc[v].y += fu[u] * bj.y;
                        ee += (bk[v].x * qj.x - bk[v].y * qj.y) + (bj.x * qk[v].x - bj.y * qk[v].y);
                        }
                    return ee;
                    });
                if (en.mine()) qll_park(epair, en, win, en.counts ? e_kj : 0.0);
                });
            // Cm of this window: its share of sum Re Cm qm, and the row of the force pass
#pragma unroll
            for (unsigned int v = 0; v < QLL_GV; ++v)
                if (win.inside(v))
                    {
                    const unsigned int c = win.slot(v);
                    cq += acc[v].x * qk[v].x - acc[v].y * qk[v].y;
                    if (c == 0)
                        r00 = acc[v].x * inv_n;
                    else if (k < a.N)
                        rows[(size_t)k * rs16 + c] = make_double2(acc[v].x * inv_n, acc[v].y * inv_n);
                    }
            }
        cq = group_sum<QLL_G>(cq);
        if (q == 0 && k < a.N) rows[(size_t)k * rs16] = make_double2(r00 + (a0 - cq * inv_n), 0.0);
        }
    }

// ---- the solid-bond count ------------------------------------------------------------------------------------------------------
// Rows here are the NORMALISED monic ones of pass 1 <QLL_BONDS>, u_c(i) = qm_c(i) / sqrt(c_i), so that with the slot weights w_c
//   d_kj = sum_c w_c Re(u_c(k) conj(u_c(j)))    in [-1, 1]: the normalised scalar product of the q vectors of the two ends of a bond.
//   k_qll_bonds           d_kj per list entry (parked in the per-entry scratch),  b_k = sum_j f_kj sigma(d_kj),  v_k = g(n_k) h(b_k),
//                         beta_k = g h'(b_k),  a0_k = g'(n_k) h(b_k),  block sums of v_k
//   k_qll_bonds_backprop  t_kj = (beta_k + beta_j) f_kj sigma'(d_kj),  Pm_c(k) = [sum_j t_kj u_c(j) - (sum_j t_kj d_kj) u_c(k)] / sqrt(c_k),
//                         Bm_c(k) = w_c conj(Pm_c(k));  the table row of the force pass R_c(k) = Bm_c(k) / n_k with
//                         a_k = a0_k - sum_c Re Bm_c(k) qm_c(k) / n_k added to slot 0 (the sum vanishes analytically: <P(k), u(k)> = 0);
//                         per list entry E_kj = (beta_k + beta_j) sigma(d_kj) in place of d_kj
// The force pass is the one of the averaged variable (AVG = true), unchanged.  beta of EVERY particle is complete before the second
// pass reads it: a launch of its own.  With more than one window the list is walked once per window: d_kj is the sum over the windows
// (qll_park, as for E in k_qll_backprop) and is read in every window of the second pass, so E replaces it in the LAST window only.  An
// entry that does not count gets E = 0.
template<typename S4>
__global__ __launch_bounds__(QLL_THREADS) void k_qll_bonds(const QlArgs<12> a, const QllOpt o, const QllRamp ramp, const unsigned int rs16,
                                                           const S4 *__restrict__ postype, const unsigned int *__restrict__ head_list,
                                                           const unsigned int *__restrict__ n_neigh, const unsigned int *__restrict__ nlist,
                                                           const double *__restrict__ n_in, const double2 *__restrict__ urows,
                                                           const double *__restrict__ wtab, double *epair, double *__restrict__ b_out,
                                                           double *__restrict__ v_out, double *__restrict__ beta_out, double *__restrict__ a0_out,
                                                           double *__restrict__ partials, const double *__restrict__ tab)
    {
    __shared__ double s_c[QLL_PPB];
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    double block_v = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre ci = row_centre(a, postype, head_list, n_neigh, chunk * QLL_PPB + p);
        const unsigned int i = ci.i, ii = ci.row(a.N);
        const double ni = ci.own(a.N, n_in);
        double bsum = 0.0;
        for (QllWindow win(rs16, q); win.more(); win.next())
            {
            const bool last = win.last();
            unsigned int cs[QLL_GV];                                                 // this lane's slots, clamped into the row
            double2 uk[QLL_GV];                                                      // w_c u_c(i); 0 for a slot past the row
#pragma unroll
            for (unsigned int v = 0; v < QLL_GV; ++v)
                {
                cs[v] = win.clamped(v);
                const double2 r = urows[(size_t)ii * rs16 + cs[v]];
                const double w = win.inside(v) ? wtab[cs[v]] : 0.0;
                uk[v] = make_double2(w * r.x, w * r.y);
                }
            qll_entries(a, postype, nlist, ci, q, tab, [&](const QllEntry &en)
                {
                unsigned int ju[QLL_G];
                quad_all(en.j, ju);
                const double d_part = quad_keep(q, [&](const unsigned int u)
                    {
                    double dd = 0.0;
#pragma unroll
                    for (unsigned int v = 0; v < QLL_GV; ++v)
                        {
                        const double2 r = urows[(size_t)ju[u] * rs16 + cs[v]];
                        dd += uk[v].x * r.x + uk[v].y * r.y;
                        }
                    return dd;
                    });
                if (en.mine())
                    {
                    const double d = qll_park(epair, en, win, d_part);
                    if (last)
                        {
                        double sg, dsg;
                        ramp(d, sg, dsg);
                        bsum += en.f * sg;                                           // f = 0 for an entry that does not count
                        }
                    }
                });
            }
        const double b = group_sum<QLL_G>(bsum);
        double h, dh, g, dg;
        qll_transform(o, b, ni, h, dh, g, dg);
        if (q == 0 && i < a.N)
            {
            b_out[i] = b;
            v_out[i] = g * h;
            beta_out[i] = g * dh;
            a0_out[i] = dg * h;
            }
        qll_chunk_sum(s_c, tid, i < a.N ? g * h : 0.0, block_v);
        }
    if (tid == 0) partials[blockIdx.x] = block_v;
    }

template<typename S4>
__global__ __launch_bounds__(QLL_THREADS) void k_qll_bonds_backprop(const QlArgs<12> a, const QllRamp ramp, const unsigned int rs16,
                                                                    const S4 *__restrict__ postype, const unsigned int *__restrict__ head_list,
                                                                    const unsigned int *__restrict__ n_neigh, const unsigned int *__restrict__ nlist,
                                                                    const double *__restrict__ n_in, const double *__restrict__ c_in,
                                                                    const double *__restrict__ beta_in, const double *__restrict__ a0_in,
                                                                    const double2 *__restrict__ urows, const double *__restrict__ wtab,
                                                                    double2 *__restrict__ rows, double *epair, const double *__restrict__ tab)
    {
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre ck = row_centre(a, postype, head_list, n_neigh, chunk * QLL_PPB + p);
        const unsigned int k = ck.i, kk = ck.row(a.N);
        const bool there = k < a.N;
        const double nk = ck.own(a.N, n_in), a0 = ck.own(a.N, a0_in), c_k = ck.own(a.N, c_in), beta_k = ck.own(a.N, beta_in);
        const double inv_n = nk > 0.0 ? 1.0 / nk : 0.0;
        const double root_c = sqrt(c_k), inv_rc = c_k > 0.0 ? 1.0 / root_c : 0.0;
        double cq = 0.0, r00 = 0.0;
        for (QllWindow win(rs16, q); win.more(); win.next())
            {
            const bool last = win.last();
            unsigned int cs[QLL_GV];
            double2 acc[QLL_GV], uk[QLL_GV];
#pragma unroll
            for (unsigned int v = 0; v < QLL_GV; ++v)
                {
                cs[v] = win.clamped(v);
                uk[v] = urows[(size_t)kk * rs16 + cs[v]];
                acc[v] = make_double2(0.0, 0.0);
                }
            double td = 0.0;                                                         // this lane's share of sum_j t_kj d_kj: whole in every window
            qll_entries(a, postype, nlist, ck, q, tab, [&](const QllEntry &en)
                {
                const double d = en.mine() ? epair[en.at()] : 0.0;
                const double bsum = beta_k + beta_in[en.j];
                double sg, dsg;
                ramp(d, sg, dsg);
                const double t = en.counts ? bsum * en.f * dsg : 0.0;
                td += t * d;
                if (en.mine() && last) epair[en.at()] = en.counts ? bsum * sg : 0.0;   // E replaces d once no window needs d again
                qll_add_rows(acc, urows, rs16, cs, en.j, t);
                });
            td = group_sum<QLL_G>(td);
            // Bm of this window: its share of sum Re Bm qm, and the row of the force pass
#pragma unroll
            for (unsigned int v = 0; v < QLL_GV; ++v)
                if (win.inside(v))
                    {
                    const unsigned int c = win.slot(v);
                    const double wc = wtab[c] * inv_rc;
                    const double bx = wc * (acc[v].x - td * uk[v].x), by = -(wc * (acc[v].y - td * uk[v].y));
                    cq += root_c * (bx * uk[v].x - by * uk[v].y);
                    if (c == 0)
                        r00 = bx * inv_n;
                    else if (there)
                        rows[(size_t)k * rs16 + c] = make_double2(bx * inv_n, by * inv_n);
                    }
            }
        cq = group_sum<QLL_G>(cq);
        if (q == 0 && there) rows[(size_t)k * rs16] = make_double2(r00 + (a0 - cq * inv_n), 0.0);
        }
    }

// ---- the largest cluster: the mask w_i of cluster.hip applied between the launches above ------------------------------------------
// The variable restricted to the largest cluster is sum_i w_i v_i with w piecewise constant: the mask enters every sum above linearly.
//   ROWS = true   (plain, switch, gate; after k_qll_accumulate) the table row R(i) times w_i — the (0, 0) slot with a_i folded in is part
//                 of the row; lane q of the quad takes slots q, q + 4, ...
//   ROWS = false  (bonds; between k_qll_bonds and k_qll_bonds_backprop) beta_i and a0_i times w_i: t_kj, E_kj and the rows then come out
//                 masked by themselves
// Both overwrite the block sums with those of w_i v_i, chunks and blocks in the order of the other passes, summed by qll_chunk_sum: no
// atomics, the same bits at every call.  v_i itself stays unmasked: it is what the clusters were built from.
template<bool ROWS>
__global__ __launch_bounds__(QLL_THREADS) void k_qll_cluster_apply(const unsigned int N, const unsigned int rs16, const double *__restrict__ w,
                                                                   const double *__restrict__ v, double2 *__restrict__ rows,
                                                                   double *__restrict__ beta, double *__restrict__ a0,
                                                                   double *__restrict__ partials)
    {
    __shared__ double s_c[QLL_PPB];
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (N + QLL_PPB - 1) / QLL_PPB;
    double block_v = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const unsigned int i = chunk * QLL_PPB + p;
        const bool there = i < N;
        const double wi = there ? w[i] : 0.0;
        if constexpr (ROWS)
            {
            if (there && wi == 0.0)                                                  // w is 0 or 1: a member's row stays as it is
                for (unsigned int c = q; c < rs16; c += QLL_G) rows[(size_t)i * rs16 + c] = make_double2(0.0, 0.0);
            }
        else if (there && q == 0 && wi == 0.0)
            {
            beta[i] = 0.0;
            a0[i] = 0.0;
            }
        qll_chunk_sum(s_c, tid, there && wi != 0.0 ? v[i] : 0.0, block_v);
        }
    if (tid == 0) partials[blockIdx.x] = block_v;
    }

// ---- host side ------------------------------------------------------------------------------------------------------------
QllLayout qll_layout(const unsigned int lmax, const double *ql_ref)
    {
    QllLayout lay;
    std::memset(&lay, 0, sizeof(lay));
    unsigned int slots = 1;                                  // slot 0: (0, 0)
    for (unsigned int l = 0; l <= lmax; ++l)
        {
        if (ql_ref[l] == 0.0) continue;
        lay.act |= 1u << l;
        if (l == 0) continue;
        lay.off[l] = slots;
        slots += l + 1;
        }
    lay.row_doubles = 2 * slots;
    return lay;
    }

bool qll_bonds_on(const mtd_ql_local_bonds *bonds) { return bonds && bonds->on; }

int qll_mode(const mtd_ql_local_options *opt, const mtd_ql_local_bonds *bonds)
    {
    if (qll_bonds_on(bonds)) return QLL_BONDS;
    if (!opt) return QLL_PLAIN;
    if (opt->average) return QLL_AVERAGE;
    return opt->switch_on || opt->gate_on ? QLL_TRANSFORM : QLL_PLAIN;
    }

// The scratch, one segment behind the other in the order of qll_scratch below; `even(x)` is x plus one double when x is odd:
//   every mode          block sums [QLL_MAX_BLOCKS] | n_i [N] | c_i [even(N)] | rows [N][(lmax + 1)(lmax + 2)]   (the most a row can take)
//   all but the plain   (one double when the above is an odd number: what the options add starts on an even offset) | v_i [even(N)]
//                       (the plain mode has no v_i: the pointer is that of c_i)
//   average and bonds   a0_i [even(N)]
//   bonds               b_i [even(N)] | beta_i [even(N)]
//   average and bonds   slot weights [even((lmax + 1)(lmax + 2) / 2)] | monic rows [N][..] (bonds: normalised)
//   average             B rows [N][..]
//   average and bonds   one double per list entry: E (bonds: d first, then E)
// A segment that a mode does not have is empty: its pointer is where the next one starts and is handed to no kernel that reads it.
struct QllScratch
    {
    double *partials, *n, *c, *rows, *v, *a0, *b, *beta, *wtab, *qrows, *brows, *epair;
    size_t total;                                          // doubles
    };

QllScratch qll_scratch(double *scratch, const size_t n, const unsigned int lmax, const size_t n_list_entries, const int mode)
    {
    const bool opts = mode != QLL_PLAIN, bonds = mode == QLL_BONDS, gathers = mode == QLL_AVERAGE || bonds;
    const size_t even_n = n + (n & 1u), row = (size_t)(lmax + 1) * (lmax + 2), slots = row / 2;
    size_t at = 0;
    const auto take = [&](const size_t len)
        {
        double *p = scratch ? scratch + at : nullptr;        // null: the caller wants the total only
        at += len;
        return p;
        };
    QllScratch s;
    s.partials = take(QLL_MAX_BLOCKS);
    s.n = take(n);
    s.c = take(even_n);
    s.rows = take(n * row);
    take(opts ? at & 1u : 0);
    s.v = opts ? take(even_n) : s.c;
    s.a0 = take(gathers ? even_n : 0);
    s.b = take(bonds ? even_n : 0);
    s.beta = take(bonds ? even_n : 0);
    s.wtab = take(gathers ? slots + (slots & 1u) : 0);
    s.qrows = take(gathers ? n * row : 0);
    s.brows = take(mode == QLL_AVERAGE ? n * row : 0);
    s.epair = take(gathers ? n_list_entries : 0);
    s.total = at;
    return s;
    }

QllOpt qll_opt(const mtd_ql_local_options *opt)
    {
    QllOpt o;
    std::memset(&o, 0, sizeof(o));
    if (!opt) return o;
    o.sw = opt->switch_on != 0;
    o.gate = opt->gate_on != 0;
    o.p = o.sw ? opt->p : 1;
    o.inv_c0 = o.sw ? 1.0 / opt->c0 : 0.0;
    o.n_lo = o.gate ? opt->n_lo : 0.0;
    o.inv_dn = o.gate ? 1.0 / (opt->n_hi - opt->n_lo) : 0.0;
    return o;
    }

// ---- one prepared call: what both terminal entry points are given, checked, and what follows from it --------------------------------
struct QllCall
    {
    unsigned int N;
    const void *postype;
    int dtype;
    const mtd_box *box;
    const unsigned int *head, *nneigh, *nlist;
    double rcut, ron;
    unsigned int lmax, type;
    const double *ql_ref;
    unsigned int n_global;
    hipStream_t s;
    int mode;
    QllLayout lay;
    QllOpt opt;
    QllRamp ramp;
    QllScratch sc;
    unsigned int blocks;
    };

// Refuses, before a device is touched and in this order: the arguments themselves; the options (a switch needs c0 > 0 and p >= 1, a gate
// 0 <= n_lo < n_hi; NaN fails every comparison); the bond count (a ramp with -1 <= d_lo < d_hi <= 1, a scalar product that is a norm: no
// negative Ql_ref[l], and not on the averaged vectors).
// NOT checked, deliberately: a scratch sized for fewer list entries than the list holds.  Neither pass is told the size of the scratch
// or the length of d_nlist (the entry points keep the argument lists of the plain ones), so it cannot be known here; the caller sizes the
// scratch with mtd_ql_local_scratch_doubles_opt(N, lmax, length of d_nlist, opt), as SteinhardtLocal::computeCV does at every step.
int qll_prepare(QllCall &k, unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head,
                const unsigned int *d_nneigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax, unsigned int type,
                const double *ql_ref, unsigned int n_global, const double *d_scratch, mtd_stream_t stream, const mtd_ql_local_options *opt,
                const mtd_ql_local_bonds *bonds)
    {
    if (!box || !ql_ref || !d_scratch || n_global == 0) return MTD_ERR_INVALID_ARGUMENT;
    if (n_particles && (!d_postype || !d_head || !d_nneigh)) return MTD_ERR_INVALID_ARGUMENT;
    if (dtype != MTD_F32 && dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    if (!(rcut > 0.0) || !(ron >= 0.0) || !(ron < rcut)) return MTD_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)d_scratch & 15u) != 0) return MTD_ERR_INVALID_ARGUMENT;       // table rows are read 16 bytes at a time
    if (lmax > 12) return MTD_ERR_UNSUPPORTED;
    if (opt && opt->switch_on && (!(opt->c0 > 0.0) || !std::isfinite(opt->c0) || opt->p == 0)) return MTD_ERR_INVALID_ARGUMENT;
    if (opt && opt->gate_on && (!(opt->n_lo >= 0.0) || !(opt->n_lo < opt->n_hi) || !std::isfinite(opt->n_hi))) return MTD_ERR_INVALID_ARGUMENT;
    QllRamp ramp = {0.0, 0.0};
    if (qll_bonds_on(bonds))
        {
        if (!(bonds->d_lo >= -1.0) || !(bonds->d_lo < bonds->d_hi) || !(bonds->d_hi <= 1.0)) return MTD_ERR_INVALID_ARGUMENT;
        for (unsigned int l = 0; l <= lmax; ++l)
            if (!(ql_ref[l] >= 0.0)) return MTD_ERR_INVALID_ARGUMENT;
        if (opt && opt->average) return MTD_ERR_UNSUPPORTED;
        ramp = {bonds->d_lo, 1.0 / (bonds->d_hi - bonds->d_lo)};
        }
    const int mode = qll_mode(opt, bonds);
    k = {n_particles, d_postype, dtype, box, d_head, d_nneigh, d_nlist, rcut, ron, lmax, type, ql_ref, n_global, (hipStream_t)stream, mode,
         qll_layout(lmax, ql_ref), qll_opt(opt), ramp, qll_scratch(const_cast<double *>(d_scratch), n_particles, lmax, 0, mode),
         row_blocks(n_particles, QLL_PPB, QLL_MAX_BLOCKS)};
    return MTD_SUCCESS;
    }

template<int LMAX> int qll_args(QlArgs<LMAX> &a, const QllCall &k)
    {
    return fill_args<LMAX>(a, k.N, k.box, k.rcut, k.ron, k.lmax, k.type, k.ql_ref, k.n_global, 0);
    }

// the cluster pass of a call: the mask of the largest cluster of the v_i just formed (cluster.hip), then k_qll_cluster_apply
struct QllCluster
    {
    const mtd_cluster_params *p;                           // NULL: off
    void *scratch;
    const double *w;
    const unsigned int *label, *summary;
    };

template<bool ROWS> int qll_cluster_pass(const QllCall &k, QllCluster &cl)
    {
    const int rc = mtd_cluster_largest(k.N, k.postype, k.dtype, k.box, k.head, k.nneigh, k.nlist, k.type, k.sc.v, cl.p, cl.scratch, &cl.label,
                                       nullptr, &cl.w, &cl.summary, (mtd_stream_t)k.s);
    if (rc) return rc;
    k_qll_cluster_apply<ROWS><<<k.blocks, QLL_THREADS, 0, k.s>>>(k.N, k.lay.row_doubles / 2, cl.w, k.sc.v, (double2 *)k.sc.rows, k.sc.beta, k.sc.a0,
                                                                  k.sc.partials);
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

template<typename S4, int LMAX> int qll_accumulate_impl(const QllCall &k, QllCluster &cl)
    {
    QlArgs<LMAX> a;
    int rc = qll_args(a, k);
    if (rc) return rc;
    QlArgs<12> a12;                                              // the gather passes need the box and the window only: one instantiation
    rc = qll_args(a12, k);
    if (rc) return rc;
    const double *tab = ql_device_table<LMAX>(k.s, rc);          // (the smoothing coefficients sit at the same place for every LMAX)
    if (rc) return rc;
    const QllScratch &sc = k.sc;
    const S4 *postype = (const S4 *)k.postype;
    const unsigned int rs16 = k.lay.row_doubles / 2;
    static_assert(QLL_PLAIN == 0 && QLL_TRANSFORM == 1 && QLL_AVERAGE == 2 && QLL_BONDS == 3, "the mode is dispatched as the count mode + 1 of 4");
    dispatch_count<4>(k.mode + 1, [&](auto m1)
        {
        constexpr int MODE = decltype(m1)::value - 1;
        k_qll_accumulate<S4, LMAX, MODE><<<k.blocks, QLL_THREADS, 0, k.s>>>(a, k.lay, k.opt, postype, k.head, k.nneigh, k.nlist, sc.n, sc.c, sc.v,
                                                                             MODE == QLL_AVERAGE || MODE == QLL_BONDS ? sc.qrows : sc.rows, sc.wtab,
                                                                             sc.partials, tab);
        });
    MTD_LAUNCH_CHECK();
    if (k.mode == QLL_BONDS)
        {
        k_qll_bonds<S4><<<k.blocks, QLL_THREADS, 0, k.s>>>(a12, k.opt, k.ramp, rs16, postype, k.head, k.nneigh, k.nlist, sc.n, (const double2 *)sc.qrows,
                                                            sc.wtab, sc.epair, sc.b, sc.v, sc.beta, sc.a0, sc.partials, tab);
        MTD_LAUNCH_CHECK();
        if (cl.p && (rc = qll_cluster_pass<false>(k, cl)) != 0) return rc;         // v_i, beta_i and a0_i of every particle are complete
        k_qll_bonds_backprop<S4><<<k.blocks, QLL_THREADS, 0, k.s>>>(a12, k.ramp, rs16, postype, k.head, k.nneigh, k.nlist, sc.n, sc.c, sc.beta, sc.a0,
                                                                     (const double2 *)sc.qrows, sc.wtab, (double2 *)sc.rows, sc.epair, tab);
        MTD_LAUNCH_CHECK();
        }
    if (k.mode == QLL_AVERAGE)
        {
        k_qll_average<S4><<<k.blocks, QLL_THREADS, 0, k.s>>>(a12, k.opt, rs16, postype, k.head, k.nneigh, k.nlist, sc.n, (const double2 *)sc.qrows,
                                                              sc.wtab, (double2 *)sc.brows, sc.c, sc.v, sc.a0, sc.partials, tab);
        MTD_LAUNCH_CHECK();
        k_qll_backprop<S4><<<k.blocks, QLL_THREADS, 0, k.s>>>(a12, rs16, postype, k.head, k.nneigh, k.nlist, sc.n, sc.a0, (const double2 *)sc.qrows,
                                                               (const double2 *)sc.brows, (double2 *)sc.rows, sc.epair, tab);
        MTD_LAUNCH_CHECK();
        }
    if (cl.p && (k.mode == QLL_PLAIN || k.mode == QLL_TRANSFORM)) return qll_cluster_pass<true>(k, cl);
    return MTD_SUCCESS;
    }

// the force pass: through LDS tiles while a table row fits one, else straight from memory
template<typename S4, int LMAX, bool AVG, bool VIR>
int qll_forces_impl(const QllCall &k, void *d_force, const double *d_bias, double bias_host, void *d_virial, unsigned int virial_pitch)
    {
    QlArgs<LMAX> a;
    int rc = qll_args(a, k);
    if (rc) return rc;
    const double *tab = ql_device_table<LMAX>(k.s, rc);
    if (rc) return rc;
    const S4 *postype = (const S4 *)k.postype;
    S4 *force = (S4 *)d_force;
    typename scalar4_traits<S4>::scalar *virial = VIR ? (typename scalar4_traits<S4>::scalar *)d_virial : nullptr;
    const double *epair = AVG ? k.sc.epair : nullptr;
    const unsigned int rs16 = k.lay.row_doubles / 2;
    if (rs16 <= QLL_TILE_MAX16)
        {
        const unsigned int ts = rs16 | 1u;                  // odd: rows of a tile start in different banks
        const size_t bytes = (size_t)QLL_TILE_ROWS * ts * sizeof(double2);
        MTD_HIP_TRY(hipFuncSetAttribute((const void *)k_qll_forces_tile<S4, LMAX, AVG, VIR>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)((size_t)QLL_TILE_ROWS * (QLL_TILE_MAX16 | 1u) * sizeof(double2))));
        k_qll_forces_tile<S4, LMAX, AVG, VIR><<<k.blocks, QLL_THREADS, bytes, k.s>>>(a, k.lay, postype, k.head, k.nneigh, k.nlist, k.sc.rows, force,
                                                                                     d_bias, bias_host, tab, ts, epair, virial, virial_pitch);
        }
    else
        k_qll_forces<S4, LMAX, AVG, VIR><<<k.blocks, QLL_THREADS, 0, k.s>>>(a, k.lay, postype, k.head, k.nneigh, k.nlist, k.sc.rows, force, d_bias,
                                                                            bias_host, tab, epair, virial, virial_pitch);
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // namespace

extern "C" {

size_t mtd_ql_local_scratch_doubles(unsigned int n_particles, unsigned int lmax)
    {
    return mtd_ql_local_scratch_doubles_opt(n_particles, lmax, 0, nullptr);
    }

size_t mtd_ql_local_scratch_doubles_opt(unsigned int n_particles, unsigned int lmax, size_t n_list_entries, const mtd_ql_local_options *opt)
    {
    return mtd_ql_local_scratch_doubles_bonds(n_particles, lmax, n_list_entries, opt, nullptr);
    }

size_t mtd_ql_local_scratch_doubles_bonds(unsigned int n_particles, unsigned int lmax, size_t n_list_entries, const mtd_ql_local_options *opt,
                                          const mtd_ql_local_bonds *bonds)
    {
    return qll_scratch(nullptr, n_particles, lmax, n_list_entries, qll_mode(opt, bonds)).total;
    }

int mtd_ql_local_accumulate(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                            const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax,
                            unsigned int type, const double *Ql_ref, unsigned int n_global, double *d_scratch, const double **d_partials,
                            unsigned int *n_partials, const double **d_c, const double **d_n, mtd_stream_t stream)
    {
    return mtd_ql_local_accumulate_opt(n_particles, d_postype, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref, n_global,
                                       d_scratch, d_partials, n_partials, d_c, d_n, stream, nullptr, nullptr);
    }

int mtd_ql_local_accumulate_opt(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                                const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax,
                                unsigned int type, const double *Ql_ref, unsigned int n_global, double *d_scratch, const double **d_partials,
                                unsigned int *n_partials, const double **d_c, const double **d_n, mtd_stream_t stream,
                                const mtd_ql_local_options *opt, const double **d_v)
    {
    return mtd_ql_local_accumulate_bonds(n_particles, d_postype, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref, n_global,
                                         d_scratch, d_partials, n_partials, d_c, d_n, stream, opt, d_v, nullptr, nullptr);
    }

int mtd_ql_local_accumulate_bonds(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                                  const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax,
                                  unsigned int type, const double *Ql_ref, unsigned int n_global, double *d_scratch, const double **d_partials,
                                  unsigned int *n_partials, const double **d_c, const double **d_n, mtd_stream_t stream,
                                  const mtd_ql_local_options *opt, const double **d_v, const mtd_ql_local_bonds *bonds, const double **d_b)
    {
    return mtd_ql_local_accumulate_cluster(n_particles, d_postype, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref,
                                           n_global, d_scratch, d_partials, n_partials, d_c, d_n, stream, opt, d_v, bonds, d_b, nullptr, nullptr,
                                           nullptr, nullptr, nullptr);
    }

int mtd_ql_local_accumulate_cluster(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box,
                                    const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut,
                                    double ron, unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global,
                                    double *d_scratch, const double **d_partials, unsigned int *n_partials, const double **d_c,
                                    const double **d_n, mtd_stream_t stream, const mtd_ql_local_options *opt, const double **d_v,
                                    const mtd_ql_local_bonds *bonds, const double **d_b, const mtd_cluster_params *cluster,
                                    void *d_cluster_scratch, const double **d_w, const unsigned int **d_label,
                                    const unsigned int **d_summary)
    {
    if (!d_partials || !n_partials) return MTD_ERR_INVALID_ARGUMENT;
    QllCall k;
    int rc = qll_prepare(k, n_particles, d_postype, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref, n_global, d_scratch,
                         stream, opt, bonds);
    if (rc) return rc;
    QllCluster cl = {nullptr, d_cluster_scratch, nullptr, nullptr, nullptr};
    if (cluster_on(cluster))
        {
        // what mtd_cluster_largest would refuse, refused here: before the first launch of this call
        if ((rc = cluster_refuse(cluster)) != 0) return rc;
        if (!d_cluster_scratch || ((uintptr_t)d_cluster_scratch & 15u) != 0 || (n_particles && !d_nlist)) return MTD_ERR_INVALID_ARGUMENT;
        if (k.mode == QLL_AVERAGE) return MTD_ERR_UNSUPPORTED;
        cl.p = cluster;
        }
    rc = dispatch_lmax(lmax, [&](auto lm)
        {
        return dispatch_s4(dtype, [&](auto t) { return qll_accumulate_impl<typename decltype(t)::type, decltype(lm)::value>(k, cl); });
        });
    if (rc) return rc;
    if (d_w) *d_w = cl.w;
    if (d_label) *d_label = cl.label;
    if (d_summary) *d_summary = cl.summary;
    *d_partials = k.sc.partials;
    *n_partials = k.blocks;
    if (d_c) *d_c = k.sc.c;
    if (d_n) *d_n = k.sc.n;
    if (d_v) *d_v = k.sc.v;
    if (d_b) *d_b = k.mode == QLL_BONDS ? k.sc.b : nullptr;
    return MTD_SUCCESS;
    }

int mtd_ql_local_forces(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                        const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                        unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                        const double *d_bias, double bias_host, mtd_stream_t stream)
    {
    return mtd_ql_local_forces_opt(n_particles, d_postype, d_force, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref, n_global,
                                   d_scratch, d_bias, bias_host, stream, nullptr);
    }

int mtd_ql_local_forces_opt(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                            const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                            unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                            const double *d_bias, double bias_host, mtd_stream_t stream, const mtd_ql_local_options *opt)
    {
    return mtd_ql_local_forces_virial(n_particles, d_postype, d_force, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref,
                                      n_global, d_scratch, d_bias, bias_host, stream, opt, nullptr, 0);
    }

int mtd_ql_local_forces_virial(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                               const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                               unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                               const double *d_bias, double bias_host, mtd_stream_t stream, const mtd_ql_local_options *opt, void *d_virial,
                               unsigned int virial_pitch)
    {
    return mtd_ql_local_forces_bonds(n_particles, d_postype, d_force, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref,
                                     n_global, d_scratch, d_bias, bias_host, stream, opt, d_virial, virial_pitch, nullptr);
    }

int mtd_ql_local_forces_bonds(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                              const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                              unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                              const double *d_bias, double bias_host, mtd_stream_t stream, const mtd_ql_local_options *opt, void *d_virial,
                              unsigned int virial_pitch, const mtd_ql_local_bonds *bonds)
    {
    QllCall k;
    const int rc = qll_prepare(k, n_particles, d_postype, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref, n_global,
                               d_scratch, stream, opt, bonds);
    if (rc) return rc;
    if (n_particles && !d_force) return MTD_ERR_INVALID_ARGUMENT;
    if (d_virial && virial_pitch < n_particles) return MTD_ERR_INVALID_ARGUMENT;
    if (n_particles == 0) return MTD_SUCCESS;
    return dispatch_lmax(lmax, [&](auto lm)
        {
        return dispatch_s4(dtype, [&](auto t)
            {
            return dispatch_bool(k.mode == QLL_AVERAGE || k.mode == QLL_BONDS, [&](auto avg)
                {
                return dispatch_bool(d_virial != nullptr, [&](auto vir)
                    {
                    return qll_forces_impl<typename decltype(t)::type, decltype(lm)::value, decltype(avg)::value, decltype(vir)::value>(
                        k, d_force, d_bias, bias_host, d_virial, virial_pitch);
                    });
                });
            });
        });
    }

} // extern "C"
