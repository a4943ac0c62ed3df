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
// duplicate and indexes no ghost particle (entries j >= N and self entries are skipped).  Known limits: a pair exactly on the z axis
// gives NaN in the force, as in mtd_ql_forces; c_i jumps from 0 to the one-neighbour value when a first neighbour enters an empty
// shell (inherent in the normalised definition; irrelevant at liquid or solid density).
//
// MI355X design.  Two launches per step, both walk chunks of 64 consecutive central particles per block and round:
//   lanes            FOUR lanes (a quad) per central particle; lane q takes entries q, q + 4, ... of the particle's row, so the
//                    per-particle sums stay in registers: no LDS atomics.  The quad's sums are added with two DPP quad_perm moves
//                    ((q0 + q1) + (q2 + q3), the same bits in all four lanes)
//   memory trips     list entry two iterations ahead, neighbour position one iteration ahead of the arithmetic
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
// Double precision throughout.
#include "mtd_device.hpp"
#include "steinhardt_device.hpp"

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

template<typename S4> __device__ __forceinline__ S4 qll_zero();
template<> __device__ __forceinline__ float4 qll_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template<> __device__ __forceinline__ double4 qll_zero<double4>() { return make_double4(0.0, 0.0, 0.0, 0.0); }

__device__ __forceinline__ double quad_sum(double v)
    {
    v += dpp_move<MTD_DPP_QUAD_XOR1>(v);
    v += dpp_move<MTD_DPP_QUAD_XOR2>(v);
    return v;
    }

// ---- pass 1: n_i, A_lm(i) -> c_i, table row, block sums of c_i ------------------------------------------------------------
template<typename S4, int LMAX>
__global__ __launch_bounds__(QLL_THREADS) void k_qll_accumulate(const QlArgs<LMAX> a, const QllLayout lay, const S4 *__restrict__ postype,
                                                                const unsigned int *__restrict__ head_list,
                                                                const unsigned int *__restrict__ n_neigh,
                                                                const unsigned int *__restrict__ nlist, double *__restrict__ n_out,
                                                                double *__restrict__ c_out, double *__restrict__ rows,
                                                                double *__restrict__ partials, const double *__restrict__ tab)
    {
    typedef QlTab<LMAX> T;
    __shared__ double s_c[QLL_PPB];
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    double block_c = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const unsigned int i = chunk * QLL_PPB + p;
        Particle pi = {0.0, 0.0, 0.0, -1};
        unsigned int start = 0, cnt = 0;
        if (i < a.N)
            {
            pi = scalar4_traits<S4>::load(postype, i);
            if ((unsigned int)pi.type == a.type)
                {
                start = head_list[i];
                cnt = n_neigh[i];
                }
            }
        cplx S[LMAX + 1][LMAX + 1];                                                // [m][l], l >= m
#pragma unroll
        for (int m = 0; m <= LMAX; ++m)
#pragma unroll
            for (int l = 0; l <= LMAX; ++l) S[m][l] = {0.0, 0.0};
        double nsum = 0.0;
        unsigned int e = q;
        unsigned int j0 = e < cnt ? nlist[start + e] : QLL_NONE;
        unsigned int j1 = e + QLL_G < cnt ? nlist[start + e + QLL_G] : QLL_NONE;
        S4 pos0 = qll_zero<S4>();
        if (j0 < a.N) pos0 = postype[j0];
#pragma unroll 1
        for (; e < cnt; e += QLL_G)
            {
            unsigned int tab_shift = 0;
            asm volatile("" : "+s"(tab_shift));                 // a zero the compiler cannot see through: the table loads stay in the loop
            const double *__restrict__ tab_k = tab + tab_shift;
            const unsigned int j2 = e + 2 * QLL_G < cnt ? nlist[start + e + 2 * QLL_G] : QLL_NONE;
            S4 pos1 = qll_zero<S4>();
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
        nsum = quad_sum(nsum);
        const double inv_n = nsum > 0.0 ? 1.0 / nsum : 0.0;
        const double inv_n2 = inv_n * inv_n;
        const bool write = q == 0 && i < a.N;
        double *__restrict__ row = rows + (size_t)(i < a.N ? i : 0) * lay.row_doubles;
        double c = 0.0, r00 = 0.0;
#pragma unroll
        for (int l = 0; l <= LMAX; ++l)
            {
#pragma unroll
            for (int m = 0; m <= l; ++m)
                {
                S[m][l].re = quad_sum(S[m][l].re);
                if (m > 0) S[m][l].im = quad_sum(S[m][l].im);
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
        // the chunk's sum of c_i: wave 0, fixed order
        __syncthreads();
        if (q == 0) s_c[p] = i < a.N ? c : 0.0;
        __syncthreads();
        if (tid < MTD_WAVE) block_c += wave_sum(s_c[tid]);
        }
    if (tid == 0) partials[blockIdx.x] = block_c;
    }

// ---- pass 2: forces, gathered --------------------------------------------------------------------------------------------
struct QllPairWeights
    {
    const double *__restrict__ rk;
    const double *__restrict__ rj;
    const QllLayout &lay;
    __device__ __forceinline__ cplx operator()(const int l, const int m, const int) const
        {
        const unsigned int s = 2 * (lay.off[l] + m);
        const double2 wk = *reinterpret_cast<const double2 *>(rk + s), wj = *reinterpret_cast<const double2 *>(rj + s);
        if (l & 1) return {wk.x - wj.x, wk.y - wj.y};
        return {wk.x + wj.x, wk.y + wj.y};
        }
    };

template<int LMAX> constexpr int qll_force_waves() { return LMAX <= 4 ? 3 : (LMAX <= 6 ? 2 : 1); }

template<typename S4, int LMAX>
__global__ __launch_bounds__(QLL_THREADS, (qll_force_waves<LMAX>())) void k_qll_forces(const QlArgs<LMAX> a, const QllLayout lay, const S4 *__restrict__ postype,
                                                            const unsigned int *__restrict__ head_list,
                                                            const unsigned int *__restrict__ n_neigh,
                                                            const unsigned int *__restrict__ nlist, const double *__restrict__ rows,
                                                            S4 *__restrict__ force, const double *__restrict__ d_bias, const double bias_host,
                                                            const double *__restrict__ tab)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    const unsigned int tid = threadIdx.x, p = tid / QLL_G, q = tid % QLL_G;
    const unsigned int n_chunks = (a.N + QLL_PPB - 1) / QLL_PPB;
    const double scale = (d_bias ? *d_bias : bias_host) / (double)a.n_global;
    const unsigned int act = __builtin_amdgcn_readfirstlane(lay.act | 1u);         // slot (0, 0) carries the -2 (c_k/n_k + c_j/n_j) grad f term
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const unsigned int k = chunk * QLL_PPB + p;
        Particle pk = {0.0, 0.0, 0.0, -1};
        unsigned int start = 0, cnt = 0;
        if (k < a.N)
            {
            pk = scalar4_traits<S4>::load(postype, k);
            if ((unsigned int)pk.type == a.type)
                {
                start = head_list[k];
                cnt = n_neigh[k];
                }
            }
        const double *__restrict__ rk = rows + (size_t)(k < a.N ? k : 0) * lay.row_doubles;
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        unsigned int e = q;
        unsigned int j0 = e < cnt ? nlist[start + e] : QLL_NONE;
        unsigned int j1 = e + QLL_G < cnt ? nlist[start + e + QLL_G] : QLL_NONE;
        S4 pos0 = qll_zero<S4>();
        if (j0 < a.N) pos0 = postype[j0];
#pragma unroll 1
        for (; e < cnt; e += QLL_G)
            {
            unsigned int tab_shift = 0;
            asm volatile("" : "+s"(tab_shift));                 // a zero the compiler cannot see through: the table loads stay in the loop
            const double *__restrict__ tab_k = tab + tab_shift;
            const unsigned int j2 = e + 2 * QLL_G < cnt ? nlist[start + e + 2 * QLL_G] : QLL_NONE;
            S4 pos1 = qll_zero<S4>();
            if (j1 < a.N) pos1 = postype[j1];
            if (j0 < a.N && j0 != k)
                {
                const Particle pj = scalar4_traits<S4>::unpack(pos0);
                double dx = pk.x - pj.x, dy = pk.y - pj.y, dz = pk.z - pj.z;
                min_image(a, dx, dy, dz);
                const double rsq = dx * dx + dy * dy + dz * dz;
                if ((unsigned int)pj.type == a.type && rsq <= a.rcutsq)
                    {
                    double fpx, fpy, fpz;
                    ql_pair_force<LMAX>(a, tab_k, QllPairWeights{rk, rows + (size_t)j0 * lay.row_doubles, lay}, act, dx, dy, dz, rsq, fpx, fpy, fpz);
                    Fx += fpx;
                    Fy += fpy;
                    Fz += fpz;
                    }
                }
            j0 = j1;
            j1 = j2;
            pos0 = pos1;
            }
        Fx = quad_sum(Fx);
        Fy = quad_sum(Fy);
        Fz = quad_sum(Fz);
        if (q == 0 && k < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + k);
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

struct QllTileWeights
    {
    const double2 *tk;                                     // LDS: the row of this lane's particle
    const double2 *tj;                                     // LDS: the row of this lane's neighbour
    const QllLayout &lay;
    __device__ __forceinline__ cplx operator()(const int l, const int m, const int) const
        {
        const unsigned int s = lay.off[l] + m;
        const double2 wk = tk[s], wj = tj[s];
        if (l & 1) return {wk.x - wj.x, wk.y - wj.y};
        return {wk.x + wj.x, wk.y + wj.y};
        }
    };

template<typename S4, int LMAX>
__global__ __launch_bounds__(QLL_THREADS, (qll_force_waves<LMAX>())) void k_qll_forces_tile(const QlArgs<LMAX> a, const QllLayout lay, const S4 *__restrict__ postype,
                                                            const unsigned int *__restrict__ head_list,
                                                            const unsigned int *__restrict__ n_neigh,
                                                            const unsigned int *__restrict__ nlist, const double *__restrict__ rows,
                                                            S4 *__restrict__ force, const double *__restrict__ d_bias, const double bias_host,
                                                            const double *__restrict__ tab, const unsigned int ts /* tile row stride, 16-byte units */)
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
        const unsigned int k = chunk * QLL_PPB + p;
        Particle pk = {0.0, 0.0, 0.0, -1};
        unsigned int start = 0, cnt = 0;
        if (k < a.N)
            {
            pk = scalar4_traits<S4>::load(postype, k);
            if ((unsigned int)pk.type == a.type)
                {
                start = head_list[k];
                cnt = n_neigh[k];
                }
            }
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
        unsigned int e = q;
        unsigned int j0 = e < cnt ? nlist[start + e] : QLL_NONE;
        unsigned int j1 = e + QLL_G < cnt ? nlist[start + e + QLL_G] : QLL_NONE;
        S4 pos0 = qll_zero<S4>();
        if (j0 < a.N) pos0 = postype[j0];
#pragma unroll 1
        while (__ballot(e < cnt) != 0ull)
            {
            unsigned int tab_shift = 0;
            asm volatile("" : "+s"(tab_shift));                 // a zero the compiler cannot see through: the table loads stay in the loop
            const double *__restrict__ tab_k = tab + tab_shift;
            const unsigned int j2 = e + 2 * QLL_G < cnt ? nlist[start + e + 2 * QLL_G] : QLL_NONE;
            S4 pos1 = qll_zero<S4>();
            if (j1 < a.N) pos1 = postype[j1];
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
                    ql_pair_force<LMAX>(a, tab_k, QllTileWeights{tile_k + (lane / QLL_G) * ts, tile_j + lane * ts, lay}, act, dx, dy, dz, rsq, fpx, fpy, fpz);
                    Fx += fpx;
                    Fy += fpy;
                    Fz += fpz;
                    }
                qll_wave_sync();                            // the tile is free for the next iteration
                }
            j0 = j1;
            j1 = j2;
            pos0 = pos1;
            e += QLL_G;
            }
        Fx = quad_sum(Fx);
        Fy = quad_sum(Fy);
        Fz = quad_sum(Fz);
        if (q == 0 && k < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + k);
        }
    }

template<typename S4, int LMAX>
int qll_launch_forces(const QlArgs<LMAX> &a, const QllLayout &lay, const unsigned int blocks, const S4 *postype, const unsigned int *d_head,
                      const unsigned int *d_nneigh, const unsigned int *d_nlist, const double *rows, S4 *force, const double *d_bias,
                      const double bias_host, const double *tab, hipStream_t s)
    {
    const unsigned int rs16 = lay.row_doubles / 2;
    if (rs16 <= QLL_TILE_MAX16)
        {
        const unsigned int ts = rs16 | 1u;                  // odd: rows of a tile start in different banks
        const size_t bytes = (size_t)QLL_TILE_ROWS * ts * sizeof(double2);
        MTD_HIP_TRY(hipFuncSetAttribute((const void *)k_qll_forces_tile<S4, LMAX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)((size_t)QLL_TILE_ROWS * (QLL_TILE_MAX16 | 1u) * sizeof(double2))));
        k_qll_forces_tile<S4, LMAX><<<blocks, QLL_THREADS, bytes, s>>>(a, lay, postype, d_head, d_nneigh, d_nlist, rows, force, d_bias, bias_host, tab, ts);
        }
    else
        k_qll_forces<S4, LMAX><<<blocks, QLL_THREADS, 0, s>>>(a, lay, postype, d_head, d_nneigh, d_nlist, rows, force, d_bias, bias_host, tab);
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
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

// scratch: block sums [QLL_MAX_BLOCKS] | n_i [N] | c_i [N] (+ one double when N is odd) | rows [N][<= (lmax + 1)(lmax + 2)]
struct QllScratch
    {
    double *partials, *n, *c, *rows;
    };

QllScratch qll_scratch(double *scratch, const unsigned int N)
    {
    QllScratch s;
    s.partials = scratch;
    s.n = scratch + QLL_MAX_BLOCKS;
    s.c = s.n + N;
    s.rows = s.c + N + (N & 1u);
    return s;
    }

unsigned int qll_blocks(const unsigned int N)
    {
    unsigned int b = (N + QLL_PPB - 1) / QLL_PPB;
    if (b < 1) b = 1;
    return b > QLL_MAX_BLOCKS ? QLL_MAX_BLOCKS : b;
    }

template<int LMAX>
int qll_accumulate_impl(unsigned int N, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head, const unsigned int *d_nneigh,
                        const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax, unsigned int type, const double *ql_ref,
                        unsigned int n_global, const QllScratch &sc, unsigned int *n_partials, hipStream_t s)
    {
    QlArgs<LMAX> a;
    int rc = fill_args<LMAX>(a, N, box, rcut, ron, lmax, type, ql_ref, n_global, 0);
    if (rc) return rc;
    const double *tab = ql_device_table<LMAX>(s, rc);
    if (rc) return rc;
    const QllLayout lay = qll_layout(lmax, ql_ref);
    const unsigned int blocks = qll_blocks(N);
    if (dtype == MTD_F32)
        k_qll_accumulate<float4, LMAX><<<blocks, QLL_THREADS, 0, s>>>(a, lay, (const float4 *)d_postype, d_head, d_nneigh, d_nlist, sc.n, sc.c, sc.rows,
                                                                        sc.partials, tab);
    else
        k_qll_accumulate<double4, LMAX><<<blocks, QLL_THREADS, 0, s>>>(a, lay, (const double4 *)d_postype, d_head, d_nneigh, d_nlist, sc.n, sc.c, sc.rows,
                                                                         sc.partials, tab);
    MTD_LAUNCH_CHECK();
    *n_partials = blocks;
    return MTD_SUCCESS;
    }

template<int LMAX>
int qll_forces_impl(unsigned int N, const void *d_postype, void *d_force, int dtype, const mtd_box *box, const unsigned int *d_head,
                    const unsigned int *d_nneigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax, unsigned int type,
                    const double *ql_ref, unsigned int n_global, const QllScratch &sc, const double *d_bias, double bias_host, hipStream_t s)
    {
    QlArgs<LMAX> a;
    int rc = fill_args<LMAX>(a, N, box, rcut, ron, lmax, type, ql_ref, n_global, 0);
    if (rc) return rc;
    const double *tab = ql_device_table<LMAX>(s, rc);
    if (rc) return rc;
    const QllLayout lay = qll_layout(lmax, ql_ref);
    const unsigned int blocks = qll_blocks(N);
    if (dtype == MTD_F32)
        return qll_launch_forces<float4, LMAX>(a, lay, blocks, (const float4 *)d_postype, d_head, d_nneigh, d_nlist, sc.rows, (float4 *)d_force, d_bias,
                                               bias_host, tab, s);
    return qll_launch_forces<double4, LMAX>(a, lay, blocks, (const double4 *)d_postype, d_head, d_nneigh, d_nlist, sc.rows, (double4 *)d_force, d_bias,
                                            bias_host, tab, s);
    }

// what both entry points refuse before a device is touched
int qll_validate(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head,
                 const unsigned int *d_nneigh, double rcut, double ron, unsigned int lmax, const double *ql_ref, unsigned int n_global,
                 const double *d_scratch)
    {
    if (!box || !ql_ref || !d_scratch || n_global == 0) return MTD_ERR_INVALID_ARGUMENT;
    if (n_particles && (!d_postype || !d_head || !d_nneigh)) return MTD_ERR_INVALID_ARGUMENT;
    if (dtype != MTD_F32 && dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    if (!(rcut > 0.0) || !(ron >= 0.0) || !(ron < rcut)) return MTD_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)d_scratch & 15u) != 0) return MTD_ERR_INVALID_ARGUMENT;       // table rows are read 16 bytes at a time
    if (lmax > 12) return MTD_ERR_UNSUPPORTED;
    return MTD_SUCCESS;
    }

} // namespace

extern "C" {

size_t mtd_ql_local_scratch_doubles(unsigned int n_particles, unsigned int lmax)
    {
    const size_t n = n_particles;
    return (size_t)QLL_MAX_BLOCKS + 2 * n + (n & 1u) + n * (size_t)(lmax + 1) * (lmax + 2);
    }

int mtd_ql_local_accumulate(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                            const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax,
                            unsigned int type, const double *Ql_ref, unsigned int n_global, double *d_scratch, const double **d_partials,
                            unsigned int *n_partials, const double **d_c, const double **d_n, mtd_stream_t stream)
    {
    if (!d_partials || !n_partials) return MTD_ERR_INVALID_ARGUMENT;
    int rc = qll_validate(n_particles, d_postype, dtype, box, d_head_list, d_n_neigh, rcut, ron, lmax, Ql_ref, n_global, d_scratch);
    if (rc) return rc;
    const QllScratch sc = qll_scratch(d_scratch, n_particles);
    hipStream_t s = (hipStream_t)stream;
    unsigned int n = 0;
#define MTD_QLL_ACC(LM) qll_accumulate_impl<LM>(n_particles, d_postype, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref, \
                                                n_global, sc, &n, s)
    if (lmax <= 4)
        rc = MTD_QLL_ACC(4);
    else if (lmax <= 6)
        rc = MTD_QLL_ACC(6);
    else if (lmax <= 8)
        rc = MTD_QLL_ACC(8);
    else
        rc = MTD_QLL_ACC(12);
#undef MTD_QLL_ACC
    if (rc) return rc;
    *d_partials = sc.partials;
    *n_partials = n;
    if (d_c) *d_c = sc.c;
    if (d_n) *d_n = sc.n;
    return MTD_SUCCESS;
    }

int mtd_ql_local_forces(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                        const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                        unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                        const double *d_bias, double bias_host, mtd_stream_t stream)
    {
    int rc = qll_validate(n_particles, d_postype, dtype, box, d_head_list, d_n_neigh, rcut, ron, lmax, Ql_ref, n_global, d_scratch);
    if (rc) return rc;
    if (n_particles && !d_force) return MTD_ERR_INVALID_ARGUMENT;
    if (n_particles == 0) return MTD_SUCCESS;
    const QllScratch sc = qll_scratch(const_cast<double *>(d_scratch), n_particles);
    hipStream_t s = (hipStream_t)stream;
#define MTD_QLL_F(LM) qll_forces_impl<LM>(n_particles, d_postype, d_force, dtype, box, d_head_list, d_n_neigh, d_nlist, rcut, ron, lmax, type, Ql_ref, \
                                          n_global, sc, d_bias, bias_host, s)
    if (lmax <= 4) return MTD_QLL_F(4);
    if (lmax <= 6) return MTD_QLL_F(6);
    if (lmax <= 8) return MTD_QLL_F(8);
    return MTD_QLL_F(12);
#undef MTD_QLL_F
    }

} // extern "C"
