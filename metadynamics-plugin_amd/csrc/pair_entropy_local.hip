// pair_entropy_local.hip — per-particle pair entropy s_i from the particle's own smoothed g_i(r) (cv.pair_entropy_local) on gfx950.
//
// No reference counterpart (Piaggi and Parrinello, J. Chem. Phys. 147, 114112; PLUMED's PAIRENTROPIES).  Definition, gradient and virial:
// include/mtd_abi.h "Local pair entropy"; restated in fp64 numpy in tests/pair_entropy_local_ref.py.  In short, over the entries (i, j)
// of a FULL list with both particles of `type`, j != i, j a central particle and r = |minImage(r_i - r_j)| <= r_cut = r_max + 4 sigma:
//     H_ib = sum_j f(r) K(r_b - r)   b in the window of pair_entropy.hip,   g_ib = H_ib / (4 pi rho r_b^2),   rho = N_t / V
//     s_i = -2 pi rho Delta sum_b r_b^2 (g ln g - g + 1)  (g < 1e-10: the bin counts as 1),   W_ib = ds_i/dH_ib = -Delta ln g_ib / 2
//     sbar_i = (s_i + sum_j f_a s_j) / (1 + n_i),  n_i = sum_j f_a     v_i = h(-sbar_i)      CV = sum_i v_i / N_global
//     gamma_i = dv_i/dsbar_i,  gn_i = gamma_i / (1 + n_i),  alpha_j = gn_j + sum_{i in row j} f_a gn_i
//     t_ij = alpha_i u_ij(W_i) + gn_i f_a'(r) (s_j - sbar_i),   N dCV/dr_k = sum_{j in row k} (t_kj + t_jk) d_kj / r
// Smoothing, minimum image, particle loads and the type test are those of the Steinhardt units; the walk, the group's sum and the store
// of the virial are those of row_walk.hpp (the walk WITHOUT ghosts: every per-particle array here ends at N, an entry j >= N is
// skipped); bin constants and the window recurrence are those of pair_entropy_device.hpp; launches go through dispatch.hpp.
//
// MI355X design.  Three launches per step, five with an average, all in fp64 arithmetic over fp32 or fp64 arrays:
//   lanes             EIGHT lanes per central particle, 32 central particles per block and round, as in pair_entropy.hip
//   k_pel_count       N_t: block counts of the particles of the type (exact in doubles); every block of the next launch adds them up
//                     itself, so N_t never visits the host and costs no launch of its own for the sum
//   k_pel_accumulate  f K into a per-PARTICLE LDS image of 64-bit fixed-point integers, 32 x B x 8 bytes per block (ds_add_u64: the
//                     eight lanes' adds commute).  The scale is a power of two chosen per central particle from ITS row length E:
//                     2^x > E K(0), scale 2^(62 - x).  The group then turns its image into g, s_i, X_i (the explicit volume derivative)
//                     and the row W_i[0 .. B) of the table (N x B doubles in the scratch, a particle's row contiguous).  Without an
//                     average sbar_i, v_i, gamma_i and alpha_i are per-particle work of the same lanes, and the block sums of v_i leave
//                     here in the fixed order of block_sum
//   k_pel_average     (average only) a gather over the window a_on .. a_cut: n_i, sbar_i, v_i, gn_i; the block sums of v_i
//   k_pel_adjoint     (average only; first launch of mtd_pel_forces) the same gather over gn: alpha_i
//   k_pel_forces      the gather over row k.  The centre's W_k sits in LDS (32 x (B + 2) doubles, a zero at either end of a row, where
//                     a bin off the table is read); the neighbour's 2w + 1 bins are read from the table.  Per bin ONE combined weight
//                     alpha_k W_kb + alpha_j W_jb, so both directions of the pair cost one pair of sums: A = sum wc K and
//                     X = sum wc K (r_b - r), r_b - r formed from the bin index (one conversion and one FMA: the image stays at 8
//                     bytes per bin and the block within 64 KB of LDS without pairs (W, W r_b)).  Fixed summation order, no atomics;
//                     VIR = false is the kernel without the virial sums, AVG = false the one without the window term
// n_bins <= 128: image and centre rows of 32 particles stay at 32 KB / 33 KB per block.
// Worst-case rounding of the accumulation: one add errs by at most half a unit, 2^(x - 63) <= E K(0) 2^-62, a bin takes at most E adds:
// |dH_ib| <= E^2 K(0) 2^-62 (E = 100, K(0) = 8: 1.7e-14 absolute).  Into s_i that enters as Delta / 2 sum_b |ln g_ib| dH_ib, below 1e-12
// at B = 128; into W_ib as dH / H: a bin at the threshold g_min has H ~ 1e-9, so its W is good to ~2e-5 relative — and such a bin lies
// > 6 sigma from every entry of the particle, where K < 1e-8 K(0): below 1e-12 of the force.  Two identical calls give identical bits.
#include "mtd_device.hpp"
#include "row_walk.hpp"
#include "pair_entropy_device.hpp"
#include "dispatch.hpp"

#include <cmath>
#include <cstring>

namespace
{

using namespace mtd;

constexpr int PEL_THREADS = 256;
constexpr int PEL_G = 8;                                   // lanes per central particle
constexpr int PEL_PPB = PEL_THREADS / PEL_G;               // central particles per block and round
constexpr unsigned int PEL_MAX_BLOCKS = ROW_MAX_BLOCKS;    // columns of block sums in the scratch
constexpr double PEL_G_MIN = 1e-10;

// the scratch, in doubles, with n = n_particles rounded up to even:
//     block counts of N_t [1024] | block sums of v_i [1024] | s [n] | sbar [n] | v [n] | gn [n] | alpha [n] | X [n] | W [n_particles][B]
constexpr size_t PEL_OFF_CNT = 0, PEL_OFF_PART = PEL_MAX_BLOCKS, PEL_OFF_ARR = 2 * (size_t)PEL_MAX_BLOCKS;
constexpr int PEL_N_ARR = 6;

struct PelOpt
    {
    double volume;
    double inv_c0;
    unsigned int p;
    int switch_on;
    };

struct PelArrays
    {
    double *s, *sbar, *v, *gn, *alpha, *X, *W;
    };

__host__ __device__ inline PelArrays pel_arrays(double *scratch, const unsigned int N)
    {
    const size_t n = row_pitch(N);
    double *a = scratch + PEL_OFF_ARR;
    return {a, a + n, a + 2 * n, a + 3 * n, a + 4 * n, a + 5 * n, a + PEL_N_ARR * n};
    }

// x^n for a wave-uniform n (binary powering)
__device__ __forceinline__ double pel_powi(double x, unsigned int n)
    {
    double r = 1.0;
    for (; n; n >>= 1)
        {
        if (n & 1u) r *= x;
        x *= x;
        }
    return r;
    }

// v = h(-sbar) and gamma = dv/dsbar = -h'(-sbar); without a switch v = sbar and gamma = 1
__device__ __forceinline__ void pel_switch(const PelOpt &o, const double sbar, double &v, double &gamma)
    {
    v = sbar;
    gamma = 1.0;
    if (o.switch_on)
        {
        const double cv = -sbar;
        const double x = fmax(cv, 0.0) * o.inv_c0, xpm1 = pel_powi(x, o.p - 1), xp = xpm1 * x, den = 1.0 / (1.0 + xp);
        const bool big = !(xp < INFINITY);                 // x^p beyond the range of a double: h -> 1, h' -> 0
        v = big ? 1.0 : xp * den;
        gamma = (big || !(cv >= 0.0)) ? 0.0 : -((double)o.p * xpm1 * o.inv_c0 * den * den);
        }
    }

// ---- N_t: the block's count of particles of the type ----------------------------------------------------------------------------
template<typename S4>
__global__ __launch_bounds__(PEL_THREADS) void k_pel_count(const unsigned int N, const unsigned int type, const S4 *__restrict__ postype,
                                                           double *__restrict__ cnt)
    {
    __shared__ double s_red[16];
    double v = 0.0;
    for (unsigned int i = blockIdx.x * PEL_THREADS + threadIdx.x; i < N; i += gridDim.x * PEL_THREADS)
        v += (unsigned int)scalar4_traits<S4>::load(postype, i).type == type ? 1.0 : 0.0;
    v = block_sum(v, s_red);
    if (threadIdx.x == 0) cnt[blockIdx.x] = v;
    }

// N_t from the block counts: integers in doubles, exact in any order
__device__ __forceinline__ double pel_n_t(const double *__restrict__ cnt, const unsigned int n_cnt, double *s_red)
    {
    double v = 0.0;
    for (unsigned int k = threadIdx.x; k < n_cnt; k += PEL_THREADS) v += cnt[k];
    return block_sum(v, s_red);
    }

// ---- pass 1: H_ib, then s_i, X_i and the row W_i; without an average everything per particle ----------------------------------------
template<typename S4, bool AVG>
__global__ __launch_bounds__(PEL_THREADS) void k_pel_accumulate(const QlArgs<4> a_in, const PeArgs p_in, const PelOpt o, const S4 *__restrict__ postype,
                                                                const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                                const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                                const unsigned int n_cnt, double *__restrict__ scratch)
    {
    extern __shared__ unsigned long long s_img[];          // [PEL_PPB][B]
    __shared__ double s_red[16];
    const QlArgs<4> a = in_vgpr(a_in);
    const PeArgs p = pe_in_vgpr(p_in);
    const unsigned int tid = threadIdx.x, g = tid / PEL_G, q = tid % PEL_G;
    const unsigned int n_chunks = (a.N + PEL_PPB - 1) / PEL_PPB;
    const PelArrays out = pel_arrays(scratch, a.N);
    const double n_t = pel_n_t(scratch + PEL_OFF_CNT, n_cnt, s_red);
    const double rho = n_t / o.volume;
    const double c2 = 2.0 * M_PI * rho * p.delta;
    unsigned long long *img = s_img + (size_t)g * p.B;
    double v_sum = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * PEL_PPB + g);
        for (unsigned int b = q; b < p.B; b += PEL_G) img[b] = 0ull;
        lds_barrier();
        int ex;
        (void)frexp(fmax((double)c.cnt, 1.0) * p.k0, &ex);     // E K(0) < 2^ex
        const double scale = ldexp(1.0, 62 - ex), inv_scale = ldexp(1.0, ex - 62);
        row_walk_entries<PEL_G, true, false>(a, postype, nlist, tab, c, q, [&](const double *tab_k, const unsigned int, const double, const double, const double, const double rsq)
            {
            const double inv_r = rsqrt(rsq);
            double f, fprime_divr;
            smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
            const double fs = f * scale;
            pe_window(p, rsq * inv_r, [&](const int b, const double k)
                {
                if ((unsigned int)b < p.B) atomicAdd(&img[b], (unsigned long long)__double2ll_rn(fs * k));
                });
            });
        lds_barrier();
        const bool central = c.i < a.N && (unsigned int)c.p.type == a.type && n_t > 0.0;
        double t_phi = 0.0, t_glg = 0.0;
        for (unsigned int b = q; b < p.B; b += PEL_G)
            {
            const double H = (double)(long long)img[b] * inv_scale;
            const double rb = ((double)b + 0.5) * p.delta, r2 = rb * rb;
            double phi = 1.0, wgt = 0.0;
            if (central)
                {
                const double gb = H / (4.0 * M_PI * rho * r2);
                if (gb >= PEL_G_MIN)
                    {
                    const double lg = log(gb);
                    phi = gb * lg - gb + 1.0;
                    wgt = -0.5 * p.delta * lg;
                    t_glg += r2 * gb * lg;
                    }
                }
            t_phi += r2 * phi;
            if (c.i < a.N) out.W[(size_t)c.i * p.B + b] = wgt;
            }
        t_phi = group_sum<PEL_G>(t_phi);
        t_glg = group_sum<PEL_G>(t_glg);
        if (q == 0 && c.i < a.N)
            {
            const double s = central ? -c2 * t_phi : 0.0;
            out.s[c.i] = s;
            out.X[c.i] = central ? -(s + c2 * t_glg) : 0.0;
            if constexpr (!AVG)
                {
                double v = 0.0, gamma = 0.0;
                if (central) pel_switch(o, s, v, gamma);
                out.sbar[c.i] = s;
                out.v[c.i] = v;
                out.gn[c.i] = gamma;
                out.alpha[c.i] = gamma;
                v_sum += v;
                }
            }
        }
    if constexpr (!AVG)
        {
        v_sum = block_sum(v_sum, s_red);
        if (tid == 0) scratch[PEL_OFF_PART + blockIdx.x] = v_sum;
        }
    }

// sum_j f_a(r_kj) and sum_j f_a(r_kj) of[j] over row k in the average window (`aa`: its cut-off and window), the same bits in the
// eight lanes of the group
template<typename S4>
__device__ __forceinline__ void pel_window_sums(const QlArgs<4> &aa, const S4 *__restrict__ postype, const unsigned int *__restrict__ nlist,
                                                const double *__restrict__ tab, const RowCentre &c, const unsigned int q,
                                                const double *__restrict__ of, double &n, double &acc)
    {
    n = 0.0;
    acc = 0.0;
    row_walk_entries<PEL_G, true, false>(aa, postype, nlist, tab, c, q, [&](const double *tab_k, const unsigned int j, const double, const double, const double, const double rsq)
        {
        const double inv_r = rsqrt(rsq);
        double f, fprime_divr;
        smoothing_tab<4>(aa, tab_k, rsq, inv_r, f, fprime_divr);
        n += f;
        acc = fma(f, of[j], acc);
        });
    n = group_sum<PEL_G>(n);
    acc = group_sum<PEL_G>(acc);
    }

// ---- average: n_i, sbar_i, v_i, gn_i = gamma_i / (1 + n_i) and the block sums of v_i ----------------------------------------------
template<typename S4>
__global__ __launch_bounds__(PEL_THREADS) void k_pel_average(const QlArgs<4> aa_in, const PelOpt o, const S4 *__restrict__ postype,
                                                             const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                             const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                             double *__restrict__ scratch)
    {
    __shared__ double s_red[16];
    const QlArgs<4> aa = in_vgpr_window(aa_in);
    const unsigned int tid = threadIdx.x, g = tid / PEL_G, q = tid % PEL_G;
    const unsigned int n_chunks = (aa.N + PEL_PPB - 1) / PEL_PPB;
    const PelArrays out = pel_arrays(scratch, aa.N);
    double v_sum = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(aa, postype, head_list, n_neigh, chunk * PEL_PPB + g);
        double n, acc;
        pel_window_sums(aa, postype, nlist, tab, c, q, out.s, n, acc);
        if (q == 0 && c.i < aa.N)
            {
            const bool central = (unsigned int)c.p.type == aa.type;
            const double inv = 1.0 / (1.0 + n);
            const double sbar = central ? (out.s[c.i] + acc) * inv : 0.0;
            double v = 0.0, gamma = 0.0;
            if (central) pel_switch(o, sbar, v, gamma);
            out.sbar[c.i] = sbar;
            out.v[c.i] = v;
            out.gn[c.i] = gamma * inv;
            v_sum += v;
            }
        }
    v_sum = block_sum(v_sum, s_red);
    if (tid == 0) scratch[PEL_OFF_PART + blockIdx.x] = v_sum;
    }

// ---- adjoint of the average: alpha_j = gn_j + sum_{i in row j} f_a gn_i -----------------------------------------------------------
template<typename S4>
__global__ __launch_bounds__(PEL_THREADS) void k_pel_adjoint(const QlArgs<4> aa_in, const S4 *__restrict__ postype,
                                                             const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                             const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                             double *__restrict__ scratch)
    {
    const QlArgs<4> aa = in_vgpr_window(aa_in);
    const unsigned int tid = threadIdx.x, g = tid / PEL_G, q = tid % PEL_G;
    const unsigned int n_chunks = (aa.N + PEL_PPB - 1) / PEL_PPB;
    const PelArrays out = pel_arrays(scratch, aa.N);
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(aa, postype, head_list, n_neigh, chunk * PEL_PPB + g);
        double n, acc;
        pel_window_sums(aa, postype, nlist, tab, c, q, out.gn, n, acc);
        if (q == 0 && c.i < aa.N) out.alpha[c.i] = (unsigned int)c.p.type == aa.type ? out.gn[c.i] + acc : 0.0;
        }
    }

// ---- pass 2: the gather over row k -----------------------------------------------------------------------------------------------
template<typename S4, bool VIR, bool AVG>
__global__ __launch_bounds__(PEL_THREADS) void k_pel_forces(const QlArgs<4> a_in, const QlArgs<4> aa, const PeArgs p_in, const S4 *__restrict__ postype,
                                                            const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                            const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                            const double *__restrict__ scratch, S4 *__restrict__ force,
                                                            const double *__restrict__ d_bias, const double bias_host,
                                                            typename scalar4_traits<S4>::scalar *__restrict__ virial, const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    extern __shared__ double s_w[];                        // [PEL_PPB][B + 2]: W_kb at [b + 1]; [0] and [B + 1] are zero
    const QlArgs<4> a = in_vgpr(a_in);
    const PeArgs p = pe_in_vgpr(p_in);
    const unsigned int tid = threadIdx.x, g = tid / PEL_G, q = tid % PEL_G;
    const unsigned int n_chunks = (a.N + PEL_PPB - 1) / PEL_PPB;
    const PelArrays in = pel_arrays(const_cast<double *>(scratch), a.N);
    const int top = (int)p.B;
    const double scale = -(d_bias ? *d_bias : bias_host) / (double)a.n_global;
    double *w = s_w + (size_t)g * (p.B + 2);
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * PEL_PPB + g);
        lds_barrier();                                     // the walks of the round before have read their rows
        for (unsigned int b = q; b < p.B + 2; b += PEL_G)
            w[b] = b >= 1 && b <= p.B && c.cnt ? in.W[(size_t)c.i * p.B + (b - 1)] : 0.0;
        lds_barrier();
        const double alpha_k = c.own(a.N, in.alpha);
        double s_k = 0.0, sbar_k = 0.0, gn_k = 0.0;
        if constexpr (AVG) s_k = c.own(a.N, in.s), sbar_k = c.own(a.N, in.sbar), gn_k = c.own(a.N, in.gn);
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        double vxx = 0.0, vxy = 0.0, vxz = 0.0, vyy = 0.0, vyz = 0.0, vzz = 0.0;
        row_walk_entries<PEL_G, true, false>(a, postype, nlist, tab, c, q, [&](const double *tab_k, const unsigned int j, const double dx, const double dy, const double dz, const double rsq)
            {
            const double inv_r = rsqrt(rsq), r = rsq * inv_r;
            double f, fprime_divr;
            smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
            const double alpha_j = in.alpha[j];
            const double *__restrict__ wj = in.W + (size_t)j * p.B;
            const double half_minus_r = 0.5 * p.delta - r;
            double A = 0.0, X = 0.0;                         // sum wc K_b and sum wc K_b (r_b - r), wc = alpha_k W_kb + alpha_j W_jb
            pe_window(p, r, [&](const int b, const double k)
                {
                const double wk = w[min(max(b, -1), top) + 1];
                const double wn = (unsigned int)b < p.B ? wj[b] : 0.0;
                const double t = (alpha_k * wk + alpha_j * wn) * k;
                A += t;
                X = fma(t, fma((double)b, p.delta, half_minus_r), X);
                });
            double u = fprime_divr * A + f * p.inv_s2 * X * inv_r;      // (t_kj + t_jk) / r
            if constexpr (AVG)
                {
                if (rsq <= aa.rcutsq)
                    {
                    double fa, fa_prime_divr;
                    smoothing_tab<4>(aa, tab_k, rsq, inv_r, fa, fa_prime_divr);
                    u += fa_prime_divr * (gn_k * (in.s[j] - sbar_k) + in.gn[j] * (s_k - in.sbar[j]));
                    }
                }
            const double gx = u * dx, gy = u * dy, gz = u * dz;
            Fx += gx;
            Fy += gy;
            Fz += gz;
            if constexpr (VIR)
                {
                vxx += dx * gx, vxy += dx * gy, vxz += dx * gz;
                vyy += dy * gy, vyz += dy * gz, vzz += dz * gz;
                }
            });
        Fx = group_sum<PEL_G>(Fx);
        Fy = group_sum<PEL_G>(Fy);
        Fz = group_sum<PEL_G>(Fz);
        if (q == 0 && c.i < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + c.i);
        if constexpr (VIR)
            {
            vxx = group_sum<PEL_G>(vxx), vxy = group_sum<PEL_G>(vxy), vxz = group_sum<PEL_G>(vxz);
            vyy = group_sum<PEL_G>(vyy), vyz = group_sum<PEL_G>(vyz), vzz = group_sum<PEL_G>(vzz);
            if (q == 0 && c.i < a.N)                             // (the explicit diagonal term: alpha_k = 0 for a particle of another type)
                row_store_virial<true>(virial + c.i, virial_pitch, vxx, vxy, vxz, vyy, vyz, vzz, 0.5 * scale, scale * alpha_k * in.X[c.i]);
            }
        }
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct PelSetup
    {
    QlArgs<4> a, aa;                                       // the window of the histogram; the window of the average
    PeArgs p;
    PelOpt o;
    bool avg;
    };

// the bin constants of pair_entropy.hip's pe_args
PeArgs pel_pe_args(double r_max, double sigma_r, unsigned int n_bins)
    {
    PeArgs p;
    std::memset(&p, 0, sizeof(p));
    p.delta = r_max / n_bins;
    p.inv_delta = n_bins / r_max;
    p.inv_s2 = 1.0 / (sigma_r * sigma_r);
    p.neg_half_inv_s2 = -1.0 / (2.0 * sigma_r * sigma_r);
    p.k0 = 1.0 / (std::sqrt(2.0 * M_PI) * sigma_r);
    p.s = std::exp(-p.delta * p.delta / (2.0 * sigma_r * sigma_r));
    p.s2 = std::exp(-p.delta * p.delta / (sigma_r * sigma_r));
    p.B = n_bins;
    const double reach = std::floor((r_max + 4.0 * sigma_r) * p.inv_delta) + 1.0;      // no centre bin lies beyond this
    const double w = std::ceil(6.0 * sigma_r / p.delta);
    p.w = w < 1048576.0 ? (unsigned int)w : 1048576u;
    p.trips = reach < (double)p.w ? (unsigned int)reach : p.w;
    return p;
    }

// Everything both entry points refuse before a device is touched, and the kernel arguments they share.  Invalid arguments first, in the
// order of mtd_pe_*, the one unsupported case (too many bins) last.
int pel_setup(PelSetup &s, const mtd_pel_params *par, const mtd_pel_call *c, bool pointers, const void *d_virial, unsigned int virial_pitch)
    {
    if (!par || !c || !c->box || !c->d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (!(par->r_max > 0.0) || !std::isfinite(par->r_max) || !(par->sigma_r > 0.0) || !std::isfinite(par->sigma_r) || par->n_bins == 0)
        return MTD_ERR_INVALID_ARGUMENT;
    int rc = refuse_row_arrays(c->n_particles, pointers, c->dtype, c->d_scratch, d_virial, virial_pitch);
    if (rc) return rc;
    const double r_cut = par->r_max + 4.0 * par->sigma_r;
    if (par->average_on && (!(par->a_on >= 0.0) || !(par->a_on < par->a_cut) || !(par->a_cut <= r_cut))) return MTD_ERR_INVALID_ARGUMENT;
    if (par->switch_on && (!(par->c0 > 0.0) || !std::isfinite(par->c0) || par->p == 0)) return MTD_ERR_INVALID_ARGUMENT;
    if (c->n_global == 0) return MTD_ERR_INVALID_ARGUMENT;
    const double volume = c->box->L[0] * c->box->L[1] * c->box->L[2];
    if (!(volume > 0.0) || !std::isfinite(volume)) return MTD_ERR_INVALID_ARGUMENT;
    if (par->n_bins > MTD_PEL_MAX_BINS) return MTD_ERR_UNSUPPORTED;
    static const double no_ref[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    rc = fill_args<4>(s.a, c->n_particles, c->box, r_cut, par->r_max + 3.0 * par->sigma_r, 0, par->type, no_ref, c->n_global, 0);
    if (rc) return rc;
    s.avg = par->average_on != 0;
    s.aa = s.a;
    if (s.avg)
        {
        rc = fill_args<4>(s.aa, c->n_particles, c->box, par->a_cut, par->a_on, 0, par->type, no_ref, c->n_global, 0);
        if (rc) return rc;
        }
    s.p = pel_pe_args(par->r_max, par->sigma_r, par->n_bins);
    s.o.volume = volume;
    s.o.switch_on = par->switch_on ? 1 : 0;
    s.o.inv_c0 = par->switch_on ? 1.0 / par->c0 : 1.0;
    s.o.p = par->switch_on ? par->p : 1;
    return MTD_SUCCESS;
    }

} // namespace

extern "C" {

size_t mtd_pel_scratch_doubles(unsigned int n_particles, unsigned int n_bins)
    {
    return PEL_OFF_ARR + PEL_N_ARR * row_pitch(n_particles) + (size_t)n_particles * n_bins;
    }

int mtd_pel_accumulate(const mtd_pel_params *par, const mtd_pel_call *c, const double **d_partials, unsigned int *n_partials,
                       const double **d_s, const double **d_sbar, const double **d_v)
    {
    if (!d_partials || !n_partials) return MTD_ERR_INVALID_ARGUMENT;
    PelSetup su;
    int rc = pel_setup(su, par, c, c && c->d_postype && c->d_head_list && c->d_n_neigh, nullptr, 0);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)c->stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int N = c->n_particles;
    const unsigned int blocks = row_blocks(N, PEL_PPB, PEL_MAX_BLOCKS);
    const size_t image = (size_t)PEL_PPB * su.p.B * sizeof(unsigned long long);
    double *scratch = c->d_scratch;
    dispatch_s4(c->dtype, [&](auto t)
        {
        typedef typename decltype(t)::type S4;
        const S4 *pos = (const S4 *)c->d_postype;
        k_pel_count<S4><<<blocks, PEL_THREADS, 0, s>>>(N, par->type, pos, scratch + PEL_OFF_CNT);
        return dispatch_bool(su.avg, [&](auto avg)
            {
            k_pel_accumulate<S4, decltype(avg)::value><<<blocks, PEL_THREADS, image, s>>>(su.a, su.p, su.o, pos, c->d_head_list, c->d_n_neigh,
                                                                                           c->d_nlist, tab, blocks, scratch);
            if (decltype(avg)::value)
                k_pel_average<S4><<<blocks, PEL_THREADS, 0, s>>>(su.aa, su.o, pos, c->d_head_list, c->d_n_neigh, c->d_nlist, tab, scratch);
            return 0;
            });
        });
    MTD_LAUNCH_CHECK();
    const PelArrays arr = pel_arrays(scratch, N);
    *d_partials = scratch + PEL_OFF_PART;
    *n_partials = blocks;
    if (d_s) *d_s = arr.s;
    if (d_sbar) *d_sbar = arr.sbar;
    if (d_v) *d_v = arr.v;
    return MTD_SUCCESS;
    }

int mtd_pel_forces(const mtd_pel_params *par, const mtd_pel_call *c, void *d_force, const double *d_bias, double bias_host, void *d_virial,
                   unsigned int virial_pitch)
    {
    PelSetup su;
    int rc = pel_setup(su, par, c, c && c->d_postype && c->d_head_list && c->d_n_neigh && d_force, d_virial, virial_pitch);
    if (rc) return rc;
    if (c->n_particles == 0) return MTD_SUCCESS;
    hipStream_t s = (hipStream_t)c->stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int blocks = row_blocks(c->n_particles, PEL_PPB, PEL_MAX_BLOCKS);
    const size_t rows = (size_t)PEL_PPB * (su.p.B + 2) * sizeof(double);
    double *scratch = c->d_scratch;
    dispatch_s4(c->dtype, [&](auto t)
        {
        typedef typename decltype(t)::type S4;
        typedef typename scalar4_traits<S4>::scalar scalar;
        const S4 *pos = (const S4 *)c->d_postype;
        if (su.avg) k_pel_adjoint<S4><<<blocks, PEL_THREADS, 0, s>>>(su.aa, pos, c->d_head_list, c->d_n_neigh, c->d_nlist, tab, scratch);
        return dispatch_bool(d_virial != nullptr, [&](auto vir)
            {
            return dispatch_bool(su.avg, [&](auto avg)
                {
                k_pel_forces<S4, decltype(vir)::value, decltype(avg)::value><<<blocks, PEL_THREADS, rows, s>>>(
                    su.a, su.aa, su.p, pos, c->d_head_list, c->d_n_neigh, c->d_nlist, tab, scratch, (S4 *)d_force, d_bias, bias_host,
                    (scalar *)d_virial, virial_pitch);
                return 0;
                });
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // extern "C"
