// env_similarity.hip — environment similarity: template-matching crystallinity per particle (cv.environment_similarity) on gfx950.
//
// No reference counterpart (Piaggi and Parrinello, J. Chem. Phys. 150, 244119; PLUMED's ENVIRONMENTSIMILARITY).  Definition, gradient and
// virial: include/mtd_abi.h "Environment similarity"; restated in fp64 numpy in tests/env_similarity_ref.py.  In short, over the entries
// (i, j) of a FULL list with both particles of `type`, j != i, d = minImage(r_j - r_i) and r = |d| <= r_cut:
//     k^e_i = (1 / M_e) sum_j f(r) sum_m phi(d - T^e_m),   phi(x) = exp(-|x|^2 / 4 sigma_env^2)
//     k_i = smooth maximum of the k^e_i (lambda),  v_i = h(k_i),  s = (1 / N_global) sum_i v_i,  beta^e_i = h'(k_i) w^e_i
//     B_e(d) = f' (d / r) S_e - f (S_e d - V_e) / (2 sigma_env^2),   S_e = sum_m phi_m,  V_e = sum_m phi_m T^e_m
//     G_kj = sum_e [ -beta^e_k B_e(d_kj) + beta^e_j B_e(-d_kj) ] / M_e,   N_global ds/dr_k = sum_{j in row k} G_kj
// with f the cosine window of steinhardt_device.hpp between r_on and r_cut.  Smoothing, minimum image, particle loads and the type test are
// those of the Steinhardt units (QlArgs<4>, smoothing_tab, min_image); the walk over a row, its centre, the group's sum and the store of
// force and virial are those of row_walk.hpp; launches and the shared refusals go through dispatch.hpp.
//
// MI355X design.  Two launches per step, fp64 arithmetic over fp32 or fp64 arrays, ONE walk over the rows for the plain
// variable with a closed environment and two otherwise:
//   lanes            FOUR lanes (a DPP quad) per central particle, 64 central particles per block and round; lane q takes entries q, q + 4,
//                    ... of the row (rows hold ~17 entries at r_cut 1.5: 5 trips per lane, 85 % of the lanes' trips used where eight lanes
//                    use 71 %), list entry two trips and neighbour position one trip ahead of the arithmetic: row_walk of row_walk.hpp
//   the table        (T_x, T_y, T_z, |T|^2) of the <= 64 template vectors arrives in the kernel arguments and is copied to LDS once per
//                    block (2 KB); the loop over m has the same trip count in every lane and reads one vector as one 32-byte broadcast:
//                    |d - T|^2 = r^2 + |T|^2 - 2 d.T is three FMAs and an add
//   the Gaussian     the library's fp64 exp, one per (entry, vector) where every environment holds -T for every T (CLOSED:
//                    B_e(-d) = -B_e(d), so G = -(beta_k + beta_j) B_e(d) / M_e), two otherwise.  No vector is skipped: the loop stays
//                    uniform and k_i keeps every term
//   k_es_accumulate  k^e_i, the smooth maximum as max + log-sum-exp of the differences, v_i, beta^e_i; block sums of v_i in the fixed order
//                    of block_sum.  With one environment and no switch beta is 1 everywhere and G_kj needs nothing the walk does not have;
//                    if that environment is closed (FUSED) the same Gaussians give sum_j G_kj and the six sums of G_a d_b, nine doubles per
//                    particle in the scratch, and the step walks the rows ONCE (the general path with its second Gaussian ran out of scalar
//                    registers in this form and keeps two walks)
//   k_row_scale      (row_scale.hpp) FUSED: force and virial are those sums times -bias / N_global, one lane per particle
//   k_es_forces      otherwise: a gather over row k that reads beta_j (<= 4 doubles) per entry — not at all when beta is 1 everywhere
//                    (CONSTB; ghost neighbours then need no table).  Fixed summation order, no atomics; the four lanes' sums are added by
//                    two DPP moves.  VIR adds the six sums -1/2 G_a d_b; VIR = false is the kernel without them
#include "mtd_device.hpp"
#include "row_scale.hpp"

#include <cmath>
#include <cstring>

namespace
{

using namespace mtd;

constexpr int ES_THREADS = 256;
constexpr int ES_G = 4;                                    // lanes per central particle
constexpr int ES_PPB = ES_THREADS / ES_G;                  // central particles per block and round
constexpr unsigned int ES_MAX_BLOCKS = ROW_MAX_BLOCKS;     // block sums in the scratch
constexpr unsigned int ES_MAX_PER_ENV = 32;

// the scratch, in doubles, with n = n_particles rounded up to even:
//     k^e_i [n][4] | beta^e_i [n][4] | k_i [n] | v_i [n] | block sums [ES_MAX_BLOCKS] | FUSED: sum_j G_kj and sum_j G_a d_b [9][n]
constexpr int ES_N_GSUMS = 9;

struct EsArgs
    {
    double neg_inv4s2;                                     // -1 / (4 sigma_env^2)
    double c;                                              // 1 / (2 sigma_env^2)
    double lambda, inv_lambda;
    double inv_c0;
    double inv_m[MTD_ES_MAX_ENV];                          // 1 / M_e
    unsigned int first[MTD_ES_MAX_ENV + 1];                // environment e holds the vectors [first[e], first[e + 1])
    unsigned int n_env, p;
    int switch_on;
    };

struct EsTable
    {
    double4 t[MTD_ES_MAX_VEC];                             // (T_x, T_y, T_z, |T|^2)
    };

// x^n for a wave-uniform n (binary powering: at most 32 trips of a scalar loop)
__device__ __forceinline__ double es_powi(double x, unsigned int n)
    {
    double r = 1.0;
    for (; n; n >>= 1)
        {
        if (n & 1u) r *= x;
        x *= x;
        }
    return r;
    }

__device__ __forceinline__ void es_load_table(const EsTable &T, double4 *s_t)
    {
    if (threadIdx.x < MTD_ES_MAX_VEC) s_t[threadIdx.x] = T.t[threadIdx.x];
    __syncthreads();
    }

// One environment's sums over its template vectors [m, m_end) for the pair vector d: S = sum phi_m and V = sum phi_m T_m; on the general
// path the same for -d as well (R, W).  d2 = -2 d, so that |d -+ T|^2 = (r^2 + |T|^2) +- d2.T; the trip count is the same in every lane
struct EsSums
    {
    double S, Vx, Vy, Vz, R, Wx, Wy, Wz;
    };

template<bool CLOSED>
__device__ __forceinline__ EsSums es_env_sums(const double4 *s_t, unsigned int m, const unsigned int m_end, const double dx2, const double dy2,
                                              const double dz2, const double rsq, const double neg_inv4s2)
    {
    EsSums s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (; m < m_end; ++m)
        {
        const double4 t = s_t[m];
        const double base = rsq + t.w;
        const double dt = fma(dx2, t.x, fma(dy2, t.y, dz2 * t.z));                              // -2 d.T
        const double phi = exp((base + dt) * neg_inv4s2);
        s.S += phi;
        s.Vx = fma(phi, t.x, s.Vx), s.Vy = fma(phi, t.y, s.Vy), s.Vz = fma(phi, t.z, s.Vz);
        if constexpr (!CLOSED)
            {
            const double psi = exp((base - dt) * neg_inv4s2);
            s.R += psi;
            s.Wx = fma(psi, t.x, s.Wx), s.Wy = fma(psi, t.y, s.Wy), s.Wz = fma(psi, t.z, s.Wz);
            }
        }
    return s;
    }

// G_kj += [ -b_k B_e(d) + b_j B_e(-d) ] / M_e with B_e(d) = d (f'/r - f c) S + f c V and B_e(-d) = -d (f'/r - f c) R + f c W; an environment
// that holds its own inverse has B_e(-d) = -B_e(d)
template<bool CLOSED>
__device__ __forceinline__ void es_fold(const EsSums &s, const double b_k, const double b_j, const double inv_m, const double radial,
                                        const double fc, const double dx, const double dy, const double dz, double &gx, double &gy, double &gz)
    {
    if constexpr (CLOSED)
        {
        const double w = -(b_k + b_j) * inv_m, wr = w * radial * s.S, wv = w * fc;
        gx += fma(wr, dx, wv * s.Vx);
        gy += fma(wr, dy, wv * s.Vy);
        gz += fma(wr, dz, wv * s.Vz);
        }
    else
        {
        const double wk = -b_k * inv_m, wj = b_j * inv_m;
        const double wr = (wk * s.S - wj * s.R) * radial;
        gx += fma(wr, dx, fc * (wk * s.Vx + wj * s.Wx));
        gy += fma(wr, dy, fc * (wk * s.Vy + wj * s.Wy));
        gz += fma(wr, dz, fc * (wk * s.Vz + wj * s.Wz));
        }
    }

// ---- pass 1: k^e_i, k_i, v_i, beta^e_i and the block's sum of v_i; FUSED (one closed environment, beta = 1): the gradient sums too ----
template<typename S4, bool FUSED>
__global__ __launch_bounds__(ES_THREADS) void k_es_accumulate(const QlArgs<4> a_in, const EsArgs p, const EsTable T,
                                                              const S4 *__restrict__ postype, const unsigned int *__restrict__ head_list,
                                                              const unsigned int *__restrict__ n_neigh, const unsigned int *__restrict__ nlist,
                                                              const double *__restrict__ tab, double *__restrict__ scratch)
    {
    __shared__ double4 s_t[MTD_ES_MAX_VEC];
    __shared__ double s_red[16];
    const QlArgs<4> a = in_vgpr_window(a_in);
    const double neg_inv4s2 = in_vgpr(p.neg_inv4s2), cs = in_vgpr(p.c);
    const unsigned int tid = threadIdx.x, g = tid / ES_G, q = tid % ES_G;
    const unsigned int n_chunks = (a.N + ES_PPB - 1) / ES_PPB;
    const size_t n_even = row_pitch(a.N);
    asm volatile("" : "+v"(scratch));                            // (the output pointers in vector registers: they are used once per particle)
    double *__restrict__ out_ke = scratch, *__restrict__ out_beta = scratch + 4 * n_even, *__restrict__ out_k = scratch + 8 * n_even,
                        *__restrict__ out_v = scratch + 9 * n_even, *__restrict__ part = scratch + 10 * n_even,
                        *__restrict__ out_g = scratch + 10 * n_even + ES_MAX_BLOCKS;
    es_load_table(T, s_t);
    const int n_env = (int)p.n_env;
    // first loop: the walks.  k^e_i of the block's particles go to the scratch; what follows the walk is a loop of its own (below), so that
    // the literals of its logarithm and exponentials are not held in scalar registers across the walk (they spilled)
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * ES_PPB + g);
        double ke[MTD_ES_MAX_ENV] = {0.0, 0.0, 0.0, 0.0};
        double gs[ES_N_GSUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // FUSED: G_x G_y G_z and G_a d_b for xx xy xz yy yz zz
        row_walk<ES_G, false>(a, postype, nlist, tab, c, q, [&](const double *tab_k, const unsigned int, const double dx, const double dy, const double dz,
                                                 const double rsq)
            {
            const double inv_r = rsqrt(rsq);
            double f, fprime_divr;
            smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
            const double dx2 = -2.0 * dx, dy2 = -2.0 * dy, dz2 = -2.0 * dz;
            if constexpr (FUSED)
                {
                const EsSums s = es_env_sums<true>(s_t, 0, p.first[1], dx2, dy2, dz2, rsq, neg_inv4s2);
                ke[0] = fma(f, s.S, ke[0]);
                const double fc = f * cs;
                double gx = 0.0, gy = 0.0, gz = 0.0;
                es_fold<true>(s, 1.0, 1.0, p.inv_m[0], fprime_divr - fc, fc, dx, dy, dz, gx, gy, gz);
                gs[0] += gx, gs[1] += gy, gs[2] += gz;
                gs[3] += gx * dx, gs[4] += gx * dy, gs[5] += gx * dz;
                gs[6] += gy * dy, gs[7] += gy * dz, gs[8] += gz * dz;
                }
            else
                {
                for (int e = 0; e < n_env; ++e)
                    {
                    const EsSums s = es_env_sums<true>(s_t, p.first[e], p.first[e + 1], dx2, dy2, dz2, rsq, neg_inv4s2);   // (S alone is used)
                    const double val = f * s.S;
#pragma unroll
                    for (int u = 0; u < MTD_ES_MAX_ENV; ++u) ke[u] += u == e ? val : 0.0;
                    }
                }
            });
#pragma unroll
        for (int u = 0; u < MTD_ES_MAX_ENV; ++u) ke[u] = group_sum<ES_G>(ke[u]) * p.inv_m[u];             // (1 / M_e is 0 for e >= E)
        if (q == 0 && c.i < a.N)
            {
#pragma unroll
            for (int u = 0; u < MTD_ES_MAX_ENV; ++u) out_ke[4 * (size_t)c.i + u] = ke[u];
            }
        if constexpr (FUSED)
            {
#pragma unroll
            for (int u = 0; u < ES_N_GSUMS; ++u) gs[u] = group_sum<ES_G>(gs[u]);
            if (q == 0 && c.i < a.N)
                {
#pragma unroll
                for (int u = 0; u < ES_N_GSUMS; ++u) out_g[u * n_even + c.i] = gs[u];
                }
            }
        }
    __syncthreads();                                           // the block reads back what its own lanes stored
    // second loop: one lane per particle of the same chunks (wave w of the block takes the block's chunks w, w + 4, ...)
    double v_sum = 0.0;
    for (unsigned int chunk = blockIdx.x + (tid / ES_PPB) * gridDim.x; chunk < n_chunks; chunk += (ES_THREADS / ES_PPB) * gridDim.x)
        {
        const unsigned int i = chunk * ES_PPB + tid % ES_PPB;
        if (i < a.N)
            {
            const bool central = (unsigned int)scalar4_traits<S4>::load(postype, i).type == a.type;
            double ke[MTD_ES_MAX_ENV];
#pragma unroll
            for (int u = 0; u < MTD_ES_MAX_ENV; ++u) ke[u] = out_ke[4 * (size_t)i + u];
            // the smooth maximum as max + log-sum-exp of the differences (lambda k never reaches an exponential on its own)
            double k = ke[0], w[MTD_ES_MAX_ENV] = {1.0, 0.0, 0.0, 0.0};
            if (n_env > 1)
                {
                double top = ke[0];
#pragma unroll
                for (int u = 1; u < MTD_ES_MAX_ENV; ++u) top = u < n_env ? fmax(top, ke[u]) : top;
                double sum = 0.0;
#pragma unroll
                for (int u = 0; u < MTD_ES_MAX_ENV; ++u)
                    {
                    w[u] = u < n_env ? exp(p.lambda * (ke[u] - top)) : 0.0;
                    sum += w[u];
                    }
                k = top + log(sum) * p.inv_lambda;
                const double inv_sum = 1.0 / sum;
#pragma unroll
                for (int u = 0; u < MTD_ES_MAX_ENV; ++u) w[u] *= inv_sum;
                }
            double v = k, dh = 1.0;
            if (p.switch_on)
                {
                const double x = k * p.inv_c0, xpm1 = es_powi(x, p.p - 1), xp = xpm1 * x, den = 1.0 / (1.0 + xp);
                v = xp * den;
                dh = (double)p.p * xpm1 * p.inv_c0 * den * den;
                }
            if (!central) k = v = dh = 0.0;
#pragma unroll
            for (int u = 0; u < MTD_ES_MAX_ENV; ++u) out_beta[4 * (size_t)i + u] = dh * w[u];
            out_k[i] = k;
            out_v[i] = v;
            v_sum += v;
            }
        }
    v_sum = block_sum(v_sum, s_red);
    if (tid == 0) part[blockIdx.x] = v_sum;
    }

// ---- pass 2 (FUSED: k_row_scale of row_scale.hpp, the sums of pass 1 times -bias / N_global); otherwise: the gather over row k
// (CONSTB: beta = 1 with an environment that is not closed; never with CLOSED) ------------------------------------------------------------
template<typename S4, bool VIR, bool CLOSED, bool CONSTB>
__global__ __launch_bounds__(ES_THREADS) void k_es_forces(const QlArgs<4> a_in, const EsArgs p, const EsTable T, const S4 *__restrict__ postype,
                                                          const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                          const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                          const double *__restrict__ scratch, S4 *__restrict__ force,
                                                          const double *__restrict__ d_bias, const double bias_host,
                                                          typename scalar4_traits<S4>::scalar *__restrict__ virial, const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    __shared__ double4 s_t[MTD_ES_MAX_VEC];
    const QlArgs<4> a = in_vgpr_window(a_in);
    const double neg_inv4s2 = in_vgpr(p.neg_inv4s2), cs = in_vgpr(p.c);
    const unsigned int tid = threadIdx.x, g = tid / ES_G, q = tid % ES_G;
    const unsigned int n_chunks = (a.N + ES_PPB - 1) / ES_PPB;
    const double *__restrict__ beta = scratch + 4 * row_pitch(a.N);
    es_load_table(T, s_t);
    const int n_env = (int)p.n_env;
    const double scale = in_vgpr(-(d_bias ? *d_bias : bias_host) / (double)a.n_global);
    // (the output pointers too: what is used once per particle need not hold scalar registers across the walk)
    asm volatile("" : "+v"(force));
    if constexpr (VIR) asm volatile("" : "+v"(virial));
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * ES_PPB + g);
        double bk[MTD_ES_MAX_ENV] = {1.0, 1.0, 1.0, 1.0};
        if constexpr (!CONSTB)
            {
            if (c.cnt)
                {
#pragma unroll
                for (int u = 0; u < MTD_ES_MAX_ENV; ++u) bk[u] = beta[4 * (size_t)c.i + u];
                }
            }
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        double vxx = 0.0, vxy = 0.0, vxz = 0.0, vyy = 0.0, vyz = 0.0, vzz = 0.0;
        row_walk<ES_G, false>(a, postype, nlist, tab, c, q, [&](const double *tab_k, const unsigned int j, const double dx, const double dy, const double dz,
                                                 const double rsq)
            {
            const double inv_r = rsqrt(rsq);
            double f, fprime_divr;
            smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
            const double fc = f * cs;
            const double dx2 = -2.0 * dx, dy2 = -2.0 * dy, dz2 = -2.0 * dz;
            double gx = 0.0, gy = 0.0, gz = 0.0;                 // G_kj
            for (int e = 0; e < n_env; ++e)
                {
                const EsSums s = es_env_sums<CLOSED>(s_t, p.first[e], p.first[e + 1], dx2, dy2, dz2, rsq, neg_inv4s2);
                double b_k = bk[0];
#pragma unroll
                for (int u = 1; u < MTD_ES_MAX_ENV; ++u) b_k = u == e ? bk[u] : b_k;
                double b_j = 1.0;                                                          // (CONSTB: no table, ghost neighbours included)
                if constexpr (!CONSTB) b_j = j < a.N ? beta[4 * (size_t)j + e] : 0.0;        // (no ghosts here: the entry point refuses them)
                es_fold<CLOSED>(s, b_k, b_j, p.inv_m[e], fprime_divr - fc, fc, dx, dy, dz, gx, gy, gz);
                }
            Fx += gx;
            Fy += gy;
            Fz += gz;
            if constexpr (VIR)
                {
                vxx += gx * dx, vxy += gx * dy, vxz += gx * dz;
                vyy += gy * dy, vyz += gy * dz, vzz += gz * dz;
                }
            });
        Fx = group_sum<ES_G>(Fx);
        Fy = group_sum<ES_G>(Fy);
        Fz = group_sum<ES_G>(Fz);
        if (q == 0 && c.i < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + c.i);
        if constexpr (VIR)
            {
            vxx = group_sum<ES_G>(vxx), vxy = group_sum<ES_G>(vxy), vxz = group_sum<ES_G>(vxz);
            vyy = group_sum<ES_G>(vyy), vyz = group_sum<ES_G>(vyz), vzz = group_sum<ES_G>(vzz);
            if (q == 0 && c.i < a.N) row_store_virial<false>(virial + c.i, virial_pitch, vxx, vxy, vxz, vyy, vyz, vzz, -0.5 * scale, 0.0);
            }
        }
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------
// what both entry points check before a device is touched, after refuse_row_arrays (dtype, arrays, alignment of the scratch, virial pitch:
// all invalid arguments, as everything here ahead of the first unsupported one), and the kernel arguments they share
struct EsSetup
    {
    QlArgs<4> a;
    EsArgs p;
    EsTable T;
    bool closed, const_beta;
    };

int es_setup(EsSetup &s, unsigned int n_particles, unsigned int n_ghost, const mtd_box *box, unsigned int type,
             const mtd_es_params *par, unsigned int n_global, const double *d_scratch)
    {
    if (!box || !par || !d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (n_global == 0) return MTD_ERR_INVALID_ARGUMENT;
    if (par->n_env == 0) return MTD_ERR_INVALID_ARGUMENT;
    if (par->n_env > MTD_ES_MAX_ENV) return MTD_ERR_UNSUPPORTED;
    unsigned int total = 0;
    for (unsigned int e = 0; e < par->n_env; ++e)
        {
        if (par->n_vec[e] == 0) return MTD_ERR_INVALID_ARGUMENT;
        if (par->n_vec[e] > ES_MAX_PER_ENV) return MTD_ERR_UNSUPPORTED;
        total += par->n_vec[e];
        }
    if (total > MTD_ES_MAX_VEC) return MTD_ERR_UNSUPPORTED;
    if (!(par->sigma_env > 0.0) || !std::isfinite(par->sigma_env) || !(par->r_on >= 0.0) || !(par->r_on < par->r_cut) || !std::isfinite(par->r_cut))
        return MTD_ERR_INVALID_ARGUMENT;
    if (par->n_env > 1 && (!(par->lambda > 0.0) || !std::isfinite(par->lambda))) return MTD_ERR_INVALID_ARGUMENT;
    if (par->switch_on && (!(par->c0 > 0.0) || !std::isfinite(par->c0) || par->p == 0)) return MTD_ERR_INVALID_ARGUMENT;
    for (unsigned int m = 0; m < total; ++m)
        {
        const double *t = par->vec[m];
        const double len2 = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
        if (!std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2]) || !(len2 > 0.0) || !(len2 < par->r_cut * par->r_cut))
            return MTD_ERR_INVALID_ARGUMENT;
        }
    s.const_beta = par->n_env == 1 && !par->switch_on;
    // beta of a ghost would have to be exchanged; with one environment and no switch it is 1 and the table is never read for a neighbour
    if (n_ghost > 0 && !s.const_beta) return MTD_ERR_UNSUPPORTED;
    static const double no_ref[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int rc = fill_args<4>(s.a, n_particles, box, par->r_cut, par->r_on, 0, type, no_ref, n_global, 0);
    if (rc) return rc;
    std::memset(&s.p, 0, sizeof(s.p));
    std::memset(&s.T, 0, sizeof(s.T));
    s.p.neg_inv4s2 = -1.0 / (4.0 * par->sigma_env * par->sigma_env);
    s.p.c = 1.0 / (2.0 * par->sigma_env * par->sigma_env);
    s.p.lambda = par->n_env > 1 ? par->lambda : 1.0;
    s.p.inv_lambda = 1.0 / s.p.lambda;
    s.p.switch_on = par->switch_on ? 1 : 0;
    s.p.inv_c0 = par->switch_on ? 1.0 / par->c0 : 1.0;
    s.p.p = par->switch_on ? par->p : 1;
    s.p.n_env = par->n_env;
    s.closed = true;
    unsigned int first = 0;
    for (unsigned int e = 0; e < par->n_env; ++e)
        {
        s.p.first[e] = first;
        s.p.inv_m[e] = 1.0 / (double)par->n_vec[e];
        for (unsigned int m = first; m < first + par->n_vec[e]; ++m)
            {
            const double *t = par->vec[m];
            s.T.t[m] = make_double4(t[0], t[1], t[2], t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
            // inversion-closed: -T is in the environment for every T, by exact comparison
            bool found = false;
            for (unsigned int k = first; k < first + par->n_vec[e] && !found; ++k)
                found = par->vec[k][0] == -t[0] && par->vec[k][1] == -t[1] && par->vec[k][2] == -t[2];
            s.closed = s.closed && found;
            }
        first += par->n_vec[e];
        }
    for (unsigned int e = par->n_env; e <= MTD_ES_MAX_ENV; ++e) s.p.first[e] = first;
    return MTD_SUCCESS;
    }

} // namespace

extern "C" {

size_t mtd_es_scratch_doubles(unsigned int n_particles)
    {
    return (10 + ES_N_GSUMS) * row_pitch(n_particles) + ES_MAX_BLOCKS;
    }

int mtd_es_accumulate(unsigned int n_particles, unsigned int n_ghost, const void *d_postype, int dtype, const mtd_box *box,
                      const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, unsigned int type,
                      const mtd_es_params *params, unsigned int n_global, double *d_scratch, const double **d_partials, unsigned int *n_partials,
                      const double **d_k, const double **d_ke, const double **d_v, mtd_stream_t stream)
    {
    if (!d_partials || !n_partials) return MTD_ERR_INVALID_ARGUMENT;
    int rc = refuse_row_arrays(n_particles, d_postype && d_head_list && d_n_neigh, dtype, d_scratch, nullptr, 0);
    if (rc) return rc;
    EsSetup su;
    rc = es_setup(su, n_particles, n_ghost, box, type, params, n_global, d_scratch);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int blocks = row_blocks(n_particles, ES_PPB, ES_MAX_BLOCKS);
    // beta = 1 everywhere and the environment closed: the walk of this pass also forms the gradient sums (FUSED)
    dispatch_s4(dtype, [&](auto t)
        {
        return dispatch_bool(su.const_beta && su.closed, [&](auto fused)
            {
            typedef typename decltype(t)::type S4;
            k_es_accumulate<S4, decltype(fused)::value><<<blocks, ES_THREADS, 0, s>>>(su.a, su.p, su.T, (const S4 *)d_postype, d_head_list, d_n_neigh,
                                                                                       d_nlist, tab, d_scratch);
            return 0;
            });
        });
    MTD_LAUNCH_CHECK();
    const size_t n = row_pitch(n_particles);
    *d_partials = d_scratch + 10 * n;
    *n_partials = blocks;
    if (d_ke) *d_ke = d_scratch;
    if (d_k) *d_k = d_scratch + 8 * n;
    if (d_v) *d_v = d_scratch + 9 * n;
    return MTD_SUCCESS;
    }

int mtd_es_forces(unsigned int n_particles, unsigned int n_ghost, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                  const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, unsigned int type,
                  const mtd_es_params *params, unsigned int n_global, const double *d_scratch, const double *d_bias, double bias_host,
                  mtd_stream_t stream, void *d_virial, unsigned int virial_pitch)
    {
    int rc = refuse_row_arrays(n_particles, d_postype && d_head_list && d_n_neigh && d_force, dtype, d_scratch, d_virial, virial_pitch);
    if (rc) return rc;
    EsSetup su;
    rc = es_setup(su, n_particles, n_ghost, box, type, params, n_global, d_scratch);
    if (rc) return rc;
    if (n_particles == 0) return MTD_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    // mtd_es_accumulate has left the gradient sums (FUSED): one lane per particle scales them by -bias / N_global and bias / (2 N_global)
    if (su.const_beta && su.closed)
        {
        const size_t pitch = row_pitch(n_particles);
        row_scale(dtype, n_particles, d_scratch + 10 * pitch + ROW_MAX_BLOCKS, pitch, nullptr, (double)n_global, -1.0, 0.5, d_force, d_bias,
                  bias_host, d_virial, virial_pitch, s);
        MTD_LAUNCH_CHECK();
        return MTD_SUCCESS;
        }
    const unsigned int blocks = row_blocks(n_particles, ES_PPB, ES_MAX_BLOCKS);
    dispatch_s4(dtype, [&](auto t)
        {
        return dispatch_bool(d_virial != nullptr, [&](auto vir)
            {
            typedef typename decltype(t)::type S4;
            typedef typename scalar4_traits<S4>::scalar scalar;
            const auto gather = [&](auto closed, auto constb)
                {
                k_es_forces<S4, decltype(vir)::value, decltype(closed)::value, decltype(constb)::value><<<blocks, ES_THREADS, 0, s>>>(
                    su.a, su.p, su.T, (const S4 *)d_postype, d_head_list, d_n_neigh, d_nlist, tab, d_scratch, (S4 *)d_force, d_bias, bias_host,
                    (scalar *)d_virial, virial_pitch);
                return 0;
                };
            if (su.const_beta) return gather(std::false_type{}, std::true_type{});
            return dispatch_bool(su.closed, [&](auto closed) { return gather(closed, std::false_type{}); });
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // extern "C"
