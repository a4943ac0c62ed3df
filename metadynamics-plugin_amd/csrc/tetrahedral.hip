// tetrahedral.hip — three-body bond-angle order of the particles of one type (cv.tetrahedral) on gfx950.
//
// No reference counterpart (the tetrahedral order parameter of Chau and Hardin and of Errington and Debenedetti in its smooth, weighted
// form; the three-body penalty of Stillinger and Weber).  Definition, gradient and virial: include/mtd_abi.h "Tetrahedral order";
// restated in fp64 numpy FROM THE PAIR SUM in tests/tetrahedral_ref.py.  In short, over the entries (i, j) of a FULL list with both
// particles of the type, j != i and r = |d| <= r_cut, d = minImage(r_j - r_i), u = d / r, f the cosine window of the Steinhardt passes:
//     n = sum f    m = sum f^2    b = sum f u    T = sum f u (x) u                                   (eleven moments of the row)
//     A = sum_{j<k} f_j f_k (u_j.u_k - cos0)^2 = 1/2 [ (T:T - m) - 2 cos0 (b.b - m) + cos0^2 (n^2 - m) ]      W = 1/2 (n^2 - m)
//     t = 1 - kappa A / W,  v = g(n) h(t)      (not normalised: v = A)      s = (1 / N_t) sum_i v_i
// The pair sum costs O(n^2) per row; its expansion in the moments costs O(n), the move the addition theorem makes for Steinhardt.  The
// force on a particle then needs alpha = dv/d(n, m, b, T) of each neighbour, eleven numbers, not the neighbour's row.
// Minimum image, particle loads and the window are those of the Steinhardt units (QlArgs<4>, min_image, smoothing_tab); the walk, the
// group's sum, the store of the virial and the sums kernel are row_walk.hpp's; launches and the shared refusals go through dispatch.hpp.
//
// MI355X design.  All arithmetic in fp64 over fp32 or fp64 arrays.
//   lanes              EIGHT lanes per central particle, 32 central particles per block and round, as in coordination.hip
//   k_tet_accumulate   one walk (row_walk_entries<8, false, false>: local entries only, every per-particle array ends at N) forms the
//                      eleven moments; lane 0 of the group forms A, W, t, v and alpha and stores n_i, t_i, v_i and the adjoint row; the
//                      block leaves its share of sum v_i and N_t
//   the adjoint table  ROW-major, twelve doubles per particle (eleven and a pad: 96 B, 16-byte aligned): a neighbour's alpha is six
//                      16-byte loads from one or two cache lines.  The per-lane cache-LINE rate bounds the force pass of this family when
//                      lanes hold different neighbours; a component-major table would touch eleven lines per entry
//   k_tet_forces       the gather over row k.  An entry gives -g_kj(d) + g_jk(-d); with beta = alpha_k (+/-) alpha_j — the sum for n, m
//                      and T, the difference for b, which is odd in d — both terms are ONE evaluation of f, f', u and of the bracket.  The
//                      centre's alpha stays in registers, the neighbour's comes from the table
//   k_row_mask         (row_mask.hpp) mtd_tetrahedral_accumulate_cluster: between k_tet_accumulate and k_row_sums, after the cluster pass of
//                      cluster.hip on the v_i just written — the adjoint row of every particle outside the largest cluster set to 0,
//                      the block sums of slot 0 replaced by those of w_i v_i.  k_tet_forces then runs unchanged on the masked table
//   k_row_sums         (row_walk.hpp) one wave per slot adds the blocks' doubles in the fixed order of wave_sum
//   k_tet_finalize     s from the (reduced) sums
// An entry with r = 0 has no direction: it takes no part.  Fixed summation order everywhere (a lane's entries in row order, the DPP tree
// of group_sum, a thread's chunks in order, block_sum, wave_sum), no atomics: two identical calls give identical bits, and a row gives
// the same bits wherever it lies in the list.
#include "mtd_device.hpp"
#include "row_walk.hpp"
#include "row_mask.hpp"
#include "dispatch.hpp"
#include "cluster_host.hpp"

#include <cmath>
#include <cstring>

namespace
{

using namespace mtd;

constexpr int TET_THREADS = 256;
constexpr int TET_G = 8;                                    // lanes per central particle
constexpr int TET_PPB = TET_THREADS / TET_G;                // central particles per block and round
constexpr unsigned int TET_MAX_BLOCKS = ROW_MAX_BLOCKS;     // columns of block sums in the scratch
constexpr int TET_N_MOMENTS = 11;                           // n, m, b[3], T[6] (xx xy xz yy yz zz)
constexpr int TET_ALPHA = 12;                               // doubles of an adjoint row: the eleven and a pad

// the scratch, in doubles: sums [2] | value, N_t [2] | (pad) | block sums [2][TET_MAX_BLOCKS]
// | n_i [n] | t_i [n] | v_i [n] | alpha [n][12], n = n_particles rounded up to 2
constexpr size_t TET_OFF_SUMS = 0, TET_OFF_VALUE = 2, TET_OFF_NT = 3, TET_OFF_PART = 16, TET_OFF_PER_PARTICLE = TET_OFF_PART + 2 * (size_t)TET_MAX_BLOCKS;
constexpr int TET_ROW_N = 0, TET_ROW_T = 1, TET_ROW_V = 2, TET_ROWS = 3;

struct TetArgs
    {
    double cos0, kappa;                                     // kappa = 1 / (1/3 + cos0^2)
    double inv_c0, n_lo, inv_dn;                            // 1 / c0, n_lo, 1 / (n_hi - n_lo)
    unsigned int p;
    int normalise, sw, gate;
    };

// h = x^p / (1 + x^p), x = max(t, 0) / c0 (h = t without a switch); g = 3 y^2 - 2 y^3, y = clip((n - n_lo) / (n_hi - n_lo), 0, 1) (g = 1
// without a gate); and their derivatives: the functions of mtd_ql_local_options, as steinhardt_local.hip forms them
__device__ __forceinline__ void tet_transform(const TetArgs &o, const double t, const double n, double &h, double &dh, double &g, double &dg)
    {
    h = t;
    dh = 1.0;
    if (o.sw)
        {
        const double x = fmax(t, 0.0) * o.inv_c0;
        double xp1 = 1.0, b = x;
        for (unsigned int k = o.p - 1; k != 0; k >>= 1)
            {
            if (k & 1u) xp1 *= b;
            b *= b;
            }
        const double xp = xp1 * x, den = 1.0 / (1.0 + xp);
        h = xp * den;
        dh = t >= 0.0 ? (double)o.p * xp1 * (den * den) * o.inv_c0 : 0.0;
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
        const double y = fmin(fmax((n - o.n_lo) * o.inv_dn, 0.0), 1.0);
        g = y * y * (3.0 - 2.0 * y);
        dg = 6.0 * y * (1.0 - y) * o.inv_dn;
        }
    }

// ---- pass 1: the moments of every row -> n_i, t_i, v_i, the adjoint row and the block's sums of v_i and of the type count --------------
template<typename S4>
__global__ __launch_bounds__(TET_THREADS) void k_tet_accumulate(const QlArgs<4> a_in, const TetArgs d, const S4 *__restrict__ postype,
                                                                const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                                const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                                double *__restrict__ part, double *__restrict__ per_particle, const size_t pitch)
    {
    __shared__ double s_red[16];
    const QlArgs<4> a = in_vgpr_window(a_in);
    const unsigned int tid = threadIdx.x, g = tid / TET_G, q = tid % TET_G;
    const unsigned int n_chunks = (a.N + TET_PPB - 1) / TET_PPB;
    asm volatile("" : "+v"(per_particle));                      // (the output pointer in vector registers: it is used once per particle)
    double v_sum = 0.0, count = 0.0;                            // lane 0 of a group: sum v_i and the centres of the type over its chunks
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * TET_PPB + g);
        double mo[TET_N_MOMENTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        row_walk_entries<TET_G, false, false>(a, postype, nlist, tab, c, q,
                                              [&](const double *tab_k, const unsigned int, const double dx, const double dy, const double dz, const double rsq)
            {
            if (rsq > 0.0)
                {
                const double inv_r = rsqrt(rsq);
                double f, fprime_divr;
                smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
                const double ux = dx * inv_r, uy = dy * inv_r, uz = dz * inv_r;
                const double fx = f * ux, fy = f * uy, fz = f * uz;
                mo[0] += f;
                mo[1] = fma(f, f, mo[1]);
                mo[2] += fx, mo[3] += fy, mo[4] += fz;
                mo[5] = fma(fx, ux, mo[5]), mo[6] = fma(fx, uy, mo[6]), mo[7] = fma(fx, uz, mo[7]);
                mo[8] = fma(fy, uy, mo[8]), mo[9] = fma(fy, uz, mo[9]), mo[10] = fma(fz, uz, mo[10]);
                }
            });
#pragma unroll
        for (int u = 0; u < TET_N_MOMENTS; ++u) mo[u] = group_sum<TET_G>(mo[u]);
        if (q == 0 && c.i < a.N)
            {
            const double n = mo[0], m = mo[1], c0 = d.cos0;
            const double bb = mo[2] * mo[2] + mo[3] * mo[3] + mo[4] * mo[4];
            const double tt = mo[5] * mo[5] + mo[8] * mo[8] + mo[10] * mo[10] + 2.0 * (mo[6] * mo[6] + mo[7] * mo[7] + mo[9] * mo[9]);
            const double w2 = n * n - m;                        // 2 W
            const double A = 0.5 * ((tt - m) - 2.0 * c0 * (bb - m) + c0 * c0 * w2), W = 0.5 * w2;
            // dA / d(n, m, b, T) = (cos0^2 n, -(1 - cos0)^2 / 2, -2 cos0 b, T);  dW / d(n, m) = (n, -1/2)
            const double dA_n = c0 * c0 * n, dA_m = -0.5 * (1.0 - c0) * (1.0 - c0), dA_b = -2.0 * c0;
            double t_i = A, v = A;
            double al_n = dA_n, al_m = dA_m, al_b = dA_b, al_T = 1.0;   // alpha_b = al_b b, alpha_T = al_T T
            if (d.normalise)
                {
                t_i = v = 0.0;
                al_n = al_m = al_b = al_T = 0.0;
                if (W >= MTD_TET_W_MIN)
                    {
                    const double inv_w = 1.0 / W, ratio = A * inv_w, k_w = -d.kappa * inv_w;   // dt/dmu = -kappa (dA_mu - (A / W) dW_mu) / W
                    t_i = 1.0 - d.kappa * ratio;
                    double h, dh, gt, dgt;
                    tet_transform(d, t_i, n, h, dh, gt, dgt);
                    v = gt * h;
                    const double s = gt * dh * k_w;
                    al_n = s * (dA_n - ratio * n) + dgt * h;
                    al_m = s * (dA_m + 0.5 * ratio);
                    al_b = s * dA_b;
                    al_T = s;
                    }
                }
            const bool of_t = (unsigned int)c.p.type == a.type;
            if (of_t)
                {
                v_sum += v;
                count += 1.0;
                }
            else
                {
                t_i = v = 0.0;                                  // (a particle of another type owns no row: its moments are 0 and so is all of this)
                al_n = al_m = al_b = al_T = 0.0;
                }
            per_particle[TET_ROW_N * pitch + c.i] = n;
            per_particle[TET_ROW_T * pitch + c.i] = t_i;
            per_particle[TET_ROW_V * pitch + c.i] = v;
            double2 *row = reinterpret_cast<double2 *>(per_particle + TET_ROWS * pitch + TET_ALPHA * (size_t)c.i);
            row[0] = make_double2(al_n, al_m);
            row[1] = make_double2(al_b * mo[2], al_b * mo[3]);
            row[2] = make_double2(al_b * mo[4], al_T * mo[5]);
            row[3] = make_double2(al_T * mo[6], al_T * mo[7]);
            row[4] = make_double2(al_T * mo[8], al_T * mo[9]);
            row[5] = make_double2(al_T * mo[10], 0.0);
            }
        }
    const double v = block_sum(v_sum, s_red);
    if (tid == 0) part[blockIdx.x] = v;
    const double n = block_sum(count, s_red);
    if (tid == 0) part[TET_MAX_BLOCKS + blockIdx.x] = n;
    }

__global__ __launch_bounds__(MTD_WAVE) void k_tet_finalize(double *__restrict__ scratch)
    {
    if (threadIdx.x != 0) return;
    const double n_t = scratch[TET_OFF_SUMS + 1];
    scratch[TET_OFF_VALUE] = n_t > 0.0 ? scratch[TET_OFF_SUMS] / n_t : 0.0;
    scratch[TET_OFF_NT] = n_t;
    }

// ---- pass 2: the gather over row k --------------------------------------------------------------------------------------------------
// An entry (k, j) with d = minImage(r_j - r_k), u = d / r gives G = -g_kj(d) + g_jk(-d) to N_t ds/dr_k.  With
//     beta_n = alpha_n(k) + alpha_n(j)   beta_m = alpha_m(k) + alpha_m(j)   beta_b = alpha_b(k) - alpha_b(j)   beta_T = alpha_T(k) + alpha_T(j)
//     S = beta_b.u    Q = u.beta_T.u    V = beta_T u
//     G = -( u [ f' (beta_n + 2 f beta_m + S + Q) - (f / r) (S + 2 Q) ] + (f / r) (beta_b + 2 V) )
// The mirror entry (j, k) gives -G exactly.  F_k = -(bias / N_t) sum G, virial_k[ab] = (bias / (2 N_t)) sum G_a d_b.
template<typename S4, bool VIR>
__global__ __launch_bounds__(TET_THREADS) void k_tet_forces(const QlArgs<4> a_in, const S4 *__restrict__ postype,
                                                            const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                            const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                            const double *__restrict__ scratch, const size_t pitch, S4 *__restrict__ force,
                                                            const double *__restrict__ d_bias, const double bias_host,
                                                            typename scalar4_traits<S4>::scalar *__restrict__ virial, const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    const QlArgs<4> a = in_vgpr_window(a_in);
    const unsigned int tid = threadIdx.x, g = tid / TET_G, q = tid % TET_G;
    const unsigned int n_chunks = (a.N + TET_PPB - 1) / TET_PPB;
    const double2 *__restrict__ alpha = reinterpret_cast<const double2 *>(scratch + TET_OFF_PER_PARTICLE + TET_ROWS * pitch);
    const double n_t = scratch[TET_OFF_NT];
    const double bias = d_bias ? *d_bias : bias_host;
    const double scale = in_vgpr(n_t > 0.0 ? -bias / n_t : 0.0);
    // (the output pointers too: what is used once per particle need not hold scalar registers across the walk)
    asm volatile("" : "+v"(force));
    if constexpr (VIR) asm volatile("" : "+v"(virial));
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * TET_PPB + g);
        double2 ak[TET_ALPHA / 2];
#pragma unroll
        for (int u = 0; u < TET_ALPHA / 2; ++u) ak[u] = make_double2(0.0, 0.0);
        if (c.cnt)
            {
#pragma unroll
            for (int u = 0; u < TET_ALPHA / 2; ++u) ak[u] = alpha[(TET_ALPHA / 2) * (size_t)c.i + u];
            }
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        double vxx = 0.0, vxy = 0.0, vxz = 0.0, vyy = 0.0, vyz = 0.0, vzz = 0.0;
        row_walk_entries<TET_G, false, false>(a, postype, nlist, tab, c, q,
                                              [&](const double *tab_k, const unsigned int j, const double dx, const double dy, const double dz, const double rsq)
            {
            if (rsq > 0.0)
                {
                double2 aj[TET_ALPHA / 2];
#pragma unroll
                for (int u = 0; u < TET_ALPHA / 2; ++u) aj[u] = alpha[(TET_ALPHA / 2) * (size_t)j + u];   // (j < N: the walk skips every other entry)
                const double inv_r = rsqrt(rsq);
                double f, fprime_divr;
                smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
                const double ux = dx * inv_r, uy = dy * inv_r, uz = dz * inv_r;
                const double fp = fprime_divr * (rsq * inv_r), fr = f * inv_r;      // f' and f / r
                const double bn = ak[0].x + aj[0].x, bm = ak[0].y + aj[0].y;
                const double bx = ak[1].x - aj[1].x, by = ak[1].y - aj[1].y, bz = ak[2].x - aj[2].x;
                const double txx = ak[2].y + aj[2].y, txy = ak[3].x + aj[3].x, txz = ak[3].y + aj[3].y;
                const double tyy = ak[4].x + aj[4].x, tyz = ak[4].y + aj[4].y, tzz = ak[5].x + aj[5].x;
                const double Vx = txx * ux + txy * uy + txz * uz, Vy = txy * ux + tyy * uy + tyz * uz, Vz = txz * ux + tyz * uy + tzz * uz;
                const double S = bx * ux + by * uy + bz * uz, Q = Vx * ux + Vy * uy + Vz * uz;
                const double radial = fp * (bn + 2.0 * f * bm + S + Q) - fr * (S + 2.0 * Q);
                const double gx = -(radial * ux + fr * (bx + 2.0 * Vx));
                const double gy = -(radial * uy + fr * (by + 2.0 * Vy));
                const double gz = -(radial * uz + fr * (bz + 2.0 * Vz));
                Fx += gx;
                Fy += gy;
                Fz += gz;
                if constexpr (VIR)
                    {
                    vxx += gx * dx, vxy += gx * dy, vxz += gx * dz;
                    vyy += gy * dy, vyz += gy * dz, vzz += gz * dz;
                    }
                }
            });
        Fx = group_sum<TET_G>(Fx);
        Fy = group_sum<TET_G>(Fy);
        Fz = group_sum<TET_G>(Fz);
        if (q == 0 && c.i < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + c.i);
        if constexpr (VIR)
            {
            vxx = group_sum<TET_G>(vxx), vxy = group_sum<TET_G>(vxy), vxz = group_sum<TET_G>(vxz);
            vyy = group_sum<TET_G>(vyy), vyz = group_sum<TET_G>(vyz), vzz = group_sum<TET_G>(vzz);
            if (q == 0 && c.i < a.N) row_store_virial<false>(virial + c.i, virial_pitch, vxx, vxy, vxz, vyy, vyz, vzz, -0.5 * scale, 0.0);
            }
        }
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the checks every entry point shares, before a device is touched; everything invalid is refused ahead of what is merely not built
int tet_check(const mtd_tet_params *p, const mtd_tet_call *c)
    {
    if (!p || !c || !c->box || !c->d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (!(p->r_on >= 0.0) || !(p->r_on < p->r_cut) || !std::isfinite(p->r_cut)) return MTD_ERR_INVALID_ARGUMENT;
    if (!(p->cos0 >= -1.0) || !(p->cos0 <= 1.0)) return MTD_ERR_INVALID_ARGUMENT;
    if (p->switch_on && (!(p->c0 > 0.0) || !std::isfinite(p->c0) || p->p == 0)) return MTD_ERR_INVALID_ARGUMENT;
    if (p->gate_on && (!(p->n_lo >= 1.0) || !(p->n_lo < p->n_hi) || !std::isfinite(p->n_hi))) return MTD_ERR_INVALID_ARGUMENT;
    if (!p->normalise && (p->switch_on || p->gate_on)) return MTD_ERR_INVALID_ARGUMENT;   // they act on t_i, which the penalty does not form
    const int rc = refuse_row_arrays(c->n_particles, c->d_postype && c->d_head_list && c->d_n_neigh, c->dtype, c->d_scratch, nullptr, 0);
    if (rc) return rc;
    // alpha of a ghost would have to be exchanged
    if (c->n_ghost > 0) return MTD_ERR_UNSUPPORTED;
    return MTD_SUCCESS;
    }

// box, cut-off and window in the argument block of the Steinhardt passes
int tet_ql_args(QlArgs<4> &a, const mtd_tet_params *p, const mtd_tet_call *c)
    {
    static const double no_ref[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    return fill_args<4>(a, c->n_particles, c->box, p->r_cut, p->r_on, 0, p->type, no_ref, 1, 0);
    }

TetArgs tet_args(const mtd_tet_params *p)
    {
    TetArgs d;
    std::memset(&d, 0, sizeof(d));
    d.cos0 = p->cos0;
    d.kappa = 1.0 / (1.0 / 3.0 + p->cos0 * p->cos0);
    d.normalise = p->normalise ? 1 : 0;
    d.sw = p->switch_on ? 1 : 0;
    d.gate = p->gate_on ? 1 : 0;
    d.inv_c0 = d.sw ? 1.0 / p->c0 : 1.0;
    d.p = d.sw ? p->p : 1;
    d.n_lo = d.gate ? p->n_lo : 0.0;
    d.inv_dn = d.gate ? 1.0 / (p->n_hi - p->n_lo) : 0.0;
    return d;
    }

} // namespace

extern "C" {

size_t mtd_tet_scratch_doubles(unsigned int n_particles)
    {
    return TET_OFF_PER_PARTICLE + (TET_ROWS + TET_ALPHA) * row_pitch(n_particles);
    }

int mtd_tet_accumulate(const mtd_tet_params *p, const mtd_tet_call *c, double **d_sums, unsigned int *n_sums)
    {
    return mtd_tetrahedral_accumulate_cluster(p, c, nullptr, nullptr, d_sums, n_sums, nullptr, nullptr, nullptr);
    }

int mtd_tetrahedral_accumulate_cluster(const mtd_tet_params *p, const mtd_tet_call *c, const mtd_cluster_params *cluster,
                                       void *d_cluster_scratch, double **d_sums, unsigned int *n_sums, const double **d_w,
                                       const unsigned int **d_label, const unsigned int **d_summary)
    {
    if (!d_sums || !n_sums) return MTD_ERR_INVALID_ARGUMENT;
    int rc = tet_check(p, c);
    const bool masked = cluster_on(cluster);
    if (masked && (rc == MTD_SUCCESS || rc == MTD_ERR_UNSUPPORTED))
        {
        // what mtd_cluster_largest would refuse, refused here: before the first launch of this call, and ahead of what is merely not built
        if (cluster_refuse(cluster) != 0) return MTD_ERR_INVALID_ARGUMENT;
        if (!d_cluster_scratch || ((uintptr_t)d_cluster_scratch & 15u) != 0 || (c->n_particles && !c->d_nlist)) return MTD_ERR_INVALID_ARGUMENT;
        if (!p->normalise) return MTD_ERR_INVALID_ARGUMENT;          // A_i is a penalty, not an order: as a switch or a gate there
        }
    if (rc) return rc;
    QlArgs<4> a;
    rc = tet_ql_args(a, p, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)c->stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int blocks = row_blocks(c->n_particles, TET_PPB, TET_MAX_BLOCKS);
    double *part = c->d_scratch + TET_OFF_PART, *per_particle = c->d_scratch + TET_OFF_PER_PARTICLE;
    const size_t pitch = row_pitch(c->n_particles);
    const TetArgs d = tet_args(p);
    dispatch_s4(c->dtype, [&](auto t)
        {
        typedef typename decltype(t)::type S4;
        k_tet_accumulate<S4><<<blocks, TET_THREADS, 0, s>>>(a, d, (const S4 *)c->d_postype, c->d_head_list, c->d_n_neigh, c->d_nlist, tab, part,
                                                            per_particle, pitch);
        return 0;
        });
    MTD_LAUNCH_CHECK();
    const double *w = nullptr;
    const unsigned int *label = nullptr, *summary = nullptr;
    if (masked)
        {
        // the nodes are the particles of the type with v_i >= v_min; the mask of the largest cluster, then the adjoint rows and the
        // block sums masked with it
        const double *v = per_particle + TET_ROW_V * pitch;
        rc = mtd_cluster_largest(c->n_particles, c->d_postype, c->dtype, c->box, c->d_head_list, c->d_n_neigh, c->d_nlist, p->type, v, cluster,
                                 d_cluster_scratch, &label, nullptr, &w, &summary, c->stream);
        if (rc) return rc;
        row_mask(c->n_particles, blocks, TET_ALPHA, w, v, per_particle + TET_ROWS * pitch, part, s);
        MTD_LAUNCH_CHECK();
        }
    k_row_sums<TET_MAX_BLOCKS><<<2, MTD_WAVE, 0, s>>>(blocks, 2, 0, part, c->d_scratch + TET_OFF_SUMS);
    MTD_LAUNCH_CHECK();
    *d_sums = c->d_scratch + TET_OFF_SUMS;
    *n_sums = 2;
    if (d_w) *d_w = w;
    if (d_label) *d_label = label;
    if (d_summary) *d_summary = summary;
    return MTD_SUCCESS;
    }

int mtd_tet_finalize(const mtd_tet_params *p, const mtd_tet_call *c, const double **d_value, const double **d_local, const double **d_switched,
                     const double **d_coordination)
    {
    if (!d_value) return MTD_ERR_INVALID_ARGUMENT;
    const int rc = tet_check(p, c);
    if (rc) return rc;
    k_tet_finalize<<<1, MTD_WAVE, 0, (hipStream_t)c->stream>>>(c->d_scratch);
    MTD_LAUNCH_CHECK();
    const size_t pitch = row_pitch(c->n_particles);
    *d_value = c->d_scratch + TET_OFF_VALUE;
    if (d_local) *d_local = c->d_scratch + TET_OFF_PER_PARTICLE + TET_ROW_T * pitch;
    if (d_switched) *d_switched = c->d_scratch + TET_OFF_PER_PARTICLE + TET_ROW_V * pitch;
    if (d_coordination) *d_coordination = c->d_scratch + TET_OFF_PER_PARTICLE + TET_ROW_N * pitch;
    return MTD_SUCCESS;
    }

int mtd_tet_forces(const mtd_tet_params *p, const mtd_tet_call *c, void *d_force, const double *d_bias, double bias_host, void *d_virial,
                   unsigned int virial_pitch)
    {
    int rc = tet_check(p, c);
    if (rc) return rc;
    rc = refuse_row_arrays(c->n_particles, d_force != nullptr, c->dtype, c->d_scratch, d_virial, virial_pitch);
    if (rc) return rc;
    QlArgs<4> a;
    rc = tet_ql_args(a, p, c);
    if (rc) return rc;
    if (c->n_particles == 0) return MTD_SUCCESS;
    hipStream_t s = (hipStream_t)c->stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int blocks = row_blocks(c->n_particles, TET_PPB, TET_MAX_BLOCKS);
    const size_t pitch = row_pitch(c->n_particles);
    dispatch_s4(c->dtype, [&](auto t)
        {
        return dispatch_bool(d_virial != nullptr, [&](auto vir)
            {
            typedef typename decltype(t)::type S4;
            typedef typename scalar4_traits<S4>::scalar scalar;
            k_tet_forces<S4, decltype(vir)::value><<<blocks, TET_THREADS, 0, s>>>(a, (const S4 *)c->d_postype, c->d_head_list, c->d_n_neigh, c->d_nlist,
                                                                                  tab, c->d_scratch, pitch, (S4 *)d_force, d_bias, bias_host,
                                                                                  (scalar *)d_virial, virial_pitch);
            return 0;
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // extern "C"
