// coordination.hip — coordination number of the particles of one type by those of another through a rational switching function
// (cv.coordination) on gfx950.
//
// No reference counterpart (PLUMED's COORDINATION / COORDINATIONNUMBER).  Definition, gradient and virial: include/mtd_abi.h
// "Coordination number"; restated in fp64 numpy in tests/coordination_ref.py.  In short, over the entries (i, j) of a FULL list with
// j != i and r = |minImage(r_i - r_j)| <= r_cut:
//     x = max(r - d_0, 0) / r_0      s = P_n(x) / P_m(x), P_k = 1 + x + ... + x^(k-1)      s~ = (s - s_c) / (1 - s_c)
//     n_i = sum_{j of type B} s~(r_ij) for i of type A      v_i = g(n_i)      s = (1 / N_A) sum_i v_i
//     ds/dr_k = (1 / N_A) sum_{j in row k} s~' d / r ( [k in A, j in B] g'(n_k) + [k in B, j in A] g'(n_j) )
// The slope of s~ at r_cut is not zero: THE FORCE IS DISCONTINUOUS AT r_cut by |s'(r_cut)| / (1 - s_c) / N_A per entry.
// Minimum image and particle loads are those of the Steinhardt units (QlArgs<4>, min_image); the walk over a row is the two-type form
// of row_walk.hpp (row_centre_pairs, row_walk_pairs), the group's sum and the store of the virial are that header's; launches and the
// shared refusals go through dispatch.hpp.
//
// MI355X design.  All arithmetic in fp64 over fp32 or fp64 arrays.
//   lanes            EIGHT lanes per central particle, 32 central particles per block and round, as in debye.hip
//   the pair term    ONE rsqrt, ONE reciprocal (cn_rcp: the hardware's estimate and two Newton steps, the sums are >= 1) and 2 (m - 1)
//                    fused multiply-adds per entry, no pow, no division, no transcendental function: P_k and P_k' by Horner's rule in
//                    one loop (every coefficient is 1, so the value after k - 1 steps IS P_k: P_n and P_n' are read off on the way to
//                    P_m), then s = P_n / P_m and s' = (P_n' - s P_m') / P_m.  All terms are positive: nothing cancels at x = 1, where
//                    the quotient (1 - x^n) / (1 - x^m) is 0 / 0.  n and m are wave-uniform: the loop is a scalar one.  An entry with
//                    r <= d_0 (r = 0 among them) counts 1 and has no gradient
//   instantiations   DEFAULT_PAIR: (n, m) = (6, 12) compiled as 1 / (1 + x^6), an identity for m = 2 n, x^6 by squaring: five
//                    multiplications and the reciprocal in place of 22 multiply-adds and their loop.  mtd_coord_set_compiled_pair(0)
//                    sends (6, 12) through the general loop for the A/B; profiles/r25/README.md has both timings
//   k_cn_walk        the one kernel over the rows, in three modes:
//                      CN_PLAIN   mtd_coord_accumulate without a switch: n_i = v_i, the particle's gradient sum and its six virial sums
//                                 into the scratch, unscaled (N_A and the bias are not known yet): Debye's stored route
//                      CN_COUNT   mtd_coord_accumulate with a switch: n_i, v_i = g(n_i) and g'(n_i) into the scratch
//                      CN_FORCE   mtd_coord_forces with a switch: the second walk, g'(n_j) read from the per-particle table; force and
//                                 (with VIR) virial scaled and stored
//                    PLAIN and COUNT leave this block's share of sum v_i and N_A
//   k_row_scale      (row_scale.hpp) mtd_coord_forces without a switch: one thread per particle scales the stored sums by -bias / N_A
//                    and -bias / (2 N_A)
//   k_row_mask       (row_mask.hpp) mtd_coord_accumulate_cluster: between the CN_COUNT walk and k_row_sums, after the cluster pass of
//                    cluster.hip on the v_i just written — g'(n_i) of every particle outside the largest cluster set to 0, the block
//                    sums of slot 0 replaced by those of w_i v_i.  CN_FORCE then runs unchanged on the masked table
//   k_row_sums       (row_walk.hpp) one wave per slot adds the blocks' doubles in the fixed order of wave_sum
//   k_cn_finalize    s from the (reduced) sums
// Fixed summation order everywhere (a lane's entries in row order, the DPP tree of group_sum, a thread's chunks in order, block_sum,
// wave_sum), no atomics: two identical calls give identical bits, and a row gives the same bits wherever it lies in the list.
#include "mtd_device.hpp"
#include "row_scale.hpp"
#include "row_mask.hpp"
#include "cluster_host.hpp"

#include <atomic>
#include <cmath>
#include <cstring>

namespace
{

using namespace mtd;

constexpr int CN_THREADS = 256;
constexpr int CN_G = 8;                                    // lanes per central particle
constexpr int CN_PPB = CN_THREADS / CN_G;                  // central particles per block and round
constexpr unsigned int CN_MAX_BLOCKS = ROW_MAX_BLOCKS;     // columns of block sums in the scratch

// the scratch, in doubles: sums [2] | value, N_A [2] | (pad) | block sums [2][CN_MAX_BLOCKS]
// | n_i [n] | v_i [n] | g'(n_i) [n] | gradient sums [3][n] | virial sums [6][n], n = n_particles rounded up to 2
constexpr size_t CN_OFF_SUMS = 0, CN_OFF_VALUE = 2, CN_OFF_NA = 3, CN_OFF_PART = 16, CN_OFF_PER_PARTICLE = CN_OFF_PART + 2 * (size_t)CN_MAX_BLOCKS;
constexpr int CN_ROW_N = 0, CN_ROW_V = 1, CN_ROW_DG = 2, CN_ROW_GRAD = 3, CN_ROWS = 12;   // (the six virial rows follow the gradient's)

enum { CN_PLAIN = 0, CN_COUNT = 1, CN_FORCE = 2 };

struct CnArgs
    {
    double d0, inv_r0;
    double s_c, inv_one_minus_sc;                          // the stretch: s~ = (s - s_c) / (1 - s_c)
    double inv_c0;
    unsigned int type_a, type_b;
    unsigned int n, m, p;
    int less;
    };

// 1 / p for p >= 1 (a sum of non-negative powers that begins with 1: no zero, no denormal, no infinity short of x^31 overflowing, which
// r_cut / r_0 does not allow): the hardware's estimate and two Newton steps, five instructions in place of the division's eleven; the
// host (s_c) divides
__host__ __device__ __forceinline__ double cn_rcp(const double p)
    {
#if defined(__HIP_DEVICE_COMPILE__)
    double y = __builtin_amdgcn_rcp(p);
    y = fma(fma(-p, y, 1.0), y, y);
    return fma(fma(-p, y, 1.0), y, y);
#else
    return 1.0 / p;
#endif
    }

// P_k(x) = 1 + x + ... + x^(k-1) and P_k'(x) for k = n and k = m in ONE Horner loop -> s = P_n / P_m and ds/dx
__host__ __device__ __forceinline__ void cn_rational(const double x, const unsigned int n, const unsigned int m, double &s, double &ds)
    {
    double p = 1.0, dp = 0.0;
    for (unsigned int k = 1; k < n; ++k)
        {
        dp = dp * x + p;
        p = p * x + 1.0;
        }
    const double pn = p, dpn = dp;
    for (unsigned int k = n; k < m; ++k)
        {
        dp = dp * x + p;
        p = p * x + 1.0;
        }
    const double inv = cn_rcp(p);
    s = pn * inv;
    ds = (dpn - s * dp) * inv;
    }

// the default pair (6, 12), compiled: with m = 2 n the quotient of the sums IS 1 / (1 + x^n) — an identity, P_2n = P_n (1 + x^n) — which
// has nothing to cancel at x = 1 either; x^6 by squaring, s' = -6 x^5 s^2
__device__ __forceinline__ void cn_rational_6_12(const double x, double &s, double &ds)
    {
    const double x2 = x * x, x3 = x2 * x;
    s = cn_rcp(1.0 + x3 * x3);
    ds = -6.0 * (x3 * x2) * (s * s);
    }

__device__ __forceinline__ double cn_powi(double x, unsigned int n)
    {
    double r = 1.0;
    for (; n; n >>= 1)
        {
        if (n & 1u) r *= x;
        x *= x;
        }
    return r;
    }

// ---- the walk over the rows ------------------------------------------------------------------------------------------------------
template<typename S4, int MODE, bool VIR, bool DEFAULT_PAIR>
__global__ __launch_bounds__(CN_THREADS) void k_cn_walk(const QlArgs<4> a_in, const CnArgs d, const S4 *__restrict__ postype,
                                                        const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                        const unsigned int *__restrict__ nlist, double *__restrict__ part,
                                                        double *__restrict__ per_particle, const size_t pitch, S4 *__restrict__ force,
                                                        const double *__restrict__ scratch, const double *__restrict__ d_bias,
                                                        const double bias_host, typename scalar4_traits<S4>::scalar *__restrict__ virial,
                                                        const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    constexpr bool SUMS = MODE != CN_FORCE, GRAD = MODE != CN_COUNT;
    __shared__ double s_red[16];
    const QlArgs<4> a = in_vgpr(a_in);
    const double d0 = in_vgpr(d.d0), inv_r0 = in_vgpr(d.inv_r0), s_c = in_vgpr(d.s_c), stretch = in_vgpr(d.inv_one_minus_sc);
    const unsigned int tid = threadIdx.x, g = tid / CN_G, q = tid % CN_G;
    const unsigned int n_chunks = (a.N + CN_PPB - 1) / CN_PPB;
    const double *__restrict__ dg = per_particle + CN_ROW_DG * pitch;   // g'(n_j) of the local particles (CN_FORCE)
    double scale_f = 0.0, scale_v = 0.0;
    if constexpr (MODE == CN_FORCE)
        {
        const double n_a = scratch[CN_OFF_NA];
        const double bias = d_bias ? *d_bias : bias_host;
        scale_f = n_a > 0.0 ? -bias / n_a : 0.0;
        scale_v = n_a > 0.0 ? -0.5 * bias / n_a : 0.0;
        }
    double v_sum = 0.0, count = 0.0;                       // lane 0 of a group: sum v_i and the centres of type A over its chunks
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre_pairs(a, d.type_a, d.type_b, postype, head_list, n_neigh, chunk * CN_PPB + g);
        const bool of_a = c.i < a.N && (unsigned int)c.p.type == d.type_a;
        double dg_own = 0.0;
        if constexpr (MODE == CN_FORCE) dg_own = c.own(a.N, dg);
        double n_row = 0.0;                                // this lane's share of n_i
        double Gx = 0.0, Gy = 0.0, Gz = 0.0;
        double vxx = 0.0, vxy = 0.0, vxz = 0.0, vyy = 0.0, vyz = 0.0, vzz = 0.0;
        row_walk_pairs<CN_G>(a, d.type_a, d.type_b, postype, nlist, c, q,
                             [&](const unsigned int j, const bool as_centre, const bool as_partner, const double dx, const double dy,
                                 const double dz, const double rsq)
            {
            const double inv_r = rsqrt(rsq), r = rsq > 0.0 ? rsq * inv_r : 0.0;
            const double over = r - d0;
            double st = 1.0;                               // s~ inside d_0 (two particles in one place among them): 1, no gradient
            if (over > 0.0)
                {
                double s, ds;
                if constexpr (DEFAULT_PAIR)
                    cn_rational_6_12(over * inv_r0, s, ds);
                else
                    cn_rational(over * inv_r0, d.n, d.m, s, ds);
                st = (s - s_c) * stretch;
                if constexpr (GRAD)
                    {
                    double w;                              // g'(n_i) of the end(s) this entry counts for
                    if constexpr (MODE == CN_FORCE)
                        w = (as_centre ? dg_own : 0.0) + (as_partner && j < a.N ? dg[j] : 0.0);
                    else
                        w = (as_centre ? 1.0 : 0.0) + (as_partner ? 1.0 : 0.0);
                    const double t = ds * (inv_r0 * stretch) * inv_r * w;   // s~' / r times the bracket
                    const double gx = t * dx, gy = t * dy, gz = t * dz;
                    Gx += gx;
                    Gy += gy;
                    Gz += gz;
                    if constexpr (VIR)
                        {
                        vxx += dx * gx, vxy += dx * gy, vxz += dx * gz;
                        vyy += dy * gy, vyz += dy * gz, vzz += dz * gz;
                        }
                    }
                }
            if constexpr (SUMS) n_row += as_centre ? st : 0.0;
            });
        if constexpr (SUMS)
            {
            n_row = group_sum<CN_G>(n_row);
            if (q == 0 && c.i < a.N)
                {
                double n_i = 0.0, v = 0.0, dv = 0.0;
                if (of_a)
                    {
                    n_i = v = n_row;
                    dv = 1.0;
                    if constexpr (MODE == CN_COUNT)
                        {
                        const double y = n_i * d.inv_c0, ypm1 = cn_powi(y, d.p - 1), yp = ypm1 * y, den = 1.0 / (1.0 + yp);
                        v = yp * den;
                        dv = (double)d.p * ypm1 * d.inv_c0 * den * den;
                        if (d.less) v = 1.0 - v, dv = -dv;
                        }
                    v_sum += v;
                    count += 1.0;
                    }
                per_particle[CN_ROW_N * pitch + c.i] = n_i;
                per_particle[CN_ROW_V * pitch + c.i] = v;
                per_particle[CN_ROW_DG * pitch + c.i] = dv;
                }
            }
        if constexpr (GRAD)
            {
            Gx = group_sum<CN_G>(Gx);
            Gy = group_sum<CN_G>(Gy);
            Gz = group_sum<CN_G>(Gz);
            if constexpr (VIR)
                {
                vxx = group_sum<CN_G>(vxx), vxy = group_sum<CN_G>(vxy), vxz = group_sum<CN_G>(vxz);
                vyy = group_sum<CN_G>(vyy), vyz = group_sum<CN_G>(vyz), vzz = group_sum<CN_G>(vzz);
                }
            if (q == 0 && c.i < a.N)
                {
                if constexpr (MODE == CN_PLAIN)
                    {
                    double *o = per_particle + CN_ROW_GRAD * pitch + c.i;
                    o[0] = Gx, o[pitch] = Gy, o[2 * pitch] = Gz;
                    o[3 * pitch] = vxx, o[4 * pitch] = vxy, o[5 * pitch] = vxz;
                    o[6 * pitch] = vyy, o[7 * pitch] = vyz, o[8 * pitch] = vzz;
                    }
                else
                    {
                    nt_store(scalar4_traits<S4>::make((scalar)(Gx * scale_f), (scalar)(Gy * scale_f), (scalar)(Gz * scale_f), (scalar)0), force + c.i);
                    if constexpr (VIR) row_store_virial<false>(virial + c.i, virial_pitch, vxx, vxy, vxz, vyy, vyz, vzz, scale_v, 0.0);
                    }
                }
            }
        }
    if constexpr (SUMS)
        {
        const double v = block_sum(v_sum, s_red);
        if (tid == 0) part[blockIdx.x] = v;
        const double n = block_sum(count, s_red);
        if (tid == 0) part[CN_MAX_BLOCKS + blockIdx.x] = n;
        }
    }

__global__ __launch_bounds__(MTD_WAVE) void k_cn_finalize(double *__restrict__ scratch)
    {
    if (threadIdx.x != 0) return;
    const double n_a = scratch[CN_OFF_SUMS + 1];
    scratch[CN_OFF_VALUE] = n_a > 0.0 ? scratch[CN_OFF_SUMS] / n_a : 0.0;
    scratch[CN_OFF_NA] = n_a;
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------
std::atomic<int> g_compiled_pair{1};

// (n, m) = (6, 12) takes the compiled pair term unless mtd_coord_set_compiled_pair(0) says otherwise
bool cn_default_pair(const mtd_coord_params *p) { return p->n == 6 && p->m == 12 && g_compiled_pair.load() != 0; }

// the checks every entry point shares, before a device is touched; everything invalid is refused ahead of what is merely not built
int cn_check(const mtd_coord_params *p, const mtd_coord_call *c)
    {
    if (!p || !c || !c->box || !c->d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (!(p->r_0 > 0.0) || !std::isfinite(p->r_0) || !(p->d_0 >= 0.0) || !std::isfinite(p->d_0)) return MTD_ERR_INVALID_ARGUMENT;
    if (!(p->r_cut > p->d_0) || !std::isfinite(p->r_cut)) return MTD_ERR_INVALID_ARGUMENT;
    if (p->n == 0 || p->n >= p->m) return MTD_ERR_INVALID_ARGUMENT;
    if (p->switch_on && (!(p->c0 > 0.0) || !std::isfinite(p->c0) || p->p == 0)) return MTD_ERR_INVALID_ARGUMENT;
    const int rc = refuse_row_arrays(c->n_particles, c->d_postype && c->d_head_list && c->d_n_neigh, c->dtype, c->d_scratch, nullptr, 0);
    if (rc) return rc;
    if (p->m > MTD_COORD_MAX_M) return MTD_ERR_UNSUPPORTED;
    // g'(n_j) of a ghost would have to be exchanged
    if (p->switch_on && c->n_ghost > 0) return MTD_ERR_UNSUPPORTED;
    return MTD_SUCCESS;
    }

// box and cut-off in the argument block of the Steinhardt passes (no smoothing window: r_on is not read; `type` is A)
int cn_ql_args(QlArgs<4> &a, const mtd_coord_params *p, const mtd_coord_call *c)
    {
    static const double no_ref[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    return fill_args<4>(a, c->n_particles, c->box, p->r_cut, 0.0, 0, p->type_a, no_ref, 1, 0);
    }

CnArgs cn_args(const mtd_coord_params *p)
    {
    CnArgs d;
    std::memset(&d, 0, sizeof(d));
    d.d0 = p->d_0;
    d.inv_r0 = 1.0 / p->r_0;
    double ds;
    cn_rational((p->r_cut - p->d_0) / p->r_0, p->n, p->m, d.s_c, ds);
    d.inv_one_minus_sc = 1.0 / (1.0 - d.s_c);
    d.inv_c0 = p->switch_on ? 1.0 / p->c0 : 1.0;
    d.type_a = p->type_a, d.type_b = p->type_b;
    d.n = p->n, d.m = p->m;
    d.p = p->switch_on ? p->p : 1;
    d.less = p->switch_on && p->less ? 1 : 0;
    return d;
    }

} // namespace

extern "C" {

size_t mtd_coord_scratch_doubles(unsigned int n_particles)
    {
    return CN_OFF_PER_PARTICLE + CN_ROWS * row_pitch(n_particles);
    }

int mtd_coord_set_compiled_pair(int enable)
    {
    g_compiled_pair.store(enable ? 1 : 0);
    return MTD_SUCCESS;
    }

int mtd_coord_accumulate(const mtd_coord_params *p, const mtd_coord_call *c, double **d_sums, unsigned int *n_sums)
    {
    return mtd_coord_accumulate_cluster(p, c, nullptr, nullptr, d_sums, n_sums, nullptr, nullptr, nullptr);
    }

int mtd_coord_accumulate_cluster(const mtd_coord_params *p, const mtd_coord_call *c, const mtd_cluster_params *cluster, void *d_cluster_scratch,
                                 double **d_sums, unsigned int *n_sums, const double **d_w, const unsigned int **d_label,
                                 const unsigned int **d_summary)
    {
    if (!d_sums || !n_sums) return MTD_ERR_INVALID_ARGUMENT;
    int rc = cn_check(p, c);
    const bool masked = cluster_on(cluster);
    if (masked && (rc == MTD_SUCCESS || rc == MTD_ERR_UNSUPPORTED))
        {
        // what mtd_cluster_largest would refuse, refused here: before the first launch of this call, and ahead of what is merely not built
        if (cluster_refuse(cluster) != 0) return MTD_ERR_INVALID_ARGUMENT;
        if (!d_cluster_scratch || ((uintptr_t)d_cluster_scratch & 15u) != 0 || (c->n_particles && !c->d_nlist)) return MTD_ERR_INVALID_ARGUMENT;
        }
    if (rc) return rc;
    if (masked)
        {
        // the plain route stores summed gradients, which cannot be masked afterwards; g'(n_j) of a ghost is not known (cn_check, with a switch)
        if (!p->switch_on || c->n_ghost > 0) return MTD_ERR_UNSUPPORTED;
        }
    QlArgs<4> a;
    rc = cn_ql_args(a, p, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)c->stream;
    const unsigned int blocks = row_blocks(c->n_particles, CN_PPB, CN_MAX_BLOCKS);
    double *part = c->d_scratch + CN_OFF_PART, *per_particle = c->d_scratch + CN_OFF_PER_PARTICLE;
    const size_t pitch = row_pitch(c->n_particles);
    const CnArgs d = cn_args(p);
    dispatch_s4(c->dtype, [&](auto t)
        {
        return dispatch_bool(p->switch_on != 0, [&](auto sw)
            {
            return dispatch_bool(cn_default_pair(p), [&](auto dp)
                {
                typedef typename decltype(t)::type S4;
                constexpr bool SW = decltype(sw)::value;
                k_cn_walk<S4, SW ? CN_COUNT : CN_PLAIN, !SW, decltype(dp)::value><<<blocks, CN_THREADS, 0, s>>>(
                    a, d, (const S4 *)c->d_postype, c->d_head_list, c->d_n_neigh, c->d_nlist, part, per_particle, pitch, nullptr, nullptr, nullptr,
                    0.0, nullptr, 0);
                return 0;
                });
            });
        });
    MTD_LAUNCH_CHECK();
    const double *w = nullptr;
    const unsigned int *label = nullptr, *summary = nullptr;
    if (masked)
        {
        // the nodes are the A particles with v_i >= v_min; the mask of the largest cluster, then g'(n_i) and the block sums masked with it
        const double *v = per_particle + CN_ROW_V * pitch;
        rc = mtd_cluster_largest(c->n_particles, c->d_postype, c->dtype, c->box, c->d_head_list, c->d_n_neigh, c->d_nlist, p->type_a, v, cluster,
                                 d_cluster_scratch, &label, nullptr, &w, &summary, c->stream);
        if (rc) return rc;
        row_mask(c->n_particles, blocks, 1, w, v, per_particle + CN_ROW_DG * pitch, part, s);
        MTD_LAUNCH_CHECK();
        }
    k_row_sums<CN_MAX_BLOCKS><<<2, MTD_WAVE, 0, s>>>(blocks, 2, 0, part, c->d_scratch + CN_OFF_SUMS);
    MTD_LAUNCH_CHECK();
    *d_sums = c->d_scratch + CN_OFF_SUMS;
    *n_sums = 2;
    if (d_w) *d_w = w;
    if (d_label) *d_label = label;
    if (d_summary) *d_summary = summary;
    return MTD_SUCCESS;
    }

int mtd_coord_finalize(const mtd_coord_params *p, const mtd_coord_call *c, const double **d_value, const double **d_local,
                       const double **d_switched)
    {
    if (!d_value) return MTD_ERR_INVALID_ARGUMENT;
    const int rc = cn_check(p, c);
    if (rc) return rc;
    k_cn_finalize<<<1, MTD_WAVE, 0, (hipStream_t)c->stream>>>(c->d_scratch);
    MTD_LAUNCH_CHECK();
    const size_t pitch = row_pitch(c->n_particles);
    *d_value = c->d_scratch + CN_OFF_VALUE;
    if (d_local) *d_local = c->d_scratch + CN_OFF_PER_PARTICLE + CN_ROW_N * pitch;
    if (d_switched) *d_switched = c->d_scratch + CN_OFF_PER_PARTICLE + CN_ROW_V * pitch;
    return MTD_SUCCESS;
    }

int mtd_coord_forces(const mtd_coord_params *p, const mtd_coord_call *c, void *d_force, const double *d_bias, double bias_host, void *d_virial,
                     unsigned int virial_pitch)
    {
    int rc = cn_check(p, c);
    if (rc) return rc;
    rc = refuse_row_arrays(c->n_particles, d_force != nullptr, c->dtype, c->d_scratch, d_virial, virial_pitch);
    if (rc) return rc;
    QlArgs<4> a;
    rc = cn_ql_args(a, p, c);
    if (rc) return rc;
    if (c->n_particles == 0) return MTD_SUCCESS;
    hipStream_t s = (hipStream_t)c->stream;
    const size_t pitch = row_pitch(c->n_particles);
    if (!p->switch_on)
        {
        row_scale(c->dtype, c->n_particles, c->d_scratch + CN_OFF_PER_PARTICLE + CN_ROW_GRAD * pitch, pitch, c->d_scratch + CN_OFF_NA, 0.0, -1.0, -0.5,
                  d_force, d_bias, bias_host, d_virial, virial_pitch, s);
        MTD_LAUNCH_CHECK();
        return MTD_SUCCESS;
        }
    const unsigned int blocks = row_blocks(c->n_particles, CN_PPB, CN_MAX_BLOCKS);
    const CnArgs d = cn_args(p);
    dispatch_s4(c->dtype, [&](auto t)
        {
        return dispatch_bool(d_virial != nullptr, [&](auto vir)
            {
            return dispatch_bool(cn_default_pair(p), [&](auto dp)
                {
                typedef typename decltype(t)::type S4;
                typedef typename scalar4_traits<S4>::scalar scalar;
                k_cn_walk<S4, CN_FORCE, decltype(vir)::value, decltype(dp)::value><<<blocks, CN_THREADS, 0, s>>>(
                    a, d, (const S4 *)c->d_postype, c->d_head_list, c->d_n_neigh, c->d_nlist, nullptr, c->d_scratch + CN_OFF_PER_PARTICLE, pitch,
                    (S4 *)d_force, c->d_scratch, d_bias, bias_host, (scalar *)d_virial, virial_pitch);
                return 0;
                });
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // extern "C"
