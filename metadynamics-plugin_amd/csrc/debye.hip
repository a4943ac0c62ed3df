// debye.hip — intensities of diffraction peaks from the Debye scattering function (cv.debye_structure_factor) on gfx950.
//
// No reference counterpart (Niu, Piaggi, Invernizzi and Parrinello, PNAS 115, 5348 (2018)).  Definition, gradient and virial:
// include/mtd_abi.h "Debye structure factor"; restated in fp64 numpy in tests/debye_ref.py.  In short, over the entries (i, j) of a FULL
// list with both particles of `type`, j != i and r = |minImage(r_i - r_j)| <= r_cut:
//     w = sin x / x, x = pi r / r_cut        phi_p = w sin(Q_p r) / (Q_p r)        A_p = sum phi_p        I_p = 1 + A_p / N_t
//     s = sum_p c_p I_p        u = sum_p c_p phi_p'        ds/dr_k = (2 / N_t) sum_{j in row k} u d / r
// The window is the published one: w(r_cut) = 0 but w'(r_cut) = -1 / r_cut, so THE FORCE IS DISCONTINUOUS AT r_cut by
// sinc(Q_p r_cut) / r_cut per entry and peak, divided by N_t.  It is kept as published.
// Minimum image, particle loads and the type test are those of the Steinhardt units (QlArgs<4>, min_image); the walk over a row, its
// centre, the group's sum and the store of the virial are those of row_walk.hpp (the smoothing table is not read: the pointer handed to
// the walk is null); launches and the shared refusals go through dispatch.hpp.
//
// MI355X design.  All arithmetic in fp64 over fp32 or fp64 arrays.
//   lanes            EIGHT lanes per central particle, 32 central particles per block and round, as in pair_entropy.hip
//   the pair term    ONE rsqrt and P + 1 sine/cosine pairs per entry (dsf_sincos of debye_device.hpp: bounded arguments, no table, no
//                    branch), no division: with 1 / r in hand, sin x / x = sin x (r_cut / pi) / r and sin y / y = sin y / (Q_p r), and
//                    the derivatives collapse to  w' = (cos x - w) / r,  (sin y / y)' = (cos y - sin y / y) / r,  so
//                    phi_p' = [ (cos x - w) j_p + w (cos y_p - j_p) ] / r  with j_p = sin y_p / y_p
//   instantiations   the peaks are unrolled for P = 1, 2, 4, 8; a count between takes the next one with its last slots switched off
//                    (weight 0, the first wave number: their sums are formed and never read).  Q_p, 1 / Q_p and c_p live in vector
//                    registers beside the box (in_vgpr of row_walk.hpp): 24 doubles at P = 8 do not fit the scalar file beside it
//   k_dsf_walk       the one kernel over the rows.  SUMS: this block's share of A_p and N_t and every particle's s_i.  GRAD: the
//                    particle's gradient sum u d / r, and with VIR its six sums d_a u d_b / r.  STORE says where they go:
//                      <SUMS, GRAD, VIR, STORE> = <1, 1, 1, 1>   mtd_dsf_accumulate by default: nine doubles per particle into the scratch,
//                                                               unscaled (N_t and the bias are not known yet)
//                      <1, 0, 0, 0>                             mtd_dsf_accumulate after mtd_dsf_set_store_gradient(0)
//                      <0, 1, VIR, 0>                           mtd_dsf_forces after the same: a second walk, force and virial scaled
//   k_row_scale      (row_scale.hpp) mtd_dsf_forces by default: one thread per particle scales the stored sums by -2 bias / N_t and
//                    -bias / N_t
//   Storing wins because the second walk repeats every sine and cosine: profiles/r24/README.md has both timings.
//   k_row_sums       (row_walk.hpp) one wave per slot adds the blocks' doubles in the fixed order of wave_sum
//   k_dsf_finalize   I_p and s from the (reduced) sums
//   k_dsf_spectrum   the diagnostic.  blockIdx.y takes EIGHT consecutive Q_m; per entry the window, sin and cos of Q_m0 r and of
//                    dQ r, then seven angle additions (at most seven steps from a directly evaluated pair: the recurrence adds
//                    ~1e-16 per step).  It sums T_m = w sin(Q_m r) / r; the division by Q_m is made once, in the finalize.
// Fixed summation order everywhere (a lane's entries in row order, the DPP tree of group_sum, a thread's chunks in order, block_sum,
// wave_sum), no atomics: two identical calls give identical bits, and a row gives the same bits wherever it lies in the list.
#include "mtd_device.hpp"
#include "row_scale.hpp"
#include "debye_device.hpp"

#include <atomic>
#include <cmath>
#include <cstring>

namespace
{

using namespace mtd;

constexpr int DSF_THREADS = 256;
constexpr int DSF_G = 8;                                   // lanes per central particle
constexpr int DSF_PPB = DSF_THREADS / DSF_G;               // central particles per block and round
constexpr unsigned int DSF_MAX_BLOCKS = ROW_MAX_BLOCKS;    // columns of block sums in the scratch
constexpr int DSF_TILE = 8;                                // wave numbers of the spectrum per block row

// the scratch, in doubles: sums [16] | value, N_t [2] | I_p [8] | (pad) | spectrum sums [258] | spectrum [256] | block sums [257][DSF_MAX_BLOCKS]
// | s_i [n] | gradient sums [3][n] | virial sums [6][n], n = n_particles rounded up to 2
constexpr size_t DSF_OFF_SUMS = 0, DSF_OFF_VALUE = 16, DSF_OFF_NT = 17, DSF_OFF_I = 18, DSF_OFF_SPEC_SUMS = 32,
                 DSF_OFF_SPEC = DSF_OFF_SPEC_SUMS + MTD_DSF_MAX_SPECTRUM + 2, DSF_OFF_PART = DSF_OFF_SPEC + MTD_DSF_MAX_SPECTRUM,
                 DSF_OFF_PER_PARTICLE = DSF_OFF_PART + (size_t)(MTD_DSF_MAX_SPECTRUM + 1) * DSF_MAX_BLOCKS;

template<int P> struct DsfArgs
    {
    double q[P], inv_q[P], c[P];
    double pi_over_rc, rc_over_pi;
    double c_sum;                                          // sum_p c_p: s_i of a particle without a neighbour
    };

template<int P> __device__ __forceinline__ DsfArgs<P> dsf_in_vgpr(DsfArgs<P> d)
    {
#pragma unroll
    for (int p = 0; p < P; ++p) d.q[p] = in_vgpr(d.q[p]), d.inv_q[p] = in_vgpr(d.inv_q[p]), d.c[p] = in_vgpr(d.c[p]);
    d.pi_over_rc = in_vgpr(d.pi_over_rc), d.rc_over_pi = in_vgpr(d.rc_over_pi);
    return d;
    }

// ---- the walk over the rows ------------------------------------------------------------------------------------------------------
template<typename S4, int P, bool SUMS, bool GRAD, bool VIR, bool STORE>
__global__ __launch_bounds__(DSF_THREADS) void k_dsf_walk(const QlArgs<4> a_in, const DsfArgs<P> d_in, const S4 *__restrict__ postype,
                                                          const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                          const unsigned int *__restrict__ nlist, double *__restrict__ part,
                                                          double *__restrict__ per_particle, const size_t pitch, S4 *__restrict__ force,
                                                          const double *__restrict__ scratch, const double *__restrict__ d_bias,
                                                          const double bias_host, typename scalar4_traits<S4>::scalar *__restrict__ virial,
                                                          const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    __shared__ double s_red[16];
    const QlArgs<4> a = in_vgpr(a_in);
    const DsfArgs<P> d = dsf_in_vgpr(d_in);
    const unsigned int tid = threadIdx.x, g = tid / DSF_G, q = tid % DSF_G;
    const unsigned int n_chunks = (a.N + DSF_PPB - 1) / DSF_PPB;
    double scale_f = 0.0, scale_v = 0.0;
    if constexpr (GRAD && !STORE)
        {
        const double n_t = scratch[DSF_OFF_NT];
        const double bias = d_bias ? *d_bias : bias_host;
        scale_f = n_t > 0.0 ? -2.0 * bias / n_t : 0.0;
        scale_v = n_t > 0.0 ? -bias / n_t : 0.0;
        }
    double A[P], count = 0.0;                              // this thread's share of A_p over its chunks; the centres of the type (lane 0)
#pragma unroll
    for (int p = 0; p < P; ++p) A[p] = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * DSF_PPB + g);
        const bool of_type = c.i < a.N && (unsigned int)c.p.type == a.type;
        double row[P];                                     // this lane's share of sum_j phi_p
#pragma unroll
        for (int p = 0; p < P; ++p) row[p] = 0.0;
        double Gx = 0.0, Gy = 0.0, Gz = 0.0;
        double vxx = 0.0, vxy = 0.0, vxz = 0.0, vyy = 0.0, vyz = 0.0, vzz = 0.0;
        row_walk<DSF_G, true>(a, postype, nlist, (const double *)nullptr, c, q,
                              [&](const double *, const unsigned int, const double dx, const double dy, const double dz, const double rsq)
            {
            if (rsq > 0.0)
                {
                const double inv_r = rsqrt(rsq), r = rsq * inv_r;
                double w, cx;
                dsf_window(r, inv_r, d.pi_over_rc, d.rc_over_pi, w, cx);
                const double dw = cx - w;                  // r w'
                double u = 0.0;                            // r sum_p c_p phi_p'
#pragma unroll
                for (int p = 0; p < P; ++p)
                    {
                    double sy, cy;
                    dsf_sincos(d.q[p] * r, sy, cy);
                    const double j = sy * (inv_r * d.inv_q[p]);
                    if constexpr (SUMS) row[p] += w * j;
                    if constexpr (GRAD) u += d.c[p] * (dw * j + w * (cy - j));
                    }
                if constexpr (GRAD)
                    {
                    const double t = u * (inv_r * inv_r);  // u / r, over r once more for the unit vector
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
            else if constexpr (SUMS)                       // two particles in one place: phi_p = 1, no gradient
                {
#pragma unroll
                for (int p = 0; p < P; ++p) row[p] += 1.0;
                }
            });
        if constexpr (SUMS)
            {
            double s_row = 0.0;
#pragma unroll
            for (int p = 0; p < P; ++p)
                {
                A[p] += row[p];
                s_row += d.c[p] * row[p];
                }
            s_row = group_sum<DSF_G>(s_row);
            if (q == 0 && c.i < a.N) per_particle[c.i] = of_type ? d.c_sum + s_row : 0.0;
            if (q == 0 && of_type) count += 1.0;
            }
        if constexpr (GRAD)
            {
            Gx = group_sum<DSF_G>(Gx);
            Gy = group_sum<DSF_G>(Gy);
            Gz = group_sum<DSF_G>(Gz);
            if constexpr (VIR)
                {
                vxx = group_sum<DSF_G>(vxx), vxy = group_sum<DSF_G>(vxy), vxz = group_sum<DSF_G>(vxz);
                vyy = group_sum<DSF_G>(vyy), vyz = group_sum<DSF_G>(vyz), vzz = group_sum<DSF_G>(vzz);
                }
            if (q == 0 && c.i < a.N)
                {
                if constexpr (STORE)
                    {
                    double *o = per_particle + pitch + c.i;
                    o[0] = Gx, o[pitch] = Gy, o[2 * pitch] = Gz;
                    if constexpr (VIR)
                        {
                        o[3 * pitch] = vxx, o[4 * pitch] = vxy, o[5 * pitch] = vxz;
                        o[6 * pitch] = vyy, o[7 * pitch] = vyz, o[8 * pitch] = vzz;
                        }
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
#pragma unroll
        for (int p = 0; p < P; ++p)
            {
            const double v = block_sum(A[p], s_red);
            if (tid == 0) part[(size_t)p * DSF_MAX_BLOCKS + blockIdx.x] = v;
            }
        const double n = block_sum(count, s_red);
        if (tid == 0) part[(size_t)P * DSF_MAX_BLOCKS + blockIdx.x] = n;
        }
    }

struct DsfPeaks
    {
    double c[MTD_DSF_MAX_Q];
    unsigned int n_q;
    };

__global__ __launch_bounds__(MTD_WAVE) void k_dsf_finalize(const DsfPeaks pk, double *__restrict__ scratch)
    {
    if (threadIdx.x != 0) return;
    const double n_t = scratch[DSF_OFF_SUMS + pk.n_q];
    double value = 0.0;
    for (unsigned int p = 0; p < MTD_DSF_MAX_Q; ++p)
        {
        const double I = p < pk.n_q && n_t > 0.0 ? 1.0 + scratch[DSF_OFF_SUMS + p] / n_t : 0.0;
        scratch[DSF_OFF_I + p] = I;
        if (p < pk.n_q) value += pk.c[p] * I;
        }
    scratch[DSF_OFF_VALUE] = value;
    scratch[DSF_OFF_NT] = n_t;
    }

// ---- the spectrum ----------------------------------------------------------------------------------------------------------------
struct DsfSpectrumArgs
    {
    double q_min, dq;
    double pi_over_rc, rc_over_pi;
    unsigned int n_q, _pad;
    };

template<typename S4>
__global__ __launch_bounds__(DSF_THREADS) void k_dsf_spectrum(const QlArgs<4> a_in, const DsfSpectrumArgs sp, const S4 *__restrict__ postype,
                                                              const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                              const unsigned int *__restrict__ nlist, double *__restrict__ part)
    {
    __shared__ double s_red[16];
    const QlArgs<4> a = in_vgpr(a_in);
    const unsigned int tid = threadIdx.x, g = tid / DSF_G, q = tid % DSF_G;
    const unsigned int n_chunks = (a.N + DSF_PPB - 1) / DSF_PPB;
    const unsigned int m0 = blockIdx.y * DSF_TILE;
    const double q0 = in_vgpr(sp.q_min + (double)m0 * sp.dq), dq = in_vgpr(sp.dq);
    const double pi_over_rc = in_vgpr(sp.pi_over_rc), rc_over_pi = in_vgpr(sp.rc_over_pi);
    double T[DSF_TILE], count = 0.0;
#pragma unroll
    for (int k = 0; k < DSF_TILE; ++k) T[k] = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * DSF_PPB + g);
        if (q == 0 && c.i < a.N && (unsigned int)c.p.type == a.type) count += 1.0;
        row_walk<DSF_G, true>(a, postype, nlist, (const double *)nullptr, c, q,
                              [&](const double *, const unsigned int, const double, const double, const double, const double rsq)
            {
            if (rsq > 0.0)
                {
                const double inv_r = rsqrt(rsq), r = rsq * inv_r;
                double w, cx;
                dsf_window(r, inv_r, pi_over_rc, rc_over_pi, w, cx);
                const double wr = w * inv_r;
                double sn, cs, sd, cd;
                dsf_sincos(q0 * r, sn, cs);
                dsf_sincos(dq * r, sd, cd);
#pragma unroll
                for (int k = 0; k < DSF_TILE; ++k)
                    {
                    T[k] += wr * sn;
                    const double s1 = sn * cd + cs * sd, c1 = cs * cd - sn * sd;
                    sn = s1;
                    cs = c1;
                    }
                }
            else                                           // sin(Q r) / (Q r) = 1: Q_m of this sum, which the finalize divides by Q_m
                {
#pragma unroll
                for (int k = 0; k < DSF_TILE; ++k) T[k] += q0 + (double)k * dq;
                }
            });
        }
#pragma unroll
    for (int k = 0; k < DSF_TILE; ++k)
        {
        const double v = block_sum(T[k], s_red);
        if (tid == 0 && m0 + k < sp.n_q) part[(size_t)(m0 + k) * DSF_MAX_BLOCKS + blockIdx.x] = v;
        }
    if (blockIdx.y == 0)
        {
        const double n = block_sum(count, s_red);
        if (tid == 0) part[(size_t)MTD_DSF_MAX_SPECTRUM * DSF_MAX_BLOCKS + blockIdx.x] = n;
        }
    }

__global__ __launch_bounds__(MTD_DSF_MAX_SPECTRUM) void k_dsf_spectrum_finalize(const DsfSpectrumArgs sp, double *__restrict__ scratch)
    {
    const unsigned int m = threadIdx.x;
    const double n_t = scratch[DSF_OFF_SPEC_SUMS + sp.n_q];
    double I = 0.0;
    if (m < sp.n_q && n_t > 0.0) I = 1.0 + scratch[DSF_OFF_SPEC_SUMS + m] / ((sp.q_min + (double)m * sp.dq) * n_t);
    scratch[DSF_OFF_SPEC + m] = I;
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------
std::atomic<int> g_store_gradient{1};

// the checks every entry point shares, before a device is touched: type and cut-off of the parameters, the call block
int dsf_check_call(const mtd_dsf_params *p, const mtd_dsf_call *c)
    {
    if (!p || !c || !c->box || !c->d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (!(p->r_cut > 0.0) || !std::isfinite(p->r_cut)) return MTD_ERR_INVALID_ARGUMENT;
    return refuse_row_arrays(c->n_particles, c->d_postype && c->d_head_list && c->d_n_neigh, c->dtype, c->d_scratch, nullptr, 0);
    }

// ... and the peaks with them: everything invalid is refused ahead of the capacity
int dsf_check(const mtd_dsf_params *p, const mtd_dsf_call *c)
    {
    const int rc = dsf_check_call(p, c);
    if (rc) return rc;
    if (p->n_q == 0) return MTD_ERR_INVALID_ARGUMENT;
    const unsigned int n = p->n_q < MTD_DSF_MAX_Q ? p->n_q : MTD_DSF_MAX_Q;
    for (unsigned int k = 0; k < n; ++k)
        if (!(p->q[k] > 0.0) || !std::isfinite(p->q[k]) || !std::isfinite(p->c[k])) return MTD_ERR_INVALID_ARGUMENT;
    if (p->n_q > MTD_DSF_MAX_Q) return MTD_ERR_UNSUPPORTED;
    return MTD_SUCCESS;
    }

int dsf_check_spectrum(const mtd_dsf_call *c, double q_min, double q_max, unsigned int n_q)
    {
    if (!c || !c->d_scratch || ((uintptr_t)c->d_scratch & 15u) != 0) return MTD_ERR_INVALID_ARGUMENT;
    if (!(q_min > 0.0) || !std::isfinite(q_min) || !std::isfinite(q_max) || q_min > q_max || n_q == 0) return MTD_ERR_INVALID_ARGUMENT;
    if (n_q > MTD_DSF_MAX_SPECTRUM) return MTD_ERR_UNSUPPORTED;
    return MTD_SUCCESS;
    }

// box, cut-off and type in the argument block of the Steinhardt passes (no smoothing window: r_on is not read)
int dsf_ql_args(QlArgs<4> &a, const mtd_dsf_params *p, const mtd_dsf_call *c)
    {
    static const double no_ref[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    return fill_args<4>(a, c->n_particles, c->box, p->r_cut, 0.0, 0, p->type, no_ref, 1, 0);
    }

template<int P> DsfArgs<P> dsf_args(const mtd_dsf_params *p)
    {
    DsfArgs<P> d;
    std::memset(&d, 0, sizeof(d));
    for (int k = 0; k < P; ++k)
        {
        const bool live = (unsigned int)k < p->n_q;
        d.q[k] = live ? p->q[k] : p->q[0];
        d.inv_q[k] = 1.0 / d.q[k];
        d.c[k] = live ? p->c[k] : 0.0;
        if (live) d.c_sum += p->c[k];
        }
    d.pi_over_rc = M_PI / p->r_cut;
    d.rc_over_pi = p->r_cut / M_PI;
    return d;
    }

DsfSpectrumArgs dsf_spectrum_args(double r_cut, double q_min, double q_max, unsigned int n_q)
    {
    DsfSpectrumArgs sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.q_min = q_min;
    sp.dq = n_q > 1 ? (q_max - q_min) / (double)(n_q - 1) : 0.0;
    sp.pi_over_rc = r_cut > 0.0 ? M_PI / r_cut : 0.0;
    sp.rc_over_pi = r_cut / M_PI;
    sp.n_q = n_q;
    return sp;
    }

// the compiled peak counts: 1, 2, 4, 8 -> f(std::integral_constant<int, P>{}); the caller has refused n_q > 8
template<typename F> auto dispatch_peaks(unsigned int n_q, F &&f)
    {
    if (n_q <= 1) return f(std::integral_constant<int, 1>{});
    if (n_q <= 2) return f(std::integral_constant<int, 2>{});
    if (n_q <= 4) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 8>{});
    }

} // namespace

extern "C" {

size_t mtd_dsf_scratch_doubles(unsigned int n_particles)
    {
    return DSF_OFF_PER_PARTICLE + 10 * row_pitch(n_particles);
    }

int mtd_dsf_set_store_gradient(int enable)
    {
    g_store_gradient.store(enable ? 1 : 0);
    return MTD_SUCCESS;
    }

int mtd_dsf_accumulate(const mtd_dsf_params *p, const mtd_dsf_call *c, double **d_sums, unsigned int *n_sums)
    {
    if (!d_sums || !n_sums) return MTD_ERR_INVALID_ARGUMENT;
    int rc = dsf_check(p, c);
    if (rc) return rc;
    QlArgs<4> a;
    rc = dsf_ql_args(a, p, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)c->stream;
    const unsigned int blocks = row_blocks(c->n_particles, DSF_PPB, DSF_MAX_BLOCKS);
    double *part = c->d_scratch + DSF_OFF_PART, *per_particle = c->d_scratch + DSF_OFF_PER_PARTICLE;
    const size_t pitch = row_pitch(c->n_particles);
    const bool store = g_store_gradient.load() != 0;
    unsigned int P_compiled = 0;
    dispatch_s4(c->dtype, [&](auto t)
        {
        return dispatch_peaks(p->n_q, [&](auto pc)
            {
            return dispatch_bool(store, [&](auto st)
                {
                typedef typename decltype(t)::type S4;
                constexpr int P = decltype(pc)::value;
                constexpr bool ST = decltype(st)::value;
                P_compiled = P;
                k_dsf_walk<S4, P, true, ST, ST, ST><<<blocks, DSF_THREADS, 0, s>>>(a, dsf_args<P>(p), (const S4 *)c->d_postype, c->d_head_list,
                                                                                  c->d_n_neigh, c->d_nlist, part, per_particle, pitch, nullptr,
                                                                                  nullptr, nullptr, 0.0, nullptr, 0);
                return 0;
                });
            });
        });
    MTD_LAUNCH_CHECK();
    k_row_sums<DSF_MAX_BLOCKS><<<p->n_q + 1, MTD_WAVE, 0, s>>>(blocks, p->n_q, P_compiled, part, c->d_scratch + DSF_OFF_SUMS);
    MTD_LAUNCH_CHECK();
    *d_sums = c->d_scratch + DSF_OFF_SUMS;
    *n_sums = p->n_q + 1;
    return MTD_SUCCESS;
    }

int mtd_dsf_finalize(const mtd_dsf_params *p, const mtd_dsf_call *c, const double **d_value, const double **d_intensity, const double **d_local)
    {
    if (!d_value || !d_intensity) return MTD_ERR_INVALID_ARGUMENT;
    const int rc = dsf_check(p, c);
    if (rc) return rc;
    DsfPeaks pk;
    std::memset(&pk, 0, sizeof(pk));
    pk.n_q = p->n_q;
    for (unsigned int k = 0; k < p->n_q; ++k) pk.c[k] = p->c[k];
    k_dsf_finalize<<<1, MTD_WAVE, 0, (hipStream_t)c->stream>>>(pk, c->d_scratch);
    MTD_LAUNCH_CHECK();
    *d_value = c->d_scratch + DSF_OFF_VALUE;
    *d_intensity = c->d_scratch + DSF_OFF_I;
    if (d_local) *d_local = c->d_scratch + DSF_OFF_PER_PARTICLE;
    return MTD_SUCCESS;
    }

int mtd_dsf_forces(const mtd_dsf_params *p, const mtd_dsf_call *c, void *d_force, const double *d_bias, double bias_host, void *d_virial,
                   unsigned int virial_pitch)
    {
    int rc = dsf_check(p, c);
    if (rc) return rc;
    rc = refuse_row_arrays(c->n_particles, d_force != nullptr, c->dtype, c->d_scratch, d_virial, virial_pitch);
    if (rc) return rc;
    QlArgs<4> a;
    rc = dsf_ql_args(a, p, c);
    if (rc) return rc;
    if (c->n_particles == 0) return MTD_SUCCESS;
    hipStream_t s = (hipStream_t)c->stream;
    const size_t pitch = row_pitch(c->n_particles);
    if (g_store_gradient.load() != 0)
        {
        row_scale(c->dtype, c->n_particles, c->d_scratch + DSF_OFF_PER_PARTICLE + pitch, pitch, c->d_scratch + DSF_OFF_NT, 0.0, -2.0, -1.0, d_force,
                  d_bias, bias_host, d_virial, virial_pitch, s);
        MTD_LAUNCH_CHECK();
        return MTD_SUCCESS;
        }
    const unsigned int blocks = row_blocks(c->n_particles, DSF_PPB, DSF_MAX_BLOCKS);
    dispatch_s4(c->dtype, [&](auto t)
        {
        return dispatch_peaks(p->n_q, [&](auto pc)
            {
            return dispatch_bool(d_virial != nullptr, [&](auto vir)
                {
                typedef typename decltype(t)::type S4;
                typedef typename scalar4_traits<S4>::scalar scalar;
                constexpr int P = decltype(pc)::value;
                k_dsf_walk<S4, P, false, true, decltype(vir)::value, false><<<blocks, DSF_THREADS, 0, s>>>(
                    a, dsf_args<P>(p), (const S4 *)c->d_postype, c->d_head_list, c->d_n_neigh, c->d_nlist, nullptr, nullptr, pitch, (S4 *)d_force,
                    c->d_scratch, d_bias, bias_host, (scalar *)d_virial, virial_pitch);
                return 0;
                });
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

int mtd_dsf_spectrum(const mtd_dsf_params *p, const mtd_dsf_call *c, double q_min, double q_max, unsigned int n_q, double **d_sums,
                     unsigned int *n_sums)
    {
    if (!d_sums || !n_sums) return MTD_ERR_INVALID_ARGUMENT;
    int rc = dsf_check_call(p, c);
    if (rc) return rc;
    rc = dsf_check_spectrum(c, q_min, q_max, n_q);
    if (rc) return rc;
    QlArgs<4> a;
    rc = dsf_ql_args(a, p, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)c->stream;
    const unsigned int blocks = row_blocks(c->n_particles, DSF_PPB, DSF_MAX_BLOCKS);
    const DsfSpectrumArgs sp = dsf_spectrum_args(p->r_cut, q_min, q_max, n_q);
    double *part = c->d_scratch + DSF_OFF_PART;
    const dim3 grid(blocks, (n_q + DSF_TILE - 1) / DSF_TILE);
    dispatch_s4(c->dtype, [&](auto t)
        {
        typedef typename decltype(t)::type S4;
        k_dsf_spectrum<S4><<<grid, DSF_THREADS, 0, s>>>(a, sp, (const S4 *)c->d_postype, c->d_head_list, c->d_n_neigh, c->d_nlist, part);
        return 0;
        });
    MTD_LAUNCH_CHECK();
    k_row_sums<DSF_MAX_BLOCKS><<<n_q + 1, MTD_WAVE, 0, s>>>(blocks, n_q, MTD_DSF_MAX_SPECTRUM, part, c->d_scratch + DSF_OFF_SPEC_SUMS);
    MTD_LAUNCH_CHECK();
    *d_sums = c->d_scratch + DSF_OFF_SPEC_SUMS;
    *n_sums = n_q + 1;
    return MTD_SUCCESS;
    }

int mtd_dsf_spectrum_finalize(const mtd_dsf_call *c, double q_min, double q_max, unsigned int n_q, const double **d_spectrum)
    {
    if (!d_spectrum) return MTD_ERR_INVALID_ARGUMENT;
    const int rc = dsf_check_spectrum(c, q_min, q_max, n_q);
    if (rc) return rc;
    k_dsf_spectrum_finalize<<<1, MTD_DSF_MAX_SPECTRUM, 0, (hipStream_t)c->stream>>>(dsf_spectrum_args(0.0, q_min, q_max, n_q), c->d_scratch);
    MTD_LAUNCH_CHECK();
    *d_spectrum = c->d_scratch + DSF_OFF_SPEC;
    return MTD_SUCCESS;
    }

} // extern "C"
