// bragg.hip — Bragg-peak intensity (cv.bragg) on gfx950: the translation-invariant companion of the lamellar order parameter.
//
// What it computes (include/mtd_abi.h "Bragg intensity"; no reference counterpart):
//     rho_k = sum_j a(type_j) exp(i q_k . r_j)  over the particles of ALL ranks,  A1 = sum_j |a_j|,  A2 = sum_j a_j^2
//     s = sum_k w_k |rho_k|^2 / A1^2            (modulus: s = sum_k w_k |rho_k| / A1)
//     F_j = -bias a_j sum_k q_k (-alpha_k sin(q_k . r_j) + beta_k cos(q_k . r_j)),  (alpha_k, beta_k) = ds / d(Re, Im) rho_k
// with q_k = 2*pi*(h b1' + k b2' + l b3'), b_i' the reciprocal rows of the GLOBAL box.
//
// The design is lamellar.hip's: the phase in turns from the fp64 fractional projections (lamellar_device.hpp: project_o), fp32
// trigonometry (cos2pi / sin2pi, the hardware instructions where lam_fast_trig allows them), every sum in a fixed order, no atomics:
// two identical calls give identical bits.  Unlike lamellar.hip the sums are fp64 from the first add on (one v_cvt_f64_f32 and one
// v_fma_f64 per term instead of a v_fma_f32): a term is the same bits wherever its particle is summed, so the ranks of a
// domain-decomposed run reproduce the single-domain value to fp64 rounding (1e-10 is asked; fp32 sums per thread and wave give 1e-8 at a
// few thousand particles, and the square of rho_k doubles it).  Three launches of its own and the reduction of the block sums
// (mtd_reduce_partials):
//     k_bragg_sums      one pass over the positions: rows of 2K + 2 block sums (Re, Im of every mode, sum |a|, sum a^2)
//     k_bragg_finalize  one wave: the (all-reduced) sums -> s, S_k = |rho_k|^2 / A2, (alpha_k, beta_k)
//     k_bragg_forces    a pure stream: one 16-byte load and one 16-byte store per particle, one sin and one cos per particle and mode
#include "lamellar_device.hpp"

#include <cmath>
#include <cstring>

#include "lamellar_host.hpp"

namespace
{

using namespace mtd;

constexpr int SUMS_THREADS = 512;
constexpr int SUMS_UNROLL = 4;
constexpr unsigned int SUMS_MAX_BLOCKS = 256;
constexpr int FORCE_THREADS = 256;
constexpr int FORCE_UNROLL = 2;
constexpr int K_MAX = MTD_BRAGG_MAX_MODES;
constexpr int ROW_MAX = 2 * K_MAX + 2;

// the scratch, in doubles (every part 16-byte aligned): the 2K + 2 sums | s | S_k | (alpha_k, beta_k) | rows of block sums
constexpr size_t OFF_SUMS = 0;
constexpr size_t OFF_VALUE = OFF_SUMS + ROW_MAX + 2;
constexpr size_t OFF_SK = OFF_VALUE + 2;
constexpr size_t OFF_GRAD = OFF_SK + K_MAX;
constexpr size_t OFF_PART = OFF_GRAD + 2 * K_MAX;
constexpr size_t SCRATCH_DOUBLES = OFF_PART + (size_t)SUMS_MAX_BLOCKS * ROW_MAX;

// ---------------------------------------------------------------------------------------------
// partials[b][2 k], [2 k + 1] = sum_{j in block b} a_j (cos, sin)(q_k . r_j);  [2 K] = sum |a_j|;  [2 K + 1] = sum a_j^2
// KC: the compiled mode capacity (accumulators are registers: the mode loop is unrolled over KC and skips k >= n_modes, a
// wave-uniform branch)
// ---------------------------------------------------------------------------------------------
template<typename S4, int KC, bool FAST, bool ORTHO>
__global__ __launch_bounds__(SUMS_THREADS) void k_bragg_sums(const LamKArgs a, const S4 *__restrict__ postype, const unsigned int N,
                                                              double *__restrict__ partials)
    {
    constexpr int U = SUMS_UNROLL;
    constexpr int ROW = 2 * KC + 2;
    __shared__ float s_coeff[MTD_MAX_TYPES];
    __shared__ float4 s_h[KC];
    __shared__ double s_wave[SUMS_THREADS / MTD_WAVE][ROW];

    const unsigned int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned int n_threads = gridDim.x * blockDim.x;
    const unsigned int K = a.n_modes;                                 // 1 <= K <= KC (the host dispatches on it)

    RawGroup<S4, U> cur;
    lam_load_group<S4, U>(postype, N, tid, n_threads, cur);
    if (threadIdx.x < MTD_MAX_TYPES) s_coeff[threadIdx.x] = a.coeff[0][threadIdx.x];
    if (threadIdx.x < KC) s_h[threadIdx.x] = a.h[threadIdx.x];
    __syncthreads();

    // fp64 from the first add on: every term is formed in fp32 and is the same bits wherever its particle is summed, so the sums of two
    // splits of the particles (one rank or several) differ by fp64 rounding only
    double re[KC], im[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) re[k] = im[k] = 0.0;
    double a1 = 0.0, a2 = 0.0;

    for (unsigned int base = tid; base < N; base += U * n_threads)
        {
        const unsigned int next = base + U * n_threads;
        RawGroup<S4, U> nxt;                                           // requested before this group is summed (lam_cv_accumulate)
        lam_load_group_nc<S4, U>(postype, N, next < N ? next : N - 1, n_threads, nxt);
        float g0[U], g1[U], g2[U];
        double w[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            {
            const Particle p = scalar4_traits<S4>::unpack(cur.v[u]);
            project_o<ORTHO>(a, p, g0[u], g1[u], g2[u]);
            w[u] = base + u * n_threads < N ? (double)s_coeff[p.type] : 0.0;   // out-of-range slots re-read the last particle: weight 0
            a1 += fabs(w[u]);
            a2 += w[u] * w[u];
            }
#pragma unroll
        for (int k = 0; k < KC; ++k)
            {
            if (k < (int)K)
                {
                const float4 h = s_h[k];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    {
                    const float t = h.x * g0[u] + h.y * g1[u] + h.z * g2[u];
                    re[k] = fma(w[u], (double)cos2pi<FAST>(t), re[k]);
                    im[k] = fma(w[u], (double)sin2pi<FAST>(t), im[k]);
                    }
                }
            }
        cur = nxt;
        }

    // wave sums, then across the waves in a fixed order (every lane takes part: the loops above have ended for all)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KC; ++k)
        {
        const double r = wave_sum(re[k]);
        const double s = wave_sum(im[k]);
        if (lane == 0)
            {
            s_wave[wave][2 * k] = r;
            s_wave[wave][2 * k + 1] = s;
            }
        }
    const double s1 = wave_sum(a1);
    const double s2 = wave_sum(a2);
    if (lane == 0)
        {
        s_wave[wave][2 * KC] = s1;
        s_wave[wave][2 * KC + 1] = s2;
        }
    __syncthreads();
    if (threadIdx.x < 2 * K + 2)
        {
        const unsigned int src = threadIdx.x < 2 * K ? threadIdx.x : 2 * KC + (threadIdx.x - 2 * K);
        double r = 0.0;
        for (int wv = 0; wv < SUMS_THREADS / MTD_WAVE; ++wv) r += s_wave[wv][src];
        partials[(size_t)blockIdx.x * (2 * K + 2) + threadIdx.x] = r;
        }
    }

// ---------------------------------------------------------------------------------------------
// sums[2 K + 2] -> s, S_k, (alpha_k, beta_k); lane k owns mode k, lane 0 adds the value in the order of k
// ---------------------------------------------------------------------------------------------
struct BraggWeights
    {
    double w[K_MAX];
    unsigned int n_modes;
    int modulus;
    };

__global__ __launch_bounds__(MTD_WAVE) void k_bragg_finalize(const BraggWeights bw, double *__restrict__ scratch)
    {
    __shared__ double s_term[K_MAX];
    const unsigned int k = threadIdx.x;
    const unsigned int K = bw.n_modes;
    const double A1 = scratch[OFF_SUMS + 2 * K], A2 = scratch[OFF_SUMS + 2 * K + 1];
    if (k < K_MAX)
        {
        double term = 0.0, S = 0.0, alpha = 0.0, beta = 0.0;
        if (k < K && A1 > 0.0)
            {
            const double re = scratch[OFF_SUMS + 2 * k], im = scratch[OFF_SUMS + 2 * k + 1];
            const double m2 = re * re + im * im;
            S = A2 > 0.0 ? m2 / A2 : 0.0;
            if (bw.modulus)
                {
                const double m = hypot(re, im);
                term = bw.w[k] * m / A1;
                if (m > 0.0)
                    {
                    alpha = bw.w[k] * re / (m * A1);
                    beta = bw.w[k] * im / (m * A1);
                    }
                }
            else
                {
                term = bw.w[k] * m2 / (A1 * A1);
                alpha = 2.0 * bw.w[k] * re / (A1 * A1);
                beta = 2.0 * bw.w[k] * im / (A1 * A1);
                }
            }
        s_term[k] = term;
        scratch[OFF_SK + k] = S;
        scratch[OFF_GRAD + 2 * k] = alpha;
        scratch[OFF_GRAD + 2 * k + 1] = beta;
        }
    __syncthreads();
    if (k == 0)
        {
        double value = 0.0;
        for (unsigned int m = 0; m < K; ++m) value += s_term[m];
        scratch[OFF_VALUE] = value;
        }
    }

// ---------------------------------------------------------------------------------------------
// F_j = a_j sum_k q_k (ca_k sin(q_k . r_j) + cb_k cos(q_k . r_j)),  ca_k = bias alpha_k,  cb_k = -bias beta_k
// ---------------------------------------------------------------------------------------------
template<typename S4, bool FAST, bool ORTHO>
__global__ __launch_bounds__(FORCE_THREADS) void k_bragg_forces(const LamKArgs a, const S4 *__restrict__ postype, S4 *__restrict__ force,
                                                                const unsigned int N, const double *__restrict__ grad,
                                                                const double *__restrict__ d_bias, const double bias_host)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    constexpr int U = FORCE_UNROLL;
    __shared__ float s_coeff[MTD_MAX_TYPES];
    __shared__ float4 s_h[K_MAX];                                     // (h, k, l, ca)
    __shared__ float4 s_q[K_MAX];                                     // (qx, qy, qz, cb)
    const unsigned int K = a.n_modes;
    if (threadIdx.x < MTD_MAX_TYPES) s_coeff[threadIdx.x] = a.coeff[0][threadIdx.x];
    if (threadIdx.x < K)
        {
        const double bias = d_bias ? *d_bias : bias_host;
        float4 h = a.h[threadIdx.x], q = a.q[threadIdx.x];
        h.w = (float)(bias * grad[2 * threadIdx.x]);
        q.w = (float)(-bias * grad[2 * threadIdx.x + 1]);
        s_h[threadIdx.x] = h;
        s_q[threadIdx.x] = q;
        }
    __syncthreads();

    const unsigned int n_threads = gridDim.x * blockDim.x;
    for (unsigned int base = blockIdx.x * blockDim.x + threadIdx.x; base < N; base += U * n_threads)
        {
        float g0[U], g1[U], g2[U], fx[U], fy[U], fz[U];
        int type[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            {
            const unsigned int i = base + u * n_threads;
            ok[u] = i < N;
            const Particle p = scalar4_traits<S4>::load(postype, ok[u] ? i : base);
            project_o<ORTHO>(a, p, g0[u], g1[u], g2[u]);
            type[u] = p.type;
            fx[u] = fy[u] = fz[u] = 0.0f;
            }
#pragma unroll 4
        for (unsigned int k = 0; k < K; ++k)
            {
            const float4 h = s_h[k];
            const float4 q = s_q[k];
#pragma unroll
            for (int u = 0; u < U; ++u)
                {
                const float t = h.x * g0[u] + h.y * g1[u] + h.z * g2[u];
                const float amp = h.w * sin2pi<FAST>(t) + q.w * cos2pi<FAST>(t);
                fx[u] += q.x * amp;
                fy[u] += q.y * amp;
                fz[u] += q.z * amp;
                }
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            {
            if (ok[u])
                {
                const float w = s_coeff[type[u]];
                nt_store(scalar4_traits<S4>::make((scalar)(fx[u] * w), (scalar)(fy[u] * w), (scalar)(fz[u] * w), (scalar)0),
                         &force[base + u * n_threads]);
                }
            }
        }
    }

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

unsigned int sums_blocks(unsigned int N)
    {
    unsigned int b = (N + SUMS_THREADS * SUMS_UNROLL - 1) / (SUMS_THREADS * SUMS_UNROLL);
    if (b < 1) b = 1;
    return b > SUMS_MAX_BLOCKS ? SUMS_MAX_BLOCKS : b;
    }

unsigned int force_blocks(unsigned int N)
    {
    unsigned int b = (N + FORCE_THREADS * FORCE_UNROLL * 2 - 1) / (FORCE_THREADS * FORCE_UNROLL * 2);
    if (b < 1) b = 1;
    return b > 1024 ? 1024 : b;
    }

// What every entry point refuses before a device is touched, everything invalid ahead of the capacity; on success `k` holds the
// argument block of the lamellar kernels for the one set of modes (fill_kargs: reciprocal rows, Miller indices, wave vectors)
int bragg_check(LamKArgs &k, const mtd_bragg_params *p, const mtd_bragg_call *c)
    {
    if (!p || !c || !c->global_box || !c->d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (p->n_modes == 0 || p->n_types == 0 || p->n_types > MTD_MAX_TYPES) return MTD_ERR_INVALID_ARGUMENT;
    if (p->trig_mode != MTD_TRIG_DEFAULT && p->trig_mode != MTD_TRIG_HARDWARE && p->trig_mode != MTD_TRIG_ACCURATE)
        return MTD_ERR_INVALID_ARGUMENT;
    const unsigned int n = p->n_modes < (unsigned int)K_MAX ? p->n_modes : (unsigned int)K_MAX;
    for (unsigned int m = 0; m < n; ++m)
        if (!std::isfinite(p->weights[m])) return MTD_ERR_INVALID_ARGUMENT;
    for (unsigned int t = 0; t < p->n_types; ++t)
        if (!std::isfinite(p->coeff[t])) return MTD_ERR_INVALID_ARGUMENT;
    if (c->n_global == 0 || (c->n_particles && !c->d_postype)) return MTD_ERR_INVALID_ARGUMENT;
    if (c->dtype != MTD_F32 && c->dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)c->d_scratch & 15u) != 0) return MTD_ERR_INVALID_ARGUMENT;
    mtd_lamellar_set set;
    std::memset(&set, 0, sizeof(set));
    set.n_cv = 1;
    set.n_types = p->n_types;
    set.n_modes = n;
    set.first[1] = n;
    for (unsigned int m = 0; m < n; ++m)
        for (int d = 0; d < 3; ++d) set.hkl[m][d] = p->hkl[m][d];
    for (unsigned int t = 0; t < p->n_types; ++t) set.coeff[0][t] = p->coeff[t];
    set.trig_mode = p->trig_mode;
    const int rc = fill_kargs(k, &set, c->global_box);               // (the box: L > 0)
    if (rc) return rc;
    if (p->n_modes > (unsigned int)K_MAX) return MTD_ERR_UNSUPPORTED;
    return MTD_SUCCESS;
    }

// the compiled capacities of the sums kernel: 2, 4, 8, 16 modes -> f(std::integral_constant<int, KC>{}); the caller has refused K > 16
template<typename F> auto dispatch_modes(unsigned int n_modes, F &&f)
    {
    if (n_modes <= 2) return f(std::integral_constant<int, 2>{});
    if (n_modes <= 4) return f(std::integral_constant<int, 4>{});
    if (n_modes <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, K_MAX>{});
    }

} // namespace

extern "C" {

size_t mtd_bragg_scratch_doubles(unsigned int n_particles)
    {
    (void)n_particles;                                                // the block sums are capped: nothing grows with the particles
    return SCRATCH_DOUBLES;
    }

int mtd_bragg_accumulate(const mtd_bragg_params *p, const mtd_bragg_call *c, double **d_sums, unsigned int *n_sums)
    {
    if (!d_sums || !n_sums) return MTD_ERR_INVALID_ARGUMENT;
    LamKArgs k;
    int rc = bragg_check(k, p, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)c->stream;
    const unsigned int blocks = sums_blocks(c->n_particles);
    const unsigned int row = 2 * p->n_modes + 2;
    dispatch_s4_fast(c->dtype, lam_fast_trig(k) != 0, [&](auto s4, auto fast_c)
        {
        return dispatch_bool(k.ortho != 0, [&](auto ortho)
            {
            return dispatch_modes(p->n_modes, [&](auto kc)
                {
                using S4 = typename decltype(s4)::type;
                k_bragg_sums<S4, decltype(kc)::value, decltype(fast_c)::value, decltype(ortho)::value><<<blocks, SUMS_THREADS, 0, s>>>(
                    k, (const S4 *)c->d_postype, c->n_particles, c->d_scratch + OFF_PART);
                return 0;
                });
            });
        });
    MTD_LAUNCH_CHECK();
    rc = mtd_reduce_partials(c->d_scratch + OFF_PART, blocks, row, row, 1.0, 0.0, c->d_scratch + OFF_SUMS, c->stream);
    if (rc) return rc;
    *d_sums = c->d_scratch + OFF_SUMS;
    *n_sums = row;
    return MTD_SUCCESS;
    }

int mtd_bragg_finalize(const mtd_bragg_params *p, const mtd_bragg_call *c, const double **d_value, const double **d_structure_factors,
                       const double **d_amplitudes, const double **d_gradient)
    {
    if (!d_value) return MTD_ERR_INVALID_ARGUMENT;
    LamKArgs k;
    const int rc = bragg_check(k, p, c);
    if (rc) return rc;
    BraggWeights bw;
    std::memset(&bw, 0, sizeof(bw));
    bw.n_modes = p->n_modes;
    bw.modulus = p->modulus ? 1 : 0;
    for (unsigned int m = 0; m < p->n_modes; ++m) bw.w[m] = p->weights[m];
    k_bragg_finalize<<<1, MTD_WAVE, 0, (hipStream_t)c->stream>>>(bw, c->d_scratch);
    MTD_LAUNCH_CHECK();
    *d_value = c->d_scratch + OFF_VALUE;
    if (d_structure_factors) *d_structure_factors = c->d_scratch + OFF_SK;
    if (d_amplitudes) *d_amplitudes = c->d_scratch + OFF_SUMS;
    if (d_gradient) *d_gradient = c->d_scratch + OFF_GRAD;
    return MTD_SUCCESS;
    }

int mtd_bragg_forces(const mtd_bragg_params *p, const mtd_bragg_call *c, void *d_force, const double *d_bias, double bias_host)
    {
    LamKArgs k;
    const int rc = bragg_check(k, p, c);
    if (rc) return rc;
    if (c->n_particles && !d_force) return MTD_ERR_INVALID_ARGUMENT;
    if (c->n_particles == 0) return MTD_SUCCESS;
    const unsigned int blocks = force_blocks(c->n_particles);
    dispatch_s4_fast(c->dtype, lam_fast_trig(k) != 0, [&](auto s4, auto fast_c)
        {
        return dispatch_bool(k.ortho != 0, [&](auto ortho)
            {
            using S4 = typename decltype(s4)::type;
            k_bragg_forces<S4, decltype(fast_c)::value, decltype(ortho)::value><<<blocks, FORCE_THREADS, 0, (hipStream_t)c->stream>>>(
                k, (const S4 *)c->d_postype, (S4 *)d_force, c->n_particles, c->d_scratch + OFF_GRAD, d_bias, bias_host);
            return 0;
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // extern "C"
