// steinhardt_device.hpp — what the pair passes of the Steinhardt variables share (steinhardt.hip: the global Q_l of the
// reference; steinhardt_local.hip: the per-particle q_l): kernel arguments, the table of recurrence constants, the smoothing
// window, the minimum image and the contracted pair gradient.  Conventions and citations: see the header of steinhardt.hip.
#pragma once

#include "mtd_device.hpp"

#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

namespace mtd
{

template<int LMAX> struct QlArgs
    {
    double lo[3], L[3], Linv[3], xy, xz, yz;
    double rcutsq, ronsq, r_on, r_cut, inv_width;
    unsigned int lmax, type, N, n_global;
    int half_nlist, _pad;
    double ql_ref[LMAX + 1];
    };

// Jacobi recurrence prefactors (spherical_harmonics.hpp:151-175) and jacobi[m][0] (:197-201).  They depend on (m, n) only,
// so in the fully unrolled loops they fold to literals: no table in the kernel arguments, no scalar registers tied up
// (a [m][n] table in the argument segment cost ~340 v_readlane per pair in spilled scalars)
__host__ __device__ __forceinline__ double jac_f0(const int m, const int n)
    {
    return 2 * sqrt(1 + (m - 0.5) / n) * sqrt(1 - (m - 0.5) / (n + 2 * m));
    }
__host__ __device__ __forceinline__ double jac_f1(const int m, const int n)
    {
    return -sqrt(1.0 + 4.0 / (2 * n + 2 * m - 3)) * sqrt(1 - 1.0 / n) * sqrt(1.0 - 1.0 / (n + 2 * m));
    }
__host__ __device__ __forceinline__ double jac_0(const int m)
    {
    double v = 0.70710678118654752440084436210484903928483593768847;    // 1 / sqrt(2)
    for (int k = 1; k <= m; ++k) v *= sqrt(1 + 1.0 / 2 / k);
    return v;
    }

struct cplx
    {
    double re, im;
    };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx cconj(cplx a) { return {a.re, -a.im}; }
__device__ __forceinline__ cplx cscale(cplx a, double s) { return {a.re * s, a.im * s}; }

template<int LMAX>
__device__ __forceinline__ void min_image(const QlArgs<LMAX> &a, double &x, double &y, double &z)
    {
    // HOOMD BoxDim::minImage: nearest image counts from the reciprocal box lengths
    double img = rint(z * a.Linv[2]);
    z -= a.L[2] * img;
    y -= a.L[2] * a.yz * img;
    x -= a.L[2] * a.xz * img;
    img = rint(y * a.Linv[1]);
    y -= a.L[1] * img;
    x -= a.L[1] * a.xy * img;
    x -= a.L[0] * rint(x * a.Linv[0]);
    }

// ---- constants of the pair passes, read through the scalar cache -------------------------------------------------------------
// Counters of round 3 (profiles/r3): the pair kernels are bound by instruction ISSUE — vector + scalar + LDS + branch
// instructions times four cycles add up to the launch time.  A 64-bit literal is two s_mov_b32, and the ~100 literals of a pair
// (recurrence prefactors, derivative factors, the smoothing polynomial) were a quarter of all issue slots (or, where the
// compiler kept them in VGPRs, a v_mov per use and 44 registers).  They now sit in a small table in device memory that the
// kernel reads with s_load_dwordx8/x16 (eight constants per issue slot) right where they are used; the table pointer carries an
// offset the compiler cannot see through (always zero), or it would hoist ~90 loads out of the pair loop and spill them.
//   [SM_SIN, +10)  [SM_COS, +10)   Taylor coefficients of sincospi_unit_tab, highest order first
//   beta(m, n)     monic form of the Jacobi recurrence of spherical_harmonics.hpp:203-211 in the degree n = l - m:
//                  J_m(n) = kappa(m, n) p_mn(x), p_m0 = 1, p_m1 = x, p_mn = x p_m,n-1 - beta(m, n) p_m,n-2
//                  (kappa(m, 0) = jacobi[m][0], kappa(m, n) = f0(m, n) kappa(m, n - 1), beta = -f1(m, n) / (f0(m, n) f0(m, n - 1)))
//   nrm(l, m)      (-1)^m kappa(m, l - m) / sqrt(2 pi): Y_lm = nrm(l, m) p_m,l-m(cos theta) (sin theta e^{i phi})^m
//   d(l, m)        sqrt((l - m)(l + m + 1)) nrm(l, m + 1) / nrm(l, m): the A_l,m+1 term of dY_lm/dtheta (:305-309)
template<int LMAX> struct QlTab
    {
    static constexpr int SM_SIN = 0, SM_COS = 10, BETA = 24;
    static constexpr int N_BETA = (LMAX - 1) * LMAX / 2;
    static constexpr int D = (BETA + N_BETA + 7) / 8 * 8;
    static constexpr int N_D = LMAX * (LMAX + 1) / 2;
    static constexpr int NRM = (D + N_D + 7) / 8 * 8;
    static constexpr int SIZE = NRM + (LMAX + 1) * (LMAX + 2) / 2;
    __host__ __device__ static constexpr int beta(const int m, const int n)         // n >= 2, m + n <= LMAX
        {
        return BETA + m * (LMAX - 1) - m * (m - 1) / 2 + (n - 2);
        }
    __host__ __device__ static constexpr int d(const int l, const int m) { return D + l * (l - 1) / 2 + m; }       // m < l
    __host__ __device__ static constexpr int nrm(const int l, const int m) { return NRM + l * (l + 1) / 2 + m; }
    };

template<int LMAX> void ql_build_table(double *t)
    {
    typedef QlTab<LMAX> T;
    for (int i = 0; i < T::SIZE; ++i) t[i] = 0.0;
    // sin: -1/21!, 1/19!, ..., 1/3! ; cos: 1/20!, -1/18!, ..., -1/2!   (sincospi_unit_tab)
    double fact = 1.0;                                       // k!
    double inv[22];
    inv[0] = 1.0;
    for (int k = 1; k <= 21; ++k)
        {
        fact *= k;
        inv[k] = 1.0 / fact;
        }
    for (int i = 0; i < 10; ++i)
        {
        const int ks = 21 - 2 * i, kc = 20 - 2 * i;
        t[T::SM_SIN + i] = (i % 2 == 0 ? -1.0 : 1.0) * inv[ks];
        t[T::SM_COS + i] = (i % 2 == 0 ? 1.0 : -1.0) * inv[kc];
        }
    double kappa[LMAX + 1][LMAX + 1];
    for (int m = 0; m <= LMAX; ++m)
        {
        kappa[m][0] = jac_0(m);
        for (int n = 1; m + n <= LMAX; ++n) kappa[m][n] = jac_f0(m, n) * kappa[m][n - 1];
        for (int n = 2; m + n <= LMAX; ++n) t[T::beta(m, n)] = -jac_f1(m, n) / (jac_f0(m, n) * jac_f0(m, n - 1));
        }
    for (int l = 0; l <= LMAX; ++l)
        for (int m = 0; m <= l; ++m)
            t[T::nrm(l, m)] = ((m % 2) ? -1.0 : 1.0) * 0.3989422804014326779399460599343818684758586311649 * kappa[m][l - m];
    for (int l = 1; l <= LMAX; ++l)
        for (int m = 0; m < l; ++m)
            t[T::d(l, m)] = std::sqrt((double)((l - m) * (l + m + 1))) * t[T::nrm(l, m + 1)] / t[T::nrm(l, m)];
    }

// the table of this LMAX on the current device (built and uploaded once per device)
template<int LMAX> const double *ql_device_table(hipStream_t s, int &rc)
    {
    static std::mutex mtx;
    static std::map<int, double *> tables;
    rc = MTD_SUCCESS;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        {
        rc = MTD_ERR_INVALID_ARGUMENT;
        return nullptr;
        }
    std::lock_guard<std::mutex> lock(mtx);
    auto it = tables.find(dev);
    if (it != tables.end()) return it->second;
    static double host[QlTab<LMAX>::SIZE];
    ql_build_table<LMAX>(host);
    double *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, sizeof(host));
    if (e == hipSuccess) e = hipMemcpy(d, host, sizeof(host), hipMemcpyHostToDevice);      // once per device: synchronous
    if (e != hipSuccess)
        {
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        rc = (int)e;
        return nullptr;
        }
    (void)s;
    tables.emplace(dev, d);
    return d;
    }

// a * b + c with c a wave-uniform constant in scalar registers: ONE v_fma_f64.  Left to itself the compiler selects the
// two-operand v_fmac_f64 and first copies the constant into the destination (two v_mov_b32 per Horner step).
__device__ __forceinline__ double fma_uniform_addend(const double a, const double b, const double c)
    {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
    }

// cos(pi x) and sin(pi x) for x in [0, 1] (the smoothing window): with y = x - 1/2, cos(pi x) = -sin(pi y) and
// sin(pi x) = cos(pi y), |pi y| <= pi/2, Taylor series in z^2 to z^21 / z^20 (truncation < 3e-16); ~25 FMAs instead of
// the ~80 instructions of the general-range library routine.  Coefficients from the table (c = table + SM_SIN).
__device__ __forceinline__ void sincospi_unit_tab(const double *__restrict__ c, const double x, double &sn, double &cs)
    {
    const double z = M_PI * (x - 0.5), z2 = z * z;
    double s = c[0];
#pragma unroll
    for (int i = 1; i < 10; ++i) s = fma_uniform_addend(s, z2, c[i]);
    const double sin_z = z - z * z2 * s;
    double k = c[10];
#pragma unroll
    for (int i = 1; i < 10; ++i) k = fma_uniform_addend(k, z2, c[10 + i]);
    const double cos_z = 1.0 + z2 * k;
    cs = -sin_z;
    sn = cos_z;
    }

template<int LMAX>
__device__ __forceinline__ void smoothing_tab(const QlArgs<LMAX> &a, const double *__restrict__ tab, const double rsq, const double inv_r,
                                              double &f, double &fprime_divr)
    {
    f = 1.0;
    fprime_divr = 0.0;
    if (rsq > a.ronsq)
        {
        double sn, cs;
        sincospi_unit_tab(tab + QlTab<LMAX>::SM_SIN, (rsq * inv_r - a.r_on) * a.inv_width, sn, cs);
        f = 0.5 * (cs + 1.0);
        fprime_divr = -(0.5 * M_PI) * inv_r * a.inv_width * sn;
        }
    }

// the pair force of one list entry (SteinhardtQl.cc:287-333 contracted as the header describes), in the monic amplitudes:
// with h = sin(theta) e^{i phi} = (dx + i dy) / r, P = p_m,l-m(cos theta) and Z_lm = h^m q_lm (q_lm = nrm(l, m) w_l conj(Q_lm)
// from the weight source),
//   U = sum P Re Z,   and per term   grad[P Re Z] = { P' Re Z (e_z - ct e_r) + m P Re(h^(m-1) q (e_x + i e_y - h e_r)) } / r
// with P' = dP/d(cos theta) = -d(l, m) p_m+1,l-m-1: a polynomial in d / r, the spherical components (1 / tan(theta), 1 / rho) never
// formed.  The sums are taken over Y_lm = h^(m-1) q_lm (m >= 1), the last factor h applied once at the end:
//   A + i B = sum m P Y,   VA = Re(h (A + i B)),   D = sum d(l, m) p_m+1,l-m-1 Re Z
// and the force is -(f'/r U d + f/r {(A, -B, 0) + (D ct - VA) (ex, ey, 0) - (VA ct + D sin^2) e_z}).  Degrees with Ql_ref[l] = 0
// are skipped as a whole (one scalar branch per degree); per order m the sums over l are kept apart (A_m, B_m) so that the
// factor m is applied once.  A pair on the z axis (dx = dy = 0) gets the finite limit, where the reference's 0 * (1 / tan(0)) is
// NaN (SteinhardtQl.cc:305, :314); tests/test_gpu_ql_axis.py holds every entry point to a rotated-frame restatement there.
// The weights q_lm come from a source object, `qsrc(l, m, idx)` with idx = l (l + 1) / 2 + m: one table per launch in LDS for the
// global variable (QlWeightsLds), the sum of two per-particle table rows for the local one (steinhardt_local.hip).
struct QlWeightsLds
    {
    const double *s_qw;
    // `opaque0` (always 0, but derived from the pair slot) keeps these reads inside the pair loop: hoisted, the
    // loop-invariant table takes ~110 registers
    unsigned int opaque0;
    __device__ __forceinline__ cplx operator()(const int, const int, const int idx) const
        {
        return {s_qw[2 * idx + opaque0], s_qw[2 * idx + 1 + opaque0]};
        }
    };

template<int LMAX, typename QSRC>
__device__ __forceinline__ void ql_pair_force(const QlArgs<LMAX> &a, const double *__restrict__ tab, const QSRC &qsrc, const unsigned int act,
                                              const double dx, const double dy, const double dz, const double rsq,
                                              double &fpx, double &fpy, double &fpz)
    {
    typedef QlTab<LMAX> T;
    const double inv_r = rsqrt(rsq);
    const double ct = dz * inv_r, ex = dx * inv_r, ey = dy * inv_r;
    double f, fprime_divr;
    smoothing_tab<LMAX>(a, tab, rsq, inv_r, f, fprime_divr);
    // monic amplitudes p[m][n], n = l - m (n = 0: 1, n = 1: cos theta)
    double p[LMAX + 1][LMAX + 1];
#pragma unroll
    for (int m = 0; m <= LMAX; ++m)
        {
        p[m][0] = 1.0;
        if (m + 1 <= LMAX) p[m][1] = ct;
#pragma unroll
        for (int n = 2; m + n <= LMAX; ++n) p[m][n] = ct * p[m][n - 1] - tab[T::beta(m, n)] * p[m][n - 2];
        }
    // h^(m - 1), m = 1 ... LMAX
    cplx h[LMAX + 1];
    h[0] = {1.0, 0.0};
    if (LMAX >= 2) h[1] = {ex, ey};
#pragma unroll
    for (int m = 2; m < LMAX; ++m) h[m] = cmul(h[m - 1], {ex, ey});
    double Am[LMAX + 1], Bm[LMAX + 1], U0 = 0.0, D0 = 0.0, Dre = 0.0, Dim = 0.0;
#pragma unroll
    for (int m = 0; m <= LMAX; ++m) Am[m] = Bm[m] = 0.0;
#pragma unroll
    for (int l = 0; l <= LMAX; ++l)
        {
        if (act & (1u << l))                                     // degrees with Ql_ref[l] != 0 (and l <= lmax)
            {
#pragma unroll
            for (int m = 0; m <= l; ++m)
                {
                const int idx = l * (l + 1) / 2 + m;
                const cplx q = qsrc(l, m, idx);
                if (m == 0)
                    {
                    if (l == 0)
                        U0 += q.re;
                    else
                        {
                        U0 += p[0][l] * q.re;
                        if (l == 1)
                            D0 += tab[T::d(l, 0)] * q.re;
                        else
                            D0 += (tab[T::d(l, 0)] * p[1][l - 1]) * q.re;
                        }
                    }
                else
                    {
                    const cplx Y = m == 1 ? q : cmul(h[m - 1], q);
                    if (m == l)
                        {
                        Am[m] += Y.re;
                        Bm[m] += Y.im;
                        }
                    else
                        {
                        Am[m] += p[m][l - m] * Y.re;
                        Bm[m] += p[m][l - m] * Y.im;
                        const double c = l - m - 1 == 0 ? tab[T::d(l, m)] : tab[T::d(l, m)] * p[m + 1][l - m - 1];
                        Dre += c * Y.re;
                        Dim += c * Y.im;
                        }
                    }
                }
            }
        }
    double A0 = 0.0, B0 = 0.0, A1 = 0.0, B1 = 0.0;
#pragma unroll
    for (int m = 1; m <= LMAX; ++m)
        {
        A0 += Am[m];
        B0 += Bm[m];
        A1 += (double)m * Am[m];
        B1 += (double)m * Bm[m];
        }
    const double U = U0 + (ex * A0 - ey * B0);
    const double VA = ex * A1 - ey * B1;                     // sum m P Re(h^m q)
    const double D = D0 + (ex * Dre - ey * Dim);             // -sum P' Re(h^m q)
    const double fa = fprime_divr * U, fr = f * inv_r;
    const double k = D * ct - VA;
    fpx = -(fa * dx + fr * (A1 + k * ex));
    fpy = -(fa * dy + fr * (k * ey - B1));
    fpz = -(fa * dz - fr * (VA * ct + D * (ex * ex + ey * ey)));
    }

template<int LMAX>
int fill_args(QlArgs<LMAX> &a, unsigned int N, const mtd_box *box, double rcut, double ron, unsigned int lmax, unsigned int type,
              const double *ql_ref, unsigned int n_global, int half)
    {
    if (!box || !ql_ref || n_global == 0 || lmax > (unsigned int)LMAX || !(rcut > 0.0) || !(ron >= 0.0) || !(ron < rcut))
        return MTD_ERR_INVALID_ARGUMENT;
    std::memset(&a, 0, sizeof(a));
    for (int i = 0; i < 3; ++i)
        {
        a.lo[i] = box->lo[i];
        a.L[i] = box->L[i];
        }
    a.xy = box->xy; a.xz = box->xz; a.yz = box->yz;
    a.rcutsq = rcut * rcut;                      // SteinhardtQl.cc:18
    a.ronsq = ron * ron;
    a.r_on = std::sqrt(a.ronsq);
    a.r_cut = std::sqrt(a.rcutsq);
    a.inv_width = 1.0 / (a.r_cut - a.r_on);
    for (int i = 0; i < 3; ++i) a.Linv[i] = 1.0 / box->L[i];
    a.lmax = lmax; a.type = type; a.N = N; a.n_global = n_global; a.half_nlist = half;
    for (unsigned int l = 0; l <= lmax; ++l) a.ql_ref[l] = ql_ref[l];
    return MTD_SUCCESS;
    }

} // namespace mtd
