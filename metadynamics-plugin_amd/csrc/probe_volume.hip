// probe_volume.hip — smoothed particle count in a probe volume (cv.probe_volume) on gfx950: the coarse-grained number N~_v of the INDUS
// method (Patel, Varilly, Chandler, Garde, J. Stat. Phys. 145, 265 (2011)), the first variable of this library that says WHERE in the
// box something happens.
//
// What it computes (include/mtd_abi.h "Probe volume"; no reference counterpart):
//     s   = sum_i a(type_i) h(d_i),   d_i = min_image(r_i - c)                   over the particles of ALL ranks
//     N_v = sum_i a(type_i) [d_i inside the sharp region]                        (a diagnostic)
//     F_i = -bias a_i grad h(d_i),    virial_i[ab] = -bias a_i (g_a d_b + g_b d_a) / 2,  g = grad h
// with h built from the cumulative G of the truncated, shifted Gaussian Phi (width sigma_s, cut-off r_c):
//     box       h = prod over the bounded axes of [G(w - d) - G(-w - d)]          (the paper's form)
//     sphere    h = G(R - |d|)                                                    (smoothed RADIALLY: not the paper's 3-d convolution,
//     cylinder  h = G(R - d_perp) [G(w - d_ax) - G(-w - d_ax)]                     the two agree for sigma_s << R)
// The centre c is handed over in fractional coordinates of the global box and so follows it affinely; widths, R, sigma_s, r_c are lengths.
//
// The design is bragg.hip's: one pass over the positions leaves rows of block sums, mtd_reduce_partials adds them in a fixed order, the
// force pass is a pure stream (one 16-byte load and one 16-byte store per particle for fp32 arrays) that recomputes grad h from the
// position.  All arithmetic behind the load is fp64, for both array types (fp32 positions are promoted exactly): a term is the same bits
// on whichever rank its particle sits.  No atomics: two identical calls give identical bits.  Only lanes inside the shell of a face
// (|u| < r_c) evaluate erf and exp, behind a branch the wave skips when none of its lanes is there; interior and exterior lanes take
// G = 1 or 0 and Phi = 0.  An unbounded axis is a half-width of +inf: w - d = +inf gives G = 1, -w - d = -inf gives G = 0, no special case.
//     k_probe_sums     rows of 2 block sums (N~, N_v)
//     k_probe_forces   forces, and with the VIRIAL switch six scalars per particle
//     k_probe_local    h_i per particle, off the step path (the getter)
// There is no finalize launch: the reduction writes the two sums where mtd_probe_finalize points (the all-reduce of a domain-decomposed
// run works on them in place).
#include "lamellar_device.hpp"

#include <cmath>
#include <cstring>

#include "dispatch.hpp"

namespace
{

using namespace mtd;

constexpr int SUMS_THREADS = 512;
constexpr int SUMS_UNROLL = 4;
constexpr unsigned int SUMS_MAX_BLOCKS = 256;
constexpr int FORCE_THREADS = 256;
constexpr int FORCE_UNROLL = 2;

// the scratch, in doubles (every part 16-byte aligned): (N~, N_v) | rows of block sums
constexpr size_t OFF_SUMS = 0;
constexpr size_t OFF_PART = 4;
constexpr size_t SCRATCH_DOUBLES = OFF_PART + (size_t)SUMS_MAX_BLOCKS * 2;

enum { BOX = MTD_PROBE_BOX, SPHERE = MTD_PROBE_SPHERE, CYLINDER = MTD_PROBE_CYLINDER };

struct ProbeArgs
    {
    double L[3], Linv[3], xy, xz, yz;          // the global box (pv_min_image)
    double c[3];                               // the centre, Cartesian, of THIS call's box
    double w[3];                               // half-widths (box: all three; cylinder: w[axis]); +inf: unbounded
    double R;
    double rc, inv_sqrt2_sigma, neg_inv_2sigma2, e_rc, inv_k, a_erf;   // Phi and G: see face()
    int axis;                                  // cylinder
    double coeff[MTD_MAX_TYPES];
    };

// HOOMD BoxDim::minImage, the operations of steinhardt_device.hpp::min_image: the result lies in |z| <= Lz/2, |y| <= Ly/2, |x| <= Lx/2
__device__ __forceinline__ void pv_min_image(const ProbeArgs &a, double &x, double &y, double &z)
    {
    double img = rint(z * a.Linv[2]);
    z -= a.L[2] * img;
    y -= a.L[2] * a.yz * img;
    x -= a.L[2] * a.xz * img;
    img = rint(y * a.Linv[1]);
    y -= a.L[1] * img;
    x -= a.L[1] * a.xy * img;
    x -= a.L[0] * rint(x * a.Linv[0]);
    }

// G(u) and (GRAD) Phi(u) of one face at signed distance u inside it:
//     Phi(u) = [exp(-u^2 / 2 sigma^2) - exp(-r_c^2 / 2 sigma^2)] / k,   G(u) = 1/2 + [sqrt(pi/2) sigma erf(u / sqrt2 sigma) - u e_rc] / k
// for |u| < r_c; outside G = 0 or 1 and Phi = 0 (u = +-inf included).  Both are continuous at |u| = r_c.
// `alive`: false for a lane whose particle lies outside region AND shell along some other direction.  Its h and its gradient are exact
// zeros whatever this face gives inside its shell (that other direction contributes a factor 0 and no slope), so it keeps the step value
// and the wave need not enter the branch for it: in a box the shells of the six faces run through the whole simulation box as slabs, and
// without this every wave met some lane in one of them (measured: 54.6 us per step for a box against 29.5 for a sphere).
template<bool GRAD> __device__ __forceinline__ void face(const ProbeArgs &a, const double u, const bool alive, double &G, double &P)
    {
    G = u > 0.0 ? 1.0 : 0.0;
    P = 0.0;
    if (alive && fabs(u) < a.rc)
        {
        G = 0.5 + (a.a_erf * erf(u * a.inv_sqrt2_sigma) - u * a.e_rc) * a.inv_k;
        if (GRAD) P = (exp(u * u * a.neg_inv_2sigma2) - a.e_rc) * a.inv_k;
        }
    }

struct ProbeTerm
    {
    double h, gx, gy, gz;                      // h and its gradient with respect to d (GRAD, else 0)
    double dx, dy, dz;                         // the minimum image of r - c
    bool inside;
    };

// The faces of a shape are visited in a loop that is NOT unrolled, so that a kernel holds one copy of erf and exp per particle slot (six
// inlined copies per slot were 3700 instructions for the box, and their hoisted constants spilled scalar registers).  The face index is
// the same in every lane: the selects below are on wave-uniform conditions.  One axis of a box: f = G(w - d) - G(-w - d),
// df/dd = Phi(-w - d) - Phi(w - d), inside = [-w <= d < w].
template<int SHAPE, bool GRAD> __device__ __forceinline__ ProbeTerm probe_term(const ProbeArgs &a, const Particle &p)
    {
    ProbeTerm t;
    double dx = p.x - a.c[0], dy = p.y - a.c[1], dz = p.z - a.c[2];
    pv_min_image(a, dx, dy, dz);
    t.dx = dx;
    t.dy = dy;
    t.dz = dz;
    t.gx = t.gy = t.gz = 0.0;
    if (SHAPE == BOX)
        {
        double fx = 0.0, fy = 0.0, fz = 0.0, ex = 0.0, ey = 0.0, ez = 0.0;
        const bool alive = fabs(dx) < a.w[0] + a.rc && fabs(dy) < a.w[1] + a.rc && fabs(dz) < a.w[2] + a.rc;
#pragma unroll 1
        for (int j = 0; j < 6; ++j)
            {
            const int ax = j >> 1;
            const bool far = j & 1;
            const double d = ax == 0 ? dx : ax == 1 ? dy : dz;
            const double w = ax == 0 ? a.w[0] : ax == 1 ? a.w[1] : a.w[2];
            double G, P;
            face<GRAD>(a, far ? -w - d : w - d, alive, G, P);
            const double sG = far ? -G : G, sP = far ? P : -P;
            fx += ax == 0 ? sG : 0.0;
            fy += ax == 1 ? sG : 0.0;
            fz += ax == 2 ? sG : 0.0;
            if (GRAD)
                {
                ex += ax == 0 ? sP : 0.0;
                ey += ax == 1 ? sP : 0.0;
                ez += ax == 2 ? sP : 0.0;
                }
            }
        t.h = fx * fy * fz;
        t.inside = (-a.w[0] <= dx && dx < a.w[0]) && (-a.w[1] <= dy && dy < a.w[1]) && (-a.w[2] <= dz && dz < a.w[2]);
        if (GRAD)
            {
            t.gx = ex * (fy * fz);
            t.gy = ey * (fx * fz);
            t.gz = ez * (fx * fy);
            }
        }
    else if (SHAPE == SPHERE)
        {
        const double r = sqrt(dx * dx + dy * dy + dz * dz);
        double G, P;
        face<GRAD>(a, a.R - r, true, G, P);
        t.h = G;
        t.inside = r < a.R;
        if (GRAD)
            {
            const double s = r > 0.0 ? -P / r : 0.0;              // (Phi(R) = 0 at the centre: the limit is 0)
            t.gx = s * dx;
            t.gy = s * dy;
            t.gz = s * dz;
            }
        }
    else
        {
        const int ax = a.axis;
        const double da = ax == 0 ? dx : ax == 1 ? dy : dz;
        const double p1 = ax == 0 ? dy : dx;
        const double p2 = ax == 2 ? dy : dz;
        const double wa = ax == 0 ? a.w[0] : ax == 1 ? a.w[1] : a.w[2];
        const double r = sqrt(p1 * p1 + p2 * p2);
        double Gr = 0.0, Pr = 0.0, fa = 0.0, ea = 0.0;
        const bool alive = r < a.R + a.rc && fabs(da) < wa + a.rc;
#pragma unroll 1
        for (int j = 0; j < 3; ++j)                                   // the mantle, then the two caps
            {
            double G, P;
            face<GRAD>(a, j == 0 ? a.R - r : j == 1 ? wa - da : -wa - da, alive, G, P);
            Gr += j == 0 ? G : 0.0;
            fa += j == 1 ? G : j == 2 ? -G : 0.0;
            if (GRAD)
                {
                Pr += j == 0 ? P : 0.0;
                ea += j == 1 ? -P : j == 2 ? P : 0.0;
                }
            }
        t.h = Gr * fa;
        t.inside = r < a.R && (-wa <= da && da < wa);
        if (GRAD)
            {
            const double s = r > 0.0 ? -Pr / r * fa : 0.0;
            const double g1 = s * p1, g2 = s * p2, ga = Gr * ea;
            t.gx = ax == 0 ? ga : g1;
            t.gy = ax == 1 ? ga : ax == 0 ? g1 : g2;
            t.gz = ax == 2 ? ga : g2;
            }
        }
    return t;
    }

// ---------------------------------------------------------------------------------------------
// partials[b][0] = sum_{i in block b} a_i h(d_i),  [1] = sum a_i [d_i inside]
// ---------------------------------------------------------------------------------------------
template<typename S4, int SHAPE>
__global__ __launch_bounds__(SUMS_THREADS) void k_probe_sums(const ProbeArgs a, const S4 *__restrict__ postype, const unsigned int N,
                                                              double *__restrict__ partials)
    {
    constexpr int U = SUMS_UNROLL;
    __shared__ double s_coeff[MTD_MAX_TYPES];
    __shared__ double s_wave[SUMS_THREADS / MTD_WAVE][2];

    const unsigned int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned int n_threads = gridDim.x * blockDim.x;

    RawGroup<S4, U> cur;
    lam_load_group<S4, U>(postype, N, tid, n_threads, cur);
    if (threadIdx.x < MTD_MAX_TYPES) s_coeff[threadIdx.x] = a.coeff[threadIdx.x];
    __syncthreads();

    double nt = 0.0, nv = 0.0;
    for (unsigned int base = tid; base < N; base += U * n_threads)
        {
        const unsigned int next = base + U * n_threads;
        RawGroup<S4, U> nxt;                                           // requested before this group is summed (lam_cv_accumulate)
        lam_load_group_nc<S4, U>(postype, N, next < N ? next : N - 1, n_threads, nxt);
#pragma unroll
        for (int u = 0; u < U; ++u)
            {
            const Particle p = scalar4_traits<S4>::unpack(cur.v[u]);
            const ProbeTerm t = probe_term<SHAPE, false>(a, p);
            // out-of-range slots re-read the last particle: weight 0
            const double w = base + u * n_threads < N ? s_coeff[p.type & (MTD_MAX_TYPES - 1)] : 0.0;
            nt = fma(w, t.h, nt);
            nv += t.inside ? w : 0.0;
            }
        cur = nxt;
        }

    // wave sums, then across the waves in a fixed order (every lane takes part: the loop above has ended for all)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const double s0 = wave_sum(nt);
    const double s1 = wave_sum(nv);
    if (lane == 0)
        {
        s_wave[wave][0] = s0;
        s_wave[wave][1] = s1;
        }
    __syncthreads();
    if (threadIdx.x < 2)
        {
        double r = 0.0;
        for (int wv = 0; wv < SUMS_THREADS / MTD_WAVE; ++wv) r += s_wave[wv][threadIdx.x];
        partials[(size_t)blockIdx.x * 2 + threadIdx.x] = r;
        }
    }

// ---------------------------------------------------------------------------------------------
// F_i = -bias a_i grad h(d_i);  VIRIAL: virial[c * pitch + i] = -bias a_i (g_a d_b + g_b d_a) / 2 for c = xx, xy, xz, yy, yz, zz
// ---------------------------------------------------------------------------------------------
template<typename S4, int SHAPE, bool VIRIAL>
__global__ __launch_bounds__(FORCE_THREADS) void k_probe_forces(const ProbeArgs a, const S4 *__restrict__ postype, S4 *__restrict__ force,
                                                                const unsigned int N, const double *__restrict__ d_bias, const double bias_host,
                                                                typename scalar4_traits<S4>::scalar *__restrict__ virial, const unsigned int pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    constexpr int U = FORCE_UNROLL;
    __shared__ double s_coeff[MTD_MAX_TYPES];                         // -bias a(t)
    if (threadIdx.x < MTD_MAX_TYPES)
        {
        const double bias = d_bias ? *d_bias : bias_host;
        s_coeff[threadIdx.x] = -bias * a.coeff[threadIdx.x];
        }
    __syncthreads();

    const unsigned int n_threads = gridDim.x * blockDim.x;
    for (unsigned int base = blockIdx.x * blockDim.x + threadIdx.x; base < N; base += U * n_threads)
        {
        S4 raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            {
            const unsigned int i = base + u * n_threads;
            raw[u] = postype[i < N ? i : base];
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            {
            const unsigned int i = base + u * n_threads;
            if (i < N)
                {
                const Particle p = scalar4_traits<S4>::unpack(raw[u]);
                const ProbeTerm t = probe_term<SHAPE, true>(a, p);
                const double w = s_coeff[p.type & (MTD_MAX_TYPES - 1)];
                const double fx = w * t.gx, fy = w * t.gy, fz = w * t.gz;
                nt_store(scalar4_traits<S4>::make((scalar)fx, (scalar)fy, (scalar)fz, (scalar)0), &force[i]);
                if (VIRIAL)
                    {
                    nt_store((scalar)(fx * t.dx), &virial[0 * (size_t)pitch + i]);
                    nt_store((scalar)(0.5 * (fx * t.dy + fy * t.dx)), &virial[1 * (size_t)pitch + i]);
                    nt_store((scalar)(0.5 * (fx * t.dz + fz * t.dx)), &virial[2 * (size_t)pitch + i]);
                    nt_store((scalar)(fy * t.dy), &virial[3 * (size_t)pitch + i]);
                    nt_store((scalar)(0.5 * (fy * t.dz + fz * t.dy)), &virial[4 * (size_t)pitch + i]);
                    nt_store((scalar)(fz * t.dz), &virial[5 * (size_t)pitch + i]);
                    }
                }
            }
        }
    }

// ---------------------------------------------------------------------------------------------
// out[i] = h(d_i) (without the weight of the type)
// ---------------------------------------------------------------------------------------------
template<typename S4, int SHAPE>
__global__ __launch_bounds__(FORCE_THREADS) void k_probe_local(const ProbeArgs a, const S4 *__restrict__ postype, const unsigned int N,
                                                               double *__restrict__ out)
    {
    const unsigned int n_threads = gridDim.x * blockDim.x;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += n_threads)
        {
        const Particle p = scalar4_traits<S4>::load(postype, i);
        out[i] = probe_term<SHAPE, false>(a, p).h;
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

bool positive_finite(double x) { return x > 0.0 && std::isfinite(x); }
bool width_ok(double w) { return w > 0.0 && !std::isnan(w); }          // finite and positive, or +inf (unbounded)

// The region with its shell must fit the cell that the minimum image maps into (include/mtd_abi.h "Probe volume", the fit rule).
// e[al]: the extent w + r_c or R + r_c along lab axis al, +inf for an unbounded axis.
bool region_fits(const mtd_box &box, const double e[3])
    {
    if (box.xy == 0.0 && box.xz == 0.0 && box.yz == 0.0)
        {
        for (int al = 0; al < 3; ++al)
            if (std::isfinite(e[al]) && !(e[al] <= 0.5 * box.L[al])) return false;
        return true;
        }
    double B[3][3];                                                   // row i of H^-1: b_i' . a_j = delta_ij
    reciprocal_rows(box, B);
    const double A[3][3] = { { box.L[0], 0.0, 0.0 }, { box.xy * box.L[1], box.L[1], 0.0 }, { box.xz * box.L[2], box.yz * box.L[2], box.L[2] } };
    for (int i = 0; i < 3; ++i)
        {
        bool concerned = false;                                       // a_i has a component along a bounded axis
        for (int al = 0; al < 3; ++al)
            if (std::isfinite(e[al]) && A[i][al] != 0.0) concerned = true;
        if (!concerned) continue;
        double sum = 0.0;
        for (int al = 0; al < 3; ++al)
            {
            if (std::isfinite(e[al]))
                sum += std::fabs(B[i][al]) * e[al];
            else if (B[i][al] != 0.0)
                return false;                                         // an unbounded axis that this lattice vector's coordinate depends on
            }
        if (!(sum <= 0.5 * (1.0 + 1e-12))) return false;              // (1e-12: the roundings of H^-1)
        }
    return true;
    }

// What every entry point refuses before a device is touched; on success `k` holds the argument block of the kernels for this call's box
int probe_check(ProbeArgs &k, const mtd_probe_params *p, const mtd_probe_call *c)
    {
    if (!p || !c || !c->global_box || !c->d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (p->shape != BOX && p->shape != SPHERE && p->shape != CYLINDER) return MTD_ERR_INVALID_ARGUMENT;
    if (p->n_types == 0 || p->n_types > MTD_MAX_TYPES) return MTD_ERR_INVALID_ARGUMENT;
    if (!positive_finite(p->sigma_s) || !positive_finite(p->r_c)) return MTD_ERR_INVALID_ARGUMENT;
    for (int d = 0; d < 3; ++d)
        if (!std::isfinite(p->centre[d])) return MTD_ERR_INVALID_ARGUMENT;
    for (unsigned int t = 0; t < p->n_types; ++t)
        if (!std::isfinite(p->coeff[t])) return MTD_ERR_INVALID_ARGUMENT;
    const double inf = INFINITY;
    double e[3] = { inf, inf, inf }, w[3] = { inf, inf, inf };
    if (p->shape == BOX)
        {
        bool bounded = false;
        for (int d = 0; d < 3; ++d)
            {
            if (!width_ok(p->half_width[d])) return MTD_ERR_INVALID_ARGUMENT;
            w[d] = p->half_width[d];
            e[d] = w[d] + p->r_c;
            bounded = bounded || std::isfinite(w[d]);
            }
        if (!bounded) return MTD_ERR_INVALID_ARGUMENT;
        }
    else
        {
        if (!std::isfinite(p->radius) || !(p->radius > p->r_c)) return MTD_ERR_INVALID_ARGUMENT;
        for (int d = 0; d < 3; ++d) e[d] = p->radius + p->r_c;
        if (p->shape == CYLINDER)
            {
            if (p->axis < 0 || p->axis > 2 || !width_ok(p->half_width[p->axis])) return MTD_ERR_INVALID_ARGUMENT;
            w[p->axis] = p->half_width[p->axis];
            e[p->axis] = w[p->axis] + p->r_c;
            }
        }
    if (c->n_global == 0 || (c->n_particles && !c->d_postype)) return MTD_ERR_INVALID_ARGUMENT;
    if (c->dtype != MTD_F32 && c->dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)c->d_scratch & 15u) != 0) return MTD_ERR_INVALID_ARGUMENT;
    const mtd_box &b = *c->global_box;
    for (int d = 0; d < 3; ++d)
        if (!positive_finite(b.L[d]) || !std::isfinite(b.lo[d])) return MTD_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(b.xy) || !std::isfinite(b.xz) || !std::isfinite(b.yz)) return MTD_ERR_INVALID_ARGUMENT;
    if (!region_fits(b, e)) return MTD_ERR_INVALID_ARGUMENT;

    std::memset(&k, 0, sizeof(k));
    for (int d = 0; d < 3; ++d)
        {
        k.L[d] = b.L[d];
        k.Linv[d] = 1.0 / b.L[d];
        k.w[d] = w[d];
        }
    k.xy = b.xy; k.xz = b.xz; k.yz = b.yz;
    // c = lo + f_0 a_1 + f_1 a_2 + f_2 a_3
    const double *f = p->centre;
    k.c[0] = b.lo[0] + f[0] * b.L[0] + f[1] * (b.xy * b.L[1]) + f[2] * (b.xz * b.L[2]);
    k.c[1] = b.lo[1] + f[1] * b.L[1] + f[2] * (b.yz * b.L[2]);
    k.c[2] = b.lo[2] + f[2] * b.L[2];
    k.R = p->radius;
    k.axis = p->shape == CYLINDER ? p->axis : 0;
    const double s = p->sigma_s, rc = p->r_c;
    k.rc = rc;
    k.inv_sqrt2_sigma = 1.0 / (std::sqrt(2.0) * s);
    k.neg_inv_2sigma2 = -1.0 / (2.0 * s * s);
    k.e_rc = std::exp(-rc * rc / (2.0 * s * s));
    const double norm = std::sqrt(2.0 * M_PI) * s * std::erf(rc / (std::sqrt(2.0) * s)) - 2.0 * rc * k.e_rc;
    if (!positive_finite(norm)) return MTD_ERR_INVALID_ARGUMENT;      // (r_c so far below sigma_s that the window has no area in fp64)
    k.inv_k = 1.0 / norm;
    k.a_erf = std::sqrt(M_PI / 2.0) * s;
    for (unsigned int t = 0; t < p->n_types; ++t) k.coeff[t] = p->coeff[t];
    return MTD_SUCCESS;
    }

// f(s4 tag, shape constant) for the array type and the shape of the call
template<typename F> auto dispatch_s4_shape(int dtype, int shape, F &&f)
    {
    return dispatch_s4(dtype, [&](auto s4)
        {
        if (shape == BOX) return f(s4, std::integral_constant<int, BOX>{});
        if (shape == SPHERE) return f(s4, std::integral_constant<int, SPHERE>{});
        return f(s4, std::integral_constant<int, CYLINDER>{});
        });
    }

} // namespace

extern "C" {

size_t mtd_probe_scratch_doubles(unsigned int n_particles)
    {
    (void)n_particles;                                                // the block sums are capped: nothing grows with the particles
    return SCRATCH_DOUBLES;
    }

int mtd_probe_accumulate(const mtd_probe_params *p, const mtd_probe_call *c, double **d_sums, unsigned int *n_sums)
    {
    if (!d_sums || !n_sums) return MTD_ERR_INVALID_ARGUMENT;
    ProbeArgs k;
    int rc = probe_check(k, p, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)c->stream;
    const unsigned int blocks = sums_blocks(c->n_particles);
    dispatch_s4_shape(c->dtype, p->shape, [&](auto s4, auto shape)
        {
        using S4 = typename decltype(s4)::type;
        k_probe_sums<S4, decltype(shape)::value><<<blocks, SUMS_THREADS, 0, s>>>(k, (const S4 *)c->d_postype, c->n_particles,
                                                                                c->d_scratch + OFF_PART);
        return 0;
        });
    MTD_LAUNCH_CHECK();
    rc = mtd_reduce_partials(c->d_scratch + OFF_PART, blocks, 2, 2, 1.0, 0.0, c->d_scratch + OFF_SUMS, c->stream);
    if (rc) return rc;
    *d_sums = c->d_scratch + OFF_SUMS;
    *n_sums = 2;
    return MTD_SUCCESS;
    }

int mtd_probe_finalize(const mtd_probe_params *p, const mtd_probe_call *c, const double **d_value, const double **d_count)
    {
    if (!d_value) return MTD_ERR_INVALID_ARGUMENT;
    ProbeArgs k;
    const int rc = probe_check(k, p, c);
    if (rc) return rc;
    *d_value = c->d_scratch + OFF_SUMS;                               // the (all-reduced) sums are the results: nothing to launch
    if (d_count) *d_count = c->d_scratch + OFF_SUMS + 1;
    return MTD_SUCCESS;
    }

int mtd_probe_forces(const mtd_probe_params *p, const mtd_probe_call *c, void *d_force, const double *d_bias, double bias_host,
                     void *d_virial, unsigned int virial_pitch)
    {
    ProbeArgs k;
    const int rc = probe_check(k, p, c);
    if (rc) return rc;
    if (c->n_particles && !d_force) return MTD_ERR_INVALID_ARGUMENT;
    if (d_virial && virial_pitch < c->n_particles) return MTD_ERR_INVALID_ARGUMENT;
    if (c->n_particles == 0) return MTD_SUCCESS;
    const unsigned int blocks = force_blocks(c->n_particles);
    hipStream_t s = (hipStream_t)c->stream;
    dispatch_s4_shape(c->dtype, p->shape, [&](auto s4, auto shape)
        {
        return dispatch_bool(d_virial != nullptr, [&](auto with_virial)
            {
            using S4 = typename decltype(s4)::type;
            typedef typename scalar4_traits<S4>::scalar scalar;
            k_probe_forces<S4, decltype(shape)::value, decltype(with_virial)::value><<<blocks, FORCE_THREADS, 0, s>>>(
                k, (const S4 *)c->d_postype, (S4 *)d_force, c->n_particles, d_bias, bias_host, (scalar *)d_virial, virial_pitch);
            return 0;
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

int mtd_probe_local(const mtd_probe_params *p, const mtd_probe_call *c, double *d_out)
    {
    ProbeArgs k;
    const int rc = probe_check(k, p, c);
    if (rc) return rc;
    if (c->n_particles && !d_out) return MTD_ERR_INVALID_ARGUMENT;
    if (c->n_particles == 0) return MTD_SUCCESS;
    const unsigned int blocks = force_blocks(c->n_particles);
    dispatch_s4_shape(c->dtype, p->shape, [&](auto s4, auto shape)
        {
        using S4 = typename decltype(s4)::type;
        k_probe_local<S4, decltype(shape)::value><<<blocks, FORCE_THREADS, 0, (hipStream_t)c->stream>>>(k, (const S4 *)c->d_postype,
                                                                                                       c->n_particles, d_out);
        return 0;
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // extern "C"
