// hexatic.hip — k-fold bond-orientational order about a lab axis of the particles of one type (cv.hexatic) on gfx950.
//
// No reference counterpart (psi_k of two-dimensional melting: Nelson and Halperin; here with the sectoral weight sin^k theta, so that it
// is a polynomial in d / r).  Definition, gradient and virial: include/mtd_abi.h "Bond-orientational order"; restated in fp64 numpy FROM
// THE DEFINITION in tests/hexatic_ref.py.  In short, over the entries (i, j) of a FULL list with both particles of the type, j != i and
// 0 < r = |d| <= r_cut, d = minImage(r_j - r_i), (u, v) the two components that follow the axis cyclically, f the cosine window of the
// Steinhardt passes:
//     z = (u + i v) / r    B = z^k    n = sum f    S = sum f B    psi = S / n    c = |psi|^2
//     local:  v_i = g(n) h(c),  s = (1 / N_t) sum v_i          global:  Psi = (1 / N_t) sum psi_i,  s = |Psi|^2
// Minimum image, particle loads and the window are those of the Steinhardt units (QlArgs<4>, min_image, smoothing_tab); the walk, the
// group's sum, the store of the virial and the sums kernel are row_walk.hpp's; launches and the shared refusals go through dispatch.hpp.
//
// MI355X design.  All arithmetic in fp64 over fp32 or fp64 arrays.
//   lanes              EIGHT lanes per central particle, 32 central particles per block and round, as in tetrahedral.hip
//   k_hex_accumulate   one walk (row_walk_entries<8, false, false>: local entries only, every per-particle array ends at N) forms n and
//                      S; lane 0 of the group forms psi, c, v, stores n_i, c_i, v_i, psi_i and the LOCAL-mode adjoint row; the block
//                      leaves its share of sum v_i, N_t, sum Re psi_i, sum Im psi_i
//   z^k                by repeated multiplication, k - 1 complex products from z: k is wave-uniform, there is no pow and no trigonometry;
//                      z^(k-1), which the gradient needs, is the chain's last link but one
//   the axis           a template argument of both walk kernels: (u, v) are picked, and the in-plane terms of the gradient added to
//                      their components, at compile time.  The body of the walk runs for the whole wave whenever ONE lane holds an
//                      entry inside the cut-off, so on a long list its fp64 instructions are the pass (profiles/r31/README.md)
//   the adjoint table  ROW-major, four doubles per particle (alpha_re, alpha_im, beta, pad: 32 B, 16-byte aligned): a neighbour's row is
//                      two 16-byte loads from one cache line (the per-lane cache-LINE rate bounds the force pass)
//   k_row_sums         (row_walk.hpp) one wave per slot adds the blocks' doubles in the fixed order of wave_sum
//   k_hex_finalize     s and Psi from the sums; in global mode it is the launch that knows Psi, and it writes the adjoint rows
//                      (2 Psi / n_i, -2 Re(conj(Psi) psi_i) / n_i) over the table, one thread per particle
//   k_hex_forces       the gather over row k, the same kernel for both modes.  B has parity (-1)^k, so with A = alpha_k + (-1)^k alpha_j
//                      and b = beta_k + beta_j both ends of an entry are ONE evaluation of f, f', z^(k-1).  The centre's row stays in
//                      registers, the neighbour's comes from the table
// An entry with r = 0 has no direction: it takes no part.  Fixed summation order everywhere (a lane's entries in row order, the DPP tree
// of group_sum, a thread's chunks in order, block_sum, wave_sum), no atomics: two identical calls give identical bits, and a row gives
// the same bits wherever it lies in the list.
#include "mtd_device.hpp"
#include "row_walk.hpp"
#include "dispatch.hpp"

#include <cmath>
#include <cstring>

namespace
{

using namespace mtd;

constexpr int HEX_THREADS = 256;
constexpr int HEX_G = 8;                                    // lanes per central particle
constexpr int HEX_PPB = HEX_THREADS / HEX_G;                // central particles per block and round
constexpr unsigned int HEX_MAX_BLOCKS = ROW_MAX_BLOCKS;     // columns of block sums in the scratch
constexpr int HEX_SUMS = 4;                                 // sum v_i, N_t, sum Re psi_i, sum Im psi_i
constexpr int HEX_ALPHA = 4;                                // doubles of an adjoint row: alpha_re, alpha_im, beta and a pad

// the scratch, in doubles: sums [4] | value, N_t, Re Psi, Im Psi [4] | (pad) | block sums [4][HEX_MAX_BLOCKS]
// | n_i [n] | c_i [n] | v_i [n] | psi_i [n][2] | alpha [n][4], n = n_particles rounded up to 2
constexpr size_t HEX_OFF_SUMS = 0, HEX_OFF_VALUE = 4, HEX_OFF_NT = 5, HEX_OFF_PSI = 6, HEX_OFF_PART = 16,
                 HEX_OFF_PER_PARTICLE = HEX_OFF_PART + HEX_SUMS * (size_t)HEX_MAX_BLOCKS;
constexpr int HEX_ROW_N = 0, HEX_ROW_C = 1, HEX_ROW_V = 2, HEX_ROW_PSI = 3, HEX_ROWS = 5;   // (psi takes two rows)

struct HexArgs
    {
    double sign;                                            // (-1)^k
    double inv_c0, n_lo, inv_dn;                            // 1 / c0, n_lo, 1 / (n_hi - n_lo)
    unsigned int k, p;
    int global, sw, gate;
    };

// h = x^p / (1 + x^p), x = max(c, 0) / c0 (h = c without a switch); g = 3 y^2 - 2 y^3, y = clip((n - n_lo) / (n_hi - n_lo), 0, 1) (g = 1
// without a gate); and their derivatives: the functions of mtd_ql_local_options, as tet_transform of tetrahedral.hip forms them
__device__ __forceinline__ void hex_transform(const HexArgs &o, const double c, const double n, double &h, double &dh, double &g, double &dg)
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
        const double y = fmin(fmax((n - o.n_lo) * o.inv_dn, 0.0), 1.0);
        g = y * y * (3.0 - 2.0 * y);
        dg = 6.0 * y * (1.0 - y) * o.inv_dn;
        }
    }

// z^(k-1) of z = zr + i zi by repeated multiplication (k wave-uniform, k >= 1; z^0 = 1): k - 2 complex products from z; z^k is one more
// product at the caller.  (The squares z^2, z^4, z^8 with one product per set bit of k - 1, written out without a loop, measured 1 %
// slower at k = 6: profiles/r31/README.md)
__device__ __forceinline__ void hex_power(const unsigned int k, const double zr, const double zi, double &wr, double &wi)
    {
    wr = k > 1 ? zr : 1.0;
    wi = k > 1 ? zi : 0.0;
    for (unsigned int m = 2; m < k; ++m)
        {
        const double t = wr * zr - wi * zi;
        wi = wr * zi + wi * zr;
        wr = t;
        }
    }

// component C of (x, y, z); the in-plane components of AXIS are U = (AXIS + 1) % 3 and V = (AXIS + 2) % 3, chosen at compile time
template<int C> __device__ __forceinline__ double hex_pick(const double x, const double y, const double z)
    {
    return C == 0 ? x : C == 1 ? y : z;
    }

// component C of radial d + tu e_u + tv e_v
template<int AXIS, int C> __device__ __forceinline__ double hex_entry(const double radial, const double dc, const double tu, const double tv)
    {
    if constexpr (C == (AXIS + 1) % 3) return fma(radial, dc, tu);
    else if constexpr (C == (AXIS + 2) % 3) return fma(radial, dc, tv);
    else return radial * dc;
    }

// ---- pass 1: n and S of every row -> n_i, c_i, v_i, psi_i, the local-mode adjoint row and the block's four sums --------------------
template<typename S4, int AXIS>
__global__ __launch_bounds__(HEX_THREADS) void k_hex_accumulate(const QlArgs<4> a_in, const HexArgs d, const S4 *__restrict__ postype,
                                                                const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                                const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                                double *__restrict__ part, double *__restrict__ per_particle, const size_t pitch)
    {
    __shared__ double s_red[16];
    const QlArgs<4> a = in_vgpr_window(a_in);
    const unsigned int tid = threadIdx.x, g = tid / HEX_G, q = tid % HEX_G;
    const unsigned int n_chunks = (a.N + HEX_PPB - 1) / HEX_PPB;
    asm volatile("" : "+v"(per_particle));                      // (the output pointer in vector registers: it is used once per particle)
    double v_sum = 0.0, count = 0.0, pr_sum = 0.0, pi_sum = 0.0;   // lane 0 of a group: its centres' sums over its chunks
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * HEX_PPB + g);
        double n = 0.0, Sr = 0.0, Si = 0.0;
        row_walk_entries<HEX_G, false, false>(a, postype, nlist, tab, c, q,
                                              [&](const double *tab_k, const unsigned int, const double dx, const double dy, const double dz, const double rsq)
            {
            if (rsq > 0.0)
                {
                const double inv_r = rsqrt(rsq);
                double f, fprime_divr;
                smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
                const double zr = hex_pick<(AXIS + 1) % 3>(dx, dy, dz) * inv_r, zi = hex_pick<(AXIS + 2) % 3>(dx, dy, dz) * inv_r;
                double wr, wi;
                hex_power(d.k, zr, zi, wr, wi);
                const double Br = wr * zr - wi * zi, Bi = wr * zi + wi * zr;
                n += f;
                Sr = fma(f, Br, Sr);
                Si = fma(f, Bi, Si);
                }
            });
        n = group_sum<HEX_G>(n);
        Sr = group_sum<HEX_G>(Sr);
        Si = group_sum<HEX_G>(Si);
        if (q == 0 && c.i < a.N)
            {
            double pr = 0.0, pi = 0.0, ci = 0.0, v = 0.0, al_r = 0.0, al_i = 0.0, be = 0.0;
            const bool of_t = (unsigned int)c.p.type == a.type;
            if (of_t)
                {
                if (n >= MTD_HEX_N_MIN)
                    {
                    const double inv_n = 1.0 / n;
                    pr = Sr * inv_n, pi = Si * inv_n;
                    ci = pr * pr + pi * pi;
                    double h, dh, gt, dgt;
                    hex_transform(d, ci, n, h, dh, gt, dgt);
                    v = gt * h;
                    const double s = 2.0 * gt * dh * inv_n;         // alpha = 2 g h' psi / n, beta = g' h - 2 g h' c / n
                    al_r = s * pr, al_i = s * pi;
                    be = dgt * h - s * ci;
                    }
                v_sum += v;                                         // (global: no switch, no gate, v = c)
                count += 1.0;
                pr_sum += pr;
                pi_sum += pi;
                }
            per_particle[HEX_ROW_N * pitch + c.i] = n;
            per_particle[HEX_ROW_C * pitch + c.i] = ci;
            per_particle[HEX_ROW_V * pitch + c.i] = v;
            *reinterpret_cast<double2 *>(per_particle + HEX_ROW_PSI * pitch + 2 * (size_t)c.i) = make_double2(pr, pi);
            if (!d.global)                                          // (global: k_hex_finalize writes the row, it knows Psi)
                {
                double2 *row = reinterpret_cast<double2 *>(per_particle + HEX_ROWS * pitch + HEX_ALPHA * (size_t)c.i);
                row[0] = make_double2(al_r, al_i);
                row[1] = make_double2(be, 0.0);
                }
            }
        }
    const double s0 = block_sum(v_sum, s_red);
    if (tid == 0) part[blockIdx.x] = s0;
    const double s1 = block_sum(count, s_red);
    if (tid == 0) part[HEX_MAX_BLOCKS + blockIdx.x] = s1;
    const double s2 = block_sum(pr_sum, s_red);
    if (tid == 0) part[2 * HEX_MAX_BLOCKS + blockIdx.x] = s2;
    const double s3 = block_sum(pi_sum, s_red);
    if (tid == 0) part[3 * HEX_MAX_BLOCKS + blockIdx.x] = s3;
    }

// s, N_t and Psi from the (reduced) sums, by thread 0 of the launch; in global mode every thread also writes the adjoint row of one
// particle: alpha = 2 Psi / n_i, beta = -2 Re(conj(Psi) psi_i) / n_i, both 0 where n_i < MTD_HEX_N_MIN (a particle of another type has n_i = 0)
__global__ __launch_bounds__(HEX_THREADS) void k_hex_finalize(double *__restrict__ scratch, const unsigned int N, const size_t pitch, const int global)
    {
    const double n_t = scratch[HEX_OFF_SUMS + 1];
    const double inv_nt = n_t > 0.0 ? 1.0 / n_t : 0.0;
    const double Pr = scratch[HEX_OFF_SUMS + 2] * inv_nt, Pi = scratch[HEX_OFF_SUMS + 3] * inv_nt;
    const unsigned int i = blockIdx.x * HEX_THREADS + threadIdx.x;
    if (i == 0)
        {
        scratch[HEX_OFF_VALUE] = global ? Pr * Pr + Pi * Pi : scratch[HEX_OFF_SUMS] * inv_nt;
        scratch[HEX_OFF_NT] = n_t;
        scratch[HEX_OFF_PSI] = Pr;
        scratch[HEX_OFF_PSI + 1] = Pi;
        }
    if (global && i < N)
        {
        const double *per_particle = scratch + HEX_OFF_PER_PARTICLE;
        const double n = per_particle[HEX_ROW_N * pitch + i];
        const double2 psi = *reinterpret_cast<const double2 *>(per_particle + HEX_ROW_PSI * pitch + 2 * (size_t)i);
        double al_r = 0.0, al_i = 0.0, be = 0.0;
        if (n >= MTD_HEX_N_MIN)
            {
            const double s = 2.0 / n;
            al_r = s * Pr, al_i = s * Pi;
            be = -s * (Pr * psi.x + Pi * psi.y);
            }
        double2 *row = reinterpret_cast<double2 *>(scratch + HEX_OFF_PER_PARTICLE + HEX_ROWS * pitch + HEX_ALPHA * (size_t)i);
        row[0] = make_double2(al_r, al_i);
        row[1] = make_double2(be, 0.0);
        }
    }

// ---- pass 2: the gather over row k --------------------------------------------------------------------------------------------------
// An entry (k, j) with d = minImage(r_j - r_k), A = alpha_k + (-1)^k alpha_j, b = beta_k + beta_j, w = z^(k-1), B = w z, R = Re(conj(A) B):
//     E = Re(conj(A) G(d)) + b grad f = d [ (f'/r) (R + b) - (k f / r^2) R ] + (k f / r) [ Re(conj(A) w) e_u + Re(conj(A) i w) e_v ]
// gives -E to N_t ds/dr_k; the mirror entry (j, k) gives +E to N_t ds/dr_j.  F_k = (bias / N_t) sum E,
// virial_k[ab] = -(bias / (2 N_t)) sum E_a d_b.
template<typename S4, int AXIS, bool VIR>
__global__ __launch_bounds__(HEX_THREADS) void k_hex_forces(const QlArgs<4> a_in, const HexArgs d, const S4 *__restrict__ postype,
                                                            const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                            const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                            const double *__restrict__ scratch, const size_t pitch, S4 *__restrict__ force,
                                                            const double *__restrict__ d_bias, const double bias_host,
                                                            typename scalar4_traits<S4>::scalar *__restrict__ virial, const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    const QlArgs<4> a = in_vgpr_window(a_in);
    const unsigned int tid = threadIdx.x, g = tid / HEX_G, q = tid % HEX_G;
    const unsigned int n_chunks = (a.N + HEX_PPB - 1) / HEX_PPB;
    const double2 *__restrict__ alpha = reinterpret_cast<const double2 *>(scratch + HEX_OFF_PER_PARTICLE + HEX_ROWS * pitch);
    const double n_t = scratch[HEX_OFF_NT];
    const double bias = d_bias ? *d_bias : bias_host;
    const double scale = in_vgpr(n_t > 0.0 ? bias / n_t : 0.0);
    const double kd = (double)d.k;
    // (the output pointers too: what is used once per particle need not hold scalar registers across the walk)
    asm volatile("" : "+v"(force));
    if constexpr (VIR) asm volatile("" : "+v"(virial));
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * HEX_PPB + g);
        double2 ak0 = make_double2(0.0, 0.0), ak1 = make_double2(0.0, 0.0);
        if (c.cnt)
            {
            ak0 = alpha[2 * (size_t)c.i];
            ak1 = alpha[2 * (size_t)c.i + 1];
            }
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        double vxx = 0.0, vxy = 0.0, vxz = 0.0, vyy = 0.0, vyz = 0.0, vzz = 0.0;
        row_walk_entries<HEX_G, false, false>(a, postype, nlist, tab, c, q,
                                              [&](const double *tab_k, const unsigned int j, const double dx, const double dy, const double dz, const double rsq)
            {
            if (rsq > 0.0)
                {
                const double2 aj0 = alpha[2 * (size_t)j], aj1 = alpha[2 * (size_t)j + 1];   // (j < N: the walk skips every other entry)
                const double inv_r = rsqrt(rsq);
                double f, fprime_divr;
                smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
                const double zr = hex_pick<(AXIS + 1) % 3>(dx, dy, dz) * inv_r, zi = hex_pick<(AXIS + 2) % 3>(dx, dy, dz) * inv_r;
                double wr, wi;
                hex_power(d.k, zr, zi, wr, wi);
                const double Ar = fma(d.sign, aj0.x, ak0.x), Ai = fma(d.sign, aj0.y, ak0.y), b = ak1.x + aj1.x;
                const double Cu = Ar * wr + Ai * wi, Cv = Ai * wr - Ar * wi;        // Re(conj(A) w), Re(conj(A) i w)
                const double R = Cu * zr + Cv * zi;                                // Re(conj(A) w z)
                const double kf_r = kd * f * inv_r;
                const double radial = fprime_divr * (R + b) - kf_r * inv_r * R;
                const double tu = kf_r * Cu, tv = kf_r * Cv;
                const double ex = hex_entry<AXIS, 0>(radial, dx, tu, tv);
                const double ey = hex_entry<AXIS, 1>(radial, dy, tu, tv);
                const double ez = hex_entry<AXIS, 2>(radial, dz, tu, tv);
                Fx += ex;
                Fy += ey;
                Fz += ez;
                if constexpr (VIR)
                    {
                    vxx += ex * dx, vxy += ex * dy, vxz += ex * dz;
                    vyy += ey * dy, vyz += ey * dz, vzz += ez * dz;
                    }
                }
            });
        Fx = group_sum<HEX_G>(Fx);
        Fy = group_sum<HEX_G>(Fy);
        Fz = group_sum<HEX_G>(Fz);
        if (q == 0 && c.i < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + c.i);
        if constexpr (VIR)
            {
            vxx = group_sum<HEX_G>(vxx), vxy = group_sum<HEX_G>(vxy), vxz = group_sum<HEX_G>(vxz);
            vyy = group_sum<HEX_G>(vyy), vyz = group_sum<HEX_G>(vyz), vzz = group_sum<HEX_G>(vzz);
            if (q == 0 && c.i < a.N) row_store_virial<false>(virial + c.i, virial_pitch, vxx, vxy, vxz, vyy, vyz, vzz, -0.5 * scale, 0.0);
            }
        }
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the checks every entry point shares, before a device is touched; everything invalid is refused ahead of what is merely not built
int hex_check(const mtd_hex_params *p, const mtd_hex_call *c)
    {
    if (!p || !c || !c->box || !c->d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (!(p->r_on >= 0.0) || !(p->r_on < p->r_cut) || !std::isfinite(p->r_cut)) return MTD_ERR_INVALID_ARGUMENT;
    if (p->k == 0 || p->axis > 2) return MTD_ERR_INVALID_ARGUMENT;
    if (p->switch_on && (!(p->c0 > 0.0) || !std::isfinite(p->c0) || p->p == 0)) return MTD_ERR_INVALID_ARGUMENT;
    if (p->gate_on && (!(p->n_lo >= 0.0) || !(p->n_lo < p->n_hi) || !std::isfinite(p->n_hi))) return MTD_ERR_INVALID_ARGUMENT;
    const int rc = refuse_row_arrays(c->n_particles, c->d_postype && c->d_head_list && c->d_n_neigh, c->dtype, c->d_scratch, nullptr, 0);
    if (rc) return rc;
    if (p->k > MTD_HEX_MAX_K) return MTD_ERR_UNSUPPORTED;
    if (p->global_order && (p->switch_on || p->gate_on)) return MTD_ERR_UNSUPPORTED;   // they act on c_i, which |Psi|^2 does not sum
    // the adjoint row of a ghost would have to be exchanged
    if (c->n_ghost > 0) return MTD_ERR_UNSUPPORTED;
    return MTD_SUCCESS;
    }

// box, cut-off and window in the argument block of the Steinhardt passes
int hex_ql_args(QlArgs<4> &a, const mtd_hex_params *p, const mtd_hex_call *c)
    {
    static const double no_ref[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    return fill_args<4>(a, c->n_particles, c->box, p->r_cut, p->r_on, 0, p->type, no_ref, 1, 0);
    }

HexArgs hex_args(const mtd_hex_params *p)
    {
    HexArgs d;
    std::memset(&d, 0, sizeof(d));
    d.k = p->k;
    d.sign = (p->k & 1u) ? -1.0 : 1.0;
    d.global = p->global_order ? 1 : 0;
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

size_t mtd_hex_scratch_doubles(unsigned int n_particles)
    {
    return HEX_OFF_PER_PARTICLE + (HEX_ROWS + HEX_ALPHA) * row_pitch(n_particles);
    }

int mtd_hex_accumulate(const mtd_hex_params *p, const mtd_hex_call *c, double **d_sums, unsigned int *n_sums)
    {
    if (!d_sums || !n_sums) return MTD_ERR_INVALID_ARGUMENT;
    int rc = hex_check(p, c);
    if (rc) return rc;
    QlArgs<4> a;
    rc = hex_ql_args(a, p, c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)c->stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int blocks = row_blocks(c->n_particles, HEX_PPB, HEX_MAX_BLOCKS);
    double *part = c->d_scratch + HEX_OFF_PART, *per_particle = c->d_scratch + HEX_OFF_PER_PARTICLE;
    const size_t pitch = row_pitch(c->n_particles);
    const HexArgs d = hex_args(p);
    dispatch_s4(c->dtype, [&](auto t)
        {
        return dispatch_count<3>(p->axis + 1, [&](auto ax)                  // (axis <= 2: hex_check)
            {
            typedef typename decltype(t)::type S4;
            k_hex_accumulate<S4, decltype(ax)::value - 1><<<blocks, HEX_THREADS, 0, s>>>(a, d, (const S4 *)c->d_postype, c->d_head_list, c->d_n_neigh,
                                                                                         c->d_nlist, tab, part, per_particle, pitch);
            return 0;
            });
        });
    MTD_LAUNCH_CHECK();
    k_row_sums<HEX_MAX_BLOCKS><<<HEX_SUMS, MTD_WAVE, 0, s>>>(blocks, HEX_SUMS, 0, part, c->d_scratch + HEX_OFF_SUMS);
    MTD_LAUNCH_CHECK();
    *d_sums = c->d_scratch + HEX_OFF_SUMS;
    *n_sums = HEX_SUMS;
    return MTD_SUCCESS;
    }

int mtd_hex_finalize(const mtd_hex_params *p, const mtd_hex_call *c, const double **d_value, const double **d_local, const double **d_switched,
                     const double **d_coordination, const double **d_psi)
    {
    if (!d_value) return MTD_ERR_INVALID_ARGUMENT;
    const int rc = hex_check(p, c);
    if (rc) return rc;
    const size_t pitch = row_pitch(c->n_particles);
    // local: thread 0 alone has work; global: a thread per particle, the adjoint rows
    const unsigned int blocks = p->global_order && c->n_particles ? (c->n_particles + HEX_THREADS - 1) / HEX_THREADS : 1;
    k_hex_finalize<<<blocks, HEX_THREADS, 0, (hipStream_t)c->stream>>>(c->d_scratch, c->n_particles, pitch, p->global_order ? 1 : 0);
    MTD_LAUNCH_CHECK();
    const double *per_particle = c->d_scratch + HEX_OFF_PER_PARTICLE;
    *d_value = c->d_scratch + HEX_OFF_VALUE;
    if (d_local) *d_local = per_particle + HEX_ROW_C * pitch;
    if (d_switched) *d_switched = per_particle + HEX_ROW_V * pitch;
    if (d_coordination) *d_coordination = per_particle + HEX_ROW_N * pitch;
    if (d_psi) *d_psi = per_particle + HEX_ROW_PSI * pitch;
    return MTD_SUCCESS;
    }

int mtd_hex_forces(const mtd_hex_params *p, const mtd_hex_call *c, void *d_force, const double *d_bias, double bias_host, void *d_virial,
                   unsigned int virial_pitch)
    {
    int rc = hex_check(p, c);
    if (rc && rc != MTD_ERR_UNSUPPORTED) return rc;
    const int rc_arrays = refuse_row_arrays(c->n_particles, d_force != nullptr, c->dtype, c->d_scratch, d_virial, virial_pitch);
    if (rc_arrays) return rc_arrays;
    if (rc) return rc;
    QlArgs<4> a;
    rc = hex_ql_args(a, p, c);
    if (rc) return rc;
    if (c->n_particles == 0) return MTD_SUCCESS;
    hipStream_t s = (hipStream_t)c->stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int blocks = row_blocks(c->n_particles, HEX_PPB, HEX_MAX_BLOCKS);
    const size_t pitch = row_pitch(c->n_particles);
    const HexArgs d = hex_args(p);
    dispatch_s4(c->dtype, [&](auto t)
        {
        return dispatch_count<3>(p->axis + 1, [&](auto ax)                  // (axis <= 2: hex_check)
            {
            return dispatch_bool(d_virial != nullptr, [&](auto vir)
                {
                typedef typename decltype(t)::type S4;
                typedef typename scalar4_traits<S4>::scalar scalar;
                k_hex_forces<S4, decltype(ax)::value - 1, decltype(vir)::value><<<blocks, HEX_THREADS, 0, s>>>(
                    a, d, (const S4 *)c->d_postype, c->d_head_list, c->d_n_neigh, c->d_nlist, tab, c->d_scratch, pitch, (S4 *)d_force, d_bias,
                    bias_host, (scalar *)d_virial, virial_pitch);
                return 0;
                });
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // extern "C"
