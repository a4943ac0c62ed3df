// pair_entropy.hip — pair entropy S2 from a Gaussian-smoothed g(r) (cv.pair_entropy) on gfx950.
//
// No reference counterpart (Piaggi, Valsson and Parrinello, PRL 119, 015701; PLUMED's PAIRENTROPY).  Definition, gradient and virial:
// include/mtd_abi.h "Pair entropy"; restated in fp64 numpy in tests/pair_entropy_ref.py.  In short, over the entries (i, j) of a FULL
// list with both particles of `type`, j != i and r = |minImage(r_i - r_j)| <= r_cut = r_max + 4 sigma:
//     H_b = sum f(r) K(r_b - r)      b in the window |b - floor(r B / r_max)| <= w = ceil(6 sigma / Delta), 0 <= b < B
//     g_b = H_b / (4 pi N_t rho r_b^2),   S = -2 pi rho Delta sum_b r_b^2 (g ln g - g + 1)        (g < 1e-10: the bin counts as 1)
//     W_b = dS/dH_b = -Delta ln g_b / (2 N_t),   u = sum_b W_b K_b [f' + f (r_b - r) / sigma^2],   dS/dr_k = 2 sum_{j in row k} u d / r
// with f the cosine window of steinhardt_device.hpp between r_max + 3 sigma and r_cut.  Smoothing, minimum image, particle loads and the
// type test are those of the Steinhardt units (QlArgs<4>, smoothing_tab, min_image); the walk over a row, its centre, the group's sum and
// the store of force and virial are those of row_walk.hpp; launches and the shared refusals go through dispatch.hpp.
//
// MI355X design.  Four launches per step, all in fp64 arithmetic over fp32 or fp64 arrays:
//   lanes            EIGHT lanes (half a DPP row) per central particle, 32 central particles per block and round; lane q takes entries
//                    q, q + 8, ... of the row (rows hold ~80-100 entries: 10-13 trips per lane), list entry two trips and neighbour
//                    position one trip ahead of the arithmetic: row_walk of row_walk.hpp
//   the window       two exponentials per entry, K_c = K(r_c - r) at the centre bin c and e = exp(-(r_c - r) Delta / sigma^2); then
//                    K_{b+1} = K_b q_b, q_{b+1} = q_b s^2 upwards from q_c = e s and K_{b-1} = K_b p_b, p_{b-1} = p_b s^2 downwards from
//                    p_c = s / e, s = exp(-Delta^2 / 2 sigma^2): every factor is <= 1, the recurrence never amplifies.  Both chains advance
//                    in ONE loop whose trip count, min(w, largest centre bin + 1), is the same in every lane: two independent chains per
//                    trip and a scalar loop.  A bin off the table (a centre past B - 1 when r > r_max, a window clipped at either end) is
//                    tested away in the accumulate pass and reads a zero weight in the force pass
//   k_pe_accumulate  f K into a per-block LDS image of 64-bit FIXED-POINT integers (ds_add_u64: integer adds commute, so the image does
//                    not depend on the order the hardware serves the lanes in).  The scale is a power of two chosen per block and call:
//                    the block first counts the entries E of the rows it will walk (an upper bound of its adds per bin), takes
//                    2^x > E K(0) and scales by 2^(62 - x), so a bin stays below 2^62 + E / 2 < 2^63.  The image is converted back
//                    (exact: a power of two) and stored as one double per bin and block, bin-major
//   k_row_sums       (row_walk.hpp) one wave per bin adds the blocks' doubles in the fixed order of wave_sum: H_0 .. H_{B-1} and N_t (slot B, a count:
//                    exact) as doubles, ready for the all-reduce of a domain-decomposed run
//   k_pe_finalize    one block: g_b, S, W_b, the explicit volume derivative, N_t; block sums in the fixed order of block_sum
//   k_pe_forces      a gather over row k with the pairs (W_b, W_b r_b) in LDS (4 KB, a zero pair at either end), so that a bin costs one
//                    16-byte LDS read and two FMAs beside the recurrence: sum W K (r_b - r) = sum W r_b K - r sum W K.  Fixed summation
//                    order, no atomics; the eight lanes' sums are added by three DPP moves.  VIR adds the six sums 1/2 d_a G_b and the explicit diagonal term; VIR = false is the kernel without it
// Worst-case rounding of the accumulation: one add errs by at most half a unit, 2^(x - 63) <= E K(0) 2^-62, a bin takes at most E adds
// per block, so |dH_b| <= sum_blocks E_blk^2 K(0) 2^-62, plus the sum over n blocks in doubles, n 2^-53 H_b.  At the shapes of the tests
// (E_blk <= 4000, K(0) = 4 .. 8, n <= 216) that is below 1e-8 absolute on H of 1e3 .. 1e5: under 1e-11 relative.  Two identical calls
// give identical bits: integer adds inside a block, fixed orders everywhere else.
#include "mtd_device.hpp"
#include "row_walk.hpp"
#include "pair_entropy_device.hpp"
#include "dispatch.hpp"

#include <cmath>
#include <cstring>

namespace
{

using namespace mtd;

constexpr int PE_THREADS = 256;
constexpr int PE_G = 8;                                    // lanes per central particle
constexpr int PE_PPB = PE_THREADS / PE_G;                  // central particles per block and round
constexpr unsigned int PE_MAX_BINS = 256;
constexpr unsigned int PE_MAX_BLOCKS = ROW_MAX_BLOCKS;     // columns of block sums in the scratch
constexpr double PE_G_MIN = 1e-10;

// the scratch, in doubles: sums [258] | value, explicit volume derivative, N_t, (pad) [4] | g [256] | (W_b, W_b r_b) [256][2] | block sums [257][PE_MAX_BLOCKS]
constexpr size_t PE_OFF_SUMS = 0, PE_OFF_VALUE = 258, PE_OFF_EXPL = 259, PE_OFF_NT = 260, PE_OFF_G = 262, PE_OFF_W = PE_OFF_G + PE_MAX_BINS,
                 PE_OFF_PART = PE_OFF_W + 2 * PE_MAX_BINS, PE_TOTAL = PE_OFF_PART + (size_t)(PE_MAX_BINS + 1) * PE_MAX_BLOCKS;

// ---- pass 1: the block's share of H_b and N_t ----------------------------------------------------------------------------------
template<typename S4>
__global__ __launch_bounds__(PE_THREADS) void k_pe_accumulate(const QlArgs<4> a_in, const PeArgs p_in, const S4 *__restrict__ postype,
                                                              const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                              const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                              double *__restrict__ part)
    {
    __shared__ unsigned long long s_h[PE_MAX_BINS + 1];
    __shared__ double s_red[16];
    const QlArgs<4> a = in_vgpr(a_in);
    const PeArgs p = pe_in_vgpr(p_in);
    const unsigned int tid = threadIdx.x, g = tid / PE_G, q = tid % PE_G;
    const unsigned int n_chunks = (a.N + PE_PPB - 1) / PE_PPB;
    for (unsigned int b = tid; b <= PE_MAX_BINS; b += PE_THREADS) s_h[b] = 0ull;
    // the entries of the rows this block walks: every row's count once (lane 0 of its group); below 2^32 by the list's format, exact in a double
    double entries = 0.0;
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const unsigned int i = chunk * PE_PPB + g;
        if (q == 0 && i < a.N) entries += (double)n_neigh[i];
        }
    entries = block_sum(entries, s_red);                   // (its barriers also publish the zeroed image)
    int ex;
    (void)frexp(fmax(entries, 1.0) * p.k0, &ex);          // E K(0) < 2^ex
    const double scale = ldexp(1.0, 62 - ex), inv_scale = ldexp(1.0, ex - 62);
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * PE_PPB + g);
        if (q == 0 && c.i < a.N && (unsigned int)c.p.type == a.type) atomicAdd(&s_h[p.B], 1ull);
        row_walk<PE_G, true>(a, postype, nlist, tab, c, q, [&](const double *tab_k, const unsigned int, const double, const double, const double, const double rsq)
            {
            const double inv_r = rsqrt(rsq);
            double f, fprime_divr;
            smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
            const double fs = f * scale;
            pe_window(p, rsq * inv_r, [&](const int b, const double k)
                {
                if ((unsigned int)b < p.B) atomicAdd(&s_h[b], (unsigned long long)__double2ll_rn(fs * k));
                });
            });
        }
    __syncthreads();
    for (unsigned int b = tid; b <= p.B; b += PE_THREADS)
        part[(size_t)b * PE_MAX_BLOCKS + blockIdx.x] = b < p.B ? (double)s_h[b] * inv_scale : (double)s_h[b];
    }

// ---- g_b, S, W_b, the explicit volume derivative ------------------------------------------------------------------------------
__global__ __launch_bounds__(PE_THREADS) void k_pe_finalize(const PeArgs p, const double volume, double *__restrict__ scratch)
    {
    __shared__ double s_red[16];
    const unsigned int b = threadIdx.x;
    const double n_t = scratch[PE_OFF_SUMS + p.B];
    double g = 0.0, wgt = 0.0, wgt_r = 0.0, t_phi = 0.0, t_glg = 0.0;
    const double rho = n_t / volume;
    if (b < p.B && n_t > 0.0)
        {
        const double rb = ((double)b + 0.5) * p.delta, r2 = rb * rb;
        g = scratch[PE_OFF_SUMS + b] / (4.0 * M_PI * n_t * rho * r2);
        double phi = 1.0;
        if (g >= PE_G_MIN)
            {
            const double lg = log(g);
            phi = g * lg - g + 1.0;
            wgt = -p.delta * lg / (2.0 * n_t);
            wgt_r = wgt * rb;
            t_glg = r2 * g * lg;
            }
        t_phi = r2 * phi;
        }
    const double sum_phi = block_sum(t_phi, s_red);
    const double sum_glg = block_sum(t_glg, s_red);
    const double c = 2.0 * M_PI * rho * p.delta;
    const double value = n_t > 0.0 ? -c * sum_phi : 0.0;
    if (b < PE_MAX_BINS)
        {
        scratch[PE_OFF_G + b] = g;
        scratch[PE_OFF_W + 2 * b] = wgt;
        scratch[PE_OFF_W + 2 * b + 1] = wgt_r;
        }
    if (b == 0)
        {
        scratch[PE_OFF_VALUE] = value;
        scratch[PE_OFF_EXPL] = n_t > 0.0 ? -(value + c * sum_glg) : 0.0;
        scratch[PE_OFF_NT] = n_t;
        }
    }

// ---- pass 2: the gather over row k -----------------------------------------------------------------------------------------------
template<typename S4, bool VIR>
__global__ __launch_bounds__(PE_THREADS) void k_pe_forces(const QlArgs<4> a_in, const PeArgs p_in, const S4 *__restrict__ postype,
                                                          const unsigned int *__restrict__ head_list, const unsigned int *__restrict__ n_neigh,
                                                          const unsigned int *__restrict__ nlist, const double *__restrict__ tab,
                                                          const double *__restrict__ scratch, S4 *__restrict__ force,
                                                          const double *__restrict__ d_bias, const double bias_host,
                                                          typename scalar4_traits<S4>::scalar *__restrict__ virial, const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    __shared__ double2 s_w[PE_MAX_BINS + 2];                  // (W_b, W_b r_b) at [b + 1]; [0] and [B + 1] are zero: where a bin off the table is read
    const QlArgs<4> a = in_vgpr(a_in);
    const PeArgs p = pe_in_vgpr(p_in);
    const unsigned int tid = threadIdx.x, g = tid / PE_G, q = tid % PE_G;
    const unsigned int n_chunks = (a.N + PE_PPB - 1) / PE_PPB;
    for (unsigned int b = tid; b < PE_MAX_BINS + 2; b += PE_THREADS)
        s_w[b] = b >= 1 && b <= p.B ? make_double2(scratch[PE_OFF_W + 2 * (b - 1)], scratch[PE_OFF_W + 2 * (b - 1) + 1]) : make_double2(0.0, 0.0);
    const int top = (int)p.B;
    const double scale = -(d_bias ? *d_bias : bias_host);
    const double n_t = scratch[PE_OFF_NT];
    const double diag = VIR && n_t > 0.0 ? scratch[PE_OFF_EXPL] / n_t : 0.0;
    __syncthreads();
    for (unsigned int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x)
        {
        const RowCentre c = row_centre(a, postype, head_list, n_neigh, chunk * PE_PPB + g);
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        double vxx = 0.0, vxy = 0.0, vxz = 0.0, vyy = 0.0, vyz = 0.0, vzz = 0.0;
        row_walk<PE_G, true>(a, postype, nlist, tab, c, q, [&](const double *tab_k, const unsigned int, const double dx, const double dy, const double dz, const double rsq)
            {
            const double inv_r = rsqrt(rsq), r = rsq * inv_r;
            double f, fprime_divr;
            smoothing_tab<4>(a, tab_k, rsq, inv_r, f, fprime_divr);
            double A = 0.0, C = 0.0;                         // sum W_b K_b and sum W_b r_b K_b
            pe_window(p, r, [&](const int b, const double k)
                {
                const double2 wv = s_w[min(max(b, -1), top) + 1];
                A += wv.x * k;
                C += wv.y * k;
                });
            const double X = C - r * A;                      // sum W_b K_b (r_b - r)
            // u / r, twice: the mirror entry (j, k) gives the same amount
            const double u2 = 2.0 * (fprime_divr * A + f * p.inv_s2 * X * inv_r);
            const double gx = u2 * dx, gy = u2 * dy, gz = u2 * dz;
            Fx += gx;
            Fy += gy;
            Fz += gz;
            if constexpr (VIR)
                {
                vxx += dx * gx, vxy += dx * gy, vxz += dx * gz;
                vyy += dy * gy, vyz += dy * gz, vzz += dz * gz;
                }
            });
        Fx = group_sum<PE_G>(Fx);
        Fy = group_sum<PE_G>(Fy);
        Fz = group_sum<PE_G>(Fz);
        if (q == 0 && c.i < a.N)
            nt_store(scalar4_traits<S4>::make((scalar)(Fx * scale), (scalar)(Fy * scale), (scalar)(Fz * scale), (scalar)0), force + c.i);
        if constexpr (VIR)
            {
            vxx = group_sum<PE_G>(vxx), vxy = group_sum<PE_G>(vxy), vxz = group_sum<PE_G>(vxz);
            vyy = group_sum<PE_G>(vyy), vyz = group_sum<PE_G>(vyz), vzz = group_sum<PE_G>(vzz);
            if (q == 0 && c.i < a.N)                             // (the explicit diagonal term: a particle of the type)
                row_store_virial<true>(virial + c.i, virial_pitch, vxx, vxy, vxz, vyy, vyz, vzz, 0.5 * scale,
                                       (unsigned int)c.p.type == a.type ? scale * diag : 0.0);
            }
        }
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The checks every entry point shares, before a device is touched.  The alignment of the scratch is refused HERE, ahead of the bin count
// (mtd_pe_finalize has no arrays to check, and a misaligned scratch with too many bins is an invalid argument, not an unsupported one);
// refuse_row_arrays, which the two passes over the list call afterwards, finds it aligned.
int pe_check(const mtd_box *box, double r_max, double sigma_r, unsigned int n_bins, const double *d_scratch)
    {
    if (!box || !d_scratch) return MTD_ERR_INVALID_ARGUMENT;
    if (!(r_max > 0.0) || !std::isfinite(r_max) || !(sigma_r > 0.0) || !std::isfinite(sigma_r) || n_bins == 0) return MTD_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)d_scratch & 15u) != 0) return MTD_ERR_INVALID_ARGUMENT;
    if (n_bins > PE_MAX_BINS) return MTD_ERR_UNSUPPORTED;
    return MTD_SUCCESS;
    }

PeArgs pe_args(double r_max, double sigma_r, unsigned int n_bins)
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
    p.w = w < 1048576.0 ? (unsigned int)w : 1048576u;      // (the walks are clipped to the table: a wider window adds no trip)
    p.trips = reach < (double)p.w ? (unsigned int)reach : p.w;
    return p;
    }

// box, window (r_on = r_max + 3 sigma, r_cut = r_max + 4 sigma) and type in the argument block of the Steinhardt passes
int pe_ql_args(QlArgs<4> &a, unsigned int N, const mtd_box *box, double r_max, double sigma_r, unsigned int type)
    {
    static const double no_ref[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    return fill_args<4>(a, N, box, r_max + 4.0 * sigma_r, r_max + 3.0 * sigma_r, 0, type, no_ref, 1, 0);
    }

} // namespace

extern "C" {

size_t mtd_pe_scratch_doubles(unsigned int n_bins)
    {
    (void)n_bins;                                          // one layout for every bin count: the offsets do not move between calls
    return PE_TOTAL;
    }

int mtd_pe_accumulate(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                      const unsigned int *d_n_neigh, const unsigned int *d_nlist, double r_max, double sigma_r, unsigned int n_bins,
                      unsigned int type, double *d_scratch, double **d_sums, unsigned int *n_sums, mtd_stream_t stream)
    {
    if (!d_sums || !n_sums) return MTD_ERR_INVALID_ARGUMENT;
    int rc = pe_check(box, r_max, sigma_r, n_bins, d_scratch);
    if (rc) return rc;
    rc = refuse_row_arrays(n_particles, d_postype && d_head_list && d_n_neigh, dtype, d_scratch, nullptr, 0);
    if (rc) return rc;
    QlArgs<4> a;
    rc = pe_ql_args(a, n_particles, box, r_max, sigma_r, type);
    if (rc) return rc;
    const PeArgs p = pe_args(r_max, sigma_r, n_bins);
    hipStream_t s = (hipStream_t)stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int blocks = row_blocks(n_particles, PE_PPB, PE_MAX_BLOCKS);
    double *part = d_scratch + PE_OFF_PART;
    dispatch_s4(dtype, [&](auto t)
        {
        typedef typename decltype(t)::type S4;
        k_pe_accumulate<S4><<<blocks, PE_THREADS, 0, s>>>(a, p, (const S4 *)d_postype, d_head_list, d_n_neigh, d_nlist, tab, part);
        return 0;
        });
    MTD_LAUNCH_CHECK();
    k_row_sums<PE_MAX_BLOCKS><<<n_bins + 1, MTD_WAVE, 0, s>>>(blocks, n_bins + 1, 0, part, d_scratch + PE_OFF_SUMS);
    MTD_LAUNCH_CHECK();
    *d_sums = d_scratch + PE_OFF_SUMS;
    *n_sums = n_bins + 1;
    return MTD_SUCCESS;
    }

int mtd_pe_finalize(const mtd_box *box, double r_max, double sigma_r, unsigned int n_bins, double *d_scratch, const double **d_value,
                    const double **d_g, mtd_stream_t stream)
    {
    if (!d_value) return MTD_ERR_INVALID_ARGUMENT;
    const int rc = pe_check(box, r_max, sigma_r, n_bins, d_scratch);
    if (rc) return rc;
    const double volume = box->L[0] * box->L[1] * box->L[2];
    if (!(volume > 0.0) || !std::isfinite(volume)) return MTD_ERR_INVALID_ARGUMENT;
    k_pe_finalize<<<1, PE_THREADS, 0, (hipStream_t)stream>>>(pe_args(r_max, sigma_r, n_bins), volume, d_scratch);
    MTD_LAUNCH_CHECK();
    *d_value = d_scratch + PE_OFF_VALUE;
    if (d_g) *d_g = d_scratch + PE_OFF_G;
    return MTD_SUCCESS;
    }

int mtd_pe_forces(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                  const unsigned int *d_n_neigh, const unsigned int *d_nlist, double r_max, double sigma_r, unsigned int n_bins, unsigned int type,
                  const double *d_scratch, const double *d_bias, double bias_host, mtd_stream_t stream, void *d_virial, unsigned int virial_pitch)
    {
    int rc = pe_check(box, r_max, sigma_r, n_bins, d_scratch);
    if (rc) return rc;
    rc = refuse_row_arrays(n_particles, d_postype && d_head_list && d_n_neigh && d_force, dtype, d_scratch, d_virial, virial_pitch);
    if (rc) return rc;
    QlArgs<4> a;
    rc = pe_ql_args(a, n_particles, box, r_max, sigma_r, type);
    if (rc) return rc;
    if (n_particles == 0) return MTD_SUCCESS;
    const PeArgs p = pe_args(r_max, sigma_r, n_bins);
    hipStream_t s = (hipStream_t)stream;
    const double *tab = ql_device_table<4>(s, rc);
    if (rc) return rc;
    const unsigned int blocks = row_blocks(n_particles, PE_PPB, PE_MAX_BLOCKS);
    dispatch_s4(dtype, [&](auto t)
        {
        return dispatch_bool(d_virial != nullptr, [&](auto vir)
            {
            typedef typename decltype(t)::type S4;
            typedef typename scalar4_traits<S4>::scalar scalar;
            k_pe_forces<S4, decltype(vir)::value><<<blocks, PE_THREADS, 0, s>>>(a, p, (const S4 *)d_postype, d_head_list, d_n_neigh, d_nlist, tab,
                                                                                 d_scratch, (S4 *)d_force, d_bias, bias_host, (scalar *)d_virial,
                                                                                 virial_pitch);
            return 0;
            });
        });
    MTD_LAUNCH_CHECK();
    return MTD_SUCCESS;
    }

} // extern "C"
