// row_scale.hpp — a particle's stored gradient and virial sums scaled into its force and virial, written once (env_similarity.hip,
// debye.hip, coordination.hip: the variables whose walk leaves the unscaled sums in the scratch because the count and the bias are not
// known yet).  k_row_scale, launched through row_scale; not on a hot path: one lane per particle, nine loads and seven stores.  The
// kernel is static: a unit that includes this has its own copy, and the linker has nothing to merge.
#pragma once

#include "row_walk.hpp"
#include "dispatch.hpp"

namespace mtd
{

constexpr int ROW_SCALE_THREADS = 256;

// The stored sums of every particle -> force and virial.  `rows` points at the x-gradient row of the first particle: three gradient rows
// and six virial rows (xx, xy, xz, yy, yz, zz) follow each other at `pitch`.  count = *d_count when d_count != NULL (a slot of the
// scratch: N_A, N_t), else count_host (N_global); bias likewise.  With q = bias / count (0 for no count) the force is f_force q times
// the gradient and the virial f_virial q times its sums.  The factors in use are powers of two, so f q has the bits of (f bias) / count,
// the form the units' own kernels had.
template<typename S4, bool VIR>
static __global__ __launch_bounds__(ROW_SCALE_THREADS) void k_row_scale(const unsigned int N, const double *__restrict__ rows, const size_t pitch,
                                                                        const double *__restrict__ d_count, const double count_host,
                                                                        const double f_force, const double f_virial, S4 *__restrict__ force,
                                                                        const double *__restrict__ d_bias, const double bias_host,
                                                                        typename scalar4_traits<S4>::scalar *__restrict__ virial,
                                                                        const unsigned int virial_pitch)
    {
    typedef typename scalar4_traits<S4>::scalar scalar;
    const unsigned int i = blockIdx.x * ROW_SCALE_THREADS + threadIdx.x;
    if (i >= N) return;
    const double count = d_count ? *d_count : count_host;
    const double bias = d_bias ? *d_bias : bias_host;
    const double q = count > 0.0 ? bias / count : 0.0;
    const double scale_f = f_force * q, scale_v = f_virial * q;
    const double *o = rows + i;
    nt_store(scalar4_traits<S4>::make((scalar)(o[0] * scale_f), (scalar)(o[pitch] * scale_f), (scalar)(o[2 * pitch] * scale_f), (scalar)0), force + i);
    if constexpr (VIR)
        row_store_virial<false>(virial + i, virial_pitch, o[3 * pitch], o[4 * pitch], o[5 * pitch], o[6 * pitch], o[7 * pitch], o[8 * pitch], scale_v,
                                0.0);
    }

// k_row_scale over n_particles > 0 particles: the array type from dtype, VIR from d_virial != NULL (both checked by the caller)
inline void row_scale(const int dtype, const unsigned int n_particles, const double *rows, const size_t pitch, const double *d_count,
                      const double count_host, const double f_force, const double f_virial, void *d_force, const double *d_bias,
                      const double bias_host, void *d_virial, const unsigned int virial_pitch, hipStream_t s)
    {
    const unsigned int blocks = (n_particles + ROW_SCALE_THREADS - 1) / ROW_SCALE_THREADS;
    dispatch_s4(dtype, [&](auto t)
        {
        return dispatch_bool(d_virial != nullptr, [&](auto vir)
            {
            typedef typename decltype(t)::type S4;
            typedef typename scalar4_traits<S4>::scalar scalar;
            k_row_scale<S4, decltype(vir)::value><<<blocks, ROW_SCALE_THREADS, 0, s>>>(n_particles, rows, pitch, d_count, count_host, f_force, f_virial,
                                                                                       (S4 *)d_force, d_bias, bias_host, (scalar *)d_virial,
                                                                                       virial_pitch);
            return 0;
            });
        });
    }

}
