// pair_entropy_device.hpp — what the two pair-entropy units share on the device (pair_entropy.hip: the global S2; pair_entropy_local.hip:
// the per-particle s_i): the bin constants of a launch, their move into vector registers and the window recurrence of one list entry.
// The design of the recurrence is stated in the header of pair_entropy.hip.
#pragma once

#include "mtd_device.hpp"
#include "row_walk.hpp"

namespace mtd
{

struct PeArgs
    {
    double delta, inv_delta;                               // r_max / B, B / r_max
    double inv_s2;                                         // 1 / sigma^2
    double neg_half_inv_s2;                                // -1 / (2 sigma^2)
    double k0;                                             // K(0) = 1 / (sqrt(2 pi) sigma)
    double s, s2;                                          // exp(-Delta^2 / 2 sigma^2) and its square
    unsigned int B, w;
    unsigned int trips, _pad;                              // min(w, the largest centre bin + 1): beyond it both chains are off the table
    };

// the bin constants beside the box (row_walk.hpp, in_vgpr): what the per-bin loop multiplies with lives in vector registers
__device__ __forceinline__ PeArgs pe_in_vgpr(PeArgs p)
    {
    p.delta = in_vgpr(p.delta), p.inv_delta = in_vgpr(p.inv_delta), p.inv_s2 = in_vgpr(p.inv_s2), p.neg_half_inv_s2 = in_vgpr(p.neg_half_inv_s2);
    p.k0 = in_vgpr(p.k0), p.s = in_vgpr(p.s), p.s2 = in_vgpr(p.s2);
    return p;
    }

// The window of one entry at distance r: calls bin(b, K_b) for the centre bin c, then for c + t and c - t, t = 1 .. trips, both chains of
// the recurrence side by side (header).  The trip count is the same for every lane (no divergent loop); b may lie OUTSIDE the table
// (below 0, above B - 1, beyond the window's clipped end): the body tests or clamps it.
template<typename F> __device__ __forceinline__ void pe_window(const PeArgs &p, const double r, F &&bin)
    {
    const int bc = (int)fmin(fmax(floor(r * p.inv_delta), 0.0), 1e9);      // (a NaN distance, two particles in one place, lands in bin 0)
    const double xc = ((double)bc + 0.5) * p.delta - r;
    const double kc = p.k0 * exp(xc * xc * p.neg_half_inv_s2);
    const double e = exp(-xc * p.delta * p.inv_s2);
    bin(bc, kc);
    double ku = kc, fu = e * p.s, kd = kc, fd = p.s / e;
    const int trips = (int)p.trips;
    for (int t = 1; t <= trips; ++t)
        {
        ku *= fu;
        fu *= p.s2;
        kd *= fd;
        fd *= p.s2;
        bin(bc + t, ku);
        bin(bc - t, kd);
        }
    }

}
