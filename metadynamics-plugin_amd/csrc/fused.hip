// fused.hip — the whole metadynamics bias step for lamellar CVs in TWO launches (headline path).
//
// Reference step being replaced (IntegratorMetaDynamics.cc:219-312, 314-588 with LamellarOrderParameterGPU):
//   CV kernel x n_wave x n_cv + final reduce + D2H + host sum  ->  host grid passes (+H2D/D2H of the
//   grid arrays around gpu_update_grid)  ->  host bias scalar  ->  force kernel per CV.
//
// On MI355X a tiny dependent kernel costs 4-7 us of pure latency (measured: profiles/), more than
// streaming the whole 16 MB position array.  So the step is cut only where a true grid-wide
// dependency sits, and everything small is recomputed redundantly per block instead of being
// handed between blocks (no atomics, no in-launch flags, every cross-block hand-off is a kernel
// boundary):
//
//   launch A  k_fused_cv     [apply blocks]  second reweighting pass + accumulate of the PREVIOUS deposit
//                            [CV blocks]     per-CV partial sums over the particles (one pass, all CVs)
//   (multi-GPU: reduce + RCCL all-reduce of n_cv doubles here)
//   launch B  k_fused_force  every block: CV values from the partial sums, V_old(s), well-tempered
//                                         scale, post-deposit node values in closed form on the
//                                         finite-difference stencil -> dV/ds_c           (redundant)
//                            [grid blocks]   Gaussian increment per cell, histogram / sigma-grid bin,
//                                            R += hist_delta, block sums of R*dV and R   (first pass)
//                            [force blocks]  forces of every CV for every particle (one pass)
//
// Round 3: launch B's critical path starts at its first instruction — wave 0 of every block requests the mode tables, the CV
// partial sums and a 6^n-cell patch of the bias grid around the last CV values (kept current by the deferred pass) before
// anything else, the streaming waves their first particles; the barrier that publishes the tables orders LDS traffic only
// (k_fused_force below).
//
// The second reweighting pass needs <dV> = sum(R dV)/sum(R) over the whole grid, i.e. a grid-wide
// dependency on the first pass: it is deferred into the next launch A (or mtd_metad_get_state /
// get_array, which flush it), so the grid arrays are "one apply behind" between B and the next A.
// Forces never wait for it: dV/ds_c only needs grid_old + dV on <= (2 n_cv + 1) 2^n_cv cells.
//
// The pieces of launch B that other kernels carry too — the LDS copy of the chain's result, the first grid pass, the publishing
// wave — are in metad_device.hpp (chain_share, grid_first_pass_*, publish_step); k_fused_force calls them and only adds its time
// stamps between them.  The launches pick their instantiation through the dispatchers of lamellar_host.hpp.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

// Diagnostic build only (-DMTD_STAMPS, tools/build_stamps.sh, tools/stamps.py): s_memrealtime (100 MHz) stamps of one grid block and
// one particle block per kernel, written to a buffer of their own; the product build has no stamps.
#ifdef MTD_STAMPS
__device__ unsigned long long g_stamps[64];
#define MTD_STAMP(slot, cond)                                                   \
    do                                                                          \
        {                                                                       \
        if (cond) g_stamps[slot] = wall_clock64();                              \
        } while (0)
extern "C" int mtd_debug_read_stamps(unsigned long long *host)
    {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 64);
    }
#else
#define MTD_STAMP(slot, cond) do { } while (0)
#endif

#include "lamellar_host.hpp"
#include "metad_host.hpp"
#include "comm_host.hpp"

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace
{

using namespace mtd;

constexpr int FCV_THREADS = 512;
constexpr int FCV_UNROLL = 4;
constexpr int FF_THREADS = 256;
constexpr int FF_UNROLL = 2;

// COMM (particle-sharded step): the last CV block to finish adds up this rank's block partial sums (fixed order) and
// stores the NCV totals into every rank's mailbox over xGMI (comm_device.hpp); launch B polls its local mailbox.
template<typename S4, int NCV, bool FAST, bool COMM, bool ORTHO, int U = FCV_UNROLL>
__global__ __launch_bounds__(FCV_THREADS) void k_fused_cv(const LamKArgs a, const S4 *__restrict__ postype, const unsigned int N,
                                                          double *partials, const MetadCfg c,
                                                          const unsigned int n_apply_blocks, const CommK ck)
    {
    __shared__ float s_coeff[MTD_MAX_CV * MTD_MAX_TYPES];
    __shared__ double s_wave[(FCV_THREADS / MTD_WAVE) * NCV];
    __shared__ double s_red[16];
    __shared__ ModeTables s_mt;

    MTD_STAMP(0, blockIdx.x == 0 && threadIdx.x == 0);
    MTD_STAMP(3, blockIdx.x == n_apply_blocks && threadIdx.x == 0);
    if (blockIdx.x < n_apply_blocks)
        {
        const unsigned int b0 = blockIdx.x * FCV_THREADS;
        apply_cells(c, b0, min(c.len, b0 + FCV_THREADS), blockIdx.x == 0, s_red);
        MTD_STAMP(1, blockIdx.x == 0 && threadIdx.x == 0);
        return;
        }
    const unsigned int block_id = blockIdx.x - n_apply_blocks;
    const unsigned int n_blocks = gridDim.x - n_apply_blocks;

    // the first group of particles is requested before the tables are staged: one memory round trip instead of two
    // (both groups of a thread requested here — the whole position array in the launch's first microsecond — measured SLOWER,
    // launch A 7.4 against 6.9 us: the table loads below queue behind twice the requests in the CU's in-order vector L1)
    RawGroup<S4, U> first;
    // (an empty system — postype may be NULL — reads the head of the partial-sum buffer instead, at least 1024 doubles by the ABI's
    // contract: unconditional loads, see lam_load_group_nc; nothing of it is used, the loop below does not run)
    const S4 *src = N ? postype : (const S4 *)partials;
    lam_load_group_nc<S4, U>(src, N ? N : 1u, block_id * FCV_THREADS + threadIdx.x, n_blocks * FCV_THREADS, first);
    // (the tables: one unconditional load per thread behind the particles' — `a` is the dense form, mtd_fused_cv_pass)
    const CvTableRegs tab = stage_cv_tables_request(a);
    stage_cv_tables_store(tab, s_coeff, s_mt);
    __syncthreads();
    MTD_STAMP(4, block_id == 0 && threadIdx.x == 0);
    float acc[NCV];
#pragma unroll
    for (int i = 0; i < NCV; ++i) acc[i] = 0.0f;
    lam_cv_accumulate<S4, NCV, FAST, U, ORTHO>(a, postype, N, block_id * FCV_THREADS + threadIdx.x, n_blocks * FCV_THREADS,
                                               s_coeff, s_mt, first, acc);
    MTD_STAMP(5, block_id == 0 && threadIdx.x == 0);
    lam_cv_block_reduce<NCV>(acc, s_wave, partials, block_id);
    MTD_STAMP(6, block_id == 0 && threadIdx.x == 0);
    if (COMM)
        {
        // every block also posts its sums for the collector (CV block 0 of this launch) in the mailbox's wire format —
        // value halves tagged with the exchange number, written through to memory: no fence (an agent-scope fence writes
        // back / invalidates the XCD's whole L2), no atomic ticket, and only the collector waits
        constexpr int NS = NCV < 3 ? NCV : 3;
        if (threadIdx.x < NS)
            ll_store(ck.ll + ((size_t)block_id * NS + threadIdx.x) * 2, ck.seq, partials[block_id * NCV + threadIdx.x]);
        if (block_id != 0 || threadIdx.x >= MTD_WAVE) return;
        double v[3] = { 0.0, 0.0, 0.0 };
        const bool expired = ll_collect_wave<NS>(ck, n_blocks, v);
        MTD_STAMP(7, threadIdx.x == 0);
        double tot[3] = { 0.0, 0.0, 0.0 };
#pragma unroll
        for (int i = 0; i < NS; ++i)
            {
            const double t = wave_sum(v[i]);                        // (every lane takes part, whatever it collected)
            tot[i] = expired ? comm_poison() : t;
            }
        MTD_STAMP(8, threadIdx.x == 0);
        comm_send_wave(ck, tot, NS);                            // this rank's totals into every rank's mailbox over xGMI
        MTD_STAMP(9, threadIdx.x == 0);
        }
    }

// Fast form (n_cv <= 3): wave 0 of every block runs the scalar chain with shuffles only while waves 1-3
// already stream their particles and form the unscaled forces; one __syncthreads joins them.
constexpr int FF_STREAM_WAVES = FF_THREADS / MTD_WAVE - 1;
constexpr int FF_STREAM_THREADS = FF_STREAM_WAVES * MTD_WAVE;
constexpr int FF_U = 4;        // particles per register group
// register groups per streaming thread: 2 (= 8 particles, every block of a 10^6-particle launch resident at once) where that fits
// 128 VGPRs WITHOUT SPILLING, else 1.  Checked against the compiler's resource report (-Rpass-analysis=kernel-resource-usage), not
// assumed: until the end of round 3 the double-precision 2-CV instantiation and the accurate-trigonometry fp32 one ran two groups
// with 36 bytes of scratch per lane — reloads from scratch have the latency of memory — and one group in two generations of blocks is
// faster (f64: launch B 33.3 -> 26.4 us, step 41.5 -> 35.1 us).
template<typename S4, int NCV, bool FAST> struct ff_groups { static constexpr int value = 1; };
template<> struct ff_groups<float4, 1, true> { static constexpr int value = 2; };
template<> struct ff_groups<float4, 2, true> { static constexpr int value = 2; };
template<> struct ff_groups<float4, 1, false> { static constexpr int value = 2; };
template<> struct ff_groups<double4, 1, true> { static constexpr int value = 2; };
template<> struct ff_groups<double4, 1, false> { static constexpr int value = 2; };

// ORTHO: the B of `a` is diagonal (LamKArgs::ortho)
template<typename S4, int NCV, bool FAST, int GROUPS, bool COMM, bool ORTHO>
__global__ __launch_bounds__(FF_THREADS, 4) void k_fused_force(const FusedEntry e, const LamKArgs a, const ForcePtrs out,
                                                            const double two_over_n, const MetadCfg c, const int deposit, const CommK ck)
    {
    __shared__ ChainResult s_chain;
    __shared__ float s_wcoef[MTD_MAX_CV * MTD_MAX_TYPES];
    __shared__ double s_red[16];
    __shared__ ModeTables s_mt;

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    // The entry block, read once and ahead of the role branch: ONE scalar round trip in front of wave 0's table and chain loads
    // and of the streaming waves' first particles (they were two, five and seven dependent trips of ~0.14 us).  The grid blocks
    // keep the lowest block indices (force blocks first, measured: the step +0.7 us, the chain of a force block 3.5 -> 4.2 us —
    // profiles/r17).
    const unsigned int n_grid_blocks = fused_entry_read(e);        // (= e.n_passenger_blocks)
    const unsigned int n_blocks = e.n_particle_blocks;
    const S4 *__restrict__ postype = (const S4 *)e.postype;
    const unsigned int N = e.N;
    const unsigned int n_modes = e.n_modes;
    const bool grid_block = blockIdx.x < n_grid_blocks;
    const unsigned int block_id = blockIdx.x - n_grid_blocks;
    const unsigned int stride = n_blocks * FF_STREAM_THREADS;
    const unsigned int first = block_id * FF_STREAM_THREADS + (wave - 1) * MTD_WAVE + lane;
    const unsigned int first1 = first + FF_U * stride;

    ForceRegs<NCV, FF_U> R, R1;
    MTD_STAMP(16, blockIdx.x == 0 && threadIdx.x == 0);
    MTD_STAMP(24, blockIdx.x == n_grid_blocks && threadIdx.x == 0);
    // The chain's wave asks for everything it reads — the partial sums and the grid patch around the last CV values — at entry,
    // right behind the mode tables it stages (the vector L1 of a CU answers in order: the tables come back first, after the
    // ~0.8 us they always took, and the barrier that publishes them orders LDS traffic only, so the chain's loads stay in flight
    // across it): one memory round trip for everything, overlapped with the table staging.  (Tables through scalar loads by
    // another wave: sixteen dependent trips, 2.3 us; tables by another wave through vector loads: they queue behind the chain's
    // requests, the streaming waves start 1.4 us late — both measured.)
    constexpr int NCH = CHAIN_MAX_CV;                  // (a mixed set's grid has more variables than this launch has lamellar CVs)
    ChainPre<NCH> pre;
    int pre_meta = 0;                                  // the patch's validity flag and origin, still in flight (chain_preload_resolve)
    constexpr bool early = !COMM;                      // (sharded step: the sums come out of the mailbox, the chain polls for them)
    float4 th = make_float4(0.f, 0.f, 0.f, 0.f), tq = th;
    float tc = 0.0f;
    if (wave == 0)
        {
        if (!grid_block)
            {
            // first in the queue: the mode tables and this lane's mode coefficient (for the weights formed right behind the chain),
            // unconditional from clamped indices like stage_cv_tables_request: nothing here waits for a count
            static_assert(MTD_MAX_MODES >= MTD_WAVE && MTD_MAX_CV * MTD_MAX_TYPES >= MTD_WAVE, "a lane is a valid index");
            th = a.h[lane];
            tq = a.q[lane];
            tc = (&a.coeff[0][0])[lane];
            }
        // (asking here for one field of every 64-byte line of the grid's configuration, so that the chain finds them in the scalar
        // cache, measured 0.15 us SLOWER per step: the chain's stalls are not scalar-cache misses)
        if (early)
            pre_meta = chain_preload<NCH>(e, pre);
        else
            pre_meta = chain_preload<NCH, false>(e, pre);      // sharded step: the grid patch alone
        }
    // the streaming waves ask for their particles now: the loads need no table, and the barrier below does not wait for them
    // (the first group only: the registers of both groups, live across the barrier beside the chain's preloaded sums — the
    // allocator cannot know that different waves hold them —, spilled)
    RawGroup<S4, FF_U> raw0;
    if (wave != 0 && !grid_block && N) lam_force_request<S4, FF_U>(postype, N, first, stride, raw0);
    if (!grid_block)
        {
        if (wave == 0)
            {
            if (lane < (int)n_modes)
                {
                s_mt.h[lane] = th;
                s_mt.q[lane] = tq;
                }
            if (lane < NCV * MTD_MAX_TYPES) s_wcoef[lane] = tc;        // raw coefficient; scaled in place behind the chain
            }
        lds_barrier();
        }
    MTD_STAMP(25, blockIdx.x == n_grid_blocks && threadIdx.x == 0);
    if (wave == 0)
        {
        ChainResult r;
        chain_preload_resolve<NCH>(pre_meta, pre);
        if constexpr (early)
            {
            double vi[3];
#pragma unroll
            for (int i = 0; i < NCH; ++i) vi[i] = (pre.x[i][0] + pre.x[i][1]) + (pre.x[i][2] + pre.x[i][3]);
            r = chain_wave(c, deposit != 0, true, nullptr, nullptr, false, &pre.patch, pre.patch_ok != 0, true, vi[0], vi[1], vi[2]);
            }
        else
            r = chain_wave(c, deposit != 0, true, &ck, nullptr, false, &pre.patch, pre.patch_ok != 0);
        MTD_STAMP(17, blockIdx.x == 0 && threadIdx.x == 0);
        MTD_STAMP(26, blockIdx.x == n_grid_blocks && threadIdx.x == 0);
        if (lane == 0) chain_share(s_chain, r);
        if (!grid_block && lane < NCV * MTD_MAX_TYPES)
            {
            const unsigned int cv = lane / MTD_MAX_TYPES;
            const unsigned int gs = cv < a.n_cv ? a.slot[cv] : 0u;                 // the grid's variable behind CV cv of the set
            const double b = gs == 0 ? r.bias[0] : (gs == 1 ? r.bias[1] : r.bias[2]);
            s_wcoef[lane] = (cv < a.n_cv) ? (float)((double)s_wcoef[lane] * b * two_over_n) : 0.0f;
            }
        }
    else if (!grid_block && N)                      // N == 0: the grid engine on its own (mtd_metad_update_bias), no particles
        {
        RawGroup<S4, FF_U> raw1;
        if (GROUPS > 1) lam_force_request<S4, FF_U>(postype, N, first1, stride, raw1);     // in flight while group 0 is summed
        lam_force_unscaled_from<S4, NCV, FAST, FF_U, ORTHO>(a, N, first, stride, s_mt, raw0, R);
        if (GROUPS > 1) lam_force_unscaled_from<S4, NCV, FAST, FF_U, ORTHO>(a, N, first1, stride, s_mt, raw1, R1);
        MTD_STAMP(27, blockIdx.x == n_grid_blocks && threadIdx.x == 64);
        }
    lds_barrier();                 // publishes s_chain / s_wcoef (LDS only: nothing that went to global memory is read back)
    MTD_STAMP(18, blockIdx.x == 0 && threadIdx.x == 0);
    MTD_STAMP(28, blockIdx.x == n_grid_blocks && threadIdx.x == 64);

    if (grid_block)
        {
        // ---- first grid pass of a deposit step (metad_device.hpp), in its two halves with a time stamp between them
        const double2 sums = grid_first_pass_cells_256(c, s_chain, blockIdx.x);
        MTD_STAMP(19, blockIdx.x == 0 && threadIdx.x == 0);
        grid_first_pass_sums_256(c, blockIdx.x, sums, s_red);
        MTD_STAMP(20, blockIdx.x == 0 && threadIdx.x == 0);
        }
    else if (wave != 0 && N)
        {
        lam_force_store<S4, NCV, FF_U>(a, out, first, stride, s_wcoef, R);
        if (GROUPS > 1) lam_force_store<S4, NCV, FF_U>(a, out, first1, stride, s_wcoef, R1);
        MTD_STAMP(29, blockIdx.x == n_grid_blocks && threadIdx.x == 64);
        }

    // one block publishes the step's scalars for the host (lazy read-back) and, on non-deposit steps,
    // owns the histogram increment (:366) and the weight read-out (the weight grid is final then)
    if (blockIdx.x == 0 && wave == 0) publish_step(c, s_chain, deposit, nullptr, COMM ? &ck : nullptr);
    }

// General form (any n_cv the grid engine supports): block-cooperative prologue, then the force pass.
template<typename S4, bool FAST>
__global__ __launch_bounds__(FF_THREADS) void k_fused_force_general(const FusedEntry e, const LamKArgs a, const ForcePtrs out,
                                                            const double two_over_n, const MetadCfg c, const int deposit)
    {
    __shared__ EvalShared sh;
    __shared__ float s_wcoef[MTD_MAX_CV * MTD_MAX_TYPES];
    __shared__ double s_red[16];
    __shared__ ModeTables s_mt;

    // grid blocks first, the force blocks behind them, as in k_fused_force
    const unsigned int n_grid_blocks = fused_entry_read_head(e);   // (= e.n_passenger_blocks)
    const unsigned int n_blocks = e.n_particle_blocks;
    const S4 *__restrict__ postype = (const S4 *)e.postype;
    const unsigned int N = e.N;
    const bool grid_block = blockIdx.x < n_grid_blocks;

    load_modes(a, s_mt, true);
    reduce_cv_sources(c, sh.cv, s_red);             // replaces getCurrentValue's D2H + host sum (.cc:323-327)
    __syncthreads();
    evaluate_bias(c, sh, deposit != 0, true);

    if (grid_block)
        {
        // ---- first grid pass of a deposit step: updateGrid (:1002-1047), updateHistogram (:1092-1119),
        //      updateSigmaGrid (:1122-1155), first loop of updateReweightedEstimator (:1070-1075)
        const unsigned int g = blockIdx.x * FF_THREADS + threadIdx.x;
        double s1 = 0.0, s2 = 0.0;
        if (g < c.len)
            {
            const double dV = (c.W * sh.scal) * exp(-gauss_exponent(c, g, sh.cv));
            c.grid_delta[g] = dV;
            unsigned int hd = c.hist_delta[g];
            if (sh.on_grid && g == sh.bin)
                {
                hd += 1;
                c.hist_delta[g] = hd;
                c.sigma_grid_delta[g] += c.det_sigma;
                c.hist_gauss_delta[g] += 1;
                }
            const double R = c.rew[g] + (double)hd;
            c.rew[g] = R;
            s1 = R * dV;
            s2 = R;
            }
        s1 = block_sum(s1, s_red);
        s2 = block_sum(s2, s_red);
        if (threadIdx.x == 0)
            {
            c.gpart[2 * blockIdx.x] = s1;
            c.gpart[2 * blockIdx.x + 1] = s2;
            }
        }

    // one block publishes the step's scalars for the host (lazy read-back) and, on non-deposit steps,
    // owns the histogram increment (:366)
    if (blockIdx.x == 0)
        {
        if (threadIdx.x < c.n_cv)
            {
            c.st->cv[threadIdx.x] = sh.cv[threadIdx.x];
            c.st->bias[threadIdx.x] = sh.bias[threadIdx.x];
            }
        if (threadIdx.x == 0)
            {
            c.st->V = sh.res[0];
            c.st->bin = sh.bin;
            c.st->on_grid = (unsigned int)sh.on_grid;
            if (deposit)
                c.st->scal = sh.scal;
            else
                {
                c.st->w = sh.res[1];
                if (sh.on_grid) c.hist_delta[sh.bin] += 1;
                }
            if (sh.oob[0]) c.st->n_oob += (deposit && c.mode == MTD_MODE_WELL_TEMPERED) ? 2 : 1;
            }
        }
    if (grid_block) return;

    // ---- force blocks
    const unsigned int block_id = blockIdx.x - n_grid_blocks;
    for (unsigned int i = threadIdx.x; i < MTD_MAX_CV * MTD_MAX_TYPES; i += blockDim.x)
        {
        const unsigned int cv = i / MTD_MAX_TYPES;
        const double b = cv < a.n_cv ? sh.bias[a.slot[cv]] : 0.0;
        s_wcoef[i] = (float)((double)a.coeff[cv][i % MTD_MAX_TYPES] * b * two_over_n);
        }
    __syncthreads();
    lam_force_pass<S4, FAST, FF_UNROLL>(a, postype, out, N, block_id * FF_THREADS + threadIdx.x, n_blocks * FF_THREADS, s_wcoef, s_mt);
    }

// ---- measurement aid: per-launch durations of launch B from the dispatch's own time stamps -----------------------------
struct ForceProfile
    {
    std::vector<hipEvent_t> ev;      // start / stop pairs
    size_t used = 0;
    };
ForceProfile g_force_profile;
std::mutex g_force_profile_mutex;      // the hook is process-wide: armed by one thread (bench.py), consulted by every launch

bool force_profile_next(hipEvent_t &start, hipEvent_t &stop)
    {
    std::lock_guard<std::mutex> lock(g_force_profile_mutex);
    ForceProfile &p = g_force_profile;
    if (p.used + 2 > p.ev.size()) return false;
    start = p.ev[p.used];
    stop = p.ev[p.used + 1];
    p.used += 2;
    return true;
    }

// The instantiation of k_fused_cv a pass launches: f(kernel, type_tag<S4>).  The sharded pass (mailbox attached) exists for the
// chain's n_cv <= 3 only.  One expression chooses the kernel whose residency is asked for and the kernel that is launched.
// n_cv: 1 .. MAXCV, with a mailbox 1 .. CHAIN_MAX_CV (fill_kargs refuses 0, mtd_fused_cv_pass the counts above).
template<typename F> int with_fused_cv_kernel(int dtype, bool fast, bool ortho, bool comm, unsigned int n_cv, F &&f)
    {
    return dispatch_s4_fast(dtype, fast, [&](auto s4, auto fast_c)
        {
        using S4 = typename decltype(s4)::type;
        constexpr bool FAST = decltype(fast_c)::value;
        return dispatch_bool(ortho, [&](auto ortho_c)
            {
            constexpr bool ORTHO = decltype(ortho_c)::value;
            if (comm)
                return dispatch_count<CHAIN_MAX_CV>(n_cv, [&](auto n) { return f(k_fused_cv<S4, decltype(n)::value, FAST, true, ORTHO>, s4); });
            return dispatch_count<MAXCV>(n_cv, [&](auto n) { return f(k_fused_cv<S4, decltype(n)::value, FAST, false, ORTHO>, s4); });
            });
        });
    }

} // namespace

namespace mtd
{
// A launch in which a block WAITS for other blocks of the same launch (the collector of the sharded CV pass, every block of the
// one-launch step) is only issued when the whole grid is resident at once: then the wait is one memory round trip after the
// slowest block, never a wait for blocks that have not started.  (With a single waiting block a larger grid could not deadlock
// either — every other block runs to completion unconditionally and frees its slot — but its wait would span whole generations
// of blocks; refused rather than slow.)
unsigned int resident_capacity(const void *kernel, int threads)
    {
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, unsigned int> cache;      // per device: a process may drive several GPUs
    int per_cu = 0, dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        {
        (void)hipGetLastError();
        return 0;
        }
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(std::make_pair(dev, kernel));
    if (it != cache.end()) return it->second;
    unsigned int cap = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) == hipSuccess)
        cap = (unsigned int)per_cu * (unsigned int)n_cu;
    else
        (void)hipGetLastError();
    cache[std::make_pair(dev, kernel)] = cap;
    return cap;
    }
} // namespace mtd

extern "C" {

int mtd_fused_cv_pass(mtd_metad *m, const mtd_lamellar_set *set, unsigned int n_particles, const void *d_postype,
                      int dtype, const mtd_box *global_box, double *d_partials, unsigned int *n_partials,
                      mtd_stream_t stream)
    {
    if (!m) return MTD_ERR_INVALID_ARGUMENT;
    if (m->h_step_err && *m->h_step_err) return MTD_ERR_COMM_TIMEOUT;      // an earlier one-launch step left the grid half-updated
    LamKArgs k;
    int rc = fill_kargs(k, set, global_box);
    if (rc) return rc;
    if (!d_partials || !n_partials || (n_particles && !d_postype)) return MTD_ERR_INVALID_ARGUMENT;
    if (dtype != MTD_F32 && dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    if (set->n_cv > (unsigned int)MAXCV) return MTD_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const unsigned int blocks = lam_cv_blocks(n_particles);
    *n_partials = blocks;
    const unsigned int n_apply = m->pending_apply ? (m->cfg.len + FCV_THREADS - 1) / FCV_THREADS : 0;
    const bool fast = lam_fast_trig(k) != 0;
    if (m->comm && (set->n_cv > (unsigned int)CHAIN_MAX_CV || set->n_cv != m->cfg.n_cv)) return MTD_ERR_UNSUPPORTED;
    const LamKArgs kd = dense_cv_args(k);                           // (the kernel stages its tables with flat loads)
    rc = with_fused_cv_kernel(dtype, fast, k.ortho != 0, m->comm != nullptr, set->n_cv, [&](auto kernel, auto s4) -> int
        {
        using S4 = typename decltype(s4)::type;
        const unsigned int grid = blocks + n_apply;
        CommK ck;
        std::memset(&ck, 0, sizeof(ck));
        if (m->comm)
            {
            // every refusal comes BEFORE the exchange number advances: a call that sends nothing must not consume a number
            // (the peers would wait for an exchange that never happens)
            if (grid > resident_capacity((const void *)kernel, FCV_THREADS)) return MTD_ERR_UNSUPPORTED;
            const int rcn = comm_next(m->comm, ck);                 // this launch sends exchange seq, launch B receives it
            if (rcn) return rcn;
            }
        kernel<<<grid, FCV_THREADS, 0, s>>>(kd, (const S4 *)d_postype, n_particles, d_partials, m->cfg, n_apply, ck);
        MTD_LAUNCH_CHECK();
        return MTD_SUCCESS;
        });
    if (rc) return rc;
    m->pending_apply = 0;
    return MTD_SUCCESS;
    }

int mtd_fused_force_pass(mtd_metad *m, const mtd_lamellar_set *set, unsigned int n_particles, const void *d_postype,
                         void *const *d_force, int dtype, unsigned int n_global, const mtd_box *global_box,
                         unsigned int timestep, mtd_stream_t stream)
    {
    if (!m || !set) return MTD_ERR_INVALID_ARGUMENT;
    if (set->n_cv != m->cfg.n_cv) return MTD_ERR_UNSUPPORTED;   // CV c of the set is CV c of the grid
    return mtd_fused_force_pass_slots(m, set, nullptr, n_particles, d_postype, d_force, dtype, n_global, global_box, timestep, stream);
    }

int mtd_fused_force_pass_slots(mtd_metad *m, const mtd_lamellar_set *set, const unsigned int *slots, unsigned int n_particles,
                               const void *d_postype, void *const *d_force, int dtype, unsigned int n_global,
                               const mtd_box *global_box, unsigned int timestep, mtd_stream_t stream)
    {
    if (!m) return MTD_ERR_INVALID_ARGUMENT;
    LamKArgs k;
    int rc = fill_kargs(k, set, global_box);
    if (rc) return rc;
    if (!d_force || n_global == 0 || (n_particles && !d_postype)) return MTD_ERR_INVALID_ARGUMENT;
    if (dtype != MTD_F32 && dtype != MTD_F64) return MTD_ERR_INVALID_ARGUMENT;
    if (set->n_cv > m->cfg.n_cv) return MTD_ERR_UNSUPPORTED;
    if (!slots && set->n_cv != m->cfg.n_cv) return MTD_ERR_INVALID_ARGUMENT;
    if (slots)
        {
        if (m->comm) return MTD_ERR_UNSUPPORTED;                // the mailbox carries the sums of a pure lamellar set only
        for (unsigned int c = 0; c < set->n_cv; ++c)
            {
            if (slots[c] >= m->cfg.n_cv) return MTD_ERR_INVALID_ARGUMENT;
            k.slot[c] = (unsigned char)slots[c];
            }
        }
    hipStream_t s = (hipStream_t)stream;
    rc = metad_flush(m, s);                                     // a deposit may only be pending across ONE cv pass
    if (rc) return rc;
    ForcePtrs out;
    for (unsigned int c = 0; c < MTD_MAX_CV; ++c) out.f[c] = nullptr;
    for (unsigned int c = 0; c < set->n_cv; ++c)
        {
        if (!d_force[c] && n_particles) return MTD_ERR_INVALID_ARGUMENT;
        out.f[c] = d_force[c];
        }
    const int dep = deposit_due(m, timestep);
    const unsigned int n_grid = dep ? m->cfg.n_gblocks : 0;
    const double two_over_n = 2.0 / (double)n_global;
    const bool fast = lam_fast_trig(k) != 0;
    static const bool force_general = std::getenv("MTD_FUSED_GENERAL") != nullptr;
    CommK ck;
    std::memset(&ck, 0, sizeof(ck));
    if (m->comm)
        {
        if (m->cfg.n_cv > (unsigned int)CHAIN_MAX_CV || force_general) return MTD_ERR_UNSUPPORTED;
        rc = comm_current(m->comm, ck);                         // the exchange the last mtd_fused_cv_pass sent
        if (rc) return rc;
        }
    if (m->cfg.n_cv <= (unsigned int)CHAIN_MAX_CV && !force_general)
        {
        // measurement aid (mtd_profile_force_begin): the launch records its own begin and end through the start / stop events of
        // hipExtLaunchKernelGGL — the dispatch's time stamps, what a kernel trace reports for it
        hipEvent_t ev_start = nullptr, ev_stop = nullptr;
        const bool timed = force_profile_next(ev_start, ev_stop);
        dispatch_s4_fast(dtype, fast, [&](auto s4, auto fast_c)
            {
            using S4 = typename decltype(s4)::type;
            constexpr bool FAST = decltype(fast_c)::value;
            // (1 <= set->n_cv: fill_kargs; set->n_cv <= cfg.n_cv <= CHAIN_MAX_CV: checked above)
            dispatch_count<CHAIN_MAX_CV>(set->n_cv, [&](auto n)
                {
                // (the force blocks of the launch: every streaming thread takes ff_groups<S4, NCV, FAST>::value groups of FF_U
                // particles — the count is formed where the instantiation is chosen, so that the two cannot disagree)
                constexpr int NCV = decltype(n)::value, G = ff_groups<S4, NCV, FAST>::value;
                const unsigned int per_block = FF_STREAM_THREADS * FF_U * G;
                unsigned int fblocks = (n_particles + per_block - 1) / per_block;
                if (fblocks == 0 && n_grid == 0) fblocks = 1;               // still one block to publish the scalars
                const unsigned int grid = n_grid + fblocks;
                dispatch_bool(m->comm != nullptr, [&](auto comm_c)
                    {
                    dispatch_bool(k.ortho != 0, [&](auto ortho_c)
                        {
                        const auto kernel = k_fused_force<S4, NCV, FAST, G, decltype(comm_c)::value, decltype(ortho_c)::value>;
                        const FusedEntry e = fused_entry(m->cfg, d_postype, n_particles, fblocks, n_grid, k.n_modes, k.n_cv);
                        if (timed)
                            hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(FF_THREADS), 0, s, ev_start, ev_stop, 0, e, k, out, two_over_n,
                                                  m->cfg, dep, ck);
                        else
                            kernel<<<grid, FF_THREADS, 0, s>>>(e, k, out, two_over_n, m->cfg, dep, ck);
                        });
                    });
                });
            });
        }
    else
        {
        unsigned int fblocks = lam_force_blocks(n_particles);
        if (n_particles == 0) fblocks = n_grid ? 0 : 1;
        const unsigned int grid = n_grid + fblocks;
        dispatch_s4_fast(dtype, fast, [&](auto s4, auto fast_c)
            {
            using S4 = typename decltype(s4)::type;
            const FusedEntry e = fused_entry(m->cfg, d_postype, n_particles, fblocks, n_grid, k.n_modes, k.n_cv);
            k_fused_force_general<S4, decltype(fast_c)::value><<<grid, FF_THREADS, 0, s>>>(e, k, out, two_over_n, m->cfg, dep);
            });
        }
    MTD_LAUNCH_CHECK();
    m->pending_apply = dep;
    m->w_stale = dep;
    return MTD_SUCCESS;
    }

int mtd_profile_force_begin(unsigned int n_launches)
    {
    std::lock_guard<std::mutex> lock(g_force_profile_mutex);
    ForceProfile &p = g_force_profile;
    for (hipEvent_t e : p.ev) (void)hipEventDestroy(e);
    p.ev.clear();
    p.used = 0;
    for (unsigned int i = 0; i < 2 * n_launches; ++i)
        {
        hipEvent_t e = nullptr;
        MTD_HIP_TRY(hipEventCreate(&e));
        p.ev.push_back(e);
        }
    return MTD_SUCCESS;
    }

int mtd_profile_force_end(double *durations_us, unsigned int capacity, unsigned int *n_out)
    {
    ForceProfile &p = g_force_profile;
    if (!durations_us || !n_out) return MTD_ERR_INVALID_ARGUMENT;
    MTD_HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lock(g_force_profile_mutex);
    unsigned int n = 0;
    for (size_t i = 0; i + 1 < p.used && n < capacity; i += 2)
        {
        float ms = 0.0f;
        MTD_HIP_TRY(hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]));
        durations_us[n++] = 1.0e3 * (double)ms;
        }
    *n_out = n;
    for (hipEvent_t e : p.ev) (void)hipEventDestroy(e);
    p.ev.clear();
    p.used = 0;
    return MTD_SUCCESS;
    }

int mtd_metad_set_comm(mtd_metad *m, mtd_comm *comm)
    {
    if (!m) return MTD_ERR_INVALID_ARGUMENT;
    if (comm && (!comm->connected || m->cfg.n_cv > (unsigned int)CHAIN_MAX_CV || comm->max_doubles < m->cfg.n_cv))
        return comm && !comm->connected ? MTD_ERR_INVALID_ARGUMENT : MTD_ERR_UNSUPPORTED;
    m->comm = comm;
    return MTD_SUCCESS;
    }

} // extern "C"

namespace mtd
{
// The grid engine on its own in the fused form (any CV set with <= 3 collective variables whose values arrive through
// mtd_metad_set_cv_source / set_cv_value): the deferred pass of the previous deposit, then ONE launch for the chain
// (CV values -> V_old -> scale -> closed-form dV/ds) and the first grid pass — instead of k_prepare, k_reweight1, k_apply,
// k_evaluate, four dependent launches of ~5 us latency each.
int fused_grid_step(mtd_metad *m, unsigned int timestep, hipStream_t s)
    {
    if (m->cfg.n_cv > (unsigned int)CHAIN_MAX_CV) return MTD_ERR_UNSUPPORTED;
    int rc = metad_flush(m, s);
    if (rc) return rc;
    LamKArgs k;
    std::memset(&k, 0, sizeof(k));
    k.n_cv = m->cfg.n_cv;
    ForcePtrs out;
    for (unsigned int c = 0; c < MTD_MAX_CV; ++c) out.f[c] = nullptr;
    const int dep = deposit_due(m, timestep);
    const unsigned int n_grid = dep ? m->cfg.n_gblocks : 0;
    const unsigned int fblocks = n_grid ? 0 : 1;                    // still one block to publish the scalars
    const unsigned int grid = n_grid + fblocks;
    CommK ck;
    std::memset(&ck, 0, sizeof(ck));
    const FusedEntry e = fused_entry(m->cfg, nullptr, 0, fblocks, n_grid, 0, k.n_cv);
    switch (m->cfg.n_cv)
        {
        case 1: k_fused_force<float4, 1, true, 1, false, false><<<grid, FF_THREADS, 0, s>>>(e, k, out, 0.0, m->cfg, dep, ck); break;
        case 2: k_fused_force<float4, 2, true, 1, false, false><<<grid, FF_THREADS, 0, s>>>(e, k, out, 0.0, m->cfg, dep, ck); break;
        default: k_fused_force<float4, 3, true, 1, false, false><<<grid, FF_THREADS, 0, s>>>(e, k, out, 0.0, m->cfg, dep, ck); break;
        }
    MTD_LAUNCH_CHECK();
    m->pending_apply = dep;
    m->w_stale = dep;
    if (dep) announce_pending_apply(m, s);              // a later kernel of the step may take the deferred pass along (metad.hip)
    return MTD_SUCCESS;
    }
} // namespace mtd
