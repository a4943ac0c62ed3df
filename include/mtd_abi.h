/* include/mtd_abi.h — C ABI of libmtd_hip.so: the MI355X (gfx950) metadynamics hot path.
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain pointers, sizes
 * and PODs (no torch / pybind / HOOMD types), enqueues work on an explicit HIP stream and returns
 * an int status (0 = success, >0 = hipError_t, <0 = MTD_ERR_*).  No entry point synchronises the
 * device unless its comment says so.  The host classes in metadynamics-plugin_amd/host (the mirror
 * of the reference's CollectiveVariable / IntegratorMetaDynamics C++ classes) and the test / bench
 * harness (ctypes) call nothing else.
 *
 * Each block cites the reference interface it replaces (file:line under
 * /root/reference/metadynamics/).  The reference's kernel drivers are C++ free functions taking
 * HOOMD PODs (BoxDim, Index2D, GPUPartition) and raw device pointers borrowed from ArrayHandle;
 * here BoxDim becomes `mtd_box`, the default stream becomes an explicit `mtd_stream_t`, and the
 * tiny per-CV configuration arrays (Miller indices, per-type mode coefficients, grid geometry) are
 * passed as HOST pointers and travel in the kernel-argument segment instead of device arrays.
 *
 * Particle arrays keep HOOMD's layout: postype = Scalar4 (x, y, z, type bit-cast into w),
 * force = Scalar4 (fx, fy, fz, energy), with Scalar selected per call by `dtype`
 * (MTD_F32: w holds the int32 type bit pattern; MTD_F64: the LOW 32 bits of w hold it, HOOMD's
 * __scalar_as_int convention).  All reductions and the whole bias grid are double precision.
 */
#ifndef MTD_ABI_H
#define MTD_ABI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTD_ABI_VERSION 1

typedef void *mtd_stream_t; /* hipStream_t */

enum mtd_dtype { MTD_F32 = 0, MTD_F64 = 1 };

enum mtd_status
    {
    MTD_SUCCESS = 0,
    MTD_ERR_INVALID_ARGUMENT = -1, /* the reference throws std::runtime_error for these */
    MTD_ERR_UNSUPPORTED = -2,
    MTD_ERR_NO_DEVICE = -3,
    MTD_ERR_COMM_TIMEOUT = -4,     /* a mailbox wait expired: the step is poisoned (NaN), sticky until the mailbox is destroyed */
    MTD_ERR_COLLECTIVE = -5        /* an RCCL call failed (mtd_rccl_last_error says which and why), or the walkers of a multiple-walker
                                      run disagree on stride / add_hills / timestep (they would enter different collectives) */
    };

/* HOOMD BoxDim as a POD (reference: hoomd/BoxDim.h, passed by const-ref to every driver) */
typedef struct mtd_box
    {
    double L[3];
    double lo[3];
    double xy, xz, yz;
    unsigned char periodic[3];
    unsigned char _pad[5];
    } mtd_box;

int mtd_abi_version(void);
const char *mtd_status_string(int status);
/* number of visible HIP devices, or a negative mtd_status */
int mtd_device_count(void);

/* ================================================================================================
 * Lamellar order parameter
 * replaces LamellarOrderParameterGPU.cuh:21-54 (gpu_calculate_fourier_modes, gpu_compute_sq_forces)
 * ============================================================================================== */

#define MTD_MAX_CV 8     /* lamellar CVs fused into one pass over the particles */
#define MTD_MAX_MODES 64 /* total Fourier modes over the fused CVs */
#define MTD_MAX_TYPES 16

/* n_cv lamellar CVs evaluated in ONE pass over the positions (the reference launches one
 * kernel grid per CV and re-reads every position n_wave times, LamellarOrderParameterGPU.cu:130). */
typedef struct mtd_lamellar_set
    {
    unsigned int n_cv;
    unsigned int n_types;
    unsigned int n_modes;                       /* total, CV-major: modes of CV c are [first[c], first[c+1]) */
    unsigned int first[MTD_MAX_CV + 1];
    int hkl[MTD_MAX_MODES][3];                  /* Miller indices (cv.py:251-256, std_vector_int3) */
    double coeff[MTD_MAX_CV][MTD_MAX_TYPES];    /* per-type mode coefficients (cv.py:242-249) */
    int trig_mode;                              /* MTD_TRIG_DEFAULT (0: the process default, mtd_lamellar_set_fast_trig), MTD_TRIG_HARDWARE
                                                   or MTD_TRIG_ACCURATE for THIS set's kernels — see below */
    } mtd_lamellar_set;

enum mtd_trig_mode { MTD_TRIG_DEFAULT = 0, MTD_TRIG_HARDWARE = 1, MTD_TRIG_ACCURATE = 2 };

/* workspace (device doubles) needed for n_particles: block partial sums */
size_t mtd_lamellar_scratch_doubles(unsigned int n_particles);

/* gpu_calculate_fourier_modes (LamellarOrderParameterGPU.cuh:21-29, .cu:104-147), one CV:
 * d_fourier_modes[2*n_wave] = sum_j a(type_j) (cos, sin)(q_k . r_j), k < n_wave, as doubles.
 * lattice_vectors / mode are HOST arrays (int[3*n_wave], double[n_types]). */
int mtd_calculate_fourier_modes(unsigned int n_wave, const int *lattice_vectors, unsigned int n_particles,
                                const void *d_postype, int dtype, const double *mode, unsigned int n_types,
                                double *d_fourier_modes, double *d_scratch, const mtd_box *global_box,
                                mtd_stream_t stream);

/* Fused hot path (no reference counterpart; replaces computeCV's kernel + D2H + host sum,
 * LamellarOrderParameterGPU.cc:34-96): for every CV c of the set,
 *   d_partials[b * n_cv + c] = sum over the particles of block b of a_c(type_j) sum_k cos(q_k . r_j)
 * for b < *n_partials.  The CV value is s_c = (1/N_global) sum_b d_partials[b*n_cv + c]; that last
 * tiny sum is done by the consumer (mtd_metad_set_cv_source) or by mtd_reduce_partials. */
int mtd_lamellar_cv_partials(const mtd_lamellar_set *set, unsigned int n_particles, const void *d_postype,
                             int dtype, const mtd_box *global_box, double *d_partials,
                             unsigned int *n_partials, mtd_stream_t stream);

/* out[c] = shift + scale * sum_{b<n_partials} d_partials[b*stride + c], c < count (one tiny block,
 * fixed summation order => bitwise reproducible) */
int mtd_reduce_partials(const double *d_partials, unsigned int n_partials, unsigned int stride,
                        unsigned int count, double scale, double shift, double *d_out, mtd_stream_t stream);

/* gpu_compute_sq_forces (LamellarOrderParameterGPU.cuh:43-54, .cu:198-236), one CV, bias as a host
 * scalar exactly like the reference: F_j = bias * (2/n_global) a(type_j) sum_k q_k sin(q_k . r_j), w = 0 */
int mtd_compute_sq_forces(unsigned int n_particles, const void *d_postype, void *d_force, int dtype,
                          unsigned int n_wave, const int *lattice_vectors, const double *mode,
                          unsigned int n_types, unsigned int n_global, double bias,
                          const mtd_box *global_box, mtd_stream_t stream);

/* Fused hot path: forces of all CVs of the set in one pass; the bias factors dV/ds_c are read from
 * DEVICE memory (d_bias[c], written by mtd_metad_update_bias) so no host round trip separates the
 * CV reduction from the force pass.  d_force[c] (host array of n_cv device pointers) receives CV c's
 * Scalar4 force array (the reference's per-CV ForceCompute::m_force). */
int mtd_lamellar_forces(const mtd_lamellar_set *set, unsigned int n_particles, const void *d_postype,
                        void *const *d_force, int dtype, unsigned int n_global, const double *d_bias,
                        const mtd_box *global_box, mtd_stream_t stream);

/* Trigonometry of the lamellar kernels.  MTD_TRIG_HARDWARE: v_sin_f32 / v_cos_f32 on the phase in turns — what the reference's
 * GPU kernels do (fast::sin / fast::cos, LamellarOrderParameterGPU.cu:36-37, 180); MTD_TRIG_ACCURATE: ocml sinpi / cospi.  The
 * mode is a property of the CV SET (mtd_lamellar_set::trig_mode); sets that leave it at MTD_TRIG_DEFAULT take the process default,
 * which this call sets (1, the initial value: hardware; 0: accurate) — two sets with different modes can run in one process.
 * PRECONDITION of the hardware mode: the instructions' domain is +-256 turns, outside it they return cos = 1 / sin = 0 without
 * any error.  A phase is sum_i hkl_i * g_i with g_i = b_i . r the fractional coordinate: positions inside the box give
 * |phase| <= (|h| + |k| + |l|) / 2.  The library therefore takes the hardware path only for mode sets with |h| + |k| + |l| <= 100
 * per mode (others run the accurate path whatever the mode says), which leaves room for particles up to FIVE box lengths outside
 * the box; a caller that hands over UNWRAPPED coordinates further out than that must select MTD_TRIG_ACCURATE (correct for any
 * range) — HOOMD keeps its particles wrapped, the reference's kernels rely on the same. */
int mtd_lamellar_set_fast_trig(int enable);
int mtd_lamellar_get_fast_trig(void);

/* ================================================================================================
 * Bias grid ("IntegratorMetaDynamics" grid engine), device resident
 * replaces IntegratorMetaDynamics.cuh:1-11 (gpu_update_grid) and moves the host passes of
 * IntegratorMetaDynamics.cc:314-588, 663-776, 1053-1155 onto the device
 * ============================================================================================== */

#define MTD_METAD_MAX_CV 6

enum mtd_metad_mode { MTD_MODE_STANDARD = 0, MTD_MODE_WELL_TEMPERED = 1 };

/* gpu_update_grid (IntegratorMetaDynamics.cuh:1-11, .cu:67-93):
 * d_grid_delta[g] += W * scal * exp(-1/2 sum_ij d_i d_j sigma_inv_ij^2) over all num_elements cells,
 * d = node coordinate - *d_current_val.  lengths/cv_min/cv_max/sigma_inv are HOST arrays,
 * d_current_val and d_grid_delta are device doubles. */
int mtd_update_grid(unsigned int num_elements, const unsigned int *lengths, unsigned int dim,
                    const double *d_current_val, double *d_grid_delta, const double *cv_min,
                    const double *cv_max, const double *sigma_inv, double scal, double W,
                    mtd_stream_t stream);

typedef struct mtd_metad mtd_metad; /* opaque; owns the ten grid arrays (IntegratorMetaDynamics.h:276-330) */

/* constructor + registerCollectiveVariable + setGrid(true) + prepRun/setupGrid
 * (IntegratorMetaDynamics.cc:23-72, .h:117-134, .cc:778-815, 121-200, 590-661).
 * Returns MTD_ERR_INVALID_ARGUMENT where the reference throws (cv_min >= cv_max, num_points < 2). */
int mtd_metad_create(mtd_metad **out, unsigned int n_cv, const double *sigma, const double *cv_min,
                     const double *cv_max, const unsigned int *num_points, double W, double T_shift,
                     double T, unsigned int stride, int mode, int add_bias);
int mtd_metad_destroy(mtd_metad *m);

int mtd_metad_set_stride(mtd_metad *m, unsigned int stride);   /* setStride  .h:205 */
int mtd_metad_set_add_hills(mtd_metad *m, int add_bias);       /* setAddHills .h:237 */
int mtd_metad_set_mode(mtd_metad *m, int mode);                /* setMode    .h:197 */
int mtd_metad_set_sigma_inv(mtd_metad *m, const double *sigma_inv /* n_cv^2, host */);
int mtd_metad_reset_histogram(mtd_metad *m, mtd_stream_t stream); /* resetHistogram .cc:1195-1203 */

/* Where the engine takes CV c's current value from (replaces the host
 * `Scalar val = cv->getCurrentValue(timestep)` of .cc:323-327):
 *   s_c = shift + scale * sum_{b<n_partials} d_partials[b*stride + offset]
 * d_partials stays owned by the caller and must stay valid; n_partials may be 1 (a plain value). */
int mtd_metad_set_cv_source(mtd_metad *m, unsigned int cv, const double *d_partials, unsigned int n_partials,
                            unsigned int stride, unsigned int offset, double scale, double shift);

/* CV c's value is a host scalar (box-shape CVs such as AspectRatio / Density): it travels in the
 * kernel arguments of the next update.  This is also the default source (value 0). */
int mtd_metad_set_cv_value(mtd_metad *m, unsigned int cv, double value);

/* device double[n_cv]: dV/ds_c after the most recent mtd_metad_update_bias — what the reference
 * hands to CollectiveVariable::setBiasFactor (.cc:578-584).  Force kernels read it in place. */
const double *mtd_metad_bias_device(const mtd_metad *m);
/* device double[n_cv]: the CV values the engine used in the most recent update */
const double *mtd_metad_cv_device(const mtd_metad *m);

/* updateBiasPotential (.cc:314-588), grid branch, entirely on the device and asynchronous:
 * histogram; on deposit steps (add_bias && timestep % stride == 0) sigma grid, well-tempered scale,
 * Gaussian deposit, reweighted estimator, accumulate + clear; then dV/ds_c (finite difference of
 * the multilinear interpolant), V(s) and the reweighting factor w(s). */
int mtd_metad_update_bias(mtd_metad *m, unsigned int timestep, mtd_stream_t stream);

/* The same split at the multiple-walker exchange (.cc:393-409): phase A fills the four delta arrays
 * (packed contiguously, see mtd_metad_delta_buffers) and returns *deposited; the caller all-reduces
 * them over the walkers (RCCL); phase B reweights, accumulates and evaluates. */
int mtd_metad_update_phase_a(mtd_metad *m, unsigned int timestep, int *deposited, mtd_stream_t stream);
int mtd_metad_update_phase_b(mtd_metad *m, int deposited, mtd_stream_t stream);
/* d_real: {grid_delta[G], sigma_grid_delta[G]} doubles; d_count: {hist_delta[G], hist_gauss_delta[G]} uint32 */
int mtd_metad_delta_buffers(mtd_metad *m, double **d_real, unsigned int **d_count, unsigned int *num_elements);

/* Host-visible state (SYNCHRONISES the stream): what getCurrentValue / the log quantities
 * "bias", "weight" (.h:161-189) report.  Any output pointer may be NULL. */
int mtd_metad_get_state(mtd_metad *m, double *cv, double *bias, double *bias_potential, double *weight,
                        unsigned int *num_gaussians, unsigned int *num_out_of_bounds, mtd_stream_t stream);
double mtd_metad_sigma_determinant(const mtd_metad *m); /* sigmaDeterminant .cc:1296-1313 */
unsigned int mtd_metad_num_elements(const mtd_metad *m);

/* raw grid arrays and the hill count for writeGrid / readGrid (.cc:831-1000); all three SYNCHRONISE the stream.  which: 0 grid, 1 grid_delta,
 * 2 reweighted, 3 weight, 4 sigma_grid, 5 sigma_grid_delta (double[G]); 6 hist, 7 hist_delta,
 * 8 hist_gauss, 9 hist_gauss_delta (uint32[G]) */
int mtd_metad_get_array(mtd_metad *m, int which, void *host_out, mtd_stream_t stream);
int mtd_metad_set_array(mtd_metad *m, int which, const void *host_in, mtd_stream_t stream);
int mtd_metad_set_num_gaussians(mtd_metad *m, unsigned int n, mtd_stream_t stream);
/* The device address of one of the arrays above (NULL for a bad index).  A caller that WRITES the bias grid (which = 0) through
 * the pointer must say so after every such write, on the stream the write ran on, with mtd_metad_grid_touched: the engine keeps
 * a small patch of grid values around the last CV values (the scalar chain's preload) which is then rewritten from the grid
 * before its next use.  Fetching the pointer for which = 0 invalidates the patch once, on the NULL stream (kept for callers
 * that write before their next update on that stream); returns NULL when that fails.  That one invalidation is NOT ordered with
 * work on a non-blocking stream: an update still queued there validates the patch again when it runs.  A caller with a stream of
 * its own must not rely on it: mtd_metad_grid_touched after every write is what tells the engine. */
void *mtd_metad_device_array(mtd_metad *m, int which);
int mtd_metad_grid_touched(mtd_metad *m, mtd_stream_t stream);

/* ================================================================================================
 * Fused bias step for lamellar CVs — the headline path (no reference counterpart: it replaces the
 * whole of IntegratorMetaDynamics::updateBiasPotential + the CVs' computeCV / computeBiasForces,
 * IntegratorMetaDynamics.cc:314-588, LamellarOrderParameterGPU.cc:34-132, by TWO launches)
 * ============================================================================================== */

/* Launch A: per-CV partial sums over the particles (as mtd_lamellar_cv_partials) and, in the same
 * launch, the deferred second reweighting pass + accumulate of the previous deposit if one is pending.
 * Between the two passes the caller registers the sums as CV sources (mtd_metad_set_cv_source, once)
 * or, multi-GPU, reduces them (mtd_reduce_partials), all-reduces over RCCL and registers the result. */
int mtd_fused_cv_pass(mtd_metad *m, const mtd_lamellar_set *set, unsigned int n_particles, const void *d_postype,
                      int dtype, const mtd_box *global_box, double *d_partials, unsigned int *n_partials,
                      mtd_stream_t stream);

/* Launch B: updateBiasPotential(timestep) for the CV values defined by the registered sources
 * (histogram; on deposit steps sigma grid, well-tempered scale, Gaussian increment, first reweighting
 * pass; dV/ds_c, V(s)) and, in the same launch, the bias forces of every CV of the set
 * (CV c of the set must be CV c of the grid).  The second reweighting pass + accumulate stay pending
 * until the next mtd_fused_cv_pass or any call that reads the grid (get_state / get_array flush it). */
int mtd_fused_force_pass(mtd_metad *m, const mtd_lamellar_set *set, unsigned int n_particles, const void *d_postype,
                         void *const *d_force, int dtype, unsigned int n_global, const mtd_box *global_box,
                         unsigned int timestep, mtd_stream_t stream);

/* The same launch for a MIXED set of collective variables: `set` holds the lamellar CVs among the grid's variables,
 * slots[c] is the grid variable behind CV c of the set (any order, each < the grid's n_cv); the other variables' values
 * arrive through their registered sources as in mtd_metad_update_bias, which this call replaces for the step, and their
 * force kernels read mtd_metad_bias_device afterwards.  slots == NULL: identity (set->n_cv must equal the grid's). */
int mtd_fused_force_pass_slots(mtd_metad *m, const mtd_lamellar_set *set, const unsigned int *slots, unsigned int n_particles,
                               const void *d_postype, void *const *d_force, int dtype, unsigned int n_global,
                               const mtd_box *global_box, unsigned int timestep, mtd_stream_t stream);

/* The whole step in ONE launch (fused_step.hip): a persistent kernel, one 1024-thread block per compute unit, keeps its
 * particles in registers between the CV phase and the force phase (the positions are read once) and hands the two grid-wide
 * sums of a step (CV sums; sum R dV, sum R of the reweighting) from block to block inside the launch in the mailbox's wire
 * format.  Both reweighting passes run in the launch: the grid arrays are final when it ends (nothing stays pending).
 * Sharded run (mtd_metad_set_comm): block 0 sends the local sums, every block's chain polls the local mailbox.
 * Envelope: n_cv <= 3, CV c of the set is CV c of the grid, at most 4096 particles per compute unit, the whole grid of
 * blocks resident at once, and the form selected (mtd_fused_step_set_mode); otherwise the call runs mtd_fused_cv_pass + mtd_fused_force_pass with
 * d_scratch (>= mtd_lamellar_scratch_doubles) as the partial-sum buffer.  Every in-launch wait is bounded
 * (MTD_COMM_TIMEOUT_MS): an expired one poisons the step (NaN) and later calls return MTD_ERR_COMM_TIMEOUT.
 * Replaces per step: LamellarOrderParameterGPU.cc:34-132 for every CV + IntegratorMetaDynamics.cc:314-588. */
int mtd_fused_step(mtd_metad *m, const mtd_lamellar_set *set, unsigned int n_particles, const void *d_postype,
                   void *const *d_force, int dtype, unsigned int n_global, const mtd_box *global_box, double *d_scratch,
                   unsigned int timestep, mtd_stream_t stream);
/* launches the last mtd_fused_step of this engine took: 1 (persistent kernel) or 2 (two-launch form); 0 before the first */
unsigned int mtd_fused_step_launches(const mtd_metad *m);
/* which form mtd_fused_step takes for this engine: 1 the persistent kernel wherever its envelope allows, 0 always the
 * two-launch form, -1 (default) the environment (MTD_FUSED_STEP=1 / 0) and without it the two-launch form, which measures
 * faster at 10^6 particles */
int mtd_fused_step_set_mode(mtd_metad *m, int mode);

/* Measurement aid (bench.py): the next n_launches launches of mtd_fused_force_pass record their own begin and end through the
 * start / stop events of hipExtLaunchKernelGGL — the dispatch's time stamps, i.e. the duration a kernel trace reports for the
 * launch, without a profiler attached.  mtd_profile_force_end SYNCHRONISES, returns the durations (microseconds) of the
 * launches made since _begin and releases the events. */
int mtd_profile_force_begin(unsigned int n_launches);
int mtd_profile_force_end(double *durations_us, unsigned int capacity, unsigned int *n_out);

/* ================================================================================================
 * RCCL all-reduce of large device buffers (rccl.hip; RCCL is bound at run time, no link-time dependency)
 * replaces: the multiple-walker exchange IntegratorMetaDynamics.cc:393-409 (four host-staged MPI_Allreduce over
 * m_partition_comm) and, for a particle-sharded mesh CV, the mesh exchange of OrderParameterMesh.cc:263-316, 659-746.
 * ============================================================================================== */
#define MTD_RCCL_ID_BYTES 128
#define MTD_ELEM_F64 1
#define MTD_ELEM_U32 2
typedef struct mtd_rccl mtd_rccl;
/* rank 0: a fresh unique id (MTD_RCCL_ID_BYTES bytes) for the caller's control plane to hand to every rank */
int mtd_rccl_unique_id(void *out_id);
/* collective over the `world` ranks holding the same id; one communicator per process and GPU */
int mtd_rccl_create(mtd_rccl **out, const void *unique_id, unsigned int rank, unsigned int world);
/* in-place sum over ranks of `count` elements (MTD_ELEM_F64 doubles or MTD_ELEM_U32 unsigned ints) on `stream` */
int mtd_comm_allreduce_large(mtd_rccl *r, void *d_buffer, size_t count, int elem, mtd_stream_t stream);
unsigned int mtd_rccl_world(const mtd_rccl *r);
unsigned int mtd_rccl_rank(const mtd_rccl *r);
int mtd_rccl_destroy(mtd_rccl *r);
/* text of the last RCCL failure of this process ("ncclAllReduce: unhandled system error", ...), "" when there was none */
const char *mtd_rccl_last_error(void);
/* Multiple walkers in one call (IntegratorMetaDynamics.cc:363-451 with m_multiple_walkers): histogram / Gaussian increments
 * of this walker (mtd_metad_update_phase_a), sum of {grid_delta, sigma_grid_delta} and {hist_delta, hist_gauss_delta} over
 * the walkers (two all-reduces: the delta groups are contiguous), reweighting + accumulate + evaluation
 * (mtd_metad_update_phase_b).  Every walker must call it with the same timestep.  walkers == NULL: one walker (the reference in
 * a run with a single partition, as test/test_2d.py:29 does). */
int mtd_metad_update_bias_walkers(mtd_metad *m, mtd_rccl *walkers, unsigned int timestep, mtd_stream_t stream);

/* ================================================================================================
 * xGMI mailbox: all-reduce (sum) of a few doubles between the GPUs of one node, one process per GPU
 * replaces the host-staged MPI_Allreduce of the per-step CV sums (LamellarOrderParameterGPU.cc:69-77,
 * SteinhardtQl.cc:183-191, WellTemperedEnsemble.cc:57-63) without a collective-library call on the
 * critical path: every rank's kernels store their values straight into the peers' mailboxes over xGMI
 * (hipIpc-mapped uncached device memory) and poll their own.  Large buffers (replicated mesh, packed
 * walker deltas) stay on RCCL.  Every wait is bounded: a peer that never arrives is a counted timeout
 * (MTD_COMM_TIMEOUT_MS, default 5000), not a hang.
 * ============================================================================================== */

#define MTD_COMM_MAX_RANKS 8     /* the GPUs of one node */
#define MTD_COMM_HANDLE_BYTES 64 /* sizeof(hipIpcMemHandle_t) */

typedef struct mtd_comm mtd_comm; /* opaque; owns this rank's mailbox and the mappings of the peers' */

/* max_doubles: largest message (per rank) in doubles, <= 4096.  SYNCHRONISES (allocation + clear). */
int mtd_comm_create(mtd_comm **out, unsigned int rank, unsigned int world, unsigned int max_doubles);
/* the IPC handle of this rank's mailbox (MTD_COMM_HANDLE_BYTES bytes) for the caller's control plane to gather */
int mtd_comm_handle(mtd_comm *c, void *out_handle);
/* handles: world * MTD_COMM_HANDLE_BYTES bytes in rank order (the own entry is ignored).  world == 1 needs no connect. */
int mtd_comm_connect(mtd_comm *c, const void *handles);
/* d_values[0..n) <- sum over ranks, added up in rank order starting from +0.0 (the same bits on every rank).  Every rank must
 * issue the same sequence of exchanges (this call and the fused step's) on its comm.  A message of more than 60000 / (8 world)
 * doubles is refused (MTD_ERR_UNSUPPORTED); a refused call takes no exchange number, so the communicator stays usable. */
int mtd_comm_allreduce_small(mtd_comm *c, double *d_values, unsigned int n, mtd_stream_t stream);
/* number of timed-out waits so far; SYNCHRONISES the stream */
int mtd_comm_status(mtd_comm *c, unsigned int *timeouts, mtd_stream_t stream);
/* Bulk buffers readable by every rank (the slab-decomposed mesh pulls its peers' slabs straight out of them over xGMI):
 * mtd_comm_share allocates `bytes` of uncached device memory on this rank (peers' reads and this GPU's writes must not
 * sit in a non-coherent L2) and returns its address, its slot number and its IPC handle; after the caller's control plane
 * has gathered the handles of that slot from all ranks, mtd_comm_open maps them: peers[r] is rank r's buffer as seen from
 * this process (peers[rank] = the local address).  At most MTD_COMM_MAX_SHARED buffers; released by mtd_comm_destroy. */
#define MTD_COMM_MAX_SHARED 8
int mtd_comm_share(mtd_comm *c, size_t bytes, void **d_local, unsigned int *slot, void *out_handle);
int mtd_comm_open(mtd_comm *c, unsigned int slot, const void *handles, void **peers);
/* Large all-reduce (sum, doubles, in place) through the mailbox's exported buffers instead of a collective library — for the
 * MB-sized per-step buffers of a domain-decomposed run (the replicated mesh of cv.mesh: M + 1 doubles; replaces the ghost-cell
 * exchange + distributed FFT of OrderParameterMesh.cc:263-316, 659-746 and the MPI_Allreduce of :630) where no RCCL communicator
 * is at hand (mtd_comm_allreduce_large is the RCCL form).  Every rank stages its buffer in an exported one, rank r sums slice r
 * of all ranks' staging buffers in rank order by remote loads (a reduce-scatter), every rank copies all slices home (an
 * all-gather); two mailbox exchanges are the barriers.  Same bits on every rank; an expired wait poisons the whole result (NaN)
 * and the communicator (MTD_ERR_COMM_TIMEOUT from then on).
 * Set-up: two buffers of mtd_comm_pull_bytes(max_doubles) bytes per rank from mtd_comm_share, opened by every rank
 * (mtd_comm_open), handed over once with mtd_comm_pull_attach (in_peers / out_peers: rank r's buffer as mapped here).
 * Layout: slices of roundup32(ceil(count / world)) doubles, rank r owns [r chunk, min((r + 1) chunk, count)) — possibly nothing.
 * count may be anything from 1 to the attached max_doubles (more, or no attach: MTD_ERR_INVALID_ARGUMENT, nothing is launched);
 * world == 1 returns MTD_SUCCESS without looking at the buffer.  The order of the additions, the layout, back-to-back re-use of the
 * buffers, the poison and the cap of MTD_COMM_MAX_SHARED slots are pinned bit for bit by tests/test_gpu_comm_pull.py.
 * Known limitation: slots are released only by mtd_comm_destroy, so a larger capacity needs a new communicator. */
size_t mtd_comm_pull_bytes(size_t max_doubles);
int mtd_comm_pull_attach(mtd_comm *c, size_t max_doubles, void *const *in_peers, void *const *out_peers);
int mtd_comm_allreduce_pull(mtd_comm *c, double *d_buffer, size_t count, mtd_stream_t stream);
unsigned int mtd_comm_world(const mtd_comm *c);
unsigned int mtd_comm_rank(const mtd_comm *c);
int mtd_comm_destroy(mtd_comm *c);

/* Particle-sharded fused step: with a comm attached, every CV block of mtd_fused_cv_pass also posts its sums for a collector
 * (the first CV block), which adds them up in a fixed order and sends the n_cv totals to every rank, and
 * mtd_fused_force_pass's scalar chain takes
 * s_c = scale_c * (sum over ranks) + shift_c from the mailbox instead of the registered partial sums (scale / shift
 * as registered with mtd_metad_set_cv_source): still two launches per step, no collective call.  n_cv <= 3.
 * comm == NULL detaches. */
int mtd_metad_set_comm(mtd_metad *m, mtd_comm *comm);

/* ================================================================================================
 * Particle-mesh order parameter (cv.mesh)
 * replaces OrderParameterMeshGPU.cuh:9-109 (gpu_bin_particles, gpu_assign_binned_particles_to_mesh,
 * gpu_update_meshes, gpu_compute_cv, gpu_compute_forces, gpu_compute_mode_sq) and the cuFFT plans of
 * OrderParameterMeshGPU.cc:57-152; single rank (no ghost cells), double precision meshes
 * ============================================================================================== */

typedef struct mtd_mesh mtd_mesh; /* opaque; owns the meshes, the cell list and the FFT twiddles */

/* OrderParameterMesh constructor + setupMesh + initializeFFT (OrderParameterMesh.cc:18-122, 191-229, 263-342).
 * mode: host double[n_types].  Mesh points per axis: 4 ... 256 (any), or a power of two up to 1024 (MTD_ERR_UNSUPPORTED otherwise). */
int mtd_mesh_create(mtd_mesh **out, unsigned int nx, unsigned int ny, unsigned int nz, const double *mode,
                    unsigned int n_types, unsigned int max_particles);
int mtd_mesh_destroy(mtd_mesh *m);
/* 1 (default): interpolation function with the reference's unsigned integer division; 0: as intended.
 * SYNCHRONISES THE DEVICE (the call has no stream): it waits for everything queued on any stream, rewrites the tables and waits
 * again, so evaluations queued before it use the old tables and everything queued after it the new ones. */
int mtd_mesh_set_bug_compat(mtd_mesh *m, int on);
/* The normalised Fourier mesh f = FFT(mesh) / N (fourier_mesh of the reference, OrderParameterMesh.cc:697-712) is only read by
 * mtd_mesh_qmax, mtd_mesh_virial and mtd_mesh_get_array(1): the spectral step writes it when `on` (default 1; 18.9 MB per
 * step at 128^3 otherwise saved).  Those three calls return MTD_ERR_INVALID_ARGUMENT when the last spectral step kept none:
 * switch it on and run mtd_mesh_spectral again (the real mesh of the step is still in place). */
int mtd_mesh_set_keep_fourier(mtd_mesh *m, int on);
/* Overlap hook: when `hip_event` (a hipEvent_t, NULL to clear) is set, mtd_mesh_spectral / mtd_mesh_compute_cv record it on
 * their stream right after the pass that completes the CV partial sums (the fused z pass) — the two inverse passes that
 * follow only feed the force pass.  A caller makes the launch that consumes the CV (the grid engine) wait for this event on
 * ANOTHER stream, so that it runs beside the inverse passes (host classes: mixed CV sets). */
int mtd_mesh_set_cv_event(mtd_mesh *m, void *hip_event);
unsigned int mtd_mesh_num_cells(const mtd_mesh *m);

/* getCurrentValue (OrderParameterMesh.cc:925-968): assignParticles -> FFT -> updateMeshes -> iFFT -> computeCV.
 * The CV is s = 1/2 * sum_{b < *n_partials} (*d_partials)[b]  (device doubles owned by the mesh): consume with
 * mtd_metad_set_cv_source(engine, slot, *d_partials, *n_partials, 1, 0, 0.5, 0.0) or mtd_reduce_partials. */
int mtd_mesh_compute_cv(mtd_mesh *m, unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box,
                        unsigned int n_global, const double **d_partials, unsigned int *n_partials, mtd_stream_t stream);

/* The two halves of mtd_mesh_compute_cv for a particle-sharded system with a replicated mesh (replaces the
 * ghost-cell exchange + distributed FFT of OrderParameterMesh.cc:263-316, 659-746 and the mode_sq all-reduce of :630):
 * _assign spreads this rank's particles, the ranks all-reduce (sum) the *count doubles at *d_buffer — the real mesh
 * followed by the sum of mode^2 — and _spectral runs FFT -> updateMeshes -> iFFT -> computeCV on the reduced mesh. */
/* Riders on the NEXT mtd_mesh_compute_cv / mtd_mesh_assign of this mesh (one-shot, tile pipeline only — MTD_ERR_UNSUPPORTED
 * otherwise, then call mtd_fused_cv_pass): the kernel that bins the particles also forms, from the positions it holds anyway, the
 * block partial sums of the lamellar CVs of `set` (at most 3; what mtd_fused_cv_pass leaves in d_partials: feed them to
 * mtd_metad_set_cv_source with n_partials = *n_partials, stride = set->n_cv, offset = c, scale 1 / N_global), and the assignment's
 * launches carry the deferred second grid pass of `engine`'s previous deposit (may be NULL).  In the bin pipeline (every assignment
 * of a mesh but its first) the sums are formed while the binning blocks wait for their atomics and the grid pass travels as extra
 * blocks of the scatter launch; the counting pipeline forms them in its particle loop / carries the pass in its row-scan launch.  A
 * mixed set (cv.lamellar + cv.mesh: LamellarOrderParameter.cc:143-179 and OrderParameterMesh.cc:517-640 both stream the positions)
 * then reads the positions once for both and spends one launch less per step.  n_particles, the stream and the position array of
 * that next call must be the ones the CVs share; d_partials: mtd_lamellar_scratch_doubles(n_particles) doubles. */
int mtd_mesh_set_lamellar_rider(mtd_mesh *mesh, mtd_metad *engine, const mtd_lamellar_set *set, const mtd_box *global_box,
                                unsigned int n_particles, double *d_partials, unsigned int *n_partials, mtd_stream_t stream);
/* disarm riders that no assignment has consumed (a caller whose mesh CV turned out to be up to date for this step);
 * *was_armed (may be NULL): 1 when they were still waiting — their sums were then NOT formed */
int mtd_mesh_clear_rider(mtd_mesh *mesh, int *was_armed);
int mtd_mesh_assign(mtd_mesh *m, unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, mtd_stream_t stream);
/* How the last assignment (mtd_mesh_assign / mtd_mesh_compute_cv / mtd_mesh_slab_*) grouped the particles by tile; waits for `stream`.
 * *pipeline: 0 the cell-level pipeline (meshes beyond 256^3, MTD_MESH_ASSIGN=cells), 1 the counting pipeline (count -> row scan ->
 * place: the first assignment of a mesh, a changed particle number, riders), 2 the bin pipeline (one launch on tile segments with
 * slack planned from the previous snapshot's exact counts).  *n_overflow: particles of a bin step that did not fit
 * their tile's planned segment and travelled through the overflow list (correct, only slower; 0 in a well-planned step). */
int mtd_mesh_assign_info(mtd_mesh *m, int *pipeline, unsigned int *n_overflow, mtd_stream_t stream);
/* The end of a step of a MIXED set — one mesh variable (grid variable `mesh_slot`) and the lamellar CVs of `set` (grid variables
 * slots[0 .. set->n_cv)) — in ONE launch: what mtd_fused_force_pass_slots (scalar chain on the CV sums -> bias factors, first grid
 * pass, lamellar forces) followed by mtd_mesh_forces with the mesh's device bias factor do in two (OrderParameterMesh.cc:925-968,
 * IntegratorMetaDynamics.cc:329-588, LamellarOrderParameterGPU.cu:60-118).  The chain runs in wave 0 of every block of the mesh's
 * force pass while the other waves stage their tile; every block streams a share of the particles for the lamellar forces and the
 * first blocks take the grid pass.  Same results as the two calls (engine state and lamellar forces to the last bits of a
 * contraction, mesh forces bitwise).  MTD_ERR_UNSUPPORTED where the shapes do not allow it (cell-level mesh pipeline, an engine with a
 * mailbox, more than three grid variables, more 256-cell grid blocks than mesh tiles, MTD_MESH_FORCE_MERGED=0): make the two calls.
 * set == NULL (slots, d_force_lamellar ignored): no lamellar CVs — the mesh variable alone on the grid, or beside variables of other
 * kinds whose sources are registered: mtd_metad_update_bias + mtd_mesh_forces in one launch. */
int mtd_mesh_forces_update_bias(mtd_mesh *mesh, mtd_metad *engine, unsigned int mesh_slot, const mtd_lamellar_set *set,
                                const unsigned int *slots, unsigned int n_particles, const void *d_postype, void *d_force_mesh,
                                void *const *d_force_lamellar, int dtype, unsigned int n_global, const mtd_box *global_box,
                                unsigned int timestep, mtd_stream_t stream);
/* Which kernels ran the last forward transform (mtd_mesh_spectral / mtd_mesh_compute_cv): 0 separate x and y passes (meshes whose
 * planes do not fit the LDS, sizes that are not powers of two), 1 x and y of a plane in one launch on the combined mesh, 2 the same
 * launch reading the assignment's per-tile images itself (meshes 128 cells wide after mtd_mesh_compute_cv: no combine launch;
 * MTD_FFT_FROM_TILES=0 switches it off).  The results are the same bits in all three. */
int mtd_mesh_transform_info(mtd_mesh *m, int *forward);
int mtd_mesh_exchange_buffer(mtd_mesh *m, double **d_buffer, size_t *count);
int mtd_mesh_spectral(mtd_mesh *m, const mtd_box *box, unsigned int n_global, const double **d_partials, unsigned int *n_partials,
                      mtd_stream_t stream);

/* interpolateForces (OrderParameterMesh.cc:749-864) from the inverse mesh AND the cell-sorted particle records of the last
 * mtd_mesh_compute_cv, i.e. of the same snapshot (the reference recomputes the CV first when needed, :1055-1056);
 * bias = *d_bias when d_bias != NULL (device resident), else bias_host */
int mtd_mesh_forces(mtd_mesh *m, unsigned int n_particles, const void *d_postype, void *d_force, int dtype,
                    const mtd_box *box, unsigned int n_global, const double *d_bias, double bias_host, mtd_stream_t stream);

/* setTable (OrderParameterMesh.cc:148-189): convolution kernel K(k) and its derivative on n equidistant points of
 * [k_min, k_max].  Like the reference, K itself is stored and never applied to the mesh; K' enters the virial.
 * SYNCHRONISES THE DEVICE (the call has no stream): it waits for everything queued on any stream before the old table is freed,
 * and the new one is in place when it returns. */
int mtd_mesh_set_table(mtd_mesh *m, const double *K, const double *d_K, unsigned int n, double k_min, double k_max);
int mtd_mesh_set_use_table(mtd_mesh *m, int use_table);

/* computeQmax (:1108-1179) on the Fourier mesh of the last compute_cv / spectral call (SYNCHRONISES):
 * out[0..2] = wave vector of the cell with the largest |f|^2 (first cell wins ties, DC bin included), out[3] = that
 * amplitude times N_global — the log quantities qx_max, qy_max, qz_max, sq_max. */
int mtd_mesh_qmax(mtd_mesh *m, const mtd_box *box, unsigned int n_global, double *out, mtd_stream_t stream);

/* computeVirial (:970-1050) (SYNCHRONISES): virial[6] (xx, xy, xz, yy, yz, zz) = bias * sum_{k != 0} |f|^4 / N^2 *
 * K'(|k|) / (2 |k|) * k_a k_b — identically zero without a table in use, exactly like the reference. */
int mtd_mesh_virial(mtd_mesh *m, const mtd_box *box, unsigned int n_global, double bias, double *virial, mtd_stream_t stream);

/* raw arrays for parity tests (SYNCHRONISES): which = 0 real mesh double[M]; 1 fourier_mesh (normalised) complex double[M];
 * 3 Re(inv_fourier_mesh) double[M] (the imaginary part is never used, OrderParameterMesh.cc:851-857); 7 sum of mode^2 */
int mtd_mesh_get_array(mtd_mesh *m, int which, void *host_out, mtd_stream_t stream);


/* Slab decomposition of the mesh over the ranks of an xGMI mailbox (replaces the ghost-cell exchange and the
 * distributed FFT of OrderParameterMesh.cc:263-316, 659-746 — dfftlib over MPI — for meshes whose replicated transform no
 * longer pays).  Rank r owns the z planes [r nz/W, (r+1) nz/W) for the x and y passes and the y rows [r ny/W, (r+1) ny/W)
 * for the z pass; the transposes between them are remote loads out of four buffers every rank exports
 * (mtd_comm_share, sizes from mtd_mesh_slab_bytes: local assignment, transformed slab, pencils of G, slab of Re(inv)).
 * nz and ny must be multiples of the number of ranks.  mtd_mesh_slab_compute_cv runs the whole forward / spectral / inverse
 * sequence with four mailbox exchanges as barriers (one carries sum mode^2, one the CV sum) and leaves the complete Re(inv)
 * on every rank for mtd_mesh_forces; *d_cv_sum is a device double, the CV is half of it.  The normalised Fourier mesh
 * (log quantities, virial) is not kept in slab runs. */
int mtd_mesh_slab_bytes(const mtd_mesh *m, unsigned int world, size_t *bytes /* [4] */);
int mtd_mesh_slab_attach(mtd_mesh *m, mtd_comm *comm, void *const *rho_peers, void *const *f_peers, void *const *g_peers,
                         void *const *inv_peers);
int mtd_mesh_slab_compute_cv(mtd_mesh *m, unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box,
                             unsigned int n_global, const double **d_cv_sum, mtd_stream_t stream);
/* ================================================================================================
 * Steinhardt Q_l (cv.steinhardt) — the reference has only a host implementation (SteinhardtQl.cc); these entry points
 * are what a GPU class of it would call.  Neighbour list in HOOMD's layout (NeighborList::getHeadList / getNNeighArray /
 * getNListArray, device uint32 arrays); half_nlist: 0 = storage mode full, 1 = storage mode half (third-law path,
 * SteinhardtQl.cc:80, 173-179, 328-333), 2 = a full list that is symmetric ((i, j) listed <=> (j, i) listed, as HOOMD builds
 * them) and indexes no ghost particle: the CV pass then visits every pair once, from its lower index — Y_lm(-d) = (-1)^l
 * Y_lm(d), so the reference's two visits add up to twice the even degrees and cancel in the odd ones, the scaling of :173-179;
 * the force pass treats 2 like 0.  Not for mtd_ql_accumulate_local with ghost particles.
 *
 * The row layout, for every entry point of this header that takes (d_head_list, d_n_neigh, d_nlist) — mtd_ql_*,
 * mtd_ql_symmetrize_half_list*, mtd_ql_local_*, mtd_cluster_largest, mtd_pe_*, mtd_es_*: the neighbours of i are
 * d_nlist[d_head_list[i] .. d_head_list[i] + d_n_neigh[i]), and nothing else is assumed.  As in a HOOMD list with a fixed capacity per
 * row, the rows may lie anywhere in d_nlist, in any order (d_head_list need not ascend, start at 0 or be the prefix sum of d_n_neigh),
 * with unused slots before, between and behind them whose contents are never read.  Results do not depend on where a row lies: the
 * same rows stored differently give the same bits (tests/test_gpu_list_layouts.py).  Where a size `n_list_entries` is asked for (the
 * `average` mode and the bond count of the local variable) it is the largest d_head_list[i] + d_n_neigh[i], the length of d_nlist up
 * to the end of its last row — not the number of listed pairs, sum_i d_n_neigh[i].
 * ============================================================================================== */

/* device doubles the two calls share (block partial sums, Q_lm tables, Q_l, CV value) */
size_t mtd_ql_scratch_doubles(unsigned int lmax);

/* SteinhardtQl::computeCV (SteinhardtQl.cc:62-201).  Ql_ref: host double[lmax+1].  On return *d_value points at the CV value,
 * *d_Ql at Q_l[lmax+1], *d_Qlm at the complex Q_lm[(lmax+1)^2] table in the reference's order (all inside d_scratch);
 * consume the value with mtd_metad_set_cv_source(engine, slot, *d_value, 1, 1, 0, 1.0, 0.0).  lmax <= 12. */
int mtd_ql_accumulate(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                      const unsigned int *d_n_neigh, const unsigned int *d_nlist, int half_nlist, double rcut, double ron,
                      unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, double *d_scratch,
                      const double **d_value, const double **d_Ql, const double **d_Qlm, mtd_stream_t stream);

/* The two halves of mtd_ql_accumulate for a particle-sharded system (the reference class has no MPI path):
 * _local leaves this rank's sums Q'_lm (m >= 0, (lmax+1)(lmax+2) doubles) at *d_sums inside d_scratch — the ranks
 * all-reduce exactly that buffer — and _finalize turns the reduced sums into Q_lm, Q_l and the CV value.
 * Neighbour indices >= n_particles address ghost particles stored behind the local ones in d_postype. */
int mtd_ql_accumulate_local(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box,
                            const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, int half_nlist,
                            double rcut, double ron, unsigned int lmax, unsigned int type, unsigned int n_global, double *d_scratch,
                            double **d_sums, unsigned int *n_sums, mtd_stream_t stream);
int mtd_ql_finalize(int half_nlist, unsigned int lmax, const double *Ql_ref, unsigned int n_global, double *d_scratch,
                    const double **d_value, const double **d_Ql, const double **d_Qlm, mtd_stream_t stream);

/* cv.steinhardt as the ONLY variable of a bias grid: mtd_ql_finalize and mtd_metad_update_bias(engine, timestep) in ONE launch
 * (SteinhardtQl.cc:173-199 + IntegratorMetaDynamics.cc:314-588): every block of the grid engine's launch forms Q_lm, Q_l and the
 * value from the sums mtd_ql_accumulate_local left in d_scratch (all-reduced by the caller in a particle-sharded run) and hands the
 * value to the engine's scalar chain in registers; the value is also registered as the variable's source.  The engine's deferred
 * pass of the deposit then travels in the next mtd_ql_forces on the same stream (full lists) instead of a launch of its own.
 * MTD_ERR_UNSUPPORTED when the grid has more than one variable or a mailbox attached (call mtd_ql_finalize +
 * mtd_metad_update_bias then).  Between the two pair passes of a step this leaves two launches where there were three. */
int mtd_ql_finalize_update_bias(mtd_metad *engine, int half_nlist, unsigned int lmax, const double *Ql_ref, unsigned int n_global,
                                double *d_scratch, unsigned int timestep, const double **d_value, const double **d_Ql,
                                const double **d_Qlm, mtd_stream_t stream);

/* SteinhardtQl::computeBiasForces (:203-339) with the Q_lm the last mtd_ql_accumulate left in d_scratch (Q20);
 * bias = *d_bias when d_bias != NULL, else bias_host.  Writes d_force[0..n_particles); with half lists the reaction force goes
 * to LOCAL partners only (j < n_particles, SteinhardtQl.cc:328), so particle-sharded runs use full lists. */
/* Half lists: how the reaction forces of the pairs are summed into the partner particles (SteinhardtQl.cc:328-333; the
 * reference's serial loop has one order, a GPU has none).  1 (default): as exact integers — bitwise reproducible, independent
 * of the order; 0: floating-point atomics — sums in arrival order, about 2.5 x faster.  Full lists need neither. */
int mtd_ql_set_half_list_exact(int enable);

/* Half lists without atomics.  Builds — once per neighbour-list update, synchronous — the symmetric full list a half list stands
 * for: every pair at both of its particles, each particle's partners in ascending order (so the result does not depend on any
 * arrival order), into caller-provided device arrays d_full_head[n], d_full_n_neigh[n], d_full_nlist[full_capacity].
 * *n_full_entries (host) receives the number of entries (twice the pairs); when it exceeds full_capacity nothing is written and
 * MTD_ERR_INVALID_ARGUMENT comes back (call again with room).  Then pass the full arrays with half_nlist = 2 to
 * mtd_ql_accumulate / mtd_ql_forces: the CV pass visits every pair once and scales like the half-list branch
 * (SteinhardtQl.cc:173-179), the force pass gathers like the full-list pass — the third-law sum of :328-333 with no atomics,
 * bitwise reproducible, at the full-list pass's cost (two pair visits instead of one visit + atomics).  A half list that
 * indexes ghost particles (j >= n_particles) is refused (MTD_ERR_UNSUPPORTED): its reaction forces would be lost (:328). */
int mtd_ql_symmetrize_half_list(unsigned int n_particles, const unsigned int *d_head_list, const unsigned int *d_n_neigh,
                                const unsigned int *d_nlist, unsigned int *d_full_head, unsigned int *d_full_n_neigh,
                                unsigned int *d_full_nlist, size_t full_capacity, size_t *n_full_entries, mtd_stream_t stream);
/* The same with a caller-owned workspace of mtd_ql_symmetrize_workspace_uints(n_particles) device unsigned ints (a host class
 * keeps it across the list updates of a run): no allocation, ONE synchronisation (the entry count must reach the host before the
 * arrays can be trusted); the fill itself is only stream-ordered. */
size_t mtd_ql_symmetrize_workspace_uints(unsigned int n_particles);
int mtd_ql_symmetrize_half_list_ws(unsigned int n_particles, const unsigned int *d_head_list, const unsigned int *d_n_neigh,
                                   const unsigned int *d_nlist, unsigned int *d_full_head, unsigned int *d_full_n_neigh,
                                   unsigned int *d_full_nlist, size_t full_capacity, size_t *n_full_entries, unsigned int *d_workspace,
                                   mtd_stream_t stream);

int mtd_ql_forces(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                  const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, int half_nlist,
                  double rcut, double ron, unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global,
                  const double *d_scratch, const double *d_bias, double bias_host, mtd_stream_t stream);

/* mtd_ql_forces with the virial of the bias force beside it, for constant-pressure runs.  For entry (k, j) of row k the pass forms
 * fp_kj, the `force` of SteinhardtQl.cc:278-322: -bias sum_l Ql_ref[l] 4 pi / ((2l + 1) N_global^2) 2 Re sum_m conj(Q_lm) grad_d (f Y_lm)(d_kj)
 * with d_kj = minImage(r_k - r_j), and adds it to particle k only (the reference's central terms).  The virial is that
 * of the force the pass applies: for the six components c = xx, xy, xz, yy, yz, zz (HOOMD's order; (a, b) with a <= b)
 *     virial_k[ab] = 1/2 sum_{j in row k} d_kj,a fp_kj,b          stored at d_virial[c * virial_pitch + k]
 * in the scalar type of the arrays (dtype), like HOOMD's ForceCompute::m_virial and mtd_ql_local_forces_virial: half of each pair at
 * each of its ends, the other half is formed in row j.  On a symmetric full list (half_nlist 0 or 2) the even-degree terms of fp are
 * antisymmetric in k <-> j and the odd-degree weights conj(Q_lm) vanish to rounding, so sum_k virial_k is the virial of the applied
 * forces, and modes 0 and 2 give the same per-particle values.
 * Relation to the strain derivative: the full-list force of the reference is HALF the gradient of the variable s, because only the
 * central terms are kept (the terms in which k appears as somebody's neighbour are dropped).  So
 *     sum_k virial_k[ab] = -1/2 bias ds/d eps_ab
 * under an affine strain of positions and box with the list kept: the virial of the force that is applied, not of -bias grad s.
 * (Checked on the CPU against central differences of the oracle's CV: tests/test_ql_virial_ref.py.)
 * Ghost particles: with a full list that indexes ghosts (j >= n_particles, stored behind the local particles) every rank writes the
 * rows of its local particles, and the ranks' sums add up to the single-rank sum.
 * d_virial == NULL is mtd_ql_forces: the same kernels, the same bits, any list mode.  Otherwise virial_pitch >= n_particles
 * (MTD_ERR_INVALID_ARGUMENT) and half_nlist != 1: the third-law pass of a half list scatters its reaction forces and forms no virial
 * (MTD_ERR_UNSUPPORTED; pass the symmetric full list of mtd_ql_symmetrize_half_list with half_nlist = 2).  Everything mtd_ql_forces
 * refuses is refused with the same code; all of it before a device is touched.  All six rows [0, n_particles) are written at every
 * call, 0 for particles of another type or without a neighbour; [n_particles, virial_pitch) is left alone.  d_force is the array of
 * mtd_ql_forces, bit for bit.  No atomics: bitwise reproducible like the force.  A deferred pass of the bias grid that is waiting on
 * the stream does not ride in this launch (it stays pending and runs as a launch of its own: the same grid, bit for bit). */
int mtd_ql_forces_virial(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                         const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, int half_nlist,
                         double rcut, double ron, unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global,
                         const double *d_scratch, const double *d_bias, double bias_host, mtd_stream_t stream, void *d_virial,
                         unsigned int virial_pitch);

/* ================================================================================================
 * Local Steinhardt bond order (cv.steinhardt_local) — no reference counterpart.  The harmonics summed over one particle's own
 * neighbours, turned into a rotational invariant PER PARTICLE, then averaged; conventions of mtd_ql_accumulate in every respect
 * (smoothing f of SteinhardtQl.cc:36-48, Condon-Shortley phase, d = minImage(r_i - r_j)).  For a particle i of `type`, over the
 * entries j of row i with type(j) == type and r_ij^2 <= r_cut^2:
 *     n_i      = sum_j f(r_ij)
 *     A_lm(i)  = sum_j f(r_ij) Y_lm(d_ij / r_ij)                        l = 0..lmax
 *     q_l^2(i) = 4 pi / (2l + 1) sum_{m = -l..l} |A_lm(i)|^2 / n_i^2     (0 when n_i == 0)
 *     c_i      = sum_l Ql_ref[l] q_l^2(i)                               (0 for particles of another type)
 *     s        = (1 / N_global) sum_i c_i
 *     F_k      = -bias ds/dr_k                                          (w component 0)
 * Not square-rooted, divided by N_global: the conventions of the global variable, with the square taken per particle.
 * Preconditions: the list is FULL and symmetric for same-type pairs within r_cut ((i, j) listed <=> (j, i) listed: what HOOMD and
 * mtd_nlist_build produce — the force pass gathers both roles of a particle from its own row), holds no duplicate and indexes no
 * ghost particle; entries j >= n_particles and self entries are skipped.  A pair exactly on the z axis of the box (a column of a
 * cubic crystal) has a finite force, here and in mtd_ql_forces, where the reference gives NaN (tests/test_gpu_ql_axis.py).  Known
 * limit: c_i jumps from 0 to the one-neighbour value when a first neighbour enters an empty shell.
 * Arguments are checked before a device is touched: MTD_ERR_INVALID_ARGUMENT for null pointers, r_cut <= 0, r_on < 0,
 * r_on >= r_cut, n_global == 0, an unknown dtype or a d_scratch that is not 16-byte aligned; MTD_ERR_UNSUPPORTED for lmax > 12.
 *
 * Options (mtd_ql_local_options, the *_opt entry points) turn the mean of c_i into what nucleation is biased with.  With
 * q_lm(i) = A_lm(i) / n_i (0 when n_i == 0):
 *     average:  qbar_lm(i) = [ q_lm(i) + sum_j f(r_ij) q_lm(j) ] / (1 + n_i)      (Lechner and Dellago, J. Chem. Phys. 129, 114707,
 *                                                                                 with the smoothing as weight; else qbar = q)
 *     c_i      = sum_l Ql_ref[l] 4 pi / (2l + 1) sum_m |qbar_lm(i)|^2             (what *d_c holds)
 *     switch:   h(c) = x^p / (1 + x^p),  x = max(c, 0) / c0,  c0 > 0, p >= 1      (else h(c) = c)
 *     gate:     g(n) = 3 t^2 - 2 t^3,  t = clip((n - n_lo) / (n_hi - n_lo), 0, 1), 0 <= n_lo < n_hi     (else g = 1)
 *     v_i      = g(n_i) h(c_i)   (0 for other types; what *d_v holds)             s = (1 / N_global) sum_i v_i
 * With a switch s is the smooth NUMBER FRACTION of solid-like particles; the gate removes the jump of c_i when a first neighbour
 * enters an empty shell.  With all three off (or opt == NULL) this is the variable above, bit for bit.  Gradient: with
 * g_l = Ql_ref[l] 4 pi / (2l + 1),
 *     B_lm(i) = g(n_i) h'(c_i) 2 g_l conj(qbar_lm(i)) / (1 + n_i)       (divided by 1 without the average)
 *     C_lm(k) = B_lm(k) + sum_{i in row k} f_ik B_lm(i)                 (C = B without the average)
 *     a_k     = g'(n_k) h(c_k) - Re sum_lm C_lm(k) q_lm(k) / n_k - [average] Re sum_lm B_lm(k) qbar_lm(k)
 *     G_kj    = Re sum_lm (C_lm(k) / n_k) grad(f Y_lm)(d_kj) + ( a_k + [average] Re sum_lm B_lm(k) q_lm(j) ) grad f(d_kj)
 *     N_global ds/dr_k = sum_j G_kj - sum_j G_jk
 * The averaged variable reaches second neighbours: it needs the same full, symmetric list, two more gather passes inside
 * mtd_ql_local_accumulate_opt and one double per list entry in the scratch.
 * ============================================================================================== */

/* all-zero = the plain variable.  c0, p are read when switch_on != 0; n_lo, n_hi when gate_on != 0 */
typedef struct
    {
    int average;
    int switch_on;
    double c0;
    unsigned int p;
    int gate_on;
    double n_lo, n_hi;
    } mtd_ql_local_options;

/* device doubles the two calls share: block sums, n_i, c_i and the per-particle table of weights the force pass gathers */
size_t mtd_ql_local_scratch_doubles(unsigned int n_particles, unsigned int lmax);

/* First pass.  Ql_ref: host double[lmax+1].  On return *d_partials points at *n_partials block sums of c_i (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_partials, *n_partials, 1, 0, 1.0 / N_global, 0.0) or mtd_reduce_partials), *d_c at
 * c_i[n_particles] and *d_n at n_i[n_particles] (d_c, d_n may be NULL), all inside d_scratch.  Sums follow the order of the list. */
int mtd_ql_local_accumulate(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                            const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax,
                            unsigned int type, const double *Ql_ref, unsigned int n_global, double *d_scratch, const double **d_partials,
                            unsigned int *n_partials, const double **d_c, const double **d_n, mtd_stream_t stream);

/* Second pass, with the table the last mtd_ql_local_accumulate (same arguments) left in d_scratch: writes d_force[0..n_particles),
 * zero for particles of another type; bias = *d_bias when d_bias != NULL, else bias_host.  No atomics: bitwise reproducible. */
int mtd_ql_local_forces(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                        const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                        unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                        const double *d_bias, double bias_host, mtd_stream_t stream);

/* The same three with options; opt == NULL or an all-zero struct is the plain variable, bit for bit (the three above forward here).
 * n_list_entries: the length of d_nlist (the largest d_head_list[i] + d_n_neigh[i], NOT the number of listed pairs: rows with slack
 * between them count with their slack, "The row layout" above) — with `average` the scratch keeps one double per slot of the list,
 * indexed like d_nlist itself, and the two calls cannot see the size of either array: size the scratch again whenever the list grows.
 * *d_partials: block sums of v_i (consumed as above); *d_c: c_i, averaged when `average` is set; *d_v (may be NULL): v_i.
 * The same opt goes to both passes.  MTD_ERR_INVALID_ARGUMENT, before a device is touched, for a switch with c0 <= 0 or p == 0
 * and for a gate without 0 <= n_lo < n_hi.  A scratch that is too small for the list is NOT detected (no size is passed): with `average`
 * the pass would write beyond it. */
size_t mtd_ql_local_scratch_doubles_opt(unsigned int n_particles, unsigned int lmax, size_t n_list_entries, const mtd_ql_local_options *opt);
int mtd_ql_local_accumulate_opt(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                                const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax,
                                unsigned int type, const double *Ql_ref, unsigned int n_global, double *d_scratch, const double **d_partials,
                                unsigned int *n_partials, const double **d_c, const double **d_n, mtd_stream_t stream,
                                const mtd_ql_local_options *opt, const double **d_v);
int mtd_ql_local_forces_opt(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                            const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                            unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                            const double *d_bias, double bias_host, mtd_stream_t stream, const mtd_ql_local_options *opt);

/* The force pass with the virial of the bias force beside it, for constant-pressure runs.  Let fp_kj be what the entry (k, j) of row k
 * adds to F_k: the force on k from the unordered pair {k, j}, bias and 1 / N_global included, antisymmetric in k <-> j; and
 * d_kj = minImage(r_k - r_j).  For the six components c = xx, xy, xz, yy, yz, zz (HOOMD's order; (a, b) with a <= b):
 *     virial_k[ab] = 1/2 sum_{j in row k} d_kj,a fp_kj,b          stored at d_virial[c * virial_pitch + k]
 * in the scalar type of the arrays (dtype), like HOOMD's ForceCompute::m_virial: half of each pair to each of its ends, HOOMD's
 * convention for pair forces.  In the scatter form of the gradient above, an ordered entry (i centre, j neighbour) with gradient
 * G_ij gives 1/2 d_ij,a (-bias G_ij,b / N_global) to i and the same to j.  sum_k virial_k[ab] = -bias ds/d eps_ab under an affine
 * strain of positions and box; the summed tensor is symmetric (the variable is rotation invariant), the per-particle one need not
 * be.  The same with every option: average, switch and gate act through the rows and E_kj, which are inside fp_kj.
 * d_virial == NULL is mtd_ql_local_forces_opt: the same kernels, the same bits.  Otherwise virial_pitch >= n_particles
 * (MTD_ERR_INVALID_ARGUMENT before a device is touched) and all six rows [0, n_particles) are written at every call, 0 for particles
 * of another type or without a neighbour; [n_particles, virial_pitch) is left alone.  d_force is the array of the _opt call, bit for
 * bit.  No atomics: bitwise reproducible like the force. */
int mtd_ql_local_forces_virial(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                               const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                               unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                               const double *d_bias, double bias_host, mtd_stream_t stream, const mtd_ql_local_options *opt, void *d_virial,
                               unsigned int virial_pitch);

/* The solid-bond count (ten Wolde, Ruiz-Montero and Frenkel, J. Chem. Phys. 104, 9932; PLUMED's LOCAL_Q6 followed by MORE_THAN):
 * a bond is solid when the normalised scalar product of the q vectors of its two ends exceeds a threshold, a particle is solid when
 * it has enough solid bonds.  With g_l = Ql_ref[l] 4 pi / (2l + 1), <a, b> = sum_l g_l Re sum_m a_lm conj(b_lm) over the degrees in
 * use and q_lm(i) = A_lm(i) / n_i (0 when n_i == 0):
 *     c_i   = <q(i), q(i)>                        the plain local value (what *d_c holds)
 *     u(i)  = q(i) / sqrt(c_i)                    0 when c_i == 0
 *     d_ij  = <u(i), u(j)>                        in [-1, 1], symmetric in i, j
 *     sigma = 3 t^2 - 2 t^3,  t = clip((d - d_lo) / (d_hi - d_lo), 0, 1),  -1 <= d_lo < d_hi <= 1
 *     b_i   = sum_{j in row i} f(r_ij) sigma(d_ij)                     the smooth number of solid bonds (what *d_b holds)
 *     v_i   = g(n_i) h(b_i)                       the switch of the options acts on b_i (x = max(b, 0) / c0; h(b) = b without one),
 *                                                 the gate on n_i (what *d_v holds)
 *     s     = (1 / N_global) sum_i v_i
 * With Ql_ref = e_6, bonds (0.5, 0.7) and a switch (6.5, 12), s N_global is the smooth number of solid particles of the literature.
 * <.,.> must be a norm: a negative Ql_ref[l] with bonds on is MTD_ERR_INVALID_ARGUMENT, as are bonds without
 * -1 <= d_lo < d_hi <= 1 (NaN included); `average` together with bonds is MTD_ERR_UNSUPPORTED.  All before a device is touched.
 * Gradient: with beta_i = g(n_i) h'(b_i) and t_kj = (beta_k + beta_j) f_kj sigma'(d_kj),
 *     P(k)    = [ sum_{j in row k} t_kj u(j) - (sum_j t_kj d_kj) u(k) ] / sqrt(c_k)          (<P(k), u(k)> = 0 identically)
 *     B_lm(k) = g_l conj(P_lm(k)),  C = B                                                   (no neighbour average)
 *     a_k     = g'(n_k) h(b_k) - Re sum_lm C_lm(k) q_lm(k) / n_k                             (the second term vanishes analytically)
 *     G_kj    = Re sum_lm (C_lm(k) / n_k) grad(f Y_lm)(d_kj) + ( a_k + beta_k sigma(d_kj) ) grad f(d_kj)
 *     N_global ds/dr_k = sum_j G_kj - sum_j G_jk
 * Like the average it reaches second neighbours and needs the full, symmetric list, two gather passes inside the accumulate call and
 * one double per list entry in the scratch.  The virial is that of mtd_ql_local_forces_virial: sigma and beta act through the rows
 * and the per-entry scalar, which are inside fp_kj.  Known limit: 1 / sqrt(c_i) makes the gradient large where a particle's q vector
 * nearly vanishes.
 * bonds == NULL or on == 0: the _opt / _virial entry points, bit for bit (those forward here).  The same opt and bonds go to both
 * passes; the scratch is sized with mtd_ql_local_scratch_doubles_bonds, again whenever the list grows.  d_b may be NULL; *d_b is NULL when bonds
 * are off. */
typedef struct
    {
    int on;
    double d_lo, d_hi;
    } mtd_ql_local_bonds;                                                      /* all-zero = off */

size_t mtd_ql_local_scratch_doubles_bonds(unsigned int n_particles, unsigned int lmax, size_t n_list_entries, const mtd_ql_local_options *opt,
                                          const mtd_ql_local_bonds *bonds);
int mtd_ql_local_accumulate_bonds(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                                  const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron, unsigned int lmax,
                                  unsigned int type, const double *Ql_ref, unsigned int n_global, double *d_scratch, const double **d_partials,
                                  unsigned int *n_partials, const double **d_c, const double **d_n, mtd_stream_t stream,
                                  const mtd_ql_local_options *opt, const double **d_v, const mtd_ql_local_bonds *bonds, const double **d_b);
int mtd_ql_local_forces_bonds(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                              const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut, double ron,
                              unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global, const double *d_scratch,
                              const double *d_bias, double bias_host, mtd_stream_t stream, const mtd_ql_local_options *opt, void *d_virial,
                              unsigned int virial_pitch, const mtd_ql_local_bonds *bonds);

/* ================================================================================================
 * Clusters — no reference counterpart.  Connected components of the "solid" particles over a neighbour list, and the mask of the
 * largest one: what nucleation studies bias is the size of the largest connected cluster of solid particles (ten Wolde, Ruiz-Montero
 * and Frenkel; PLUMED's DFSCLUSTERING followed by CLUSTER_NATOMS or CLUSTER_PROPERTIES ... SUM).  The unit stands alone: d_v is any
 * per-particle value (the v_i of mtd_ql_local_accumulate_bonds, the k_i of the environment similarity, ...).
 *     nodes   particles i < n_particles with type(i) == type and d_v[i] >= v_min (NaN is not a node)
 *     edges   list entries (i, j), j in row i, with both ends nodes, j != i, j < n_particles and
 *             |minImage(r_i - r_j)|^2 <= r_link^2
 * The list need not be symmetric for this pass: an edge seen from either end unites.  Ghost entries (j >= n_particles) are skipped, so a
 * cluster that crosses a domain boundary is cut there: single-domain runs only.
 * Outputs, all inside d_scratch (mtd_cluster_scratch_bytes(n_particles) bytes, 16-byte aligned), stream-ordered, nothing synchronised:
 *     label[i]   the smallest particle index of i's component; MTD_CLUSTER_NONE for a particle that is not a node
 *     size[r]    the member count at every root r (label[r] == r), 0 elsewhere
 *     summary    { root of the largest cluster, its member count, number of clusters, number of nodes }; largest = most members, a tie
 *                goes to the smaller root; without any node the root is MTD_CLUSTER_NONE and the count 0
 *     w[i]       1.0 for the members of the largest cluster, 0.0 for everybody else
 * Every output is a function of the input alone: only integer atomics are used, two calls give the same bits.  Any of the four output
 * pointers may be NULL.
 * MTD_ERR_INVALID_ARGUMENT, before a device is touched, for a null box, scratch or (with particles) array, an unknown dtype, a scratch
 * that is not 16-byte aligned, r_link <= 0 or not finite, v_min not finite, and for p == NULL or p->on == 0: "off" is the caller's
 * business (mtd_ql_local_accumulate_cluster).  r_link is not compared with the reach of the list, which is unknown here.
 * ============================================================================================== */
typedef struct
    {
    int on;
    double v_min, r_link;
    } mtd_cluster_params;                                                      /* all-zero = off */
#define MTD_CLUSTER_NONE 0xffffffffu

size_t mtd_cluster_scratch_bytes(unsigned int n_particles);
int mtd_cluster_largest(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                        const unsigned int *d_n_neigh, const unsigned int *d_nlist, unsigned int type, const double *d_v,
                        const mtd_cluster_params *p, void *d_scratch, const unsigned int **d_label, const unsigned int **d_size,
                        const double **d_w, const unsigned int **d_summary, mtd_stream_t stream);

/* The local Steinhardt variable restricted to the largest cluster of solid particles:
 *     s = (1 / N_global) sum_{i in the largest cluster} v_i = (1 / N_global) sum_i w_i v_i
 * with the clusters of mtd_cluster_largest built from the v_i of this call (v_i >= v_min, linked within r_link).  With the bond count
 * and a switch, s N_global is the smooth SIZE OF THE LARGEST NUCLEUS.  Membership is piecewise constant, so the gradient is the one
 * above with v_i -> w_i v_i (PLUMED's treatment); the variable jumps when clusters merge or split.  The mask enters linearly and is
 * applied between the launches of the passes above: plain / switch / gate — the table row of i times w_i; bonds — beta_i and a0_i times
 * w_i before the back-propagation.  mtd_ql_local_forces_bonds (and its virial) then runs unchanged on the masked table, with the same
 * opt and bonds: there is no force entry point of its own.  *d_partials: the block sums of w_i v_i; *d_v stays the UNMASKED v_i, the
 * solid-ness the clusters were built from.  d_cluster_scratch: mtd_cluster_scratch_bytes(n_particles) bytes, separate from d_scratch,
 * whose layout and size do not change; *d_w, *d_label, *d_summary (each may be NULL) point into it as mtd_cluster_largest leaves them.
 * cluster == NULL or on == 0: mtd_ql_local_accumulate_bonds, bit for bit (that entry point forwards here); the three pointers are set
 * to NULL.  Refused before a device is touched: what mtd_cluster_largest refuses (MTD_ERR_INVALID_ARGUMENT), and `average` together with a
 * cluster (MTD_ERR_UNSUPPORTED: its B rows and the extra a_k term would need the mask too). */
int mtd_ql_local_accumulate_cluster(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box,
                                    const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, double rcut,
                                    double ron, unsigned int lmax, unsigned int type, const double *Ql_ref, unsigned int n_global,
                                    double *d_scratch, const double **d_partials, unsigned int *n_partials, const double **d_c,
                                    const double **d_n, mtd_stream_t stream, const mtd_ql_local_options *opt, const double **d_v,
                                    const mtd_ql_local_bonds *bonds, const double **d_b, const mtd_cluster_params *cluster,
                                    void *d_cluster_scratch, const double **d_w, const unsigned int **d_label,
                                    const unsigned int **d_summary);

/* ================================================================================================
 * Pair entropy (cv.pair_entropy) — no reference counterpart.  The two-body excess entropy S2 from a Gaussian-smoothed g(r) (Piaggi,
 * Valsson and Parrinello, PRL 119, 015701; PLUMED's PAIRENTROPY): a bias variable for nucleation that needs no knowledge of the target
 * structure.  Parameters r_max > 0, sigma_r > 0, n_bins = B (1 .. 256) and a particle type t.
 *     Delta = r_max / B,  r_b = (b + 1/2) Delta (b = 0 .. B-1),  r_on = r_max + 3 sigma_r,  r_cut = r_max + 4 sigma_r,
 *     w = ceil(6 sigma_r / Delta),  K(x) = exp(-x^2 / 2 sigma_r^2) / (sqrt(2 pi) sigma_r),  g_min = 1e-10
 * Entries (i, j) of a FULL list take part when i and j are both of type t, j != i and r = |minImage(r_i - r_j)| <= r_cut.  The central
 * particles are the n_particles local ones; neighbour indices may address ghost particles stored behind them, as in
 * mtd_ql_accumulate_local.  f(r) is the cosine window of the Steinhardt passes between r_on and r_cut (SteinhardtQl.cc:36-60); an entry
 * counts in bin b iff |b - b_c| <= w and 0 <= b < B, with b_c = floor(r (B / r_max)) in fp64.
 *     H_b = sum_entries f(r) K(r_b - r)             N_t = central particles of type t (slot B of the sums: the all-reduce makes it global)
 *     rho = N_t / V,  V = Lx Ly Lz                  g_b = H_b / (4 pi N_t rho r_b^2)
 *     phi_b = g_b ln g_b - g_b + 1 where g_b >= g_min, else 1        (PLUMED's convention)
 *     S = -2 pi rho Delta sum_b r_b^2 phi_b         in units of k_B; N_t == 0: S = 0 and no forces
 * Gradient: W_b = dS/dH_b = -Delta ln g_b / (2 N_t) where g_b >= g_min, else 0; an entry with pair vector d = r_i - r_j has
 *     u = sum_{b in window} W_b [ f'(r) K_b + f(r) K_b (r_b - r) / sigma_r^2 ]
 * and gives +u d / r to dS/dr_i and -u d / r to dS/dr_j.  As a gather over row k of a full list: dS/dr_k = 2 sum_{j in row k} u_kj d_kj / r_kj
 * (the mirror entry (j, k) gives the same amount, whether j is local or a ghost: no reaction force on ghosts).  F = -bias dS/dr.
 * Virial (only with a virial pointer): sum_k virial_k = -bias dS/d eps under an affine strain of positions and box.  With
 * G_kj = 2 u_kj d_kj / r_kj, virial_k[ab] = -bias 1/2 sum_{j in row k} d_kj,a G_kj,b; and because rho and the normalisation of g depend
 * on V, dS/d eps_ab|explicit = -(S + 2 pi rho Delta sum_{g_b >= g_min} r_b^2 g_b ln g_b) delta_ab, spread evenly: every central particle
 * of type t gets -bias (that value) / N_t on xx, yy, zz.  Layout and scalar type of mtd_ql_forces_virial (virial[c * pitch + k], six
 * components); every row [0, n_particles) is written at every call.
 * A step is _accumulate, (mtd_comm_allreduce_small of *d_sums in a domain-decomposed run), _finalize, _forces, with the same r_max,
 * sigma_r, n_bins, type and scratch.  Sums are fixed-point integers inside a block and fixed-order sums elsewhere: two identical calls
 * give identical bits (csrc/pair_entropy.hip has the rounding bound).  Arguments are checked before a device is touched:
 * MTD_ERR_INVALID_ARGUMENT for null pointers, a non-finite or non-positive r_max or sigma_r, n_bins == 0, an unknown dtype, a d_scratch
 * that is not 16-byte aligned or a virial pitch below n_particles; MTD_ERR_UNSUPPORTED for n_bins > 256.
 * ============================================================================================== */

/* device doubles the calls of a step share (sums, value, g_b, W_b, block sums) */
size_t mtd_pe_scratch_doubles(unsigned int n_bins);

/* This rank's sums: on return *d_sums points at *n_sums = n_bins + 1 doubles inside d_scratch, H_0 .. H_{B-1} and N_t, ready for
 * mtd_comm_allreduce_small. */
int mtd_pe_accumulate(unsigned int n_particles, const void *d_postype, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                      const unsigned int *d_n_neigh, const unsigned int *d_nlist, double r_max, double sigma_r, unsigned int n_bins,
                      unsigned int type, double *d_scratch, double **d_sums, unsigned int *n_sums, mtd_stream_t stream);

/* The (reduced) sums -> g_b, S, W_b and the explicit virial term.  *d_value points at S, one device double (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_value, 1, 1, 0, 1.0, 0.0)), *d_g (d_g may be NULL) at g_b[n_bins], both inside d_scratch. */
int mtd_pe_finalize(const mtd_box *box, double r_max, double sigma_r, unsigned int n_bins, double *d_scratch, const double **d_value,
                    const double **d_g, mtd_stream_t stream);

/* Writes d_force[0..n_particles) (w component 0; 0 for particles of another type) with the W_b the last mtd_pe_finalize left in
 * d_scratch; bias = *d_bias when d_bias != NULL, else bias_host.  d_virial == NULL: no virial, the kernel without the switch; the force
 * array is the same, bit for bit, either way.  No atomics: bitwise reproducible. */
int mtd_pe_forces(unsigned int n_particles, const void *d_postype, void *d_force, int dtype, const mtd_box *box, const unsigned int *d_head_list,
                  const unsigned int *d_n_neigh, const unsigned int *d_nlist, double r_max, double sigma_r, unsigned int n_bins, unsigned int type,
                  const double *d_scratch, const double *d_bias, double bias_host, mtd_stream_t stream, void *d_virial,
                  unsigned int virial_pitch);

/* ================================================================================================
 * Environment similarity (cv.environment_similarity) — no reference counterpart.  The template-matching crystallinity of Piaggi and
 * Parrinello (J. Chem. Phys. 150, 244119; PLUMED's ENVIRONMENTSIMILARITY): every particle's neighbourhood is compared, in a FIXED
 * orientation, with one or more template environments, each a short list of lattice vectors.  It selects one polymorph (fcc against bcc
 * or hcp, cubic against hexagonal ice) and one orientation, which neither the Steinhardt variables nor the pair entropy can.
 * Parameters: a particle type t; E environments (1 <= E <= MTD_ES_MAX_ENV), environment e with M_e template vectors T^e_m
 * (1 <= M_e <= 32, sum_e M_e <= MTD_ES_MAX_VEC, every vector finite with 0 < |T| < r_cut); sigma_env > 0; 0 <= r_on < r_cut; lambda > 0,
 * read only when E > 1; an optional switch with c0 > 0 and integer p >= 1.
 * Entries (i, j) of a FULL list take part when i and j are both of type t, j != i and r = |d| <= r_cut, with
 * d = minImage(r_j - r_i): the vector FROM the central particle TO the neighbour, in the lab frame.  The central particles are the
 * n_particles local ones; entries may address ghost particles stored behind them.  f(r) is the cosine window of the Steinhardt passes
 * between r_on and r_cut (SteinhardtQl.cc:36-60).
 *     phi(x) = exp(-|x|^2 / (4 sigma_env^2))
 *     k^e_i  = (1 / M_e) sum_{j in row i} f(r_ij) sum_m phi(d_ij - T^e_m)          (~1 on the perfect lattice, ~0.1 in a liquid)
 *     k_i    = k^1_i                                          for E = 1
 *     k_i    = (1 / lambda) ln sum_e exp(lambda k^e_i)        for E > 1: PLUMED's smooth maximum, formed as max + log-sum-exp of the differences
 *     w^e_i  = exp(lambda k^e_i) / sum_e' exp(lambda k^e'_i)  (1 for E = 1)
 *     v_i    = h(k_i),  h(k) = x^p / (1 + x^p), x = k / c0    (h(k) = k without a switch; the switch of mtd_ql_local_options)
 *     s      = (1 / N_global) sum_i v_i                       (particles of another type: k^e = k = v = 0)
 * Gradient: with beta^e_i = h'(k_i) w^e_i, an entry has
 *     g_ij = sum_e (beta^e_i / M_e) [ f'(r) (d / r) sum_m phi_m - f(r) sum_m phi_m (d - T^e_m) / (2 sigma_env^2) ]      (= d(N s) / d d_ij)
 * and gives +g_ij to d(N s)/dr_j and -g_ij to d(N s)/dr_i.  As a gather over row k of a symmetric list:
 *     N ds/dr_k = sum_{j in row k} [ -g_kj(d_kj) + g_jk(-d_kj) ]          (the second term needs beta_j),       F = -bias ds/dr.
 * The pair term is not parallel to d: the variable is not rotation invariant; sum_k F_k = 0 still holds on a single domain.  An
 * environment that holds -T for every T (fcc, bcc, sc; detected by exact comparison of the vectors) has g_jk(-d) = -(beta^e_j / beta^e_k)
 * g_kj(d): one evaluation per entry serves both terms.  Diamond's two environments are each other's inverse, not closed themselves:
 * two evaluations per entry.
 * Virial (only with a virial pointer).  The templates stay FIXED in the lab frame under strain.  The six stored components (a, b),
 * a <= b, in HOOMD's order xx, xy, xz, yy, yz, zz are the derivatives under the cell deformations a HOOMD box can make,
 * x_a -> x_a + eps x_b of positions and box:
 *     sum_k virial_k[ab] = -bias ds/d eps_ab = -(bias / N_global) sum_entries g_a d_b
 * The tensor is NOT symmetric (yx, zx, zy differ from xy, xz, yz); the three stored off-diagonals are xy, xz, yz, those of the upper
 * triangular deformations.  Per particle half of every entry goes to each of its ends; in the gather
 *     virial_k[ab] = -(bias / N_global) 1/2 sum_{j in row k} [ g_kj,a d_kj,b + g_jk,a d_jk,b ]
 * Layout, scalar type and pitch rule of mtd_ql_local_forces_virial (virial[c * pitch + k], six components); every row [0, n_particles)
 * is written at every call, [n_particles, pitch) is left alone.
 * A step is _accumulate then _forces with the same arguments and scratch.  Fixed summation orders, no atomics: two identical calls give
 * identical bits.  Arguments are checked before a device is touched: MTD_ERR_INVALID_ARGUMENT for null pointers, an unknown dtype, a
 * d_scratch that is not 16-byte aligned, n_global == 0, a virial pitch below n_particles, non-finite or out-of-range parameters,
 * n_env == 0 or an n_vec[e] == 0, a template vector that is non-finite, zero or not shorter than r_cut; MTD_ERR_UNSUPPORTED for
 * n_env > 4, an n_vec[e] > 32, a total above 64, and for n_ghost > 0 together with E > 1 or a switch (beta of a ghost would have to be
 * exchanged; with E = 1 and no switch beta = 1, the table is never read for a neighbour, and ghosts work).
 * ============================================================================================== */

#define MTD_ES_MAX_ENV 4
#define MTD_ES_MAX_VEC 64

typedef struct
    {
    unsigned int n_env;                    /* E */
    unsigned int n_vec[MTD_ES_MAX_ENV];    /* M_e */
    double vec[MTD_ES_MAX_VEC][3];         /* the template vectors, packed environment after environment */
    double sigma_env, r_on, r_cut;
    double lambda;                         /* read when n_env > 1 */
    int switch_on;                         /* c0, p are read when switch_on != 0 */
    double c0;
    unsigned int p;
    } mtd_es_params;

/* device doubles the two calls share: per particle k^e_i [4], beta^e_i [4], k_i, v_i; block sums; and nine gradient sums per particle,
 * which the first pass fills when beta = 1 everywhere and the environment is closed (the second pass then only scales them) */
size_t mtd_es_scratch_doubles(unsigned int n_particles);

/* First pass.  On return *d_partials points at *n_partials block sums of v_i (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_partials, *n_partials, 1, 0, 1.0 / N_global, 0.0) or mtd_reduce_partials), *d_k at
 * k_i[n_particles], *d_ke at k^e_i as [n_particles][4] (columns e >= n_env are 0) and *d_v at v_i[n_particles] (d_k, d_ke, d_v may be
 * NULL), all inside d_scratch.  n_ghost: the particles stored behind the n_particles local ones that entries may address. */
int mtd_es_accumulate(unsigned int n_particles, unsigned int n_ghost, const void *d_postype, int dtype, const mtd_box *box,
                      const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, unsigned int type,
                      const mtd_es_params *params, unsigned int n_global, double *d_scratch, const double **d_partials, unsigned int *n_partials,
                      const double **d_k, const double **d_ke, const double **d_v, mtd_stream_t stream);

/* Second pass, with the beta^e_i the last mtd_es_accumulate (same arguments) left in d_scratch: writes d_force[0..n_particles) (w
 * component 0; 0 for particles of another type); bias = *d_bias when d_bias != NULL, else bias_host.  d_virial == NULL: no virial, the
 * kernel without the sums; the force array is the same, bit for bit, either way.  n_particles == 0 is success.  No atomics: bitwise
 * reproducible. */
int mtd_es_forces(unsigned int n_particles, unsigned int n_ghost, const void *d_postype, void *d_force, int dtype, const mtd_box *box,
                  const unsigned int *d_head_list, const unsigned int *d_n_neigh, const unsigned int *d_nlist, unsigned int type,
                  const mtd_es_params *params, unsigned int n_global, const double *d_scratch, const double *d_bias, double bias_host,
                  mtd_stream_t stream, void *d_virial, unsigned int virial_pitch);

/* ================================================================================================
 * Local pair entropy (cv.pair_entropy_local) — no reference counterpart.  The local-entropy fingerprint of Piaggi and Parrinello
 * (J. Chem. Phys. 147, 114112; PLUMED's PAIRENTROPIES): a pair entropy s_i from particle i's OWN smoothed g_i(r), optionally averaged
 * over the first shell and counted through a switch — the smooth number of solid-like particles without a reference value, a template
 * or an orientation.  The conventions of "Pair entropy" above hold wherever nothing else is said.
 * Parameters: r_max > 0, sigma_r > 0, n_bins = B (1 .. MTD_PEL_MAX_BINS), a particle type t; an optional average window
 * 0 <= a_on < a_cut <= r_max + 4 sigma_r; an optional switch with c0 > 0 and integer p >= 1.  Delta, r_b, r_on = r_max + 3 sigma_r,
 * r_cut = r_max + 4 sigma_r, w, K, b_c and g_min = 1e-10 are those of the global variable.
 * Entries (i, j) of a FULL list take part when both particles are of type t, j != i and r = |d| <= r_cut, d = minImage(r_i - r_j); f is
 * the cosine window between r_on and r_cut.  EVERY LIST ENTRY MUST ADDRESS A CENTRAL PARTICLE (j < n_particles): the force on k reads
 * W_j, alpha_j, s_j of its neighbours, which ghosts do not have; an entry j >= n_particles is skipped.  Single-domain runs only.
 *     H_ib  = sum_{j in row i} f(r_ij) K(r_b - r_ij)        over the window |b - b_c| <= w, 0 <= b < B
 *     N_t   = central particles of type t,  rho = N_t / V,  V = Lx Ly Lz
 *     g_ib  = H_ib / (4 pi rho r_b^2)
 *     phi_ib = g ln g - g + 1 where g_ib >= g_min, else 1   (empty bins are the common case here)
 *     s_i   = -2 pi rho Delta sum_b r_b^2 phi_ib  (<= 0)    particles of another type: s = sbar = v = 0, no force
 *     n_i   = sum_j f_a(r_ij),  sbar_i = (s_i + sum_j f_a(r_ij) s_j) / (1 + n_i)
 *             f_a: the cosine window a_on .. a_cut over the same entries; without an average sbar_i = s_i and n_i = 0
 *     v_i   = h(-sbar_i),  h(c) = x^p / (1 + x^p), x = max(c, 0) / c0;  without a switch v_i = sbar_i
 *     CV    = (1 / N_global) sum_i v_i
 * Gradient:
 *     W_ib  = ds_i/dH_ib = -Delta ln g_ib / 2 where g_ib >= g_min, else 0
 *     gamma_i = dv_i/dsbar_i  (= -h'(-sbar_i), or 1 without a switch; 0 for the other type)
 *     alpha_j = gamma_j / (1 + n_j) + sum_{i in row j} f_a(r_ij) gamma_i / (1 + n_i)        (alpha = gamma without an average)
 *     u_ij(W) = sum_{b in window} W_b K_b [ f'(r) + f(r) (r_b - r) / sigma_r^2 ]
 *     t_ij  = alpha_i u_ij(W_i) + gamma_i f_a'(r_ij) (s_j - sbar_i) / (1 + n_i)
 * Entry (i, j) gives +t_ij d / r to d(N CV)/dr_i and -t_ij d / r to d(N CV)/dr_j.  As a gather over row k of the symmetric list:
 *     N dCV/dr_k = sum_{j in row k} (t_kj + t_jk) d_kj / r              F = -bias dCV/dr
 * Virial (only with a virial pointer), layout, scalar type and pitch rule of mtd_ql_local_forces_virial:
 *     virial_k[ab] = -(bias / N_global) [ 1/2 sum_{j in row k} d_a (t_kj + t_jk) d_b / r + delta_ab alpha_k X_k ]
 *     X_k = -( s_k + 2 pi rho Delta sum_{g_kb >= g_min} r_b^2 g_kb ln g_kb )        the explicit volume derivative of s_k through rho
 * A step is _accumulate then _forces with the same parameters, call block and scratch.  H_ib is summed in fixed-point integers, every
 * other sum in a fixed order: two identical calls give identical bits (csrc/pair_entropy_local.hip has the rounding bound).  Arguments
 * are checked before a device is touched: MTD_ERR_INVALID_ARGUMENT for null pointers, a non-finite or non-positive r_max or sigma_r,
 * n_bins == 0, an unknown dtype, a d_scratch that is not 16-byte aligned, a virial pitch below n_particles, a bad average window or
 * switch, n_global == 0; MTD_ERR_UNSUPPORTED for n_bins > MTD_PEL_MAX_BINS.
 * ============================================================================================== */

#define MTD_PEL_MAX_BINS 128

typedef struct
    {
    double r_max, sigma_r;
    unsigned int n_bins, type;
    int average_on;                        /* a_on, a_cut are read when average_on != 0 */
    double a_on, a_cut;
    int switch_on;                         /* c0, p are read when switch_on != 0 */
    double c0;
    unsigned int p;
    } mtd_pel_params;                      /* options all-zero = off */

/* what the two calls of a step share beside the parameters: the fields of mtd_row_call (below, "Debye structure factor"), with N_global
 * in the place of n_ghost */
typedef struct
    {
    unsigned int n_particles, n_global;
    const void *d_postype;
    int dtype;
    const mtd_box *box;
    const unsigned int *d_head_list, *d_n_neigh, *d_nlist;
    double *d_scratch;
    mtd_stream_t stream;
    } mtd_pel_call;

/* device doubles the two calls share: block sums, six per-particle arrays and the table W_ib [n_particles][n_bins] */
size_t mtd_pel_scratch_doubles(unsigned int n_particles, unsigned int n_bins);

/* First pass.  On return *d_partials points at *n_partials block sums of v_i (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_partials, *n_partials, 1, 0, 1.0 / N_global, 0.0) or mtd_reduce_partials), *d_s at
 * s_i[n_particles], *d_sbar at sbar_i and *d_v at v_i (each may be NULL), all inside c->d_scratch. */
int mtd_pel_accumulate(const mtd_pel_params *p, const mtd_pel_call *c, const double **d_partials, unsigned int *n_partials,
                       const double **d_s, const double **d_sbar, const double **d_v);

/* Second pass, with what the last mtd_pel_accumulate (same p and c) left in c->d_scratch: writes d_force[0..n_particles) (w component
 * 0; 0 for particles of another type); bias = *d_bias when d_bias != NULL, else bias_host.  d_virial == NULL: no virial, the kernel
 * without the sums; the force array is the same, bit for bit, either way.  n_particles == 0 is success.  No atomics: bitwise
 * reproducible. */
int mtd_pel_forces(const mtd_pel_params *p, const mtd_pel_call *c, void *d_force, const double *d_bias, double bias_host,
                   void *d_virial, unsigned int virial_pitch);

/* ================================================================================================
 * Debye structure factor (cv.debye_structure_factor) — no reference counterpart.  The intensity of diffraction peaks from the Debye
 * scattering function (Niu, Piaggi, Invernizzi and Parrinello, PNAS 115, 5348 (2018)): a bias variable for crystallisation that needs
 * only wave numbers Q read off a diffraction pattern, invariant under rotation and translation; peaks with weights of opposite sign
 * select one polymorph against another.  The conventions of "Pair entropy" above hold wherever nothing else is said.
 * Parameters: a particle type t, a cut-off r_cut > 0, P = n_q wave numbers Q_p > 0 (1 <= P <= MTD_DSF_MAX_Q), weights c_p (finite,
 * any sign).  Entries (i, j) of a FULL list take part when both particles are of type t, j != i and r = |d| <= r_cut,
 * d = minImage(r_i - r_j).  The central particles are the n_particles local ones; entries may address the n_ghost particles stored
 * behind them.
 *     x = pi r / r_cut,  w(r) = sin x / x              (the window of the literature; w(r_cut) = 0)
 *     y_p = Q_p r,       phi_p = w(r) sin y_p / y_p
 *     w'(r)  = (pi / r_cut) (x cos x - sin x) / x^2
 *     phi_p' = w' sin y_p / y_p + w Q_p (y_p cos y_p - sin y_p) / y_p^2
 *     A_p = sum_entries phi_p(r_ij)                     N_t = central particles of type t (slot P of the sums: the all-reduce makes
 *                                                       both global)
 *     I_p = 1 + A_p / N_t,  s = sum_p c_p I_p           (N_t == 0: s = 0, I_p = 0, no forces)
 *     s_i = sum_p c_p (1 + sum_{j in row i} phi_p(r_ij)) for type t, else 0;  s = (1 / N_t) sum_i s_i
 * An entry with r = 0 exactly counts with phi_p = 1 and u = 0.
 * Gradient: u_kj = sum_p c_p phi_p'(r_kj), ds/dr_k = (2 / N_t) sum_{j in row k} u_kj d_kj / r_kj (the mirror entry gives the same amount
 * whether j is local or a ghost: no reaction force on ghosts), F = -bias ds/dr.
 * Virial (only with a virial pointer): virial_k[ab] = -(bias / N_t) sum_{j in row k} u_kj d_a d_b / r_kj, symmetric, half of every pair at
 * each end; no explicit volume term, because the normalisation is N_t and not a density.  sum_k virial_k = -bias ds/d eps.  Layout,
 * scalar type and pitch rule of mtd_pe_forces.
 * THE FORCE IS DISCONTINUOUS AT r_cut: w is the published window, w(r_cut) = 0 but w'(r_cut) = -1 / r_cut, so an entry that crosses the
 * cut-off changes ds/dr by sinc(Q_p r_cut) / r_cut per peak, divided by N_t (with the factor 2 of the mirror entry).  The window is
 * kept as published.
 * Spectrum (a diagnostic, not biased): I(Q_m) = 1 + (1 / N_t) sum_entries w(r) sin(Q_m r) / (Q_m r) on
 * Q_m = q_min + m (q_max - q_min) / (n_q - 1), m = 0 .. n_q - 1 (n_q == 1: Q_0 = q_min); 1 <= n_q <= MTD_DSF_MAX_SPECTRUM,
 * 0 < q_min <= q_max.
 * A step is _accumulate, (mtd_comm_allreduce_small of *d_sums in a domain-decomposed run), _finalize, _forces with the same parameters,
 * call block and scratch.  By default the first pass also stores every particle's unscaled gradient and virial sums, and _forces only
 * scales them by bias / N_t (mtd_dsf_set_store_gradient).  Every sum has a fixed order and there are no atomics: two identical calls
 * give identical bits.  Arguments are checked before a device is touched: MTD_ERR_INVALID_ARGUMENT for null pointers, a non-finite or
 * non-positive r_cut or Q, a non-finite weight, n_q == 0, an unknown dtype, a d_scratch that is not 16-byte aligned, a virial pitch
 * below n_particles, q_min > q_max; MTD_ERR_UNSUPPORTED for n_q above the two capacities.
 * ============================================================================================== */

#define MTD_DSF_MAX_Q 8
#define MTD_DSF_MAX_SPECTRUM 256

typedef struct
    {
    unsigned int type;
    double r_cut;
    unsigned int n_q;                      /* P */
    double q[MTD_DSF_MAX_Q], c[MTD_DSF_MAX_Q];
    } mtd_dsf_params;

/* The call block of the variables that walk the rows of a full neighbour list: what the calls of a step share beside the parameters —
 * particles, box, list, scratch and the stream the launches go to.  One structure under the name of each unit that takes it. */
typedef struct
    {
    unsigned int n_particles, n_ghost;     /* d_postype holds n_particles + n_ghost entries */
    const void *d_postype;
    int dtype;
    const mtd_box *box;
    const unsigned int *d_head_list, *d_n_neigh, *d_nlist;
    double *d_scratch;
    mtd_stream_t stream;
    } mtd_row_call;
typedef mtd_row_call mtd_dsf_call;

/* device doubles the calls share: sums, value, intensities, spectrum, block sums and ten per-particle arrays */
size_t mtd_dsf_scratch_doubles(unsigned int n_particles);

/* 1 (default): mtd_dsf_accumulate stores the unscaled gradient and the six virial sums of every particle, mtd_dsf_forces scales them;
 * 0: mtd_dsf_forces walks the rows a second time.  Process-wide, read by both calls: change it between steps, not inside one.
 * profiles/r24/README.md has the timings of both. */
int mtd_dsf_set_store_gradient(int enable);

/* This rank's sums: on return *d_sums points at *n_sums = P + 1 doubles inside c->d_scratch, A_0 .. A_{P-1} and N_t, ready for
 * mtd_comm_allreduce_small. */
int mtd_dsf_accumulate(const mtd_dsf_params *p, const mtd_dsf_call *c, double **d_sums, unsigned int *n_sums);

/* The (reduced) sums -> s and I_p.  *d_value points at s, one device double (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_value, 1, 1, 0, 1.0, 0.0)), *d_intensity at I_p[P], *d_local (may be NULL) at
 * s_i[n_particles] of the last mtd_dsf_accumulate, all inside c->d_scratch. */
int mtd_dsf_finalize(const mtd_dsf_params *p, const mtd_dsf_call *c, const double **d_value, const double **d_intensity,
                     const double **d_local);

/* Writes d_force[0..n_particles) (w component 0; 0 for particles of another type) with what the last mtd_dsf_accumulate and
 * mtd_dsf_finalize (same p and c) left in c->d_scratch; bias = *d_bias when d_bias != NULL, else bias_host.  d_virial == NULL: no
 * virial; the force array is the same, bit for bit, either way.  Every row [0, n_particles) of the virial is written,
 * [n_particles, virial_pitch) is left alone.  n_particles == 0 is success. */
int mtd_dsf_forces(const mtd_dsf_params *p, const mtd_dsf_call *c, void *d_force, const double *d_bias, double bias_host, void *d_virial,
                   unsigned int virial_pitch);

/* The spectrum of the configuration in c (p gives type and r_cut; its peaks are not read).  _spectrum leaves this rank's sums, n_q + 1
 * doubles (T_m = sum_entries w(r) sin(Q_m r) / r and N_t), at *d_sums inside c->d_scratch, ready for mtd_comm_allreduce_small;
 * _spectrum_finalize turns the (reduced) sums into I(Q_m)[n_q] at *d_spectrum.  They use their own part of the scratch: a step's
 * results stay valid. */
int mtd_dsf_spectrum(const mtd_dsf_params *p, const mtd_dsf_call *c, double q_min, double q_max, unsigned int n_q, double **d_sums,
                     unsigned int *n_sums);
int mtd_dsf_spectrum_finalize(const mtd_dsf_call *c, double q_min, double q_max, unsigned int n_q, const double **d_spectrum);

/* ================================================================================================
 * Coordination number (cv.coordination) — no reference counterpart.  The coordination number of the particles of one type A by those of
 * a type B through a rational switching function (PLUMED's COORDINATION / COORDINATIONNUMBER), plain or counted through a switch: the
 * variable of ion pairing, nucleation from solution, demixing and solvation shells, and the first one here that looks at pairs of two
 * different types.  The conventions of "Debye structure factor" above hold wherever nothing else is said.
 * Parameters: types A (centres) and B (partners), A = B allowed; r_0 > 0, d_0 >= 0, r_cut > d_0; integers 1 <= n < m <= MTD_COORD_MAX_M.
 * Entries (i, j) of a FULL list take part when type_i = A and type_j = B, j != i and r = |minImage(r_i - r_j)| <= r_cut.  The centres
 * are the n_particles local particles; entries may address the n_ghost particles stored behind them.
 *     x    = max(r - d_0, 0) / r_0
 *     s(x) = (1 - x^n) / (1 - x^m) = P_n(x) / P_m(x),   P_k(x) = 1 + x + ... + x^(k-1)
 * The geometric-sum form IS the definition: it has no singularity at x = 1 and no cancellation near it (s(1) = n / m,
 * ds/dx(1) = n (n - m) / (2 m)); the quotient form is 0 / 0 there and loses digits beside it.  The kernels evaluate P_k and P_k' by
 * Horner's rule, as tests/coordination_ref.py does; the default pair (6, 12) is compiled as 1 / (1 + x^6), which is the same function.
 * Stretched, as PLUMED's default:  s~(r) = (s - s_c) / (1 - s_c),  s_c = s((r_cut - d_0) / r_0), formed once on the host in fp64.
 * s~(r <= d_0) = 1 with gradient 0, s~(r_cut) = 0.  THE FORCE IS DISCONTINUOUS AT r_cut: the slope there is not zero, so an entry that
 * crosses the cut-off changes ds/dr by |s'(r_cut)| / (1 - s_c) / N_A.  The function is kept as published.
 *     n_i = sum_{j in row i, taking part} s~(r_ij)  for i of type A, else 0
 *     v_i = g(n_i),   s = (1 / N_A) sum_i v_i       N_A = centres of type A; N_A == 0: s = 0, no forces
 * g(c) = c (plain), or with switch_on  h(c) = y^p / (1 + y^p), y = c / c0 (p >= 1, c0 > 0), or 1 - h with `less`: s N_A is then the
 * smooth number of A particles with at least (at most) c0 B neighbours.
 * Gradient, in the gather form on a full list, for every local k:
 *     ds/dr_k = (1 / N_A) sum_{j in row k, j != k, r <= r_cut} s~'(r_kj) d_kj / r_kj ( [k in A, j in B] g'(n_k) + [k in B, j in A] g'(n_j) )
 * with d_kj = minImage(r_k - r_j); F = -bias ds/dr.  Both brackets count when A = B.  Particles of neither type get F = 0, and so do
 * entries with r = 0 or r <= d_0.
 * Virial (only with a virial pointer): virial_k[ab] = -(bias / (2 N_A)) sum_{same entries} s~' d_a d_b / r (same bracket): half of
 * every pair at each end, symmetric, sum_k virial_k = -bias ds/d eps, no explicit volume term.  Layout, scalar type and pitch rule of
 * mtd_pe_forces.
 * Domain decomposition: the plain variable needs no per-particle value of a neighbour and runs with ghosts; its only exchange is one
 * mtd_comm_allreduce_small of the two sums.  With a switch g'(n_j) of a ghost is not known: n_ghost > 0 together with switch_on is
 * MTD_ERR_UNSUPPORTED.
 * A step is _accumulate, (mtd_comm_allreduce_small of *d_sums in a domain-decomposed run), _finalize, _forces with the same parameters,
 * call block and scratch.  Plain: _accumulate walks the rows once and stores n_i and every particle's unscaled gradient and virial sums,
 * _forces scales them by bias / N_A.  With a switch: _accumulate forms n_i, v_i and g'(n_i), _forces walks the rows a second time and
 * reads g'(n_j) of the neighbours.  Every sum has a fixed order and there are no atomics: two identical calls give identical bits.
 * Arguments are checked before a device is touched: MTD_ERR_INVALID_ARGUMENT for null pointers, non-finite or out-of-range parameters
 * (r_0, d_0, r_cut, n = 0, n >= m, and with switch_on c0 and p), an unknown dtype, a d_scratch that is not 16-byte aligned, a virial
 * pitch below n_particles; MTD_ERR_UNSUPPORTED for m > MTD_COORD_MAX_M and for a switch with ghosts.
 * ============================================================================================== */

#define MTD_COORD_MAX_M 32

typedef struct
    {
    unsigned int type_a, type_b;           /* centres and partners */
    double r_0, d_0;
    unsigned int n, m;
    double r_cut;
    int switch_on;
    double c0;
    unsigned int p;
    int less;                              /* 1 - h in place of h */
    } mtd_coord_params;

typedef mtd_row_call mtd_coord_call;     /* "Debye structure factor" */

/* device doubles the calls share: sums, value, block sums and twelve per-particle arrays */
size_t mtd_coord_scratch_doubles(unsigned int n_particles);

/* 1 (default): (n, m) = (6, 12) runs the pair term compiled for it, 1 / (1 + x^6) (an identity for m = 2 n); 0: it takes the general
 * Horner loop like every other pair.  Both meet the tolerances at and around x = 1.  Process-wide, read by _accumulate and _forces:
 * change it between steps, not inside one.  profiles/r25/README.md has the timings of both. */
int mtd_coord_set_compiled_pair(int enable);

/* This rank's sums: on return *d_sums points at *n_sums = 2 doubles inside c->d_scratch, sum_i v_i and N_A, ready for
 * mtd_comm_allreduce_small. */
int mtd_coord_accumulate(const mtd_coord_params *p, const mtd_coord_call *c, double **d_sums, unsigned int *n_sums);

/* The switched coordination number restricted to the largest cluster ("Clusters" above):
 *     s = (1 / N_A) sum_i w_i v_i,   N_A the UNMASKED count of the centres
 * with the clusters of mtd_cluster_largest built from the v_i of this call, type = A: the nodes are the A particles with v_i >= v_min
 * ("liquid-like": at least c0 neighbours; with `less` at most c0: cavitation), linked within r_link — the variable of ten Wolde and
 * Frenkel for vapour-liquid nucleation and of nucleation from solution.  With two types the nodes are still the A particles only, and
 * the list must hold the A-A pairs up to r_link although the variable itself reads A-B pairs only; a device-built list with two
 * attached types builds all pairs.  Membership is piecewise constant (PLUMED's treatment): the gradient is the one above with
 * g'(n_i) -> w_i g'(n_i), and the variable jumps when clusters merge or split.  The launches: the walk of mtd_coord_accumulate,
 * mtd_cluster_largest on the v row just written, one launch that stores 0 over g'(n_i) of every particle with w_i = 0 (stored, not
 * multiplied: a non-finite entry comes out 0 too) and leaves the block sums of w_i v_i, the sums kernel.  mtd_coord_finalize and
 * mtd_coord_forces (with its virial) then run unchanged on the masked table: there is no force entry point of its own.  *d_switched of
 * mtd_coord_finalize stays the UNMASKED v_i, the values the clusters were built from.  d_cluster_scratch:
 * mtd_cluster_scratch_bytes(n_particles) bytes, 16-byte aligned, separate from c->d_scratch, whose layout and size do not change;
 * *d_w, *d_label, *d_summary (each may be NULL) point into it as mtd_cluster_largest leaves them.  The stream is c->stream.
 * cluster == NULL or on == 0: mtd_coord_accumulate, bit for bit (that entry point forwards here); the three pointers are set to NULL.
 * With the option on, before a device is touched: everything mtd_coord_accumulate refuses, as there; MTD_ERR_INVALID_ARGUMENT for
 * r_link <= 0 or not finite, v_min not finite, a NULL or misaligned d_cluster_scratch, c->d_nlist == NULL with particles;
 * MTD_ERR_UNSUPPORTED without a switch (the plain route stores summed gradients, which cannot be masked afterwards) and for
 * n_ghost > 0 (single-domain runs only: a cluster would be cut at the domain boundary). */
int mtd_coord_accumulate_cluster(const mtd_coord_params *p, const mtd_coord_call *c, const mtd_cluster_params *cluster,
                                 void *d_cluster_scratch, double **d_sums, unsigned int *n_sums, const double **d_w,
                                 const unsigned int **d_label, const unsigned int **d_summary);

/* The (reduced) sums -> s.  *d_value points at s, one device double (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_value, 1, 1, 0, 1.0, 0.0)), *d_local (may be NULL) at n_i[n_particles] and *d_switched (may
 * be NULL) at v_i[n_particles] of the last mtd_coord_accumulate (v_i = n_i without a switch), all inside c->d_scratch. */
int mtd_coord_finalize(const mtd_coord_params *p, const mtd_coord_call *c, const double **d_value, const double **d_local,
                       const double **d_switched);

/* Writes d_force[0..n_particles) (w component 0; 0 for particles of neither type) with what the last mtd_coord_accumulate and
 * mtd_coord_finalize (same p and c) left in c->d_scratch; bias = *d_bias when d_bias != NULL, else bias_host.  d_virial == NULL: no
 * virial; the force array is the same, bit for bit, either way.  Every row [0, n_particles) of the virial is written,
 * [n_particles, virial_pitch) is left alone.  n_particles == 0 is success. */
int mtd_coord_forces(const mtd_coord_params *p, const mtd_coord_call *c, void *d_force, const double *d_bias, double bias_host,
                     void *d_virial, unsigned int virial_pitch);

/* ================================================================================================
 * Tetrahedral order (cv.tetrahedral) — no reference counterpart.  The angle between two bonds of one particle, what tells a tetrahedral
 * network from a dense liquid: the tetrahedral order parameter q of Chau and Hardin (Mol. Phys. 93, 511) and of Errington and
 * Debenedetti (Nature 409, 318) in a smooth, weighted form over all neighbours inside the window, or the three-body penalty of
 * Stillinger and Weber, sum_{j<k} h_ij h_ik (cos theta_jik + 1/3)^2: ice, silicon, germanium, mW water, clathrates.  Rotation invariant,
 * unlike "Environment similarity".  The conventions of "Debye structure factor" above hold wherever nothing else is said.
 * Parameters: a particle type t; 0 <= r_on < r_cut; cos0 in [-1, 1] (-1/3: the tetrahedral angle); `normalise`; with `normalise` an
 * optional switch (c0 > 0, integer p >= 1) and an optional gate (1 <= n_lo < n_hi), the functions of mtd_ql_local_options.
 * Entries (i, j) of a FULL list take part when i and j are both of type t, j != i and 0 < r = |d| <= r_cut, with
 * d = minImage(r_j - r_i) and u = d / r (an entry with r = 0 has no direction and takes no part).  f(r) is the cosine window of the
 * Steinhardt passes between r_on and r_cut.  SINGLE-DOMAIN ONLY: every per-particle array ends at n_particles, an entry j >= n_particles
 * is skipped, and n_ghost > 0 is MTD_ERR_UNSUPPORTED.
 * Per central particle i, over its entries j:
 *     n_i = sum f_ij                 m_i = sum f_ij^2
 *     b_i = sum f_ij u_ij   (3)      T_i = sum f_ij u_ij (x) u_ij   (symmetric, 6 stored)
 *     A_i = sum_{j<k} f_ij f_ik (u_ij.u_ik - cos0)^2
 *         = 1/2 [ (T:T - m) - 2 cos0 (b.b - m) + cos0^2 (n^2 - m) ]          T:T = sum_ab T_ab^2 over all nine
 *     W_i = sum_{j<k} f_ij f_ik = 1/2 (n^2 - m)
 *     kappa = 1 / (1/3 + cos0^2)     (9/4 at cos0 = -1/3: the Errington-Debenedetti normalisation, 0 for uniformly random directions)
 *     normalise:      t_i = 1 - kappa A_i / W_i  where W_i >= MTD_TET_W_MIN, else t_i = 0 with zero gradient
 *                     v_i = g(n_i) h(t_i),  h(t) = x^p / (1 + x^p), x = max(t, 0) / c0   (h(t) = t without a switch, g = 1 without a gate)
 *     not normalised: v_i = A_i          (the three-body penalty; switch and gate are MTD_ERR_INVALID_ARGUMENT)
 *     s = (1 / N_t) sum_i v_i,   N_t the particles of the type; N_t = 0: s = 0, no forces
 * The kernels evaluate the moment form, O(n) per row; tests/tetrahedral_ref.py restates the pair sum.  Lattice values: t_i = 1 and
 * A_i = 0 on the four diamond vectors, t_i = 3/11 on the twelve fcc vectors (cos0 = -1/3).
 * Gradient.  The adjoint of particle i is alpha = dv_i / d(n, m, b, T), eleven numbers (alpha_T a symmetric matrix), from
 *     dA/dn = cos0^2 n      dA/dm = -(1 - cos0)^2 / 2      dA/db = -2 cos0 b      dA/dT = T
 *     dW/dn = n             dW/dm = -1/2
 *     dt/dmu = -kappa (dA/dmu W - A dW/dmu) / W^2
 *     alpha_mu = g h'(t) dt/dmu + [mu = n] g'(n) h(t)                         (not normalised: alpha = dA/dmu)
 * An entry has
 *     g_ij = dv_i/dd_ij = u [ f' (alpha_n + 2 f alpha_m + alpha_b.u + u.alpha_T.u) - (f/r) (alpha_b.u + 2 u.alpha_T.u) ] + (f/r) [ alpha_b + 2 alpha_T u ]
 * and gives +g_ij to d(N_t s)/dr_j and -g_ij to d(N_t s)/dr_i.  As a gather over row k of a symmetric list:
 *     N_t ds/dr_k = sum_{j in row k} [ -g_kj(d_kj) + g_jk(-d_kj) ],     F = -bias ds/dr
 * The second term reads alpha_j of the neighbour.  The pair term is NOT parallel to d, although the variable is rotation invariant:
 * sum_k F_k = 0 and the torque sum_k r_k x F_k = 0 both hold.
 * Virial (only with a virial pointer): half of every entry at each of its ends,
 *     virial_k[ab] = -(bias / N_t) 1/2 sum_{j in row k} [ g_kj,a d_kj,b + g_jk,a d_jk,b ]
 * with no explicit volume term; a particle's six stored components (xx xy xz yy yz zz, the first index the force's) need not be those of
 * a symmetric matrix, the sum over k is symmetric.  Layout, scalar type and pitch rule of mtd_pe_forces.
 * KNOWN PROPERTY.  Without a gate a particle whose pair weight W_i is tiny but not zero (one neighbour well inside the window, a second
 * one just entering it) has a bounded t_i and a gradient of order 1 / f: inherent to a weighted mean.  The gate with n_lo >= 1 removes
 * it: for 1 < n <= 2, W >= n - 1, and g vanishes quadratically at n_lo.  Dilute systems should use the gate.
 * A step is _accumulate, _finalize, _forces with the same parameters, call block and scratch.  _accumulate walks the rows once and
 * stores n_i, t_i (A_i when not normalised), v_i and the adjoint row of every particle — ROW-major, twelve doubles (eleven and a pad);
 * _forces walks the rows a second time and reads alpha_j of the neighbours.  Every sum has a fixed order and there are no atomics: two
 * identical calls give identical bits.  Arguments are checked before a device is touched: MTD_ERR_INVALID_ARGUMENT for null pointers,
 * non-finite or out-of-range parameters (r_on, r_cut, cos0, with switch_on c0 and p, with gate_on n_lo and n_hi), a switch or a gate
 * without `normalise`, an unknown dtype, a d_scratch that is not 16-byte aligned, a virial pitch below n_particles;
 * MTD_ERR_UNSUPPORTED for n_ghost > 0.
 * ============================================================================================== */

#define MTD_TET_W_MIN 1e-12

typedef struct
    {
    unsigned int type;
    double r_cut, r_on;
    double cos0;
    int normalise;
    int switch_on;
    double c0;
    unsigned int p;
    int gate_on;
    double n_lo, n_hi;
    } mtd_tet_params;

typedef mtd_row_call mtd_tet_call;       /* "Debye structure factor" */

/* device doubles the calls share: sums, value, block sums, three per-particle arrays and the adjoint table */
size_t mtd_tet_scratch_doubles(unsigned int n_particles);

/* This rank's sums: on return *d_sums points at *n_sums = 2 doubles inside c->d_scratch, sum_i v_i and N_t. */
int mtd_tet_accumulate(const mtd_tet_params *p, const mtd_tet_call *c, double **d_sums, unsigned int *n_sums);

/* The tetrahedral order restricted to the largest cluster ("Clusters" above):
 *     s = (1 / N_t) sum_i w_i v_i,   N_t the UNMASKED count of the type
 * with the clusters of mtd_cluster_largest built from the v_i of this call: the nodes are the particles of the type with v_i >= v_min,
 * linked within r_link — the ice, silicon or mW-water nucleus.  Membership is piecewise constant (PLUMED's treatment): the gradient is
 * the one above with alpha_i -> w_i alpha_i, and the variable jumps when clusters merge or split.  The launches: the walk of
 * mtd_tet_accumulate, mtd_cluster_largest on the v row just written, one launch that stores 0 over the adjoint row of every particle
 * with w_i = 0 (stored, not multiplied: a non-finite entry comes out 0 too) and leaves the block sums of w_i v_i, the sums kernel.
 * mtd_tet_finalize and mtd_tet_forces (with its virial) then run unchanged on the masked table: there is no force entry point of its
 * own.  *d_switched of mtd_tet_finalize stays the UNMASKED v_i, the values the clusters were built from.  d_cluster_scratch:
 * mtd_cluster_scratch_bytes(n_particles) bytes, 16-byte aligned, separate from c->d_scratch, whose layout and size do not change;
 * *d_w, *d_label, *d_summary (each may be NULL) point into it as mtd_cluster_largest leaves them.  The stream is c->stream.
 * cluster == NULL or on == 0: mtd_tet_accumulate, bit for bit (that entry point forwards here); the three pointers are set to NULL.
 * With the option on, before a device is touched: everything mtd_tet_accumulate refuses, as there (n_ghost > 0 among it:
 * MTD_ERR_UNSUPPORTED); MTD_ERR_INVALID_ARGUMENT for r_link <= 0 or not finite, v_min not finite, a NULL or misaligned
 * d_cluster_scratch, c->d_nlist == NULL with particles, and for normalise == 0 (A_i is a penalty, not an order: the status a switch or a
 * gate has there).
 * The name spells the unit out: the four mtd_tet_* entry points above are the plain variable's, a set its own tests count. */
int mtd_tetrahedral_accumulate_cluster(const mtd_tet_params *p, const mtd_tet_call *c, const mtd_cluster_params *cluster,
                                       void *d_cluster_scratch, double **d_sums, unsigned int *n_sums, const double **d_w,
                                       const unsigned int **d_label, const unsigned int **d_summary);

/* The sums -> s.  *d_value points at s, one device double (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_value, 1, 1, 0, 1.0, 0.0)), *d_local (may be NULL) at t_i[n_particles] (A_i when not
 * normalised), *d_switched (may be NULL) at v_i[n_particles] and *d_coordination (may be NULL) at n_i[n_particles] of the last
 * mtd_tet_accumulate, all inside c->d_scratch. */
int mtd_tet_finalize(const mtd_tet_params *p, const mtd_tet_call *c, const double **d_value, const double **d_local,
                     const double **d_switched, const double **d_coordination);

/* Writes d_force[0..n_particles) (w component 0; 0 for particles of another type) with what the last mtd_tet_accumulate and
 * mtd_tet_finalize (same p and c) left in c->d_scratch; bias = *d_bias when d_bias != NULL, else bias_host.  d_virial == NULL: no
 * virial; the force array is the same, bit for bit, either way.  Every row [0, n_particles) of the virial is written,
 * [n_particles, virial_pitch) is left alone.  n_particles == 0 is success. */
int mtd_tet_forces(const mtd_tet_params *p, const mtd_tet_call *c, void *d_force, const double *d_bias, double bias_host,
                   void *d_virial, unsigned int virial_pitch);

/* ================================================================================================
 * Bond-orientational order (cv.hexatic) — no reference counterpart.  The k-fold bond-orientational order psi_k about a lab axis: the
 * order WITHIN a layer of two-dimensional and layered matter (2-d melting through the hexatic phase, monolayers at interfaces, confined
 * films, the in-layer order of smectic-B and lamellar phases).  Not rotation invariant: psi_k is the single m = +-k component in the
 * frame of the layer normal, and it carries a phase whose coherence over the box tells a hexatic or a solid from a polycrystal, which
 * q_6 of "Local Steinhardt bond order" cannot.  The conventions of "Debye structure factor" above hold wherever nothing else is said.
 * Parameters: a particle type t; an integer k, 1 <= k <= MTD_HEX_MAX_K; an axis a in {0, 1, 2} = {x, y, z}, the layer normal, with
 * the in-plane components (u, v) the two that follow it cyclically (z -> (x, y), x -> (y, z), y -> (z, x)); 0 <= r_on < r_cut;
 * `global_order`; with global_order = 0 only an optional switch (c0 > 0, integer p >= 1) and an optional gate (0 <= n_lo < n_hi), the
 * functions of mtd_ql_local_options.
 * Entries (i, j) of a FULL list take part when i and j are both of type t, j != i, j is a local particle and 0 < r = |d| <= r_cut,
 * with d = minImage(r_j - r_i) (an entry with r = 0 has no direction and takes no part).  f(r) is the cosine window of the Steinhardt
 * passes between r_on and r_cut.  SINGLE-DOMAIN ONLY: every per-particle array ends at n_particles, an entry j >= n_particles is
 * skipped, and n_ghost > 0 is MTD_ERR_UNSUPPORTED.
 * THIS IS THE DEFINITION:
 *     z_ij  = (u_ij + i v_ij) / r_ij             B_ij = z_ij^k      ( = sin^k(theta) e^{i k phi}: the sectoral harmonic )
 *     n_i   = sum_j f(r_ij)                      S_i  = sum_j f(r_ij) B_ij
 *     psi_i = S_i / n_i     (n_i < MTD_HEX_N_MIN: psi_i = 0 with zero gradient)                  c_i = |psi_i|^2
 *     local  (global_order = 0):   v_i = g(n_i) h(c_i),  s = (1 / N_t) sum_i v_i      (h(c) = c, g = 1 without options)
 *     global (global_order = 1):   Psi = (1 / N_t) sum_i psi_i,  s = |Psi|^2          (v_i = c_i is still stored)
 * with h(c) = x^p / (1 + x^p), x = max(c, 0) / c0, and g the smoothstep of n from n_lo to n_hi.  N_t is the number of centres of the
 * type; N_t = 0: s = 0, no forces.  For a bond in the plane B is exactly the textbook e^{i k phi}; a bond out of the plane is
 * de-weighted by sin^k theta.  B is a polynomial in d / r, so a bond ALONG the axis is an ordinary point (the form (x + i y) / rho has a
 * 1 / rho singularity there).  |psi_i| < 1 on a rippled but perfect layer is therefore INTENDED, not an error of the implementation.
 * c_i is used, not |psi_i|, because it is smooth at 0.  Lattice values: c_i = 1 and |Psi|^2 = 1 on a perfect triangular monolayer with
 * k = 6, for any in-plane rotation, and 0 with k = 3; psi_i = -1/6, s = 1/36 in both modes on perfect fcc with the window over the first
 * shell only, k = 4 and any of the three axes (in the plane 4 (-1), out of it 8 (1/4) (+1), over n = 12).
 * Gradient.  With G(d) = grad_d [ f(|d|) B(d) ] = f' B d/r + f [ (k z^(k-1) / r) (e_u + i e_v) - (k B / r^2) d ] every centre has an
 * adjoint (alpha_i complex, beta_i real) with d(N_t s) = sum_i [ Re(conj(alpha_i) dS_i) + beta_i dn_i ]:
 *     local:    alpha_i = 2 g h' psi_i / n_i       beta_i = g' h - 2 g h' c_i / n_i
 *     global:   alpha_i = 2 Psi / n_i              beta_i = -2 Re(conj(Psi) psi_i) / n_i
 * both 0 where n_i < MTD_HEX_N_MIN.  An entry has g_ij = Re(conj(alpha_i) G(d_ij)) + beta_i grad f(d_ij) and gives +g_ij to
 * d(N_t s)/dr_j and -g_ij to d(N_t s)/dr_i.  B has parity (-1)^k, so as a gather over row k of a symmetric list
 *     N_t ds/dr_k = - sum_{j in row k} [ Re( conj(alpha_k + (-1)^k alpha_j) G(d_kj) ) + (beta_k + beta_j) grad f(d_kj) ],   F = -bias ds/dr
 * The second terms read the adjoint of the neighbour.  sum_k F_k = 0 on a single domain.  The pair term is NOT parallel to d, and the
 * variable is NOT invariant under a rotation that tilts the axis: there is a net torque about every direction but the axis.
 * Virial (only with a virial pointer), in the convention of mtd_es_forces: the six stored components (a, b), a <= b, are derivatives
 * under x_a -> x_a + eps x_b of positions and box, sum_k virial_k[ab] = -(bias / N_t) sum_entries g_ij,a d_ij,b; the tensor is not
 * symmetric; half of every entry goes to each of its ends; no explicit volume term.  Layout, scalar type and pitch rule of
 * mtd_tet_forces.
 * KNOWN PROPERTY.  Without a gate a particle whose shell is nearly empty (one neighbour just entering the window) has |psi_i| = 1 and a
 * jump-free but steep gradient of order 1 / f: inherent to a weighted mean.  The gate removes it; dilute systems should use one.
 * A step is _accumulate, _finalize, _forces with the same parameters, call block and scratch.  _accumulate walks the rows once and
 * stores n_i, c_i, v_i, psi_i and, in local mode, the adjoint row of every particle — ROW-major, four doubles (alpha_re, alpha_im, beta
 * and a pad); _finalize forms s and Psi and, in global mode, writes the adjoint rows, which need Psi; _forces walks the rows a second time
 * and reads the rows of the neighbours.  Every sum has a fixed order and there are no atomics: two identical calls give identical bits,
 * and a row gives the same bits wherever it lies in the list.  Arguments are checked before a device is touched:
 * MTD_ERR_INVALID_ARGUMENT for null pointers, a non-finite or out-of-range window, k = 0, axis > 2, a bad switch (c0, p) or gate
 * (n_lo, n_hi), an unknown dtype, a d_scratch that is not 16-byte aligned, a virial pitch below n_particles; MTD_ERR_UNSUPPORTED for
 * k > MTD_HEX_MAX_K, a switch or a gate together with global_order, and n_ghost > 0 (the force reads a neighbour's adjoint row, which a
 * ghost does not have).
 * ============================================================================================== */

#define MTD_HEX_MAX_K 12
#define MTD_HEX_N_MIN 1e-12

typedef struct
    {
    unsigned int type;
    unsigned int k;
    unsigned int axis;                   /* 0, 1, 2: x, y, z — the layer normal */
    double r_cut, r_on;
    int global_order;
    int switch_on;
    double c0;
    unsigned int p;
    int gate_on;
    double n_lo, n_hi;
    } mtd_hex_params;

typedef mtd_row_call mtd_hex_call;       /* "Debye structure factor" */

/* device doubles the calls share: sums, value, block sums, the per-particle arrays and the adjoint table */
size_t mtd_hex_scratch_doubles(unsigned int n_particles);

/* This rank's sums: on return *d_sums points at *n_sums = 4 doubles inside c->d_scratch, in both modes: sum_i v_i, N_t, sum_i Re psi_i,
 * sum_i Im psi_i — ready for mtd_comm_allreduce_small. */
int mtd_hex_accumulate(const mtd_hex_params *p, const mtd_hex_call *c, double **d_sums, unsigned int *n_sums);

/* The sums -> s.  *d_value points at s, one device double (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_value, 1, 1, 0, 1.0, 0.0)) followed by N_t, Re Psi and Im Psi (Psi in both modes);
 * *d_local (may be NULL) at c_i[n_particles], *d_switched (may be NULL) at v_i[n_particles], *d_coordination (may be NULL) at
 * n_i[n_particles] and *d_psi (may be NULL) at psi_i as n_particles interleaved (Re, Im) pairs of the last mtd_hex_accumulate, all inside
 * c->d_scratch.  In global mode this is the launch that completes the adjoint rows. */
int mtd_hex_finalize(const mtd_hex_params *p, const mtd_hex_call *c, const double **d_value, const double **d_local,
                     const double **d_switched, const double **d_coordination, const double **d_psi);

/* Writes d_force[0..n_particles) (w component 0; 0 for particles of another type) with what the last mtd_hex_accumulate and
 * mtd_hex_finalize (same p and c) left in c->d_scratch; bias = *d_bias when d_bias != NULL, else bias_host.  d_virial == NULL: no
 * virial; the force array is the same, bit for bit, either way.  Every row [0, n_particles) of the virial is written,
 * [n_particles, virial_pitch) is left alone.  n_particles == 0 is success. */
int mtd_hex_forces(const mtd_hex_params *p, const mtd_hex_call *c, void *d_force, const double *d_bias, double bias_host,
                   void *d_virial, unsigned int virial_pitch);

/* ================================================================================================
 * Bragg intensity (cv.bragg) — no reference counterpart.  The intensity of chosen Bragg peaks, i.e. the structure factor at chosen
 * reciprocal-lattice vectors: the phase-free companion of "Lamellar order parameter" above.  That variable takes Re rho_k and so depends
 * on where the density wave sits in the box (a shift by a quarter period takes it from its maximum to zero); |rho_k| does not.  It is
 * what order-disorder studies of block copolymers bias, the variable of the interface-pinning method (Pedersen, J. Chem. Phys. 139,
 * 104102) and of crystallisation along a chosen lattice direction.  Oriented, unlike "Debye structure factor"; O(N K), no neighbour list.
 * Parameters: K = n_modes integer triples (h, k, l), 1 <= K <= MTD_BRAGG_MAX_MODES; an amplitude a(t) per particle type (finite, any
 * sign, n_types <= MTD_MAX_TYPES); weights w_k (finite, any sign; the Python layer defaults to 1 / K); `modulus`; the trigonometry of
 * "Lamellar order parameter" (trig_mode; same precondition, same rule for when the hardware instructions are taken).
 *     q_k   = 2 pi (h b1' + k b2' + l b3'),  b_i' the reciprocal rows of the GLOBAL box
 *     rho_k = sum_j a(type_j) exp(i q_k . r_j)         over ALL particles of all ranks
 *     A1 = sum_j |a_j|,  A2 = sum_j a_j^2
 *     s = sum_k w_k |rho_k|^2 / A1^2                   (default)
 *     s = sum_k w_k |rho_k| / A1                       (modulus != 0)
 *     S_k = |rho_k|^2 / A2                             (the structure factor at q_k: a diagnostic, 0 when A2 = 0)
 * Both forms lie in [0, sum_k w_k] for weights >= 0: 1 for a perfect density wave of one sign, O(1 / N) (default) or O(1 / sqrt N)
 * (modulus) for N random positions.  A1 = 0 (no particle with an amplitude): s = 0, S_k = 0, every coefficient 0, no forces; nothing NaN.
 * Gradient, with phi_kj = q_k . r_j, alpha_k = ds / d Re rho_k and beta_k = ds / d Im rho_k:
 *     default:  (alpha_k, beta_k) = 2 w_k (Re rho_k, Im rho_k) / A1^2
 *     modulus:  (alpha_k, beta_k) = w_k (Re rho_k, Im rho_k) / (|rho_k| A1), both 0 when |rho_k| = 0 (the modulus has a cusp there; the
 *               force of a mode stays below w_k |q_k| |a_j| |bias| / A1 however small |rho_k| is)
 *     ds/dr_j = a_j sum_k q_k (-alpha_k sin phi_kj + beta_k cos phi_kj),   F_j = -bias ds/dr_j,  force.w = 0
 * This is the exact gradient: the factor 2 of the lamellar force (quirk Q1) has no place here.  s does not change when all particles are
 * shifted together, so sum_j F_j = 0.  The phase depends on fractional coordinates only, so s does not change under an affine strain of
 * box and positions either: THE BIAS FORCE HAS NO VIRIAL and these entry points write none.
 * Arithmetic of the lamellar kernels: fractional projections in fp64, the phase in turns rounded once to fp32, fp32 trigonometry; every
 * term is added in fp64, in a fixed order, no atomics: two identical calls give identical bits, and two splits of the particles over
 * ranks give sums that differ by fp64 rounding only.
 * A step is _accumulate, (mtd_comm_allreduce_small of *d_sums in a domain-decomposed run: any split of the particles over the ranks
 * will do, there are no ghosts), _finalize, _forces with the same parameters, call block and scratch.  Arguments are checked before a
 * device is touched: MTD_ERR_INVALID_ARGUMENT for null pointers, n_modes == 0, n_types == 0 or above MTD_MAX_TYPES, a non-finite
 * weight or amplitude, an unknown dtype or trig mode, a d_scratch that is not 16-byte aligned, n_global == 0, a box without volume;
 * MTD_ERR_UNSUPPORTED for n_modes > MTD_BRAGG_MAX_MODES.
 * ============================================================================================== */

#define MTD_BRAGG_MAX_MODES 16

typedef struct
    {
    unsigned int n_modes;                      /* K */
    int hkl[MTD_BRAGG_MAX_MODES][3];
    unsigned int n_types;
    double coeff[MTD_MAX_TYPES];               /* a(t) */
    double weights[MTD_BRAGG_MAX_MODES];       /* w_k */
    int modulus;
    int trig_mode;                             /* enum mtd_trig_mode */
    } mtd_bragg_params;

/* What the calls of a step share beside the parameters.  n_global, the particles of all ranks, enters no formula (the normalisation is
 * A1); it tells an empty system, which is refused, from a rank that happens to hold no particle (n_particles == 0), which is not. */
typedef struct
    {
    unsigned int n_particles;
    const void *d_postype;
    int dtype;
    const mtd_box *global_box;
    unsigned int n_global;
    double *d_scratch;
    mtd_stream_t stream;
    } mtd_bragg_call;

/* device doubles the calls share: sums, value, S_k, coefficients and the rows of block sums; the same for every particle count */
size_t mtd_bragg_scratch_doubles(unsigned int n_particles);

/* This rank's sums: on return *d_sums points at *n_sums = 2 K + 2 doubles inside c->d_scratch — Re rho_0, Im rho_0, ..., A1, A2 —
 * ready for mtd_comm_allreduce_small. */
int mtd_bragg_accumulate(const mtd_bragg_params *p, const mtd_bragg_call *c, double **d_sums, unsigned int *n_sums);

/* The (reduced) sums -> s, S_k and the coefficients.  *d_value points at s, one device double (consume with
 * mtd_metad_set_cv_source(engine, slot, *d_value, 1, 1, 0, 1.0, 0.0)); *d_structure_factors at S_k[K]; *d_amplitudes at the K pairs
 * (Re rho_k, Im rho_k), which are the sums themselves; *d_gradient at the K pairs (alpha_k, beta_k) — each of the three may be NULL —
 * all inside c->d_scratch. */
int mtd_bragg_finalize(const mtd_bragg_params *p, const mtd_bragg_call *c, const double **d_value, const double **d_structure_factors,
                       const double **d_amplitudes, const double **d_gradient);

/* Writes d_force[0..n_particles) (w component 0) with the coefficients the last mtd_bragg_finalize (same p and c) left in
 * c->d_scratch; bias = *d_bias when d_bias != NULL, else bias_host.  n_particles == 0 is success. */
int mtd_bragg_forces(const mtd_bragg_params *p, const mtd_bragg_call *c, void *d_force, const double *d_bias, double bias_host);

/* ================================================================================================
 * Probe volume (cv.probe_volume) — no reference counterpart.  The coarse-grained number of particles in a region fixed in space, the
 * variable of the INDUS method (Patel, Varilly, Chandler, Garde, J. Stat. Phys. 145, 265 (2011)): it is biased to empty a cavity next to
 * a surface, to fill or drain a pore, to drive cavitation at a chosen place, to hold a slab at a given filling.  Every other variable
 * here is a property of the whole box; this one says where.  O(N), positions and types only, no neighbour list.
 *     s   = N~_v = sum_i a(type_i) h(d_i),   d_i = min_image(r_i - c)            over ALL particles of all ranks
 *     N_v        = sum_i a(type_i) [d_i inside the sharp region]                 (a diagnostic, not biased)
 * a(t): a weight per particle type (finite, any sign, n_types <= MTD_MAX_TYPES); c: the centre; min_image: HOOMD's BoxDim::minImage of
 * the GLOBAL box.  Smoothing is one-dimensional, the truncated and shifted Gaussian of the paper with width sigma_s and cut-off r_c:
 *     Phi(u) = [exp(-u^2 / 2 sigma_s^2) - exp(-r_c^2 / 2 sigma_s^2)] / k      for |u| < r_c, else 0
 *     k      = sqrt(2 pi) sigma_s erf(r_c / (sqrt2 sigma_s)) - 2 r_c exp(-r_c^2 / 2 sigma_s^2)
 *     G(u)   = 0 (u <= -r_c),  1 (u >= r_c),  else  1/2 + [sqrt(pi/2) sigma_s erf(u / (sqrt2 sigma_s)) - u exp(-r_c^2 / 2 sigma_s^2)] / k
 * G' = Phi; both are continuous and Phi(+-r_c) = 0, so h and the bias force are continuous (the force has a kink at the shell's edge).
 * Shapes:
 *     MTD_PROBE_BOX       half-widths w along the lab axes, each > 0 or +inf (unbounded: a slab, a channel), at least one finite:
 *                         h = prod over the bounded axes of [G(w - d) - G(-w - d)]  (the paper's form),
 *                         dh/dd_al = [Phi(-w_al - d_al) - Phi(w_al - d_al)] (the other factors)
 *     MTD_PROBE_SPHERE    radius R > r_c:  h = G(R - |d|),  grad h = -Phi(R - |d|) d / |d|  (0 at |d| = 0, where Phi(R) = 0)
 *     MTD_PROBE_CYLINDER  axis along lab x, y or z (axis = 0, 1, 2), radius R > r_c, half-length half_width[axis] > 0 or +inf:
 *                         h = G(R - d_perp) [G(w - d_ax) - G(-w - d_ax)]
 * Sphere and cylinder smooth RADIALLY.  That is not the paper's three-dimensional convolution of the indicator; the two agree for
 * sigma_s << R.  "Inside the sharp region": -w_al <= d_al < w_al on every bounded axis, |d| < R, d_perp < R.
 * The centre is handed over in FRACTIONAL coordinates f of the global box, c = lo + f_0 a_1 + f_1 a_2 + f_2 a_3 with the lattice
 * vectors a_1 = (Lx, 0, 0), a_2 = (xy Ly, Ly, 0), a_3 = (xz Lz, yz Lz, Lz): under a box change it follows the box affinely.  Widths, R,
 * sigma_s and r_c stay absolute lengths.
 * THE FIT RULE.  Region and shell must lie inside the cell that min_image maps into; it is checked against the box of every call (the
 * box changes in constant-pressure runs) and a region that does not fit is refused with MTD_ERR_INVALID_ARGUMENT.  With the extent
 * e_al = w_al + r_c (box; cylinder axis) or R + r_c (sphere; across a cylinder) on every bounded lab axis al:
 *     a box with xy = xz = yz = 0:   e_al <= L_al / 2;
 *     any other box: with b_i' row i of the inverse of the matrix of lattice vectors (b_i' . a_j = delta_ij), for every lattice vector
 *                    a_i that has a non-zero component along a bounded axis: sum over the bounded al of |b_i'[al]| e_al <= (1 + 1e-12) / 2
 *                    (1e-12 for the roundings of the inverse), and b_i'[al] = 0 for every unbounded al.
 * Force: F_i = -bias a_i grad h(d_i), the exact gradient, written for EVERY particle (0 outside region and shell; force.w = 0).  The
 * region is an external object: THE BIAS FORCES DO NOT SUM TO ZERO, and that is correct.
 * Virial (only with a virial pointer): positions and box strained together, the centre following; then ds/d eps_ab = sum_i a_i
 * dh/dd_a d_b, and  virial_i[ab] = -bias a_i (d_a h d_b + d_b h d_a) / 2,  so that sum_i virial_i = -bias (symmetrised ds/d eps).
 * Layout, scalar type and pitch rule of mtd_ql_local_forces_virial (virial[c * pitch + i], c = xx, xy, xz, yy, yz, zz); every row
 * [0, n_particles) is written, [n_particles, virial_pitch) is left alone.  The force array is the same, bit for bit, with and without.
 * Arithmetic: everything behind the load is fp64 for both array types (fp32 positions are promoted exactly), so a term is the same bits
 * on whichever rank its particle sits; sums in a fixed order, no atomics: two identical calls give identical bits.  Only lanes with
 * |u| < r_c on some face evaluate erf and exp.
 * A step is _accumulate, (mtd_comm_allreduce_small of *d_sums in a domain-decomposed run: any split of the particles over the ranks will
 * do, ghosts are not handed over), _finalize, _forces with the same parameters, call block and scratch.  Arguments are checked before a
 * device is touched: MTD_ERR_INVALID_ARGUMENT for null pointers, an unknown shape, axis, dtype; sigma_s or r_c not positive and finite;
 * a half-width that is not positive (NaN included) or a box without a bounded axis; R not finite or not above r_c; a non-finite centre
 * or weight; n_types == 0 or above MTD_MAX_TYPES; a d_scratch that is not 16-byte aligned; n_global == 0; a box without volume; a region
 * that does not fit; a virial pitch below n_particles.
 * ============================================================================================== */

enum mtd_probe_shape { MTD_PROBE_BOX = 0, MTD_PROBE_SPHERE = 1, MTD_PROBE_CYLINDER = 2 };

typedef struct
    {
    int shape;                                 /* enum mtd_probe_shape */
    int axis;                                  /* cylinder: 0, 1, 2 for x, y, z; ignored otherwise */
    double centre[3];                          /* FRACTIONAL coordinates of the centre in the global box */
    double half_width[3];                      /* box: w_x, w_y, w_z; cylinder: half_width[axis] is the half-length; +inf: unbounded */
    double radius;                             /* sphere, cylinder: R */
    double sigma_s;
    double r_c;
    unsigned int n_types;
    double coeff[MTD_MAX_TYPES];               /* a(t) */
    } mtd_probe_params;

/* What the calls of a step share beside the parameters.  n_global, the particles of all ranks, enters no formula; it tells an empty
 * system, which is refused, from a rank that happens to hold no particle (n_particles == 0), which is not. */
typedef struct
    {
    unsigned int n_particles;                  /* local particles only: ghosts are not counted */
    const void *d_postype;
    int dtype;
    const mtd_box *global_box;
    unsigned int n_global;
    double *d_scratch;
    mtd_stream_t stream;
    } mtd_probe_call;

/* device doubles the calls share: the two sums and the rows of block sums; the same for every particle count */
size_t mtd_probe_scratch_doubles(unsigned int n_particles);

/* This rank's sums: on return *d_sums points at *n_sums = 2 doubles inside c->d_scratch, (N~_v, N_v), ready for
 * mtd_comm_allreduce_small. */
int mtd_probe_accumulate(const mtd_probe_params *p, const mtd_probe_call *c, double **d_sums, unsigned int *n_sums);

/* *d_value points at s = N~_v, one device double (consume with mtd_metad_set_cv_source(engine, slot, *d_value, 1, 1, 0, 1.0, 0.0)),
 * *d_count (may be NULL) at N_v, both inside c->d_scratch.  The (reduced) sums ARE the results: this call launches nothing. */
int mtd_probe_finalize(const mtd_probe_params *p, const mtd_probe_call *c, const double **d_value, const double **d_count);

/* Writes d_force[0..n_particles) from the positions alone (nothing of _accumulate is read); bias = *d_bias when d_bias != NULL, else
 * bias_host.  d_virial == NULL: no virial, and the kernel is the one without it.  n_particles == 0 is success. */
int mtd_probe_forces(const mtd_probe_params *p, const mtd_probe_call *c, void *d_force, const double *d_bias, double bias_host,
                     void *d_virial, unsigned int virial_pitch);

/* Off the step path: d_out[0..n_particles) = h(d_i), one device double per particle, WITHOUT the weight of its type. */
int mtd_probe_local(const mtd_probe_params *p, const mtd_probe_call *c, double *d_out);

/* ================================================================================================
 * Neighbour list of the stand-alone path (cell list, built on the device)
 * no reference counterpart: HOOMD's md::NeighborList is HOOMD core.  Produces the three arrays SteinhardtQl.cc:80-85 reads, in
 * HOOMD's layout: the neighbours of particle i are d_nlist[d_head_list[i] .. d_head_list[i] + d_n_neigh[i]).
 * ============================================================================================== */

typedef struct mtd_nlist mtd_nlist;

/* A handle owns its device buffers and grows them geometrically.  _create touches no device (buffers come with the first build);
 * it returns hipErrorOutOfMemory (as a positive status) when the host allocation of the handle fails. */
int mtd_nlist_create(mtd_nlist **out);
int mtd_nlist_destroy(mtd_nlist *h);

/* All pairs with |minimum_image(r_i - r_j)|^2 <= r_list^2, tested in fp64 (MTD_F32 positions are widened first) under HOOMD's
 * BoxDim::minImage of `box`, for the n_local particles at the front of d_postype; the n_ghost particles behind them are partners
 * only and own no row (entries may index them, as n_local, n_local + 1, ...).
 *   half_nlist = 0: full list, (i, j) listed <=> (j, i) listed for local i, j;  != 0: every pair once, in the row of its smaller
 *                   index (MTD_ERR_UNSUPPORTED together with ghosts: SteinhardtQl refuses that combination)
 *   type >= 0:      only pairs whose two particles are both of that type (cv.steinhardt.get_rcut, cv.py:603-622); -1: all pairs
 * Cells per direction: floor(d_k / r_list), d_k = distance between the k-th pair of faces of the box (tilt included), at least 1.
 * In a box that is large against the particle number the count is capped at cbrt(2 N) per direction (not below 3, not above 1024),
 * so that a dilute system does not pay for millions of empty cells: fewer, larger cells give the same list.
 * r_list <= d_k / 2 is required in every periodic direction (then no cell is visited twice and the image is unique), else
 * MTD_ERR_INVALID_ARGUMENT; directions with box->periodic[k] == 0 take no image and do not wrap.  Arguments (null handle,
 * r_list <= 0, unknown dtype, r_list against the box) are checked before the device is touched.
 * The result does not depend on the arrival order of any atomic: two builds of the same input give the same bits, whatever the
 * handle built before.  Rows are ordered by cell, inside a cell by particle index.
 * Synchronises the stream ONCE (the entry count sizes d_nlist); the fill itself is only stream-ordered.  The returned device
 * pointers belong to the handle and stay valid until its next build or its destruction; *n_entries (host) = sum of d_n_neigh. */
int mtd_nlist_build(mtd_nlist *h, unsigned int n_local, unsigned int n_ghost, const void *d_postype, int dtype,
                    const mtd_box *box, double r_list, int half_nlist, int type, const unsigned int **d_head_list,
                    const unsigned int **d_n_neigh, const unsigned int **d_nlist, size_t *n_entries, mtd_stream_t stream);

/* HOOMD's displacement check: *needs_rebuild (host) = 1 when some particle of the last build (locals and ghosts, the same N and
 * order) has moved by more than r_buff / 2 since then, under minimum image (a particle that was wrapped into the box has not
 * moved by L); also 1, without any device work, when the box or the dtype differ from the last build's or nothing was built yet.
 * A caller whose particle number changed builds anew (the check has the last build's N).  One launch and one stream
 * synchronisation. */
int mtd_nlist_check(mtd_nlist *h, const void *d_postype, int dtype, const mtd_box *box, double r_buff, int *needs_rebuild,
                    mtd_stream_t stream);

/* cells per direction of the handle's last build, the cap of mtd_nlist_build applied (host, no device work);
 * MTD_ERR_INVALID_ARGUMENT before the first build */
int mtd_nlist_cells(const mtd_nlist *h, unsigned int dim[3]);

/* ================================================================================================
 * WellTemperedEnsemble (potential energy as CV)
 * replaces WellTemperedEnsemble.cuh:3-19 (gpu_scale_netforce, gpu_reduce_potential_energy)
 * ============================================================================================== */

size_t mtd_wte_scratch_doubles(unsigned int n_particles);

/* gpu_reduce_potential_energy (.cu:195-243): block partial sums of net_force.w.
 * PE = external_energy + sum_b d_partials[b]; consume with mtd_metad_set_cv_source / mtd_reduce_partials */
int mtd_wte_energy_partials(unsigned int n_particles, const void *d_net_force, int dtype,
                            double *d_partials, unsigned int *n_partials, mtd_stream_t stream);

/* gpu_scale_netforce (.cu:53-89): net_force.xyz, net_torque.xyz and the six net_virial rows are
 * multiplied by (1 + bias); bias = *d_bias when d_bias != NULL (device resident), else bias_host.
 * scale_torque_w != 0 also scales net_torque.w like the reference CPU path (WellTemperedEnsemble.cc:169). */
int mtd_wte_scale_netforce(unsigned int n_particles, void *d_net_force, void *d_net_torque,
                           void *d_net_virial, unsigned int virial_pitch, int dtype, const double *d_bias,
                           double bias_host, int scale_torque_w, mtd_stream_t stream);

/* ================================================================================================
 * CollectiveWrapper (energy of an arbitrary ForceCompute as CV)
 * replaces CollectiveWrapper.cc:74-134 (computeCVGPU / computeBiasForcesGPU, which reuse the WTE drivers)
 * ============================================================================================== */

/* energy = external_energy + sum_j force_j.w: use mtd_wte_energy_partials on the wrapped force array.
 * computeBiasForces (:125, :153): force.xyz, torque.xyz(w) and the six virial rows of the WRAPPED compute are
 * multiplied by the bias factor itself (not 1 + bias as in the WTE) */
int mtd_wrapper_scale_forces(unsigned int n_particles, void *d_force, void *d_torque, void *d_virial,
                             unsigned int virial_pitch, int dtype, const double *d_bias, double bias_host,
                             int scale_torque_w, mtd_stream_t stream);

/* ================================================================================================
 * Adaptive Gaussians
 * replaces IntegratorMetaDynamics::computeSigma (IntegratorMetaDynamics.cc:1205-1294)
 * ============================================================================================== */

size_t mtd_sigma_scratch_doubles(void);

/* sigmasq[i*n_cv+j] = sigma_g^2 * sum_n f_i(n).f_j(n) over this rank's particles (:1241-1246), for the CVs whose
 * d_force[c] != NULL (those that can compute derivatives); all other entries come back 0 and are the caller's
 * (:1249: diagonal sigma^2 on the root rank).  Synchronous: sigmasq is a HOST array of n_cv^2 doubles; in a
 * domain-decomposed run it is all-reduced before mtd_sigma_inverse (:1259-1268). */
int mtd_sigma_products(unsigned int n_cv, const void *const *d_force, unsigned int n_particles, int dtype, double sigma_g,
                       double *d_scratch, double *sigmasq, mtd_stream_t stream);

/* sigma_inv = inverse(element-wise sqrt(sigmasq)) (:1273-1286), host arrays of n_cv^2 doubles */
int mtd_sigma_inverse(unsigned int n_cv, const double *sigmasq, double *sigma_inv);

/* ================================================================================================
 * Diagnostic exports: the two pieces of device code whose reference counterparts COULD be compiled (oracle/_ref), exposed so
 * that tests hold the kernels' own arithmetic — not only the oracle's — against the vectors the reference code produced
 * (tests/golden/, tests/test_gpu_golden.py).  Host arrays in and out, synchronous; not part of the hot path.
 * ============================================================================================== */

/* Y_lm of n directions (h_separations: n x 3, any length) as the Steinhardt pair kernels evaluate them; h_out:
 * n x (lmax+1)^2 x (re, im) in fsph's order (spherical_harmonics.hpp:229-246 with full_m) */
int mtd_debug_sph_harmonics(unsigned int lmax, unsigned int n, const double *h_separations, double *h_out);
/* IndexGrid::getCoordinates (IndexGrid.cc:46-58) and getIndex (:20-44) as the grid kernels compute them */
int mtd_debug_index_decode(unsigned int n_cv, const unsigned int *lengths, unsigned int n, const unsigned int *h_indices,
                           unsigned int *h_coords, unsigned int *h_index_back);
/* The agreement check of mtd_metad_update_bias_walkers as two pure-host functions (no device needed; tests/test_abi_exports.py):
 * _pack writes the 12 doubles a walker contributes for (stride, add_bias, timestep) — each quantity split into 16-bit halves,
 * every half followed by its square, so that sums over <= 2^16 walkers stay exact integers below 2^53 whatever the order of
 * the reduction; _verify returns 1 when `sums` (the all-reduced 12 doubles) say that all `world` walkers sent what `mine` holds. */
void mtd_debug_walker_check_pack(unsigned int stride, int add_bias, unsigned int timestep, double *out12);
int mtd_debug_walker_check_verify(const double *sums12, const double *mine12, unsigned int world);

#ifdef __cplusplus
}
#endif
#endif /* MTD_ABI_H */
