"""GPU parity: the block roles of the fused two-launch step (mtd_fused_cv_pass + mtd_fused_force_pass), as they ARE.

The order of the blocks is the one the step always had: passengers first (apply block j / grid block g = blockIdx.x <
n_passenger_blocks), the particle blocks (CV blocks / force blocks) behind them.  Particle blocks first was built and measured
slower (profiles/r17/README.md) and is not in the tree; this file does not test a new order, it PINS the existing one together
with what did change: launch B gets its two block counts, the particle array and the resolved addresses of the chain's partial
sums from an entry block filled by the host.  Block 0 publishes the step's scalars: grid block 0 where the launch has grid
blocks, force block 0 otherwise.  A mix-up of a role, of a block -> particle or block -> cell
mapping, of a count in the entry block or of the publishing block shows at the smallest shapes already, so these are small:
particle counts around one force block of the fp32 hardware-trigonometry instantiation (1536 = 192 threads x 4 particles x 2
groups; fp64 arrays and the other trigonometry run other group counts, hence other block counts) and one CV block's first group
(512 x 4), grids with fewer cells than one passenger block, with a partial last block, in one, two and three dimensions, every
launch with passengers (stride 1) and launches without grid blocks / without apply blocks on alternate steps (stride 2, no
hills), the grid engine on its own, and the sharded form with a one-rank mailbox (the chain's sums come out of the mailbox, the
entry block's are switched off).

Every sequence is run twice, as tests/test_gpu_fused.py does: with a read-back after every step (every array, V, w, the bias
factors and the forces against the oracle, step by step — the read-back flushes the deferred pass, so launch A has no apply
blocks) and without any (the deferred pass rides in the next launch A as its apply blocks), then everything once at the end.

Tolerances are those of tests/test_gpu_fused.py: the first CV to 1e-6 relative, the cancelling ones to max(1e-6 |s|, 1e-6 * 8 /
sqrt(N)); forces to 1e-5 of max|F|; grid arrays, V, w and the bias factors through test_gpu_metad.compare (integer arrays bit
for bit).  With ONE particle every CV is a cancelling one and gets the second form, as test_one_launch_step_shapes there gives
it at N = 1: the value is the sum of that particle's eight cosines, terms of order one in fp32 (6e-8 each, and half an ulp of a
phase of 1.5 turns is 3.7e-7 in a cosine's argument) that cancel to a third of one term — nothing averages over particles, and
1e-6 of the cancelled total is less than eight fp32 roundings of its terms.  Measured with the first CV held to 1e-6 relative
everywhere: |deviation| / bound at most 0.24 at N = 63, at most 0.11 from N = 1535 up, and 3.0 - 3.8 at N = 1 (-0.3584186 against
-0.3584175, both trigonometries, fp32 and fp64 arrays: that is the launch-A kernel, unchanged code).  check_cvs
prints every CV's deviation in units of its bound before it asserts.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import util
from test_gpu_fused import Fused, make_traj
from test_gpu_metad import GpuMetad, compare

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STEPS = 5
L_BOX = 20.0
ALL_CVS = [(util.CV1_VECTORS, util.MODE_AB), (util.CV2_VECTORS, util.MODE_AB), ([(0, 0, 3), (1, 2, 0), (2, 0, -1)], [0.5, -1.5])]
CV_MIN, CV_MAX = [-0.6, -0.3, -0.5], [0.4, 0.3, 0.5]

# grids by name: (number of variables, points per variable)
GRIDS = {
    "5x7": (2, [5, 7]),                 # fewer cells than one block: one grid block, one apply block
    "33x31": (2, [33, 31]),             # 1023 cells: a partial last block
    "1d_512": (1, [512]),
    "9x8x7": (3, [9, 8, 7]),
}
PARTICLE_GRIDS = {1: "1d_512", 2: "33x31", 3: "9x8x7"}


def grid_kw(name, stride=1, add_bias=True):
    n, pts = GRIDS[name]
    # hills about one cell wide, so that a cell written by the wrong block, or not at all, is far outside compare()'s 1e-11 — but
    # not narrower than 3 % of the variable's range: the variables move by a few per cent of it per step, and the bias force at
    # the new values must stay a number fp32 force arrays can hold (behind a hill of 0.0016 it was 1e-160 of nothing)
    sigma = [max(0.8 / (pts[i] - 1), 0.03) * (CV_MAX[i] - CV_MIN[i]) for i in range(n)]
    return dict(sigma=sigma, cv_min=CV_MIN[:n], cv_max=CV_MAX[:n], num_points=pts, W=1.0, T_shift=7.0, T=1.0, stride=stride,
                mode="well_tempered", add_bias=add_bias)


@functools.lru_cache(maxsize=None)
def trajectory(N, dtype_name):
    """positions of every step (make_traj of test_gpu_fused.py, cut to N particles) — computed once, shared, never changed"""
    dtype = np.dtype(dtype_name).type
    traj, types = make_traj(max(N, 1), L_BOX, STEPS, dtype)
    traj = tuple(np.ascontiguousarray(p[:N]) for p in traj)
    for p in traj:
        p.setflags(write=False)
    return traj, types[:N]


@functools.lru_cache(maxsize=None)
def oracle_cvs(N, dtype_name, n_cv):
    import mtd_ref
    traj, types = trajectory(N, dtype_name)
    rbox = mtd_ref.Box.make(L_BOX)
    out = []
    for p in traj:
        opt = util.oracle_postype(p, types)
        out.append([mtd_ref.lamellar_cv(v, opt, m, rbox, n_global=max(N, 1)) for v, m in ALL_CVS[:n_cv]])
    return out


def check_cvs(cv, s_ref, N, where):
    for c, (got, want) in enumerate(zip(cv, s_ref)):
        tol = 1e-6 * abs(want)
        if c > 0 or N == 1:
            tol = max(tol, 1e-6 * 8 / np.sqrt(max(N, 1)))
        print("cv %d: |dev| / bound = %.3f (%s)" % (c, abs(got - want) / tol if tol > 0 else float(got != want), where))
        assert abs(got - want) <= tol, (where, c, got, want, tol)


def run_sequence(abi, ref, N, dtype, grid, stride, add_bias, fast, attach=None, detach=None):
    """STEPS steps of the two-launch form, twice (read-back after every step / none); attach(g) / detach(g): called on each
    engine before its first step and before it is closed (the sharded case attaches its mailbox)"""
    lib = abi.load()
    n_cv = GRIDS[grid][0]
    cvs = ALL_CVS[:n_cv]
    kw = grid_kw(grid, stride, add_bias)
    traj, types = trajectory(N, np.dtype(dtype).name)
    s_refs = oracle_cvs(N, np.dtype(dtype).name, n_cv)
    box, rbox = abi.Box.make(L_BOX), ref.Box.make(L_BOX)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_traj = [torch.from_numpy(util.pack_postype(p, types, dtype)).cuda() if N else torch.zeros((1, 4), dtype=tdt, device="cuda")
              for p in traj]
    where = "N=%d %s %s stride=%d hills=%d fast=%d" % (N, np.dtype(dtype).name, grid, stride, add_bias, fast)
    abi.check(lib.mtd_lamellar_set_fast_trig(fast))
    try:
        # run 1: read back after every step
        g = GpuMetad(abi, **kw)
        r = ref.Metad(**kw)
        cv_log = []
        try:
            if attach:
                attach(g)
            f = Fused(abi, g, N, dtype, False, cvs)
            for t in range(STEPS):
                f.step(t, d_traj[t], box, n_global=max(N, 1))
                torch.cuda.synchronize()
                F = [x.cpu().numpy().astype(np.float64) for x in f.forces]       # formed before any flush: grab them first
                st = g.state()
                check_cvs(st["cv"], s_refs[t], N, (where, t))
                cv_log.append(st["cv"].copy())
                b = r.update_bias(t, st["cv"])                                   # oracle grid driven with the device's CV values
                compare(g, r, b, label="%s step %d" % (where, t))
                if N == 0:
                    continue
                opt = util.oracle_postype(traj[t], types)
                for c, (v, m) in enumerate(cvs):
                    F_ref = ref.lamellar_forces(v, opt, m, rbox, b[c], n_global=N)
                    scale = np.abs(F_ref[:, :3]).max()
                    if scale > 0:
                        assert np.abs(F[c][:, :3] - F_ref[:, :3]).max() <= 1e-5 * scale, (where, t, c)
                    else:
                        assert np.all(F[c][:, :3] == 0.0), (where, t, c)
                    assert np.all(F[c][:, 3] == 0.0)
        finally:
            if detach:
                detach(g)
            g.close()

        # run 2: no read-back between the steps — the deferred pass is launch A's apply blocks
        g = GpuMetad(abi, **kw)
        r = ref.Metad(**kw)
        try:
            if attach:
                attach(g)
            f = Fused(abi, g, N, dtype, False, cvs)
            for t in range(STEPS):
                f.step(t, d_traj[t], box, n_global=max(N, 1))
            torch.cuda.synchronize()
            F_last = [x.cpu().numpy().astype(np.float64) for x in f.forces]
            for t in range(STEPS):
                b = r.update_bias(t, cv_log[t])
            compare(g, r, b, label="%s deferred" % where)
            assert np.array_equal(g.state()["cv"], cv_log[-1])                   # deterministic: the bits of run 1
            if N:
                opt = util.oracle_postype(traj[-1], types)
                for c, (v, m) in enumerate(cvs):
                    F_ref = ref.lamellar_forces(v, opt, m, rbox, b[c], n_global=N)
                    scale = np.abs(F_ref[:, :3]).max()
                    if scale > 0:
                        assert np.abs(F_last[c][:, :3] - F_ref[:, :3]).max() <= 1e-5 * scale, (where, "deferred", c)
                    else:
                        assert np.all(F_last[c][:, :3] == 0.0), (where, "deferred", c)
        finally:
            if detach:
                detach(g)
            g.close()
    finally:
        abi.check(lib.mtd_lamellar_set_fast_trig(0))


# 1536 particles per force block of the fp32 hardware-trigonometry instantiations with two groups; 2049: one past the first
# group of one CV block (512 threads x 4)
@pytest.mark.parametrize("fast", [1, 0], ids=["hw_trig", "ocml_trig"])
@pytest.mark.parametrize("n_cv", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [0, 1, 63, 1535, 1536, 1537, 2049, 3073])
def test_particle_counts(abi, ref, N, dtype, n_cv, fast):
    """stride 1: every launch B has grid blocks in front of its force blocks, every launch A of the second run apply blocks in
    front of its CV blocks"""
    run_sequence(abi, ref, N, dtype, PARTICLE_GRIDS[n_cv], 1, True, fast)


@pytest.mark.parametrize("fast", [1, 0], ids=["hw_trig", "ocml_trig"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("stride,add_bias", [(1, True), (2, True), (1, False)], ids=["stride1", "stride2", "no_hills"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_grids_and_schedules(abi, ref, grid, stride, add_bias, dtype, fast):
    """stride 2 / no hills: launch B without grid blocks (force block 0 publishes and owns the histogram increment) and launch A
    without apply blocks on alternate / all steps"""
    run_sequence(abi, ref, 1537, dtype, grid, stride, add_bias, fast)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_engine_alone(abi, ref, grid):
    """mtd_metad_update_bias with host-provided values (launch B's kernel with N = 0, every source of the entry block off): with
    a deposit the launch is grid blocks only and grid block 0 publishes, without one it is a single force block without particles"""
    n = GRIDS[grid][0]
    rng = np.random.default_rng(3)
    vals = [[CV_MIN[i] + (0.3 + 0.4 * rng.random()) * (CV_MAX[i] - CV_MIN[i]) for i in range(n)] for _ in range(6)]
    kw = grid_kw(grid, stride=2)
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        for t, v in enumerate(vals):
            g.step(t, v)
            b = r.update_bias(t, v)
            compare(g, r, b, label="engine alone %s step %d" % (grid, t))
        assert g.state()["num_gaussians"] == 3
    finally:
        g.close()
    # and without a read-back in between: the deferred pass of each deposit runs wherever the engine puts it
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        for t, v in enumerate(vals):
            g.step(t, v)
            b = r.update_bias(t, v)
        compare(g, r, b, label="engine alone %s deferred" % grid)
    finally:
        g.close()


def test_sharded_form_single_rank(abi, ref):
    """COMM = true with the rank talking to itself: CV block 0 collects the block sums and sends the totals, launch B's chains
    read them from the mailbox"""
    from metadynamics import xgmi
    lib = abi.load()
    h = C.c_void_p()
    rc = lib.mtd_comm_create(C.byref(h), 0, 1, 8)
    if rc != 0:
        pytest.skip("no one-rank mailbox on this machine (mtd_comm_create: %d)" % rc)
    mbox = xgmi.Mailbox(h, 0, 1)
    attached = []

    def attach(g):
        abi.check(lib.mtd_metad_set_comm(g.h, mbox.handle))
        attached.append(g)

    def detach(g):
        abi.check(lib.mtd_metad_set_comm(g.h, None))

    try:
        run_sequence(abi, ref, 3073, np.float32, "33x31", 1, True, 1, attach=attach, detach=detach)
        assert len(attached) == 2 and mbox.timeouts() == 0
    finally:
        mbox.close()
