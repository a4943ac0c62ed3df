"""GPU parity of the bias step above three collective variables.

A grid with more than CHAIN_MAX_CV = 3 variables leaves the one-wave chain: mtd_metad_update_bias runs the four-launch sequence
(k_prepare, k_reweight1<true, true>, k_apply, k_evaluate), launch A is k_fused_cv<NCV = 4, 5, 6>, launch B is
k_fused_force_general, mtd_fused_step falls back to the two-launch form whatever the particle count, and the host classes run
four or more cv.lamellar through exactly these kernels.  Everything is checked against the oracle with the tolerances of the
<= 3-variable tests: grid arrays through compare() (1e-11, integer arrays bit for bit), CV values to
max(1e-6 |s_ref|, tol_trig n_modes max|a| max(1, max(|h| + |k| + |l|)) / sqrt(N)) with tol_trig = 1e-6 (accurate) / 3e-6 (hardware
trigonometry), forces to 1e-5 of max|F_ref| with w == 0.

Grid ranges are taken PER VARIABLE from the oracle's CV values (min - 0.2, max + 0.3, sigma a quarter of the range): on a common
range the fifth and sixth CV of the set below lie off the grid, V = 0, every bias factor is exactly 0 and every force comparison
passes trivially.  The tests assert that the bias factors they compare are not zero.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from test_gpu_fused import Fused, make_traj
from test_gpu_metad import GpuMetad, compare

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- 1. the grid engine on its own ------------------------------------------------------------------------------------------------
# ragged grids of several 256-cell blocks with a short last one: 840 = 3 x 256 + 72, 576 = 2 x 256 + 64, 2160 = 8 x 256 + 112 cells;
# the 5-variable grid has an axis with the minimum of 2 points (both edge branches of the finite difference apply there, the forward
# one comes first)
GRID_POINTS = {4: [7, 5, 6, 4], 5: [2, 4, 6, 3, 4], 6: [4, 3, 5, 3, 4, 3]}
INTERIOR = [[0.37, 0.52, 0.61, 0.44, 0.58, 0.41], [0.55, 0.40, 0.47, 0.63, 0.36, 0.57], [0.43, 0.58, 0.39, 0.52, 0.49, 0.62],
            [0.61, 0.45, 0.55, 0.38, 0.64, 0.47], [0.48, 0.36, 0.50, 0.57, 0.42, 0.53]]


def grid_kw(n_cv, mode, stride, add_bias=True):
    lo = [-1.0 + 0.3 * i for i in range(n_cv)]
    hi = [l + 1.5 + 0.2 * i for i, l in enumerate(lo)]
    return dict(sigma=[0.3 * (h - l) for l, h in zip(lo, hi)], cv_min=lo, cv_max=hi, num_points=GRID_POINTS[n_cv], W=1.3, T_shift=4.0,
                T=0.8, stride=stride, mode=mode, add_bias=add_bias)


def grid_trajectory(kw):
    """ten deterministic steps: interior points; one within a spacing of the lower edge on axis 0 and of the upper edge on axis 1 at
    once; one exactly on a node; cv_max - 1e-12 on the last axis; off the grid on the last axis only; off the grid on the first axis
    only; back to the interior"""
    lo, hi, pts = np.array(kw["cv_min"]), np.array(kw["cv_max"]), np.array(kw["num_points"])
    n = len(lo)
    d = (hi - lo) / (pts - 1)
    at = lambda k: lo + np.array(INTERIOR[k][:n]) * (hi - lo)
    near = at(0)
    near[0], near[1] = lo[0] + 0.4 * d[0], hi[1] - 0.3 * d[1]
    node = lo + d * np.minimum(np.array([2, 1, 3, 1, 2, 1][:n]), pts - 2)
    top = at(1)
    top[-1] = hi[-1] - 1e-12
    off_last = at(2)
    off_last[-1] = hi[-1] + 0.1 * (hi[-1] - lo[-1])
    off_first = at(3)
    off_first[0] = lo[0] - 0.1 * (hi[0] - lo[0])
    return [at(0), at(1), near, node, top, off_last, off_first, at(2), at(3), at(4)]


def run_grid_pair(abi, ref, kw, trajectory, t0=0, sigma_inv=None):
    """test_gpu_metad.run_pair, also returning the oracle's bias factors of the last step"""
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    b = None
    try:
        if sigma_inv is not None:
            abi.check(g.lib.mtd_metad_set_sigma_inv(g.h, util.dbl_array(sigma_inv.reshape(-1))))
            r.set_sigma_inv(sigma_inv)
            assert g.lib.mtd_metad_sigma_determinant(g.h) == pytest.approx(r.sigma_determinant, rel=1e-14)
        for i, vals in enumerate(trajectory):
            g.step(t0 + i, vals)
            b = r.update_bias(t0 + i, vals)
            compare(g, r, b, label="%d variables step %d" % (g.n_cv, t0 + i))
            if i in (5, 6):
                assert g.state()["oob"] > 0 and r.num_oob_warnings > 0
    finally:
        g.close()
    return r, b


@pytest.mark.parametrize("mode,stride,t0,add_bias", [("standard", 1, 0, True), ("well_tempered", 1, 0, True), ("standard", 3, 1, True),
                                                     ("well_tempered", 3, 1, True), ("well_tempered", 1, 0, False)],
                         ids=["standard", "well_tempered", "standard_stride3", "well_tempered_stride3", "no_hills"])
@pytest.mark.parametrize("n_cv", [4, 5, 6])
def test_grid_engine_four_to_six_variables(abi, ref, n_cv, mode, stride, t0, add_bias):
    """mtd_metad_update_bias above three variables: k_prepare, k_reweight1<true, true>, k_apply, k_evaluate step by step against the
    oracle (6 variables: the size EvalShared is dimensioned for, 14 points x 64 corners)"""
    kw = grid_kw(n_cv, mode, stride, add_bias)
    r, b = run_grid_pair(abi, ref, kw, grid_trajectory(kw), t0)
    if add_bias:                        # (without hills the grid stays zero by definition: the histogram arrays are what is compared)
        assert np.all(b != 0.0), b      # the last step is an interior one
        assert np.abs(r.array("grid")).max() > 0.0
    else:
        assert r.num_gaussians == 0 and r.array("hist_delta").sum() > 0


def test_six_variables_full_sigma_matrix(abi, ref):
    """a full (non-diagonal) inverse-width matrix on the 6-variable grid: 36 element-wise squared entries in every exponent (Q12) and
    the 6 x 6 determinant"""
    kw = grid_kw(6, "well_tempered", 1)
    rng = np.random.default_rng(5)
    sinv = rng.uniform(-0.4, 0.4, (6, 6)) + np.diag([2.0, 1.6, 1.9, 1.4, 1.7, 1.3])         # (not symmetric: entry ij is not entry ji)
    r, b = run_grid_pair(abi, ref, kw, grid_trajectory(kw), sigma_inv=sinv)
    assert np.all(b != 0.0) and np.abs(r.array("grid")).max() > 0.0


# ---- 2. the fused two-launch step through the C ABI --------------------------------------------------------------------------------
CVS6 = [(util.CV1_VECTORS, util.MODE_AB), (util.CV2_VECTORS, util.MODE_AB), ([(0, 0, 3), (1, 2, 0), (2, 0, -1)], [0.5, -1.5]),
        ([(1, 0, 2), (0, 2, 1), (2, 1, 0), (1, 1, 0)], [0.8, -1.2]), ([(0, 0, 0), (0, 1, 1), (1, 0, -1)], [1.0, 0.2]),
        ([(0, 0, 0), (0, 0, 3), (1, 1, 0), (0, 3, 0)], [-1.5, -0.8])]
BOXES = {"cubic": dict(L=20.0), "triclinic": dict(L=[20.0, 22.0, 24.0], xy=0.2, xz=-0.1, yz=0.15)}
N_FUSED, STEPS = 5003, 5
_snapshots = {}


def snapshot(ref, box, dtype, N=N_FUSED, n_global=None, steps=STEPS, cvs=CVS6):
    """make_traj's snapshot (made for L = 20), its oracle form, the oracle's CV values of every step and the grid ranges that follow
    from them — computed once per configuration and shared (read-only) by the tests"""
    key = (box, np.dtype(dtype).name, N, n_global, steps, len(cvs))
    if key not in _snapshots:
        traj, types = make_traj(max(N, 1), 20.0, steps, dtype)
        traj, types = [p[:N] for p in traj], types[:N]
        kw = {k: v for k, v in BOXES[box].items() if k != "L"}
        rbox = ref.Box.make(BOXES[box]["L"], **kw)
        opts = [util.oracle_postype(p, types) for p in traj]
        ng = n_global or max(N, 1)
        s = np.array([[ref.lamellar_cv(v, o, m, rbox, n_global=ng) for v, m in cvs] for o in opts])
        lo, hi = s.min(axis=0) - 0.2, s.max(axis=0) + 0.3
        _snapshots[key] = dict(traj=traj, types=types, opts=opts, rbox=rbox, s=s, lo=lo, hi=hi, n_global=ng)
    return _snapshots[key]


def fused_kw(snap, n_cv, stride=2, mode="well_tempered", add_bias=True):
    lo, hi = snap["lo"][:n_cv], snap["hi"][:n_cv]
    return dict(sigma=list(0.25 * (hi - lo)), cv_min=list(lo), cv_max=list(hi), num_points=[5, 4, 6, 4, 3, 4][:n_cv], W=1.0, T_shift=7.0, T=1.0,
                stride=stride, mode=mode, add_bias=add_bias)


def cv_tolerance(cv, s_ref, N, fast):
    vecs, coeff = cv
    index = max(sum(abs(x) for x in hkl) for hkl in vecs)
    floor = (3e-6 if fast else 1e-6) * len(vecs) * max(abs(a) for a in coeff) * max(1, index) / np.sqrt(max(N, 1))
    return max(1e-6 * abs(s_ref), floor)


def check_forces(ref, cvs, snap, t, b, F, N, expect_bias=True):
    for c, (v, m) in enumerate(cvs):
        if N == 0:
            continue
        F_ref = ref.lamellar_forces(v, snap["opts"][t], m, snap["rbox"], b[c], n_global=snap["n_global"])
        scale = np.abs(F_ref[:, :3]).max()
        if expect_bias:
            assert scale > 0.0, (t, c)
        if scale > 0.0:
            assert np.abs(F[c][:, :3] - F_ref[:, :3]).max() <= 1e-5 * scale, (t, c, np.abs(F[c][:, :3] - F_ref[:, :3]).max() / scale)
        else:
            assert np.all(F[c][:, :3] == 0.0), (t, c)
        assert np.all(F[c][:, 3] == 0.0), (t, c)


def run_fused(abi, ref, n_cv, dtype, box, fast, N=N_FUSED, n_global=None, kw_change=None, expect_bias=True, second_run=True, **kw_args):
    """STEPS steps of mtd_fused_cv_pass + mtd_fused_force_pass with a read-back after every step (CV values, every grid array and
    scalar, the forces of every CV against the oracle), then the same steps without any read-back: the final state against the oracle,
    the CV values bit for bit those of the first run.  Returns the last state, the oracle and its last bias factors."""
    lib = abi.load()
    cvs = CVS6[:n_cv]
    snap = snapshot(ref, box, dtype, N, n_global)
    kw = fused_kw(snap, n_cv, **kw_args)
    if kw_change:
        kw_change(kw)
    abox = abi.Box.make(BOXES[box]["L"], **{k: v for k, v in BOXES[box].items() if k != "L"})
    d_traj = [torch.from_numpy(util.pack_postype(p, snap["types"], dtype)).cuda() if N else torch.zeros((1, 4), device="cuda") for p in snap["traj"]]
    lib.mtd_lamellar_set_fast_trig(int(fast))
    g, r = GpuMetad(abi, **kw), ref.Metad(**kw)
    cv_log = []
    try:
        f = Fused(abi, g, N, dtype, cvs=cvs)
        for t in range(STEPS):
            f.step(t, d_traj[t], abox, n_global=snap["n_global"])
            torch.cuda.synchronize()
            F = [x.cpu().numpy().astype(np.float64) for x in f.forces]      # formed from the closed-form bias, before any flush
            st = g.state()
            for c in range(n_cv):
                s_ref = snap["s"][t][c]
                assert abs(st["cv"][c] - s_ref) <= cv_tolerance(cvs[c], s_ref, N, fast), (t, c, st["cv"][c], s_ref)
            cv_log.append(st["cv"].copy())
            b = r.update_bias(t, st["cv"])
            compare(g, r, b, label="%d CVs %s step %d" % (n_cv, box, t))
            check_forces(ref, cvs, snap, t, b, F, N, expect_bias)
    finally:
        g.close()
    if second_run:
        g2, r2 = GpuMetad(abi, **kw), ref.Metad(**kw)
        try:
            f = Fused(abi, g2, N, dtype, cvs=cvs)
            for t in range(STEPS):
                f.step(t, d_traj[t], abox, n_global=snap["n_global"])
            for t in range(STEPS):
                b2 = r2.update_bias(t, cv_log[t])
            compare(g2, r2, b2, label="%d CVs %s deferred" % (n_cv, box))
            assert np.array_equal(g2.state()["cv"], cv_log[-1])
        finally:
            g2.close()
    lib.mtd_lamellar_set_fast_trig(0)
    return st, r, b


@pytest.mark.parametrize("fast", [1, 0], ids=["hw_trig", "accurate_trig"])
@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_cv", [4, 5, 6])
def test_fused_step_four_to_six_cvs(abi, ref, n_cv, dtype, box, fast):
    """every k_fused_cv<S4, NCV = 4 | 5 | 6, FAST, false, ORTHO> with k_fused_force_general<S4, FAST> behind it: deposit and
    non-deposit launches alternate (stride 2), well-tempered"""
    st, r, b = run_fused(abi, ref, n_cv, dtype, box, fast)
    assert np.all(b != 0.0), b
    assert st["oob"] == 0 and r.num_oob_warnings == 0


@pytest.mark.parametrize("N", [0, 1, 777])
def test_fused_step_six_cvs_small_counts(abi, ref, N):
    """a deposit launch without a force block and a non-deposit launch of one block (N = 0), one particle, one partial row (777);
    n_global = max(N, 1)"""
    st, r, b = run_fused(abi, ref, 6, np.float32, "cubic", 0, N=N, expect_bias=False)
    assert st["oob"] == 0
    if N:
        assert np.all(b != 0.0), b


@pytest.mark.parametrize("case", ["n_global", "no_hills", "standard"])
def test_fused_step_six_cvs_variants(abi, ref, case):
    if case == "n_global":              # a shard of a four times larger system
        st, r, b = run_fused(abi, ref, 6, np.float32, "cubic", 0, n_global=4 * N_FUSED)
    elif case == "no_hills":
        st, r, b = run_fused(abi, ref, 6, np.float32, "cubic", 0, add_bias=False, expect_bias=False)
        assert np.all(b == 0.0) and r.num_gaussians == 0 and r.array("hist_delta").sum() == STEPS
    else:
        st, r, b = run_fused(abi, ref, 6, np.float32, "cubic", 0, mode="standard")
    assert st["oob"] == 0
    if case != "no_hills":
        assert np.all(b != 0.0), b


def test_fused_step_six_cvs_last_one_off_the_grid(abi, ref):
    """the sixth CV above its cv_max from the first step on: the reference's warning path (V = 0, :677-683), every force exactly zero"""
    def lower_the_top(kw):
        kw["cv_min"][5] -= 1.0
        kw["cv_max"][5] = kw["cv_min"][5] + 0.5          # (the CV's values lie 0.2 above the old cv_min and higher)
    st, r, b = run_fused(abi, ref, 6, np.float32, "cubic", 0, kw_change=lower_the_top, expect_bias=False)
    assert np.all(b == 0.0) and r.curr_bias == 0.0
    assert st["oob"] > 0 and r.num_oob_warnings > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fused_step_entry_point_takes_two_launches_above_three_cvs(abi, ref, dtype):
    """mtd_fused_step with the one-launch form switched on and 4 CVs: two launches (the persistent kernel exists for the chain's
    <= 3 variables), forces and CV values bit for bit those of mtd_fused_cv_pass + mtd_fused_force_pass on an identical engine"""
    lib = abi.load()
    cvs = CVS6[:4]
    snap = snapshot(ref, "cubic", dtype)
    kw = fused_kw(snap, 4)
    abox = abi.Box.make(20.0)
    ga, gb = GpuMetad(abi, **kw), GpuMetad(abi, **kw)
    try:
        fa, fb = Fused(abi, ga, N_FUSED, dtype, cvs=cvs), Fused(abi, gb, N_FUSED, dtype, cvs=cvs)
        abi.check(lib.mtd_fused_step_set_mode(ga.h, 1))
        for t in range(STEPS):
            d_pos = torch.from_numpy(util.pack_postype(snap["traj"][t], snap["types"], dtype)).cuda()
            abi.check(lib.mtd_fused_step(ga.h, C.byref(fa.lset), N_FUSED, abi.ptr(d_pos), fa.fptr, fa.dt, N_FUSED, C.byref(abox),
                                         abi.ptr(fa.scratch), t, None))
            assert lib.mtd_fused_step_launches(ga.h) == 2
            fb.step(t, d_pos, abox)
            torch.cuda.synchronize()
            for c in range(4):
                A, B = fa.forces[c].cpu().numpy(), fb.forces[c].cpu().numpy()
                assert np.abs(B[:, :3]).max() > 0 and np.array_equal(A, B), (t, c)
            sa, sb = ga.state(), gb.state()
            assert np.array_equal(sa["cv"], sb["cv"]) and np.array_equal(sa["bias"], sb["bias"]) and sa["V"] == sb["V"]
            assert np.all(sa["bias"] != 0.0) and sa["oob"] == 0
        for name in abi.ARRAY_NAMES:
            assert np.array_equal(ga.array(name), gb.array(name)), name
    finally:
        ga.close()
        gb.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_slot_map_through_the_general_kernel(abi, ref, dtype):
    """mtd_fused_force_pass_slots on a 5-variable grid: the three lamellar CVs of the set are variables 4, 0 and 2, variables 1 and 3
    are host scalars that move every step — against mtd_metad_update_bias + mtd_lamellar_forces on an identical engine (2e-6 of
    max|B|, as on the 3-variable grid of test_fused_force_pass_with_slot_map)"""
    lib = abi.load()
    cvs = CVS6[:3]
    snap = snapshot(ref, "cubic", dtype)
    N = N_FUSED
    slots = (4, 0, 2)
    lo, hi = [0.0] * 5, [0.0] * 5
    for c, s in enumerate(slots):
        lo[s], hi[s] = snap["lo"][c], snap["hi"][c]
    lo[1], hi[1], lo[3], hi[3] = -2.0, 2.0, 0.5, 3.5
    kw = dict(sigma=[0.25 * (h - l) for l, h in zip(lo, hi)], cv_min=lo, cv_max=hi, num_points=[4, 5, 3, 6, 4], W=1.0, T_shift=7.0, T=1.0,
              stride=1, mode="well_tempered")
    abox = abi.Box.make(20.0)
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    lset = abi.LamellarSet.make(cvs)
    ga, gb = GpuMetad(abi, **kw), GpuMetad(abi, **kw)
    scratch = torch.zeros(lib.mtd_lamellar_scratch_doubles(N), dtype=torch.float64, device="cuda")
    fa = [torch.zeros((N, 4), dtype=tdt, device="cuda") for _ in cvs]
    fb = [torch.zeros((N, 4), dtype=tdt, device="cuda") for _ in cvs]
    pa, pb = (C.c_void_p * 3)(*[f.data_ptr() for f in fa]), (C.c_void_p * 3)(*[f.data_ptr() for f in fb])
    try:
        for t in range(4):
            d_pos = torch.from_numpy(util.pack_postype(snap["traj"][t], snap["types"], dtype)).cuda()
            n_part = C.c_uint()
            abi.check(lib.mtd_lamellar_cv_partials(C.byref(lset), N, d_pos.data_ptr(), dt, C.byref(abox), scratch.data_ptr(), C.byref(n_part), None))
            for g in (ga, gb):
                abi.check(lib.mtd_metad_set_cv_value(g.h, 1, 0.4 * t - 0.7))
                abi.check(lib.mtd_metad_set_cv_value(g.h, 3, 2.2 - 0.3 * t))
                for c, s in enumerate(slots):
                    abi.check(lib.mtd_metad_set_cv_source(g.h, s, scratch.data_ptr(), n_part.value, 3, c, 1.0 / N, 0.0))
            abi.check(lib.mtd_fused_force_pass_slots(ga.h, C.byref(lset), (C.c_uint * 3)(*slots), N, d_pos.data_ptr(), pa, dt, N, C.byref(abox), t, None))
            abi.check(lib.mtd_metad_update_bias(gb.h, t, None))
            d_bias = lib.mtd_metad_bias_device(gb.h)
            for c, s in enumerate(slots):
                one = abi.LamellarSet.make([cvs[c]])
                abi.check(lib.mtd_lamellar_forces(C.byref(one), N, d_pos.data_ptr(), (C.c_void_p * 1)(fb[c].data_ptr()), dt, N, d_bias + 8 * s,
                                                  C.byref(abox), None))
            torch.cuda.synchronize()
            for c in range(3):
                A, B = fa[c].cpu().numpy().astype(np.float64), fb[c].cpu().numpy().astype(np.float64)
                assert np.abs(B).max() > 0
                assert np.abs(A - B).max() <= 2e-6 * np.abs(B).max(), (t, c)
        sa, sb = ga.state(), gb.state()
        assert np.array_equal(sa["cv"], sb["cv"])
        assert np.allclose(sa["bias"], sb["bias"], rtol=1e-9, atol=1e-12) and sa["V"] == pytest.approx(sb["V"], rel=1e-12)
        assert np.all(sb["bias"] != 0.0) and sa["oob"] == 0
        assert lib.mtd_fused_force_pass_slots(ga.h, C.byref(lset), (C.c_uint * 3)(5, 0, 2), N, d_pos.data_ptr(), pa, dt, N, C.byref(abox), 9, None) == -1
    finally:
        ga.close()
        gb.close()


def test_refusals_above_the_grid_engine_s_six_variables(abi, ref):
    """a 7-CV set in mtd_fused_cv_pass (the grid engine holds 6 variables): MTD_ERR_UNSUPPORTED; a set whose CV count is not the
    grid's in mtd_fused_force_pass: MTD_ERR_UNSUPPORTED"""
    lib = abi.load()
    N = 100
    kw = grid_kw(6, "well_tempered", 1)
    g = GpuMetad(abi, **kw)
    try:
        seven = abi.LamellarSet.make(CVS6 + [([(1, 0, 0)], [1.0, -1.0])])
        five = abi.LamellarSet.make(CVS6[:5])
        abox = abi.Box.make(20.0)
        d_pos = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
        scratch = torch.zeros(lib.mtd_lamellar_scratch_doubles(N), dtype=torch.float64, device="cuda")
        forces = [torch.zeros((N, 4), dtype=torch.float32, device="cuda") for _ in range(7)]
        fptr = (C.c_void_p * 7)(*[f.data_ptr() for f in forces])
        n_part = C.c_uint()
        assert lib.mtd_fused_cv_pass(g.h, C.byref(seven), N, d_pos.data_ptr(), abi.MTD_F32, C.byref(abox), scratch.data_ptr(), C.byref(n_part), None) == -2
        assert lib.mtd_fused_force_pass(g.h, C.byref(seven), N, d_pos.data_ptr(), fptr, abi.MTD_F32, N, C.byref(abox), 0, None) == -2
        assert lib.mtd_fused_force_pass(g.h, C.byref(five), N, d_pos.data_ptr(), fptr, abi.MTD_F32, N, C.byref(abox), 0, None) == -2
        abi.check(lib.mtd_fused_step_set_mode(g.h, 1))
        assert lib.mtd_fused_step(g.h, C.byref(five), N, d_pos.data_ptr(), fptr, abi.MTD_F32, N, C.byref(abox), scratch.data_ptr(), 0, None) == -2
        torch.cuda.synchronize()
        assert g.state()["num_gaussians"] == 0 and not g.array("grid").any()       # nothing ran
    finally:
        g.close()


# ---- 3. the general forms under the randomised campaigns ---------------------------------------------------------------------------
@pytest.mark.parametrize("tool,seconds,seed,env", [("fuzz_fused.py", 8, 202, "MTD_FUSED_GENERAL"), ("fuzz_slots.py", 6, 205, "MTD_FUSED_GENERAL"),
                                                   ("fuzz_grid.py", 6, 201, "MTD_METAD_FOUR_LAUNCHES")])
def test_randomised_campaign_in_the_general_forms(tool, seconds, seed, env):
    """tools/fuzz_fused.py and tools/fuzz_slots.py with k_fused_force_general as launch B of every case (MTD_FUSED_GENERAL, read once
    per process: each campaign is a fresh child), tools/fuzz_grid.py with the four-launch sequence on <= 3 variables too
    (MTD_METAD_FOUR_LAUNCHES) — the tools' own tolerances"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), str(seconds), str(seed)], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **{env: "1"}))
    assert r.returncode == 0, "%s failed:\n%s\n%s" % (tool, r.stdout[-3000:], r.stderr[-3000:])
    last = [l for l in r.stdout.splitlines() if l.startswith("fuzz_")]
    assert last and "random" in last[-1], r.stdout[-1000:]


# ---- 5. the host classes ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _dumped_grid(meta, stem):
    import glob
    meta.dump_grid(stem)
    files = glob.glob(stem + "_*")
    assert len(files) == 1, files
    return np.loadtxt(files[0], skiprows=4)


def _oracle_grid(r, stem, n_cv):
    r.write_grid(stem, 0, ["cv%d" % c for c in range(n_cv)])
    return np.loadtxt(stem + "_0", skiprows=4)


def _host_run(api, ref, tmp_path, kinds, fused, tag):
    """six steps (stride 2: the deposits of time steps 0, 2, 4, 6) of integrate.mode_metadynamics over cv.lamellar (CVS6, in order) and
    cv.density variables on a static modulated snapshot; grid ranges per variable from the oracle's values"""
    context, cv, integrate = api
    N, L, steps = 20011, 30.0, 6
    pos, types = util.snapshot_random(N, L, seed=8, modulated=True, dtype=np.float32)
    rbox = ref.Box.make(L)
    opt = util.oracle_postype(pos, types)
    lam_sets = [CVS6[i] for i in range(sum(k == "lam" for k in kinds))]
    s_ref, which, i = [], [], 0
    for k in kinds:
        if k == "lam":
            v, m = lam_sets[i]
            s_ref.append(ref.lamellar_cv(v, opt, m, rbox))
            which.append(i)
            i += 1
        else:
            s_ref.append(ref.density(rbox, N))
            which.append(None)
    kw = dict(sigma=[0.125] * len(kinds), cv_min=[s - 0.2 for s in s_ref], cv_max=[s + 0.3 for s in s_ref], num_points=[6, 5, 4, 5][:len(kinds)],
              W=0.5, T_shift=5.0, T=1.0, stride=2, mode="well_tempered")
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float32)
    meta = integrate.mode_metadynamics(dt=0.005, stride=2, mode="well_tempered", W=0.5, deltaT=5.0, T=1.0)
    variables = []
    for c, k in enumerate(kinds):
        if k == "lam":
            v, m = lam_sets[which[c]]
            x = cv.lamellar(sigma=kw["sigma"][c], mode=dict(A=m[0], B=m[1]), lattice_vectors=v, name="v%d" % c)
        else:
            x = cv.density(sigma=kw["sigma"][c])
        x.set_grid(kw["cv_min"][c], kw["cv_max"][c], kw["num_points"][c])
        variables.append(x)
    if fused is not None:
        meta.cpp_integrator.setFusedPath(fused)
    context.run(steps)
    integ = meta.cpp_integrator
    out = dict(used=integ.usedFusedPath(), cv=np.array(integ.getCurrentValues()), bias=np.array(integ.getBiasFactors()), n=integ.getNumGaussians(),
               F=[x.cpp_force.getForces().astype(np.float64) if k == "lam" else None for x, k in zip(variables, kinds)],
               grid=_dumped_grid(meta, str(tmp_path / ("grid_" + tag))))
    context.current = None
    # the oracle, driven with the device's CV values (the particles do not move: the same values in every step)
    r = ref.Metad(**kw)
    for t in range(steps + 1):                  # prepRun(0) + the updates of time steps 1 ... 6
        b = r.update_bias(t, out["cv"])
    return out, dict(r=r, b=b, s=s_ref, opt=opt, rbox=rbox, lam=lam_sets, which=which, N=N)


def _check_host_run(ref, out, o, kinds, tmp_path, tag):
    r, b = o["r"], o["b"]
    assert out["n"] == r.num_gaussians == 4
    for c, k in enumerate(kinds):
        if k == "lam":
            assert abs(out["cv"][c] - o["s"][c]) <= cv_tolerance(o["lam"][o["which"][c]], o["s"][c], o["N"], False), (c, out["cv"][c], o["s"][c])
        else:
            assert out["cv"][c] == pytest.approx(o["s"][c], rel=1e-12)
    assert np.all(b != 0.0), b
    assert np.allclose(out["bias"], b, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(r.array("grid")).max())), (out["bias"], b)
    want = _oracle_grid(r, str(tmp_path / ("oracle_" + tag)), len(kinds))
    assert out["grid"].shape == want.shape == (r.len, len(kinds) + 6)
    assert np.allclose(out["grid"], want, rtol=1e-9, atol=1e-12)
    assert want[:, len(kinds)].max() > 0
    for c, k in enumerate(kinds):
        if k != "lam":
            continue
        v, m = o["lam"][o["which"][c]]
        F_ref = ref.lamellar_forces(v, o["opt"], m, o["rbox"], b[c])
        scale = np.abs(F_ref[:, :3]).max()
        assert scale > 0
        assert np.abs(out["F"][c][:, :3] - F_ref[:, :3]).max() <= 1e-5 * scale, (c, np.abs(out["F"][c][:, :3] - F_ref[:, :3]).max() / scale)
        assert np.all(out["F"][c][:, 3] == 0.0)


def test_four_lamellar_cvs_through_the_host_classes(api, ref, tmp_path):
    """four cv.lamellar on one grid: planStep() takes the fused step for them (up to 6), the step is k_fused_cv<..., 4, ...> +
    k_fused_force_general; the same run with setFusedPath(False) (every CV its own kernels, the four-launch grid sequence) leaves the same
    grid; CV values, bias factors, the dumped grid and the forces of the last step against the oracle's 4-variable engine"""
    kinds = ["lam"] * 4
    fused, o = _host_run(api, ref, tmp_path, kinds, True, "fused")
    assert fused["used"]
    _check_host_run(ref, fused, o, kinds, tmp_path, "fused")
    plain, o2 = _host_run(api, ref, tmp_path, kinds, False, "plain")
    assert not plain["used"]
    _check_host_run(ref, plain, o2, kinds, tmp_path, "plain")
    assert np.allclose(fused["grid"], plain["grid"], rtol=1e-9, atol=1e-14)


def test_three_lamellar_cvs_and_a_density_through_the_host_classes(api, ref, tmp_path):
    """a mixed 4-variable set: planStep() shares lamellar launches in sets of at most three variables, so every CV runs its own kernels and the grid the
    four-launch sequence — against the oracle driven with the device's CV values"""
    kinds = ["lam", "density", "lam", "lam"]
    out, o = _host_run(api, ref, tmp_path, kinds, None, "mixed")
    assert not out["used"]
    _check_host_run(ref, out, o, kinds, tmp_path, "mixed")
