"""GPU parity on chosen paths: the bias grid's cached patch (MetadState::patch_v) — hits, misses, edges, host writes.

Every bias step with at most three variables reads its stencil from a 6^n-cell patch of the bias grid around the previous
step's values and loads from the grid only where a lane's cell lies outside it.  The paths of tests/grid_paths.py choose, cell
by cell, which of the two a step takes (tests/test_grid_paths.py shows on the oracle that a stale patch on their `hit` steps is
an error of >= 1e-6 against the 1e-9 compared here).  The patch is tested through results only: every array, V, w, the bias
factors and the Gaussian count against the oracle (test_gpu_metad.compare), forces at the 1e-5 of test_gpu_fused.
"""

import numpy as np
import pytest

import grid_paths
import util
from test_gpu_fused import Fused
from test_gpu_metad import GpuMetad, compare

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def device_rows(abi, g, rows_bias, rows_cv, t):
    """row t of the two [steps, n_cv] tensors <- the engine's bias factors / CV values, copied by a kernel (no read-back)"""
    n = g.n_cv
    abi.check(g.lib.mtd_reduce_partials(g.lib.mtd_metad_bias_device(g.h), 1, n, n, 1.0, 0.0, rows_bias.data_ptr() + 8 * n * t, None))
    abi.check(g.lib.mtd_reduce_partials(g.lib.mtd_metad_cv_device(g.h), 1, n, n, 1.0, 0.0, rows_cv.data_ptr() + 8 * n * t, None))


def assert_chain_bias(chain_bias, bias_ref, r, label):
    """the bias factors as the step's own launch left them (copied out by a kernel BEFORE any read-back: mtd_metad_get_state
    behind a deposit evaluates them again on the final grid and overwrites them, with other roundings, so compare() alone never
    sees what the chain — and with it the patch — produced) against the oracle's, at compare()'s tolerance for bias factors"""
    atol = 1e-9 * max(1.0, np.abs(r.array("grid")).max())
    assert np.allclose(chain_bias, bias_ref, rtol=1e-9, atol=atol), (label, "chain bias", list(chain_bias), list(bias_ref))


def check_step(abi, g, r, bias_ref, label):
    """compare() plus the chain's own bias factors, fetched ahead of compare()'s read-back"""
    row_b = torch.zeros((1, g.n_cv), dtype=torch.float64, device="cuda")
    row_s = torch.zeros((1, g.n_cv), dtype=torch.float64, device="cuda")
    device_rows(abi, g, row_b, row_s, 0)
    chain_bias = row_b.cpu().numpy()[0]
    compare(g, r, bias_ref, label=label)
    assert_chain_bias(chain_bias, bias_ref, r, label)


def first_difference(rows, log, labels, what):
    """one message naming the first step (and its label) at which two runs differ"""
    for t, (a, b) in enumerate(zip(rows, log)):
        if not np.array_equal(a, b):
            return "%s differ first at step %d (%s): %r against %r" % (what, t, labels[t], list(a), list(b))
    return None


# ------------------------------------------------------------------------------------------------ a. the engine alone

@pytest.mark.parametrize("stride,mode", [(1, "well_tempered"), (3, "well_tempered"), (1, "standard")])
@pytest.mark.parametrize("n_cv", [1, 2, 3])
def test_engine_on_cell_paths(abi, ref, n_cv, stride, mode):
    """mtd_metad_set_cv_value + mtd_metad_update_bias along the whole path.  Run 1 compares everything after every step; run 2
    reads nothing back between the steps (bias factors and CV values leave through mtd_reduce_partials) and must reproduce
    run 1 bit for bit."""
    kw = grid_paths.settings(n_cv, stride, mode)
    traj = grid_paths.values(grid_paths.path(n_cv), n_cv)
    labels = [label for _, label in traj]
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        rows_b = torch.zeros((len(traj), n_cv), dtype=torch.float64, device="cuda")
        rows_s = torch.zeros((len(traj), n_cv), dtype=torch.float64, device="cuda")
        for t, (v, label) in enumerate(traj):
            where = "run 1 step %d (%s)" % (t, label)
            g.step(t, v)
            device_rows(abi, g, rows_b, rows_s, t)
            b = r.update_bias(t, v)
            compare(g, r, b, label=where)
            assert_chain_bias(rows_b[t].cpu().numpy(), b, r, where)
            assert np.array_equal(g.state()["cv"], v), where
        bias_log = rows_b.cpu().numpy()
    finally:
        g.close()

    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        rows_b = torch.zeros((len(traj), n_cv), dtype=torch.float64, device="cuda")
        rows_s = torch.zeros((len(traj), n_cv), dtype=torch.float64, device="cuda")
        for t, (v, _) in enumerate(traj):
            g.step(t, v)
            device_rows(abi, g, rows_b, rows_s, t)
        torch.cuda.synchronize()
        assert g.lib.mtd_metad_cv_device(g.h) and g.lib.mtd_metad_cv_device(g.h) != g.lib.mtd_metad_bias_device(g.h)
        bad = first_difference(rows_s.cpu().numpy(), [v for v, _ in traj], labels, "CV values of run 2 and the values set")
        assert bad is None, bad
        bad = first_difference(rows_b.cpu().numpy(), bias_log, labels, "bias factors of run 2 and run 1")
        assert bad is None, bad
        for t, (v, _) in enumerate(traj):
            b = r.update_bias(t, v)
        compare(g, r, b, label="run 2")
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ b. the particle step

# CV c of the set is the single lattice vector e_c with mode coefficient 1; every particle has type 0 and sits at
# x_c = L / (2 pi) acos(s_c), so that s_c = cos(2 pi x_c / L) is the path's value
PARTICLE_CVS = [([(1, 0, 0)], [1.0]), ([(0, 1, 0)], [1.0]), ([(0, 0, 1)], [1.0])]
SCHEDULES = {"two_launches": (2,), "one_launch": (1,), "alternating": (2, 2, 1, 2, 1, 1, 2, 2)}
N_PARTICLES, BOX_L = 257, 10.0                          # one block plus one particle


def particle_snapshots(n_cv, dtype):
    """[(cell, label, positions[N, 3] in dtype)] of the path on the particle grid.  float32 drops the two exact-edge
    steps (fractions 0.0 and 0.999); in float64 the s == cv_min step sits 1e-9 of its angle inside the grid, because
    cos(acos(cv_min)) may round to either side of cv_min."""
    g = grid_paths.grid(n_cv, particle=True)
    out = []
    for cell, frac, label in grid_paths.path(n_cv, particle=True):
        if dtype == np.float32 and frac in (0.0, 0.999):
            continue
        s = np.array(grid_paths.value(g, cell, frac))
        assert np.all(np.abs(s) <= 1.0), s
        theta = np.arccos(s)
        if frac == 0.0:
            theta *= 1.0 - 1e-9
        pos = np.zeros((N_PARTICLES, 3))
        pos[:, :n_cv] = BOX_L / (2 * np.pi) * theta
        out.append((cell, label, pos.astype(dtype)))
    return out


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_cv", [1, 2, 3])
def test_particle_step_on_cell_paths(abi, ref, n_cv, dtype, schedule):
    """the same paths through mtd_fused_cv_pass + mtd_fused_force_pass (the deferred pass rides in launch A, the preload
    includes the partial sums), through mtd_fused_step's one-launch kernel (chain_prefetch) and alternating on one engine
    (the one-launch step invalidates the patch: the next two-launch step loads from the grid, the one after hits again)"""
    kw = grid_paths.settings(n_cv, 1, "well_tempered", particle=True)
    grid = grid_paths.grid(n_cv, particle=True)
    cvs = PARTICLE_CVS[:n_cv]
    snaps = particle_snapshots(n_cv, dtype)
    labels = [label for _, label, _ in snaps]
    types = np.zeros(N_PARTICLES, dtype=np.int32)
    box, rbox = abi.Box.make(BOX_L), ref.Box.make(BOX_L)
    pattern = SCHEDULES[schedule]
    d_traj = [torch.from_numpy(util.pack_postype(pos, types, dtype)).cuda() for _, _, pos in snaps]

    # run 1: everything against the oracle after every step (the read-back runs the deferred pass on its own)
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    cv_log = []
    try:
        f = Fused(abi, g, N_PARTICLES, dtype, False, cvs)
        rows_b = torch.zeros((len(snaps), n_cv), dtype=torch.float64, device="cuda")
        rows_s = torch.zeros((len(snaps), n_cv), dtype=torch.float64, device="cuda")
        for t, (cell, label, pos) in enumerate(snaps):
            where = "%s step %d (%s)" % (schedule, t, label)
            f.one_launch = pattern[t % len(pattern)] == 1
            f.step(t, d_traj[t], box)
            device_rows(abi, g, rows_b, rows_s, t)
            torch.cuda.synchronize()
            F = [x.cpu().numpy().astype(np.float64) for x in f.forces]
            st = g.state()
            assert grid_paths.cell_of(grid, st["cv"]) == cell, (where, st["cv"])
            cv_log.append(st["cv"].copy())
            b = r.update_bias(t, st["cv"])                      # oracle grid driven with the device's CV values
            compare(g, r, b, label=where)
            assert_chain_bias(rows_b[t].cpu().numpy(), b, r, where)
            assert np.array_equal(rows_s[t].cpu().numpy(), st["cv"]), where
            opt = util.oracle_postype(pos, types)
            for c, (v, m) in enumerate(cvs):
                F_ref = ref.lamellar_forces(v, opt, m, rbox, b[c])
                scale = np.abs(F_ref[:, :3]).max()
                if scale > 0:
                    assert np.abs(F[c][:, :3] - F_ref[:, :3]).max() <= 1e-5 * scale, (where, c)
                else:
                    assert np.all(F[c][:, :3] == 0.0), (where, c)
                assert np.all(F[c][:, 3] == 0.0)
        bias_log = rows_b.cpu().numpy()
    finally:
        g.close()

    # run 2: no read-back between the steps
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        f = Fused(abi, g, N_PARTICLES, dtype, False, cvs)
        rows_b = torch.zeros((len(snaps), n_cv), dtype=torch.float64, device="cuda")
        rows_s = torch.zeros((len(snaps), n_cv), dtype=torch.float64, device="cuda")
        for t in range(len(snaps)):
            f.one_launch = pattern[t % len(pattern)] == 1
            f.step(t, d_traj[t], box)
            device_rows(abi, g, rows_b, rows_s, t)
        torch.cuda.synchronize()
        bad = first_difference(rows_s.cpu().numpy(), cv_log, labels, "%s: CV values of run 2 and run 1" % schedule)
        assert bad is None, bad
        bad = first_difference(rows_b.cpu().numpy(), bias_log, labels, "%s: bias factors of run 2 and run 1" % schedule)
        assert bad is None, bad
        for t in range(len(snaps)):
            b = r.update_bias(t, cv_log[t])
        compare(g, r, b, label="%s run 2" % schedule)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ c. host writes

WARM = 11            # the loop's first step (nothing cached yet) and ten `hit` steps: the patch is valid and centred on c0
AFTER = 8


def walk_values(n_cv, count, start=0):
    return grid_paths.values(grid_paths.hit_walk(n_cv, count, start=start), n_cv)


def linear_index(num_points, cell):
    idx, factor = 0, 1
    for c, n in zip(cell, num_points):                   # variable 0 runs fastest (IndexGrid)
        idx += c * factor
        factor *= n
    return idx


def continue_and_compare(abi, g, r, n_cv, what):
    for k, (v, label) in enumerate(walk_values(n_cv, AFTER, start=WARM)):
        g.step(WARM + k, v)
        b = r.update_bias(WARM + k, v)
        check_step(abi, g, r, b, "%s: step %d after the write (%s)" % (what, k, label))


@pytest.mark.parametrize("n_cv", [2, 3])
def test_set_array_into_warm_patch(abi, ref, n_cv):
    """mtd_metad_set_array(h, 0, ...): the current grid plus a smooth bump of height 5 over the 4^n cells around c0"""
    kw = grid_paths.settings(n_cv)
    n, c0 = kw["num_points"], grid_paths.centre(n_cv)
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        for t, (v, _) in enumerate(walk_values(n_cv, WARM)):
            g.step(t, v)
            b = r.update_bias(t, v)
        compare(g, r, b, label="warm")
        bump = np.zeros(g.len)
        shape = {-1: 0.5, 0: 1.0, 1: 1.0, 2: 0.5}
        for off in np.ndindex(*([4] * n_cv)):
            cell = [c + o - 1 for c, o in zip(c0, off)]
            assert ref.index_get(n, cell) == linear_index(n, cell)
            bump[linear_index(n, cell)] = 5.0 * np.prod([shape[o - 1] for o in off])
        new = g.array("grid") + bump
        abi.check(g.lib.mtd_metad_set_array(g.h, 0, new.ctypes.data, None))
        r.array("grid")[:] += bump
        assert np.array_equal(g.array("grid"), new)
        continue_and_compare(abi, g, r, n_cv, "set_array")
    finally:
        g.close()


@pytest.mark.parametrize("pending", [False, True], ids=["nothing_pending", "deferred_pass_pending"])
@pytest.mark.parametrize("n_cv", [2, 3])
def test_device_write_and_grid_touched(abi, ref, n_cv, pending):
    """a write through the pointer of mtd_metad_device_array(h, 0), on the stream, followed by mtd_metad_grid_touched.  The
    pointer is fetched before the first step, so that nothing but mtd_metad_grid_touched tells the engine of the write.  The
    write adds a constant to a few cells next to c0 (grid -> temporary -> grid through mtd_reduce_partials: out = shift + in);
    an addition commutes with a pending `grid += dV`, so the oracle receives the same addition."""
    kw = grid_paths.settings(n_cv)
    n, c0 = kw["num_points"], grid_paths.centre(n_cv)
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        lib = g.lib
        d_grid = lib.mtd_metad_device_array(g.h, 0)
        assert d_grid
        for t, (v, _) in enumerate(walk_values(n_cv, WARM)):
            g.step(t, v)
            b = r.update_bias(t, v)
        if not pending:
            compare(g, r, b, label="warm")               # the read-back ran the deferred pass
        cells = [c0, tuple(c + (1 if i == 0 else 0) for i, c in enumerate(c0)),
                 tuple(c + (1 if i == n_cv - 1 else 0) for i, c in enumerate(c0)), tuple(c - 1 for c in c0)]
        tmp = torch.zeros(1, dtype=torch.float64, device="cuda")
        for k, cell in enumerate(cells):
            idx = linear_index(n, cell)
            shift = 0.75 + 0.5 * k
            abi.check(lib.mtd_reduce_partials(d_grid + 8 * idx, 1, 1, 1, 1.0, shift, tmp.data_ptr(), None))
            abi.check(lib.mtd_reduce_partials(tmp.data_ptr(), 1, 1, 1, 1.0, 0.0, d_grid + 8 * idx, None))
            r.array("grid")[idx] += shift
        abi.check(lib.mtd_metad_grid_touched(g.h, None))
        continue_and_compare(abi, g, r, n_cv, "device write, %s" % ("deferred pass pending" if pending else "nothing pending"))
    finally:
        g.close()


@pytest.mark.parametrize("n_cv", [2, 3])
def test_transplant_into_warm_patch(abi, ref, n_cv):
    """engine A walks in the low corner, engine B around c0; then all ten arrays and the Gaussian count go from A into B, which
    continues around c0 — its own warm region, where A's grid differs.  The oracle that follows is A's, holding the arrays B
    received."""
    kw = grid_paths.settings(n_cv)
    ga, gb = GpuMetad(abi, **kw), GpuMetad(abi, **kw)
    ra = ref.Metad(**kw)
    try:
        grid = grid_paths.grid(n_cv)
        corner = [((0,) * n_cv, 0.6), ((1,) * n_cv, 0.37), ((0,) * n_cv, 0.05), ((1,) * n_cv, 0.61), ((0,) * n_cv, 0.37),
                  ((1,) * n_cv, 0.61), ((0,) * n_cv, 0.37)]
        for t, (cell, frac) in enumerate(corner):
            v = grid_paths.value(grid, cell, frac)
            ga.step(t, v)
            b = ra.update_bias(t, v)
        compare(ga, ra, b, label="engine A")
        for t, (v, _) in enumerate(walk_values(n_cv, WARM)):
            gb.step(t, v)
        assert gb.state()["num_gaussians"] == WARM != len(corner)
        assert np.abs(gb.array("grid") - ga.array("grid")).max() > 0.1
        for which, name in enumerate(abi.ARRAY_NAMES):
            arr = ga.array(name)
            abi.check(gb.lib.mtd_metad_set_array(gb.h, which, arr.ctypes.data, None))
            ra.array(name)[:] = arr
        abi.check(gb.lib.mtd_metad_set_num_gaussians(gb.h, ga.state()["num_gaussians"], None))
        continue_and_compare(abi, gb, ra, n_cv, "transplant")
    finally:
        ga.close()
        gb.close()


# ------------------------------------------------------------------------------------------------ d. setters mid-run

def run_with_events(abi, ref, kw, count, before=None, between=None):
    """`count` steps of the two-variable loop with check_step() after every one.  before[t](g, r) runs ahead of step t;
    between[t](g, r) runs right behind step t's launch, ahead of its read-back (a deposit of that step is still pending)."""
    before, between = before or {}, between or {}
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        for t, (v, label) in enumerate(walk_values(2, count)):
            if t in before:
                before[t](g, r)
            g.step(t, v)
            b = r.update_bias(t, v)
            if t in between:
                between[t](g, r)
            check_step(abi, g, r, b, "step %d (%s)" % (t, label))
    finally:
        g.close()


def test_set_stride_mid_run(abi, ref):
    def to(s):
        def f(g, r):
            abi.check(g.lib.mtd_metad_set_stride(g.h, s))
            r.set_stride(s)
        return f
    run_with_events(abi, ref, grid_paths.settings(2), 22, before={6: to(3), 15: to(2)})


def test_set_add_hills_mid_run(abi, ref):
    def to(on):
        def f(g, r):
            abi.check(g.lib.mtd_metad_set_add_hills(g.h, on))
            r.set_add_bias(on)
        return f
    run_with_events(abi, ref, grid_paths.settings(2), 17, before={6: to(0), 11: to(1)})


def test_set_mode_mid_run(abi, ref):
    def to(mode):
        def f(g, r):
            abi.check(g.lib.mtd_metad_set_mode(g.h, {"standard": 0, "well_tempered": 1}[mode]))
            r.set_mode(mode)
        return f
    run_with_events(abi, ref, grid_paths.settings(2), 18, before={6: to("standard"), 12: to("well_tempered")})


def test_reset_histogram_mid_run(abi, ref):
    """stride 3: once right behind the deposit of step 6 (its deferred pass pending) and once between the steps 10 and 11,
    neither of which deposits"""
    def reset(g, r):
        abi.check(g.lib.mtd_metad_reset_histogram(g.h, None))
        r.reset_histogram()
    run_with_events(abi, ref, grid_paths.settings(2, stride=3), 14, before={11: reset}, between={6: reset})


def test_walker_sequence_mid_run(abi, ref):
    """three steps through mtd_metad_update_bias_walkers(h, NULL, t) — phase A / phase B, four launches, which never say where
    the next patch should sit — between steps of mtd_metad_update_bias"""
    kw = grid_paths.settings(2)
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        for t, (v, label) in enumerate(walk_values(2, 14)):
            if 5 <= t < 8:
                for c, x in enumerate(v):
                    abi.check(g.lib.mtd_metad_set_cv_value(g.h, c, float(x)))
                abi.check(g.lib.mtd_metad_update_bias_walkers(g.h, None, t, None))
            else:
                g.step(t, v)
            b = r.update_bias(t, v)
            check_step(abi, g, r, b, "step %d (%s)%s" % (t, label, " through the walker sequence" if 5 <= t < 8 else ""))
    finally:
        g.close()
