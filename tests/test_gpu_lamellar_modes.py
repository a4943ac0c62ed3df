"""GPU parity of the fused two-launch step over mode sets and boxes.

Both launches project positions with 3 products when the box has no tilt (LamKArgs::ortho) and with the general 3 x 3 product
otherwise.  Orthorhombic and triclinic boxes, every zero pattern of the Miller indices, sets with and without folded second
harmonics, one to three CVs, particle counts that are not a multiple of the per-thread group and smaller than a wave, fp32 /
fp64 particles and both trigonometry modes are checked against the oracle: CV values to 1e-6, forces to 1e-5 of max|F|.
"""
import numpy as np
import pytest

import util
from test_gpu_fused import Fused
from test_gpu_metad import GpuMetad

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

# every zero pattern of (h, k, l), each with and without its second harmonic in the same CV
ALL_PATTERNS = [(1, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0),
                (1, 1, 0), (2, 2, 0), (0, 1, -2), (1, 0, 1), (2, 0, 2), (1, -1, 2), (2, -2, 4), (-1, 2, 1)]
NO_FOLD = [(1, 2, 3), (0, 2, 1), (3, 0, 0), (0, 0, 5), (2, -1, 0)]
ONLY_FOLD = [(0, 0, 1), (0, 0, 2), (1, 1, 1), (2, 2, 2)]
MODE_SETS = {
    "config2": [(util.CV1_VECTORS, util.MODE_AB), (util.CV2_VECTORS, util.MODE_AB)],
    "patterns": [(ALL_PATTERNS, util.MODE_AB)],
    "mixed3": [(NO_FOLD, util.MODE_AB), (ONLY_FOLD, [0.5, -1.5]), (ALL_PATTERNS, [-1.0, 0.25])],
    "nofold2": [(NO_FOLD, util.MODE_AB), (util.CV1_VECTORS, [1.0, 0.5])],
}
BOXES = {
    "ortho": dict(L=[30.0, 34.0, 38.0]),
    "triclinic": dict(L=[30.0, 34.0, 38.0], xy=0.2, xz=-0.1, yz=0.15),
}


def run_case(abi, ref, cvs, box_kw, N, dtype, fast):
    lib = abi.load()
    rng = np.random.default_rng(N + 7 * len(cvs))
    L = np.array(box_kw["L"])
    pos = (rng.random((N, 3)) * L - L / 2).astype(dtype)
    types = (np.arange(N) % 2).astype(np.int32)
    extra = {k: v for k, v in box_kw.items() if k != "L"}
    box, rbox = abi.Box.make(box_kw["L"], **extra), ref.Box.make(box_kw["L"], **extra)
    n_cv = len(cvs)
    kw = dict(sigma=[0.02] * n_cv, cv_min=[-0.5] * n_cv, cv_max=[0.5] * n_cv, num_points=[32] * n_cv, W=1.0, T_shift=7.0,
              T=1.0, stride=1, mode="well_tempered")
    lib.mtd_lamellar_set_fast_trig(fast)
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        f = Fused(abi, g, N, dtype, cvs=cvs)
        d_pos = torch.from_numpy(util.pack_postype(pos, types, dtype)).cuda()
        opt = util.oracle_postype(pos, types)
        s_ref = [ref.lamellar_cv(v, opt, m, rbox) for v, m in cvs]
        for t in range(2):
            f.step(t, d_pos, box)
            torch.cuda.synchronize()
            F = [x.cpu().numpy().astype(np.float64) for x in f.forces]
            st = g.state()
            for c, (v, _) in enumerate(cvs):
                tol = max(1e-6 * abs(s_ref[c]), 1e-6 * len(v) / np.sqrt(N))
                assert abs(st["cv"][c] - s_ref[c]) <= tol, (t, c, st["cv"][c], s_ref[c])
            b = r.update_bias(t, st["cv"])
            for c, (v, m) in enumerate(cvs):
                F_ref = ref.lamellar_forces(v, opt, m, rbox, b[c])
                scale = np.abs(F_ref[:, :3]).max()
                if scale > 0:
                    assert np.abs(F[c][:, :3] - F_ref[:, :3]).max() <= 1e-5 * scale, (t, c)
                else:                       # (a CV value off the grid: no bias force)
                    assert np.all(F[c][:, :3] == 0.0), (t, c)
                assert np.all(F[c][:, 3] == 0.0)
    finally:
        lib.mtd_lamellar_set_fast_trig(0)
        g.close()


@pytest.mark.parametrize("fast", [1, 0], ids=["hw_trig", "accurate_trig"])
@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("modes", list(MODE_SETS))
def test_mode_sets_and_boxes(abi, ref, modes, box, fast):
    run_case(abi, ref, MODE_SETS[modes], BOXES[box], 20011, np.float32, fast)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("N", [1, 37, 1001])
def test_small_and_ragged_counts(abi, ref, N, box, dtype):
    run_case(abi, ref, MODE_SETS["mixed3"], BOXES[box], N, dtype, 1)


@pytest.mark.parametrize("fast", [1, 0], ids=["hw_trig", "accurate_trig"])
@pytest.mark.parametrize("box", list(BOXES))
def test_f64_particles(abi, ref, box, fast):
    run_case(abi, ref, MODE_SETS["config2"], BOXES[box], 30011, np.float64, fast)
