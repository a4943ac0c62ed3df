"""GPU parity of the lamellar kernels at the capacity of a CV set: MTD_MAX_CV = 8 CVs, MTD_MAX_MODES = 64 modes, MTD_MAX_TYPES = 16
particle types.

k_lamellar_cv_partials<NCV = 4 ... 8> (partial rows n_cv wide), the one-load-per-thread table staging of launch A (64 modes, 128
coefficients), the corder[] / nact[] bookkeeping of folded second harmonics, s_coeff[c * 16 + type] up to c = 7, type = 15, and the
force kernels' mode loops over all 64 modes are checked against the oracle: CV values to
max(1e-6 |s_ref|, tol_trig n_modes max|a| max(1, max(|h| + |k| + |l|)) / sqrt(N)), tol_trig = 1e-6 (accurate) / 3e-6 (hardware), forces to
1e-5 of max|F_ref| with w == 0.  The Miller indices stay at |h| + |k| + |l| <= 6 (BASELINE.json's configs): the fp32 phase carries its
rounding that many times.
"""
import ctypes as C

import numpy as np
import pytest

import util
from test_gpu_fused import Fused
from test_gpu_lamellar import gpu_forces
from test_gpu_metad import GpuMetad, compare

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LS, TILT = (11.0, 13.5, 9.25), dict(xy=0.3, xz=-0.2, yz=0.15)
N_FULL = 3001
BIAS = [0.8, -1.7, 0.5, 1.1, -0.6, 2.0, -1.3, 0.9]
TRIG_HARDWARE, TRIG_ACCURATE = 1, 2


def _modes_and_coefficients():
    """64 distinct Miller triples in eight blocks of eight: five fundamentals with 0 < |h| + |k| + |l| <= 3 (at least one odd component)
    and the second harmonics of three of them, in a fixed random order inside the block — harmonics in front of, behind and between
    their fundamentals, 24 folds in all when a CV holds whole blocks —, and 8 x 16 mode coefficients.  The snapshot's density wave lies
    along (0, 0, 1): that mode leads the list, so the first CV of every set has a value."""
    rng = np.random.default_rng(64)
    fund = [(h, k, l) for h in range(-3, 4) for k in range(-3, 4) for l in range(-3, 4)
            if 0 < abs(h) + abs(k) + abs(l) <= 3 and (h % 2 or k % 2 or l % 2) and (h, k, l) != (0, 0, 1)]
    pick = [(0, 0, 1)] + [fund[i] for i in rng.permutation(len(fund))[:39]]
    modes = []
    for c in range(8):
        blk = pick[5 * c:5 * c + 5]
        blk = blk + [tuple(2 * x for x in m) for m in blk[:3]]
        rest = [blk[i] for i in (rng.permutation(7) + 1)]
        modes += [blk[0]] + rest
    assert len(set(modes)) == 64 and modes[0] == (0, 0, 1)
    coeff = rng.uniform(0.3, 1.5, (8, 16))
    coeff[:, 1::2] *= -1.0                              # sign by type parity, as the modulation
    return modes, [[float(x) for x in row] for row in coeff]


MODES, COEFF = _modes_and_coefficients()


def split(counts):
    """CVs of the given mode counts, cut from the 64 modes in order"""
    assert sum(counts) <= 64 and len(counts) <= 8
    first = np.concatenate([[0], np.cumsum(counts)])
    return [(MODES[first[c]:first[c + 1]], COEFF[c]) for c in range(len(counts))]


SETS = {"8x8": split([8] * 8), "1x64": split([64]), "8x1": split([1] * 8)}
for _n in range(4, 9):
    SETS["odd%d" % _n] = split([2 * c + 1 for c in range(_n)])      # 1, 3, 5, ... modes: n_cv = 8 totals 64

_snap = {}


def snapshot(abi, ref, N, dtype, steps=1):
    """N particles of 16 types (every type present at N = 3001; type 15 is the first and the last particle) in a triclinic box, with a
    density wave along the third lattice direction whose sign follows the type's parity; made once per (N, dtype), read-only"""
    key = (N, np.dtype(dtype).name, steps)
    if key not in _snap:
        rng = np.random.default_rng(77)
        f0 = rng.random((N_FULL, 3))[:N]
        types = rng.integers(0, 16, N_FULL).astype(np.int32)[:N]
        types[0] = types[-1] = 15
        if N == N_FULL:
            assert len(set(types.tolist())) == 16
        a1 = np.array([LS[0], 0, 0])
        a2 = np.array([TILT["xy"] * LS[1], LS[1], 0])
        a3 = np.array([TILT["xz"] * LS[2], TILT["yz"] * LS[2], LS[2]])
        traj = []
        for t in range(steps):
            f = f0.copy()
            f[:, 2] += 0.04 * (t + 1) * np.where(types % 2 == 0, 1.0, -1.0) * np.sin(2 * np.pi * f[:, 2])
            traj.append((-0.5 * np.array(LS) + f[:, :1] * a1 + f[:, 1:2] * a2 + f[:, 2:3] * a3).astype(dtype))
        _snap[key] = dict(traj=traj, types=types, opts=[util.oracle_postype(p, types) for p in traj],
                          packed=[util.pack_postype(p, types, dtype) for p in traj], box=abi.Box.make(LS, **TILT), rbox=ref.Box.make(LS, **TILT))
    return _snap[key]


def cv_tolerance(cv, s_ref, N, hardware):
    vecs, coeff = cv
    index = max(sum(abs(x) for x in hkl) for hkl in vecs)
    floor = (3e-6 if hardware else 1e-6) * len(vecs) * max(abs(a) for a in coeff) * max(1, index) / np.sqrt(N)
    return max(1e-6 * abs(s_ref), floor)


def gpu_cv(abi, cvs, postype_np, box, trig_mode, n_rows_check=True):
    """mtd_lamellar_cv_partials + mtd_reduce_partials with the set's own trigonometry mode; the partial rows are n_cv wide"""
    lib = abi.load()
    N = postype_np.shape[0]
    dt = abi.MTD_F32 if postype_np.dtype == np.float32 else abi.MTD_F64
    d_pos = torch.from_numpy(postype_np).cuda()
    lset = abi.LamellarSet.make(cvs, trig_mode=trig_mode)
    scratch = torch.full((lib.mtd_lamellar_scratch_doubles(N),), np.nan, dtype=torch.float64, device="cuda")
    n_part = C.c_uint(0)
    abi.check(lib.mtd_lamellar_cv_partials(C.byref(lset), N, abi.ptr(d_pos), dt, C.byref(box), abi.ptr(scratch), C.byref(n_part), None))
    out = torch.zeros(len(cvs), dtype=torch.float64, device="cuda")
    abi.check(lib.mtd_reduce_partials(abi.ptr(scratch), n_part.value, len(cvs), len(cvs), 1.0 / N, 0.0, abi.ptr(out), None))
    torch.cuda.synchronize()
    if n_rows_check:                    # exactly n_partials rows of n_cv sums were written, nothing behind them
        used = n_part.value * len(cvs)
        head = scratch[:used + 8].cpu().numpy()
        assert np.isfinite(head[:used]).all() and np.isnan(head[used:]).all()
    return out.cpu().numpy()


def check_set(abi, ref, cvs, N, dtype, fast):
    snap = snapshot(abi, ref, N, dtype)
    opt, packed = snap["opts"][0], snap["packed"][0]
    s = gpu_cv(abi, cvs, packed, snap["box"], TRIG_HARDWARE if fast else TRIG_ACCURATE)
    F = gpu_forces(abi, cvs, packed, snap["box"], BIAS[:len(cvs)], fast=bool(fast))
    for c, (v, m) in enumerate(cvs):
        s_ref = ref.lamellar_cv(v, opt, m, snap["rbox"])
        assert abs(s[c] - s_ref) <= cv_tolerance(cvs[c], s_ref, N, fast), (c, s[c], s_ref)
        F_ref = ref.lamellar_forces(v, opt, m, snap["rbox"], BIAS[c])
        scale = np.abs(F_ref[:, :3]).max()
        assert scale > 0
        assert np.abs(F[c][:, :3] - F_ref[:, :3]).max() <= 1e-5 * scale, (c, np.abs(F[c][:, :3] - F_ref[:, :3]).max() / scale)
        assert np.all(F[c][:, 3] == 0.0)
    return s


@pytest.mark.parametrize("fast", [1, 0], ids=["hw_trig", "accurate_trig"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(SETS))
def test_sets_at_capacity(abi, ref, name, dtype, fast):
    """8 CVs x 8 modes, one CV of 64 modes, 4 ... 8 CVs of 1, 3, 5, ... modes (every width of a partial row), 8 CVs x 1 mode; 16 types"""
    s = check_set(abi, ref, SETS[name], N_FULL, dtype, fast)
    assert abs(s[0]) > 0.01              # the first CV holds the modulation's harmonics: a value, not a cancellation


@pytest.mark.parametrize("fast", [1, 0], ids=["hw_trig", "accurate_trig"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [1, 63])
@pytest.mark.parametrize("name", ["8x8", "odd8"])
def test_sets_at_capacity_few_particles(abi, ref, name, N, dtype, fast):
    """one particle (of type 15) and less than a wave"""
    check_set(abi, ref, SETS[name], N, dtype, fast)


FOLD_CHAINS = {
    "ascending": [(0, 0, 1), (0, 0, 2), (0, 0, 4)],
    "descending": [(0, 0, 4), (0, 0, 2), (0, 0, 1)],
    "middle_first": [(0, 0, 2), (0, 0, 1), (0, 0, 4)],
    "duplicate": [(0, 0, 1), (0, 0, 1), (0, 0, 2)],
    "chain_with_duplicate": [(1, -1, 2), (2, -2, 4), (4, -4, 8), (2, -2, 4)],
    "with_zero": [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 0)],
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(FOLD_CHAINS))
def test_fold_chains_of_harmonics(abi, ref, name, dtype):
    """h, 2h, 4h inside one CV: the CV pass folds a second harmonic into its fundamental ONE level deep (cos 2x = 2 cos^2 x - 1), every
    mode at most once, whatever the order — the value is the oracle's plain sum over all modes, in the hardware trigonometry
    (3e-6) and in the accurate one (1e-6), and the two agree to the hardware tolerance.  A second CV behind the chain shows that the
    bookkeeping of the first leaves the next one's modes where they belong."""
    snap = snapshot(abi, ref, N_FULL, dtype)
    cvs = [(FOLD_CHAINS[name], COEFF[0]), (MODES[3:8], COEFF[1])]
    s_hw = gpu_cv(abi, cvs, snap["packed"][0], snap["box"], TRIG_HARDWARE)
    s_acc = gpu_cv(abi, cvs, snap["packed"][0], snap["box"], TRIG_ACCURATE)
    for c, (v, m) in enumerate(cvs):
        s_ref = ref.lamellar_cv(v, snap["opts"][0], m, snap["rbox"])
        assert abs(s_hw[c] - s_ref) <= cv_tolerance(cvs[c], s_ref, N_FULL, True), (c, s_hw[c], s_ref)
        assert abs(s_acc[c] - s_ref) <= cv_tolerance(cvs[c], s_ref, N_FULL, False), (c, s_acc[c], s_ref)
        assert abs(s_hw[c] - s_acc[c]) <= cv_tolerance(cvs[c], s_ref, N_FULL, True), (c, s_hw[c], s_acc[c])
    assert abs(s_acc[0]) > 0.005


@pytest.mark.parametrize("fast", [1, 0], ids=["hw_trig", "accurate_trig"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fused_step_at_capacity(abi, ref, dtype, fast):
    """the fused two-launch step with as much as the grid engine and a set hold together: 6 CVs of 11, 11, 11, 11, 10, 10 = 64 modes, 16
    types; grid ranges per CV from the oracle's values; three steps (deposit, none, deposit) against the oracle"""
    lib = abi.load()
    steps = 3
    cvs = split([11, 11, 11, 11, 10, 10])
    snap = snapshot(abi, ref, N_FULL, dtype, steps)
    s_all = np.array([[ref.lamellar_cv(v, o, m, snap["rbox"]) for v, m in cvs] for o in snap["opts"]])
    lo, hi = s_all.min(axis=0) - 0.2, s_all.max(axis=0) + 0.3
    kw = dict(sigma=list(0.25 * (hi - lo)), cv_min=list(lo), cv_max=list(hi), num_points=[3, 4, 3, 4, 3, 3], W=1.0, T_shift=7.0, T=1.0, stride=2,
              mode="well_tempered")
    lib.mtd_lamellar_set_fast_trig(int(fast))
    g, r = GpuMetad(abi, **kw), ref.Metad(**kw)
    try:
        f = Fused(abi, g, N_FULL, dtype, cvs=cvs)
        for t in range(steps):
            d_pos = torch.from_numpy(snap["packed"][t]).cuda()
            f.step(t, d_pos, snap["box"])
            torch.cuda.synchronize()
            F = [x.cpu().numpy().astype(np.float64) for x in f.forces]
            st = g.state()
            for c in range(6):
                assert abs(st["cv"][c] - s_all[t][c]) <= cv_tolerance(cvs[c], s_all[t][c], N_FULL, fast), (t, c, st["cv"][c], s_all[t][c])
            b = r.update_bias(t, st["cv"])
            compare(g, r, b, label="capacity step %d" % t)
            assert np.all(b != 0.0) and st["oob"] == 0, (t, b)
            for c, (v, m) in enumerate(cvs):
                F_ref = ref.lamellar_forces(v, snap["opts"][t], m, snap["rbox"], b[c])
                scale = np.abs(F_ref[:, :3]).max()
                assert scale > 0
                assert np.abs(F[c][:, :3] - F_ref[:, :3]).max() <= 1e-5 * scale, (t, c, np.abs(F[c][:, :3] - F_ref[:, :3]).max() / scale)
                assert np.all(F[c][:, 3] == 0.0)
    finally:
        lib.mtd_lamellar_set_fast_trig(0)
        g.close()


def test_sets_beyond_capacity_are_refused(abi, ref):
    """n_cv = 9, n_modes = 65, n_types = 17 written into the struct: MTD_ERR_INVALID_ARGUMENT from mtd_lamellar_cv_partials and from
    mtd_fused_step, before anything is launched"""
    lib = abi.load()
    N = 64
    snap = snapshot(abi, ref, N_FULL, np.float32)
    d_pos = torch.from_numpy(snap["packed"][0][:N].copy()).cuda()
    scratch = torch.full((lib.mtd_lamellar_scratch_doubles(N),), np.nan, dtype=torch.float64, device="cuda")
    forces = [torch.zeros((N, 4), dtype=torch.float32, device="cuda") for _ in range(8)]
    fptr = (C.c_void_p * 8)(*[f.data_ptr() for f in forces])
    g = GpuMetad(abi, sigma=[0.1] * 6, cv_min=[-1.0] * 6, cv_max=[1.0] * 6, num_points=[3] * 6, W=1.0, T_shift=7.0, T=1.0, stride=1,
                 mode="well_tempered")
    try:
        for field, value in (("n_cv", 9), ("n_modes", 65), ("n_types", 17)):
            lset = abi.LamellarSet.make(SETS["8x8"])
            setattr(lset, field, value)
            n_part = C.c_uint(0)
            assert lib.mtd_lamellar_cv_partials(C.byref(lset), N, d_pos.data_ptr(), abi.MTD_F32, C.byref(snap["box"]), scratch.data_ptr(),
                                                C.byref(n_part), None) == -1, field
            assert lib.mtd_fused_step(g.h, C.byref(lset), N, d_pos.data_ptr(), fptr, abi.MTD_F32, N, C.byref(snap["box"]), scratch.data_ptr(), 0,
                                      None) == -1, field
        torch.cuda.synchronize()
        assert np.isnan(scratch[:64].cpu().numpy()).all() and g.state()["num_gaussians"] == 0
    finally:
        g.close()
