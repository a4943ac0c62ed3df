"""CPU: the `frame` argument of the five Steinhardt restatements (ql_local_ref, ql_local_avg_ref, ql_local_bonds_ref,
ql_local_virial_ref, ql_virial_ref) is checked before tests/test_gpu_ql_axis.py holds the kernels against it.

The restatements write the gradient in spherical components and divide by sin(theta): in the lab frame a bond on the z axis of the box
gives NaN, and next to the axis the quotient loses its digits.  Every variable is rotation invariant, so the same restatement in a
rotated frame (pair vectors d @ Q.T, gradients back with G @ Q) is a reference without a pole on those bonds.  Checked here:
    off the axis (each file's usual noisy snapshot)   frame = Q equals frame = None to 1e-12 of the largest entry, every output
    on the axis (util.columns: bcc_columns, sc_columns)
        frame = None contains NaN (why the frame exists); two unrelated frames agree to 1e-12;
        the gradient of six particles (frame Q1) meets central differences (h = 1e-6) of the value to 1e-5 of the largest gradient
        entry — the value taken in the OTHER frame Q2: in the lab frame it is finite on the axis, but its theta comes from arccos, and
        a bond moved 1e-6 off the axis has lost half its digits there (for the global variable: ql_virial_ref.value, held to the
        oracle's value below); the summed virial meets the strain derivative with the bound the file of that restatement uses.
Nothing here needs a GPU."""
import numpy as np
import pytest

import ql_local_avg_ref as avg_ref
import ql_local_bonds_ref as bonds_ref
import ql_local_ref as loc_ref
import ql_local_virial_ref as lvir_ref
import ql_virial_ref as gvir_ref
import util

BIAS = 0.9
QL_46 = [0, 0, 0, 0, 1, 0, 1]
E6 = [0, 0, 0, 0, 0, 0, 1]
Q1, Q2 = util.random_rotation(1), util.random_rotation(2)


def _global(ref, case, frame, half=False):
    """the global variable: the oracle's lab-frame Q_lm, the restatement's forces and virial in `frame`; grad = ds/dr from the force sums
    (the pass keeps the central terms only: F = -1/2 bias ds/dr, see tests/test_ql_virial_ref.py)"""
    s, Qlm = gvir_ref.oracle_cv(ref, **case, half=half)
    out = gvir_ref.compute(**case, Qlm=Qlm, bias=BIAS, half=half, frame=frame)
    return dict(s=s, fp=out["fp"], virial=out["virial"], W=out["W"], grad=-2.0 / BIAS * out["F"])


# name: (run(ref, case, frame) -> dict of outputs, value(ref, case) -> s in the lab frame, off-axis case, degrees and options)
def _off_local():
    return loc_ref.issue_case()


def _off_fcc108():
    pos, L = util.fcc_lattice(3)
    pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
    return dict(pos=pos, types=np.zeros(len(pos), dtype=np.int32), L=L, nl=util.build_nlist(pos, L, 1.55), r_cut=1.4, r_on=1.2, lmax=6,
                type_id=0, Ql_ref=QL_46)


AVG_OPT = dict(average=True, switch=(0.5, 3), gate=(4, 8))         # c_i is 0.26 on bcc, 0.37 on fcc, 0.71 on sc: no switch saturated
BONDS_OPT = dict(bonds=(0.5, 0.7), switch=(6.5, 6))
LVIR_OPT = dict(average=True, switch=(0.5, 3))

RESTATEMENTS = {
    "ql_local_ref": dict(
        run=lambda ref, case, frame: loc_ref.compute(**case, frame=frame),
        value=lambda ref, case: loc_ref.compute(**case, gradient=False, frame=Q2)["s"],
        off=_off_local, degrees=QL_46),
    "ql_local_avg_ref": dict(
        run=lambda ref, case, frame: avg_ref.compute(**case, **AVG_OPT, frame=frame),
        value=lambda ref, case: avg_ref.compute(**case, **AVG_OPT, gradient=False, frame=Q2)["s"],
        off=_off_local, degrees=QL_46),
    "ql_local_bonds_ref": dict(
        run=lambda ref, case, frame: bonds_ref.compute(**case, **BONDS_OPT, bias=BIAS, frame=frame),
        value=lambda ref, case: bonds_ref.compute(**case, **BONDS_OPT, gradient=False, frame=Q2)["s"],
        strain=lambda ref, case: (-BIAS * bonds_ref.strain_derivative(**case, eps=1e-6, **BONDS_OPT, frame=Q2), 1e-8),
        off=lambda: {**_off_local(), "Ql_ref": E6}, degrees=E6),
    "ql_local_virial_ref": dict(
        run=lambda ref, case, frame: lvir_ref.compute(**case, bias=BIAS, **LVIR_OPT, frame=frame),
        value=lambda ref, case: avg_ref.compute(**case, **LVIR_OPT, gradient=False, frame=Q2)["s"],
        strain=lambda ref, case: (-BIAS * lvir_ref.strain_derivative(**case, eps=1e-6, **LVIR_OPT, frame=Q2), 1e-8),
        off=_off_fcc108, degrees=QL_46),
    "ql_virial_ref": dict(
        run=_global,
        value=lambda ref, case: gvir_ref.value(**case, frame=Q2),
        strain=lambda ref, case: (-0.5 * BIAS * gvir_ref.strain_derivative(ref, **case, eps=1e-6, frame=Q2), 4.7e-8),
        off=_off_fcc108, degrees=QL_46),
}
NAMES = sorted(RESTATEMENTS)
ARRAYS = ("s", "c", "n", "v", "b", "dent", "grad", "virial", "W", "tensor", "fp")

_cache = {}


def on_axis(ref, name, snap, frame_id):
    """(case, n_on, outputs) computed once and left unchanged; frame_id 0: None, 1 / 2: Q1 / Q2"""
    key = (name, snap, frame_id)
    if key not in _cache:
        case, n_on = util.columns(snap)
        case = dict(case, lmax=6, Ql_ref=RESTATEMENTS[name]["degrees"])
        with np.errstate(all="ignore"):
            _cache[key] = (case, n_on, RESTATEMENTS[name]["run"](ref, case, (None, Q1, Q2)[frame_id]))
    return _cache[key]


def largest_difference(a, b, name):
    """largest difference of every output the two runs share, relative to that output's largest entry"""
    worst = 0.0
    seen = []
    for k in ARRAYS:
        if a.get(k) is None:
            continue
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        assert np.isfinite(x).all() and np.isfinite(y).all(), (name, k)
        top = np.abs(x).max()
        err = np.abs(x - y).max() / top if top > 0 else np.abs(y).max()
        print("%s %-7s largest difference %.3e of %.4g" % (name, k, err, top))
        worst = max(worst, err)
        seen.append(k)
    assert "s" in seen and ("grad" in seen)
    return worst


def test_rotation_is_proper_and_frames_differ():
    for q in (Q1, Q2):
        assert np.abs(q @ q.T - np.eye(3)).max() < 1e-14 and np.linalg.det(q) == pytest.approx(1.0, abs=1e-14)
        assert np.abs(q[2]).max() < 0.95                                 # the box's z axis is no axis of the frame
    assert np.abs(Q1 - Q2).max() > 0.3


@pytest.mark.parametrize("lmax", [4, 6, 12])
def test_rotate_qlm_is_the_table_of_the_rotated_vectors(lmax):
    """Q'_lm = sum w Y_lm(Q d) formed directly against rotate_qlm of sum w Y_lm(d)"""
    from scipy.special import sph_harm_y
    rng = np.random.default_rng(5)
    d = rng.normal(size=(40, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    w = rng.uniform(0.1, 1, 40)

    def table(u):
        t, p = np.arccos(u[:, 2]), np.arctan2(u[:, 1], u[:, 0])
        out = np.zeros((lmax + 1) ** 2, dtype=np.complex128)
        for l in range(lmax + 1):
            for m in range(-l, l + 1):
                out[gvir_ref.qlm_index(l, m)] = (w * sph_harm_y(l, m, t, p)).sum()
        return out

    got, want = gvir_ref.rotate_qlm(table(d), lmax, Q1), table(d @ Q1.T)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", NAMES)
def test_off_the_axis_the_frame_changes_nothing(ref, name):
    R = RESTATEMENTS[name]
    case = R["off"]()
    a, b = R["run"](ref, case, None), R["run"](ref, case, Q1)
    assert largest_difference(a, b, name) <= 1e-12


@pytest.mark.parametrize("snap", sorted(util.COLUMNS))
@pytest.mark.parametrize("name", NAMES)
def test_on_the_axis_the_lab_frame_is_nan_and_two_frames_agree(ref, name, snap):
    case, n_on, lab = on_axis(ref, name, snap, 0)
    print("%s on %s: %d of %d entries on the axis" % (name, snap, n_on, len(case["nl"][2])))
    assert np.isnan(lab["grad"]).any()                                   # why the frame exists
    assert np.isfinite(lab["s"])                                         # the value has no pole
    a, b = on_axis(ref, name, snap, 1)[2], on_axis(ref, name, snap, 2)[2]
    assert np.abs(a["grad"]).max() > 0                                   # the noise broke the inversion symmetry
    assert largest_difference(a, b, name) <= 1e-12
    assert a["s"] == pytest.approx(lab["s"], rel=1e-13)
    assert RESTATEMENTS[name]["value"](ref, case) == pytest.approx(lab["s"], rel=1e-13)   # the value the differences below use


@pytest.mark.parametrize("snap", sorted(util.COLUMNS))
@pytest.mark.parametrize("name", NAMES)
def test_on_the_axis_the_gradient_meets_central_differences(ref, name, snap):
    case, n_on, out = on_axis(ref, name, snap, 1)
    value = RESTATEMENTS[name]["value"]
    N = len(case["pos"])
    picked = np.random.default_rng(6).choice(N, 6, replace=False)
    h = 1e-6
    fd = np.zeros((6, 3))
    for a, k in enumerate(picked):
        for c in range(3):
            s = []
            for sign in (1.0, -1.0):
                p = case["pos"].copy()
                p[k, c] += sign * h
                s.append(value(ref, dict(case, pos=p)))
            fd[a, c] = (s[0] - s[1]) / (2 * h)
    top = np.abs(out["grad"]).max()
    err = np.abs(out["grad"][picked] - fd).max() / top
    print("%s on %s: gradient of particles %s against central differences: %.3e of max|grad| %.4g" % (name, snap, picked, err, top))
    assert np.abs(fd).max() > 0.05 * top
    assert err <= 1e-5


@pytest.mark.parametrize("snap", sorted(util.COLUMNS))
@pytest.mark.parametrize("name", [n for n in NAMES if "strain" in RESTATEMENTS[n]])
def test_on_the_axis_the_summed_virial_meets_the_strain_derivative(ref, name, snap):
    case, n_on, out = on_axis(ref, name, snap, 1)
    fd, bound = RESTATEMENTS[name]["strain"](ref, case)
    W = out["W"]
    top = np.abs(W).max()
    err = np.abs(fd - W).max()
    print("%s on %s: W = %s\n  strain derivative %s\n  largest difference %.3e of max|W| %.4g" % (name, snap, W, fd, err / top, top))
    assert top > 0
    assert err <= bound * top


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("snap", sorted(util.COLUMNS))
def test_near_axis_snapshots_span_the_range(snap, dtype):
    """near_axis: a quarter of the columns exactly on the axis, the other bonds inside columns from the smallest offset the storage
    holds up to 1e-2; both frames agree there as well (the plain local variable)"""
    case, n_on = util.near_axis(snap, dtype=dtype)
    assert np.array_equal(case["pos"], case["pos"].astype(dtype).astype(np.float64))
    _, _, d = loc_ref.pairs(case["pos"], case["types"], case["nl"], 0, case["r_cut"], L=case["L"])
    sin_t = np.hypot(d[:, 0], d[:, 1]) / np.sqrt((d * d).sum(axis=1))
    near = sin_t[(sin_t > 0) & (sin_t < 0.05)]
    print("%s %s: %d entries on the axis, %d within 0.05 of it, sin(theta) from %.3e to %.3e"
          % (snap, np.dtype(dtype).name, n_on, len(near), near.min(), near.max()))
    assert n_on >= 40 and len(near) >= 100
    assert near.min() < (1e-11 if dtype == np.float64 else 2e-6) and near.max() > 3e-3
    case = dict(case, lmax=6, Ql_ref=QL_46)
    a, b = loc_ref.compute(**case, frame=Q1), loc_ref.compute(**case, frame=Q2)
    assert largest_difference(a, b, "ql_local_ref") <= 1e-12
