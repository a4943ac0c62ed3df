"""CPU: the yardstick of the global Steinhardt variable's virial (tests/ql_virial_ref.py) is checked before anything is held against
it.  Its per-entry forces add up to the oracle's ql_compute_forces (full and half lists, cubic and triclinic boxes); the per-particle
virial of a symmetrised half list is the full-list one; and its summed virial is -1/2 bias ds/d eps_ab by central differences of the
oracle's CV under an affine strain of positions and box with the list kept — HALF the strain derivative, because the reference's force
keeps only the central terms of the gradient.  Nothing here needs a GPU.

Strain differences at eps = 1e-6, relative to max|W| (measured when this file was written; 108-particle noisy fcc, bias 0.9):
    degrees 4 and 6:           cubic 4.0e-9 full list, 2.2e-9 half list; triclinic 2.0e-9 full, 1.7e-9 half
    l = 0, 2, 3 (odd), 4:      cubic 4.7e-9 full list, 2.9e-9 half list; triclinic 2.5e-9 full, 2.3e-9 half
(1.3e-8 / 5e-9 at eps = 1e-5, 2e-8 ... 5e-8 at eps = 1e-7: rounding of the CV, about 1e-16 of s, divided by eps, meets the eps^2
truncation near 1e-6.)  The bound is ten times the largest, 4.7e-8 of max|W|; a wrong factor or a missing term shows at order 1."""
import numpy as np
import pytest

import ql_virial_ref as vir_ref
import util

BIAS = 0.9
R_CUT, R_ON = 1.4, 1.2
QL_46 = (6, [0, 0, 0, 0, 1, 0, 1])
QL_L0_ODD = (4, [0.2, 0, 1, 0.5, 1])
TILT = dict(xy=0.1, xz=-0.05, yz=0.08)
STRAIN_BOUND = 4.7e-8

_snap = {}
_results = {}


def snapshot(triclinic):
    """the 108-particle noisy fcc snapshot with its full and half lists at r_cut + 0.15; the triclinic one is its affine image"""
    if not _snap:
        pos, L = util.fcc_lattice(3)
        pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
        _snap.update(pos=pos, L=L, types=np.zeros(len(pos), dtype=np.int32),
                     lists={half: util.build_nlist(pos, L, R_CUT + 0.15, half=half) for half in (False, True)})
    pos, L = _snap["pos"], _snap["L"]
    if triclinic:
        H = np.array([[L, TILT["xy"] * L, TILT["xz"] * L], [0, L, TILT["yz"] * L], [0, 0, L]])
        pos = (pos / L) @ H.T
    return pos, L, _snap["types"], _snap["lists"]


def result(ref, degrees, triclinic, half):
    """(case, restatement) computed once and left unchanged"""
    key = (degrees[0], triclinic, half)
    if key not in _results:
        pos, L, types, lists = snapshot(triclinic)
        case = dict(pos=pos, types=types, L=L, nl=lists[half], r_cut=R_CUT, r_on=R_ON, lmax=degrees[0], type_id=0, Ql_ref=degrees[1],
                    tilt=TILT if triclinic else None, half=half)
        _, Qlm = vir_ref.oracle_cv(ref, **case)
        _results[key] = (case, Qlm, vir_ref.compute(**case, Qlm=Qlm, bias=BIAS))
    return _results[key]


CASES = [(d, t, h) for d in (QL_46, QL_L0_ODD) for t in (False, True) for h in (False, True)]
IDS = ["lmax%d-%s-%s" % (d[0], "triclinic" if t else "cubic", "half" if h else "full") for d, t, h in CASES]


@pytest.mark.parametrize("degrees,triclinic,half", CASES, ids=IDS)
def test_force_sums_are_the_oracles(ref, degrees, triclinic, half):
    case, Qlm, out = result(ref, degrees, triclinic, half)
    box = ref.Box.make(case["L"], **(case["tilt"] or {}))
    F = ref.ql_compute_forces(util.oracle_postype(case["pos"], case["types"]), box, *case["nl"], R_CUT, R_ON, case["lmax"], 0, case["Ql_ref"], Qlm,
                              BIAS, half=half)
    top = np.abs(F[:, :3]).max()
    err = np.abs(out["F"] - F[:, :3]).max()
    print("force sums: largest difference %.3e of max|F| %.4g" % (err, top))
    assert top > 0
    assert err <= 1e-12 * top


@pytest.mark.parametrize("degrees", [QL_46, QL_L0_ODD], ids=["lmax6", "lmax4-l0-odd"])
@pytest.mark.parametrize("triclinic", [False, True], ids=["cubic", "triclinic"])
def test_symmetrised_half_list_gives_the_full_list_virial(ref, degrees, triclinic):
    """mode 2: the Q_lm of the half-list CV (even degrees doubled, odd ones zero) on the symmetric full list the half list stands for,
    in the gather form (row k only), against the half list's scatter form"""
    case, Qlm, out = result(ref, degrees, triclinic, True)
    pos, L, types, lists = snapshot(triclinic)
    sym = vir_ref.compute(**{**case, "nl": lists[False], "half": False}, Qlm=Qlm, bias=BIAS)
    top = np.abs(out["virial"]).max()
    err = np.abs(sym["virial"] - out["virial"]).max()
    print("per-particle virial, symmetric full list against half list: %.3e of %.4g" % (err, top))
    assert top > 0
    assert err <= 1e-13 * top
    assert np.abs(sym["F"] - out["F"]).max() <= 1e-13 * np.abs(out["F"]).max()
    # and, for even degrees only, the plain full-list virial (its Q_lm are the same numbers then)
    if degrees is QL_46:
        full = result(ref, degrees, triclinic, False)[2]
        assert np.abs(full["virial"] - out["virial"]).max() <= 1e-12 * top


@pytest.mark.parametrize("degrees,triclinic,half", CASES, ids=IDS)
def test_summed_virial_is_half_the_strain_derivative(ref, degrees, triclinic, half):
    case, Qlm, out = result(ref, degrees, triclinic, half)
    W = out["W"]
    top = np.abs(W).max()
    fd = -0.5 * BIAS * vir_ref.strain_derivative(ref, **case, eps=1e-6)
    err = np.abs(fd - W).max()
    print("W = %s\n  -1/2 bias ds/d eps = %s\n  largest difference %.3e (%.3e of max|W| = %.4g)" % (W, fd, err, err / top, top))
    assert top > 1.0
    assert err <= STRAIN_BOUND * top


def test_shapes_zero_rows_and_scaling(ref):
    """particles of another type have zero rows; the virial scales with 1 / N_global^2 times the Q_lm's 1 (a table given, not recomputed)"""
    pos, L, types, lists = snapshot(False)
    types = (np.random.default_rng(1).random(len(pos)) < 0.3).astype(np.int32)
    case = dict(pos=pos, types=types, L=L, nl=lists[False], r_cut=R_CUT, r_on=R_ON, lmax=6, type_id=0, Ql_ref=QL_46[1])
    _, Qlm = vir_ref.oracle_cv(ref, **case)
    one = vir_ref.compute(**case, Qlm=Qlm, bias=BIAS)
    three = vir_ref.compute(**case, Qlm=Qlm, bias=BIAS, n_global=3 * len(pos))
    assert one["virial"].shape == (len(pos), 6) and np.isfinite(one["virial"]).all()
    assert np.all(one["virial"][types == 1] == 0.0) and np.all(one["F"][types == 1] == 0.0)
    assert np.abs(one["virial"]).max() > 0
    assert np.abs(one["virial"] - 9.0 * three["virial"]).max() <= 1e-14 * np.abs(one["virial"]).max()
    assert np.abs(one["W"] - one["virial"].sum(axis=0)).max() == 0.0
