"""CPU: the yardstick of the local Steinhardt variable's virial (tests/ql_local_virial_ref.py) is checked before anything is held
against it.  Its restated per-entry gradient reproduces the value and the gradient of ql_local_avg_ref; its summed virial is
-bias ds/d eps_ab by central differences of that module's s under an affine strain of positions and box; the summed 3 x 3 tensor is
symmetric; the gate is checked where its ramp is populated.  Nothing here needs a GPU.

Strain differences, eps = 1e-6, relative to max|W| (measured when this file was written): 1.4e-10 plain, 2.9e-10 switch, 1.6e-10 average,
3.0e-10 average+switch+gate, 1.2e-9 with l = 0 and an odd degree, 4.8e-10 on the dilute case; every case about 1e-8 at eps = 1e-5 (the
error falls as eps^2).  The bound is 1e-8 max|W|."""
import numpy as np
import pytest

import ql_local_avg_ref as avg_ref
import ql_local_virial_ref as vir_ref
import util

BIAS = 0.9
QL_46 = [0, 0, 0, 0, 1, 0, 1]

_dense = {}


def dense_case():
    """the 108-particle noisy fcc snapshot: list at 1.55, r_cut 1.4, r_on 1.2, lmax 6, degrees 4 and 6"""
    if not _dense:
        pos, L = util.fcc_lattice(3)
        pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
        _dense.update(pos=pos, types=np.zeros(len(pos), dtype=np.int32), L=L, nl=util.build_nlist(pos, L, 1.55), r_cut=1.4, r_on=1.2, lmax=6,
                      type_id=0, Ql_ref=QL_46)
    return dict(_dense)


def dilute():
    case = avg_ref.dilute_case()
    opt = {k: case.pop(k) for k in ("average", "switch", "gate")}
    return case, opt


CASES = {
    "plain": lambda: (dense_case(), {}),
    "switch": lambda: (dense_case(), avg_ref.COMBINATIONS["switch"]),
    "average": lambda: (dense_case(), avg_ref.COMBINATIONS["average"]),
    "average+switch+gate": lambda: (dense_case(), avg_ref.COMBINATIONS["average+switch+gate"]),
    "average+switch+gate(10,16)": lambda: (dense_case(), dict(average=True, switch=(0.12, 3), gate=(10, 16))),
    "l0-and-odd": lambda: ({**dense_case(), "lmax": 4, "Ql_ref": [0.2, 0, 1, 0.5, 1]}, {}),
    "dilute": dilute,
}

_results = {}


def result(name):
    """the reference's answer for a case, computed once and left unchanged"""
    if name not in _results:
        case, opt = CASES[name]()
        _results[name] = (case, opt, vir_ref.compute(**case, bias=BIAS, **opt))
    return _results[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_gradient_is_the_restatements(name):
    case, opt, out = result(name)
    r = avg_ref.compute(**case, **opt)
    print("s %.15g vs %.15g; gradient: largest difference %.3e of %.3e" % (out["s"], r["s"], np.abs(out["grad"] - r["grad"]).max(), np.abs(r["grad"]).max()))
    assert out["s"] == pytest.approx(r["s"], rel=1e-14)
    assert np.abs(out["grad"] - r["grad"]).max() <= 1e-14 * np.abs(r["grad"]).max()
    assert np.array_equal(out["n"], r["n"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_summed_virial_against_strain_differences(name):
    case, opt, out = result(name)
    W = out["W"]
    top = np.abs(W).max()
    fd = -BIAS * vir_ref.strain_derivative(**case, eps=1e-6, **opt)
    err = np.abs(fd - W).max()
    print("%s: W = %s\n  -bias ds/d eps = %s\n  largest difference %.3e (%.3e of max|W| = %.4g)" % (name, W, fd, err, err / top, top))
    assert top > 0.05
    assert err <= 1e-8 * top


@pytest.mark.parametrize("name", sorted(CASES))
def test_summed_tensor_is_symmetric_and_holds_the_six(name):
    case, opt, out = result(name)
    T, W = out["tensor"], out["W"]
    top = np.abs(W).max()
    anti = np.abs(T - T.T).max() / 2
    print("%s: antisymmetric part %.3e of max|W| %.4g" % (name, anti, top))
    assert anti <= 1e-12 * top
    six = np.array([T[a, b] for a, b in vir_ref.COMPONENTS])
    assert np.abs(six - W).max() <= 1e-13 * top                         # the per-particle halves add up to the sum over the entries
    assert np.isfinite(out["virial"]).all() and out["virial"].shape == (len(case["pos"]), 6)


def test_gate_moves_the_virial_where_its_ramp_is_populated():
    """gate=(4, 8) is saturated on the dense crystal (g = 1 for every particle: it gives the plain virial, so it tests nothing);
    (10, 16) has particles inside its ramp there, and the dilute case has them inside (2, 6)"""
    case, opt, out = result("average+switch+gate(10,16)")
    n = out["n"]
    inside = ((n > 10) & (n < 16)).sum()
    sat = vir_ref.compute(**case, bias=BIAS, average=True, switch=(0.12, 3), gate=(4, 8))
    no_gate = vir_ref.compute(**case, bias=BIAS, average=True, switch=(0.12, 3))
    print("particles inside the ramp (10, 16): %d of %d; max|W| %.4g gated, %.4g with (4, 8), %.4g without a gate"
          % (inside, len(n), np.abs(out["W"]).max(), np.abs(sat["W"]).max(), np.abs(no_gate["W"]).max()))
    assert inside > 0
    assert np.array_equal(sat["virial"], no_gate["virial"])               # saturated: every digit
    assert abs(np.abs(out["W"]).max() - np.abs(no_gate["W"]).max()) > 0.1 * np.abs(no_gate["W"]).max()
    case, opt, out = result("dilute")
    n = out["n"]
    assert ((n > 2) & (n < 6)).sum() > 0 and (n == 0).sum() > 0
    assert np.all(out["virial"][n == 0] == 0.0)


def test_other_type_rows_are_zero_and_values_scale_with_n_global():
    case = dense_case()
    types = (np.random.default_rng(1).random(len(case["pos"])) < 0.3).astype(np.int32)
    case["types"] = types
    opt = avg_ref.COMBINATIONS["average+switch"]
    one = vir_ref.compute(**case, bias=BIAS, **opt)
    three = vir_ref.compute(**case, bias=BIAS, n_global=3 * len(types), **opt)
    assert np.all(one["virial"][types == 1] == 0.0)
    assert np.abs(one["virial"]).max() > 0
    assert np.abs(one["virial"] - 3.0 * three["virial"]).max() <= 1e-15 * np.abs(one["virial"]).max()


def test_triclinic_strain():
    """the same identity in a tilted box: d_kj is the minimum image with tilt"""
    case = dense_case()
    tilt = dict(xy=0.1, xz=-0.05, yz=0.08)
    L = case["L"]
    H = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    case["pos"] = (case["pos"] / L) @ H.T
    case["tilt"] = tilt
    opt = avg_ref.COMBINATIONS["average+switch"]
    out = vir_ref.compute(**case, bias=BIAS, **opt)
    fd = -BIAS * vir_ref.strain_derivative(**case, eps=1e-6, **opt)
    top = np.abs(out["W"]).max()
    print("triclinic: largest difference %.3e of max|W| %.4g" % (np.abs(fd - out["W"]).max(), top))
    assert top > 0.05
    assert np.abs(fd - out["W"]).max() <= 1e-8 * top
