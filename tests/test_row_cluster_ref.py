"""CPU: the restatement of the coordination number and the tetrahedral order restricted to the largest cluster (tests/row_cluster_ref.py)
that the GPU tests compare against is itself checked here: the fixtures have the clusters and the margins the tests rely on, the gradient
with a FROZEN mask is the derivative of sum_i w_i v_i / N_type (central differences, step and tolerance of tests/test_coordination_ref.py
and tests/test_tetrahedral_ref.py), the virial sums are its strain derivative, and with w = 1 it reproduces coordination_ref.compute and
tetrahedral_ref.compute."""
import numpy as np
import pytest

import coordination_ref as cn
import row_cluster_ref as rc
import tetrahedral_ref as tr

# (largest, next, the least margins in v and in r / r_link the issue of this variable states for the fixture)
COORD_EXPECT = {"switch": (145, 15, 8e-3, 1.2e-3)}
TET_EXPECT = {"plain": (165, 48, 0.014, 2e-3), "switch": (165, 48, 0.014, 2e-3), "switch+gate": (102, 23, 0.014, 2e-3)}


def _check_fixture(c, expect):
    ref = c["ref"]
    sizes = np.sort(ref["size"])[::-1]
    print("cluster", c["cluster"], "margins", c["margins"], "summary", ref["summary"], "sizes", sizes[:3], "s", ref["s"])
    assert c["margins"][0] > 1e-6 and c["margins"][1] > 1e-6            # rounding cannot flip a node or an edge: masks compare exactly
    if expect is not None:
        largest, second, mv, mr = expect
        assert (sizes[0], sizes[1]) == (largest, second) and ref["summary"][1] == largest
        assert c["margins"][0] >= 0.99 * mv and c["margins"][1] >= 0.99 * mr     # (the figures are quoted to two digits)
        assert np.isin(np.nonzero(ref["w"])[0], c["big"]).all()          # all members lie in the big crystallite
    assert ref["w"].sum() == ref["summary"][1] and ref["summary"][1] > 0
    assert np.all(ref["w"][c["types"] != 0] == 0.0)


@pytest.mark.parametrize("name", list(rc.COORD_COMBOS))
def test_coordination_fixture(name):
    c = rc.coordination_case(name)
    assert 0.2 < c["cluster"][0] < 0.8 and 1.15 < c["cluster"][1] < 1.3
    if name == "switch":
        assert 0.2 < c["cluster"][0] < 0.5
    _check_fixture(c, COORD_EXPECT.get(name))


@pytest.mark.parametrize("name", list(rc.TET_COMBOS))
def test_tetrahedral_fixture(name):
    c = rc.tetrahedral_case(name)
    lo, hi = rc.TET_COMBOS[name][1]
    assert lo < c["cluster"][0] < hi and 1.1 < c["cluster"][1] < 1.35
    assert len(c["big"]) == 216 and len(c["small"]) == 64 and len(c["pos"]) == 980
    _check_fixture(c, TET_EXPECT[name])


def _cases():
    return [("coordination", n) for n in rc.COORD_COMBOS] + [("tetrahedral", n) for n in rc.TET_COMBOS]


def _case(kind, name):
    return (rc.coordination_case if kind == "coordination" else rc.tetrahedral_case)(name)


@pytest.mark.parametrize("kind,name", _cases())
def test_gradient_with_a_frozen_mask_against_central_differences(kind, name):
    c = _case(kind, name)
    ref, w = c["ref"], c["ref"]["w"]
    top = np.abs(ref["grad"]).max()
    assert top > 1e-5
    members = np.nonzero(w)[0]
    # two members, two non-members next to a member (their gradient comes from the members' rows alone), one particle of the other type
    near = [k for k in np.nonzero(w == 0.0)[0] if c["types"][k] == 0 and np.abs(ref["grad"][k]).max() > 1e-3 * top][:2]
    other = int(np.nonzero(c["types"] != 0)[0][0])
    assert len(near) == 2
    h, worst = 1e-5, 0.0
    for k in [int(members[0]), int(members[len(members) // 2])] + [int(k) for k in near] + [other]:
        for a in range(3):
            p, m = c["pos"].copy(), c["pos"].copy()
            p[k, a] += h
            m[k, a] -= h
            fd = (rc.masked_value(kind, p, c["types"], c["L"], c["nl"], c["par"], w)
                  - rc.masked_value(kind, m, c["types"], c["L"], c["nl"], c["par"], w)) / (2 * h)
            worst = max(worst, abs(fd - ref["grad"][k, a]))
    print("%s, %s: gradient vs central differences %.3e of max |ds/dr| %.3e" % (kind, name, worst / top, top))
    assert worst <= 1e-7 * top
    assert np.all(ref["grad"][c["types"] != 0] == 0.0)
    assert np.abs(ref["grad"].sum(axis=0)).max() <= 1e-13 * top * len(w)                 # no net force
    far = rc.far_from_members(c["pos"], c["L"], w, 2.0 * c["par"]["r_cut"])
    assert far.any() and np.all(ref["grad"][far] == 0.0) and np.all(ref["virial"][far] == 0.0)


@pytest.mark.parametrize("kind,name", _cases())
def test_virial_sums_are_the_strain_derivative(kind, name):
    c = _case(kind, name)
    ref, w, L = c["ref"], c["ref"]["w"], c["L"]
    top = np.abs(ref["virial_sum"]).max()
    assert top > 1e-4
    e, worst = 1e-6, 0.0
    for c6, (x, y) in enumerate(rc.PAIRS6):
        vals = []
        for sgn in (1.0, -1.0):
            F = np.eye(3)
            F[x, y] += sgn * e
            h2 = F @ np.diag([L, L, L])
            L2 = np.array([h2[0, 0], h2[1, 1], h2[2, 2]])
            t2 = dict(xy=h2[0, 1] / L2[1], xz=h2[0, 2] / L2[2], yz=h2[1, 2] / L2[2])
            vals.append(rc.masked_value(kind, c["pos"] @ F.T, c["types"], L2, c["nl"], c["par"], w, tilt=t2))
        fd = (vals[0] - vals[1]) / (2 * e)
        worst = max(worst, abs(fd + ref["virial_sum"][c6]))
        print("%s, %s, eps_%d%d: difference %.10g, -virial sum %.10g" % (kind, name, x, y, fd, -ref["virial_sum"][c6]))
    assert worst <= 1e-6 * top


@pytest.mark.parametrize("kind,name", _cases())
def test_all_ones_reproduces_the_plain_restatement(kind, name):
    c = _case(kind, name)
    if kind == "coordination":
        plain = cn.compute(c["pos"], c["types"], c["L"], c["nl"], c["par"])
        mine = rc.coordination(c["pos"], c["types"], c["L"], c["nl"], c["par"])
        grad = plain["gather"]
    else:
        plain = tr.compute(c["pos"], c["types"], c["L"], c["nl"], c["par"])
        mine = rc.tetrahedral(c["pos"], c["types"], c["L"], c["nl"], c["par"])
        grad = plain["grad"]
    top, vtop = np.abs(grad).max(), np.abs(plain["virial"]).max()
    assert mine["s"] == pytest.approx(plain["s"], rel=1e-14)
    assert np.array_equal(mine["switched"], plain["switched"])
    assert np.abs(mine["grad"] - grad).max() <= 1e-13 * top
    assert np.abs(mine["virial"] - plain["virial"]).max() <= 1e-13 * vtop
    # and the masked variable is a different one: the mask takes something away
    assert c["ref"]["s"] < plain["s"] and np.abs(c["ref"]["grad"] - grad).max() > 1e-3 * top
