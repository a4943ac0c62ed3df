"""CPU: the numpy restatement of the Debye structure factor (tests/debye_ref.py) that the GPU tests compare against is itself checked
here: its analytic gradient against central differences of its value, its virial against differences of the value under strained
positions and box (tilted), the sum rule of the gradient, s as the mean of s_i, a perfect fcc crystal against the closed sum over its
shells, the invariance under a rigid motion, the spectrum against the peaks, the contrast between crystal and liquid, and that one
dropped or one stale list entry moves the result (so a GPU pass that loses or invents an entry cannot agree with it)."""
import math

import numpy as np
import pytest

import debye_ref as dsf
import util

Q111, Q200 = 7.695, 8.886            # the first two peaks of fcc with nearest-neighbour distance 1: 2 pi sqrt(3) / a, 4 pi / a, a = sqrt(2)
R_CUT = 2.4
Q3, C3 = (Q111, Q200, 12.57), (1.0, -0.5, 0.25)


def snapshot(noise, n=5, seed=777):
    pos, L = util.fcc_lattice(n)
    pos = pos + np.random.default_rng(seed).normal(0, noise, pos.shape)
    return pos, np.zeros(len(pos), dtype=np.int32), L


@pytest.fixture(scope="module")
def crystal():
    pos, types, L = snapshot(0.05)
    nl = util.build_nlist(pos, L, R_CUT)
    return dict(pos=pos, types=types, L=L, nl=nl, r=dsf.compute(pos, types, L, nl, Q3, R_CUT, 0, c=C3))


def test_gather_form_is_the_gradient_on_a_symmetric_list_and_sums_to_zero(crystal):
    r = crystal["r"]
    top = np.abs(r["grad"]).max()
    assert top > 1e-3
    assert np.abs(r["gather"] - r["grad"]).max() <= 1e-14 * top
    assert np.abs(r["grad"].sum(axis=0)).max() <= 1e-13 * top * len(r["grad"])


def test_value_is_the_mean_of_the_local_values(crystal):
    r = crystal["r"]
    assert r["n_t"] == 500
    assert r["local"].mean() == pytest.approx(r["s"], rel=1e-13)
    assert r["s"] == pytest.approx(float(np.dot(C3, r["I"])), rel=1e-15)


def test_gradient_against_central_differences(crystal):
    pos, types, L, nl, r = (crystal[k] for k in ("pos", "types", "L", "nl", "r"))
    top = np.abs(r["grad"]).max()
    h, worst = 1e-5, 0.0
    for k in (0, 7, 123, 256, 499):
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[k, a] += h
            m[k, a] -= h
            fd = (dsf.value(p, types, L, nl, Q3, R_CUT, 0, c=C3) - dsf.value(m, types, L, nl, Q3, R_CUT, 0, c=C3)) / (2 * h)
            worst = max(worst, abs(fd - r["grad"][k, a]))
    print("gradient vs central differences: %.3e of max |ds/dr| %.3e" % (worst / top, top))
    assert worst <= 1e-8 * top


def test_strain_derivatives_and_gradient_tilted_box():
    """the six derivatives of s under x -> (1 + eps) x of positions and box, against -virial_sum / bias, in a sheared box"""
    pos, L = util.fcc_lattice(4)
    pos = pos + np.random.default_rng(11).normal(0, 0.05, pos.shape)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = (pos / L) @ h.T
    types = np.zeros(len(pos), dtype=np.int32)
    r_cut = 2.0
    nl = dsf.brute_nlist(pos, h, r_cut + 0.05)
    r = dsf.compute(pos, types, L, nl, Q3, r_cut, 0, c=C3, tilt=tilt, bias=1.0)
    e, worst = 1e-6, 0.0
    top = np.abs(r["virial_sum"]).max()
    for c6, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        vals = []
        for sgn in (1.0, -1.0):
            # an upper-triangular strain keeps the cell in HOOMD's form: eps_ab with a <= b moves x_a by eps x_b
            F = np.eye(3)
            F[a, b] += sgn * e
            h2 = F @ h
            L2 = np.array([h2[0, 0], h2[1, 1], h2[2, 2]])
            t2 = dict(xy=h2[0, 1] / L2[1], xz=h2[0, 2] / L2[2], yz=h2[1, 2] / L2[2])
            vals.append(dsf.value(pos @ F.T, types, L2, nl, Q3, r_cut, 0, c=C3, tilt=t2))
        fd = (vals[0] - vals[1]) / (2 * e)
        worst = max(worst, abs(fd + r["virial_sum"][c6]))
        print("eps_%d%d: difference %.10g, -virial sum %.10g" % (a, b, fd, -r["virial_sum"][c6]))
    assert top > 0.1
    assert worst <= 1e-6 * top          # central differences of step 1e-6 on a value of order 1: ~1e-10 / 1e-6 rounding, O(e^2) truncation
    # the virial is symmetric: xy formed as d_x G_y equals d_y G_x; and the gradient in the tilted box
    gtop, hh, gworst = np.abs(r["grad"]).max(), 1e-5, 0.0
    for k in (3, 100, 255):
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[k, a] += hh
            m[k, a] -= hh
            fd = (dsf.value(p, types, L, nl, Q3, r_cut, 0, c=C3, tilt=tilt) - dsf.value(m, types, L, nl, Q3, r_cut, 0, c=C3, tilt=tilt)) / (2 * hh)
            gworst = max(gworst, abs(fd - r["grad"][k, a]))
    assert gworst <= 1e-8 * gtop
    assert np.abs(r["grad"].sum(axis=0)).max() <= 1e-13 * gtop * len(pos)


def test_perfect_fcc_against_the_closed_shell_sum():
    pos, L = util.fcc_lattice(5)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, R_CUT)
    r = dsf.compute(pos, types, L, nl, (Q111, Q200), R_CUT, 0)
    shells = [(12, 1.0), (6, math.sqrt(2.0)), (24, math.sqrt(3.0)), (12, 2.0), (24, math.sqrt(5.0))]
    for p, Q in enumerate((Q111, Q200)):
        want = 1.0 + sum(n * (math.sin(math.pi * d / R_CUT) / (math.pi * d / R_CUT)) * math.sin(Q * d) / (Q * d) for n, d in shells)
        assert r["I"][p] == pytest.approx(want, rel=1e-12)
    assert np.abs(r["grad"]).max() <= 1e-12                              # every site is a centre of inversion
    assert np.allclose(r["local"], r["s"], rtol=1e-12)


def test_invariance_under_a_rigid_motion_of_a_finite_cluster():
    pos, _ = util.fcc_lattice(3)
    pos = pos + np.random.default_rng(3).normal(0, 0.05, pos.shape)
    extent = np.ptp(pos, axis=0).max() * math.sqrt(3.0)
    L = extent + 2 * R_CUT + 1.0                                         # wider than the cluster plus 2 r_cut in any orientation
    types = np.zeros(len(pos), dtype=np.int32)
    a = dsf.compute(pos, types, L, util.build_nlist(pos, L, R_CUT), Q3, R_CUT, 0, c=C3)
    R = util.random_rotation(5)
    moved = pos @ R.T + np.array([0.3, -0.2, 0.1])
    assert np.abs(moved).max() < L / 2
    b = dsf.compute(moved, types, L, util.build_nlist(moved, L, R_CUT), Q3, R_CUT, 0, c=C3)
    assert b["s"] == pytest.approx(a["s"], rel=1e-12)
    assert np.abs(b["I"] - a["I"]).max() <= 1e-12
    assert np.abs(b["local"] - a["local"]).max() <= 1e-11
    assert np.abs(b["grad"] - a["grad"] @ R.T).max() <= 1e-11 * np.abs(a["grad"]).max()


def test_spectrum_at_the_peaks_is_the_intensity(crystal):
    pos, types, L, nl, r = (crystal[k] for k in ("pos", "types", "L", "nl", "r"))
    for p, Q in enumerate(Q3):
        Qm, I = dsf.spectrum(pos, types, L, nl, R_CUT, 0, Q, Q, 1)
        assert Qm[0] == Q and I[0] == pytest.approx(r["I"][p], rel=1e-14)
    Qm, I = dsf.spectrum(pos, types, L, nl, R_CUT, 0, 5.0, 14.0, 181)
    assert Qm[0] == 5.0 and Qm[-1] == pytest.approx(14.0, rel=1e-15) and len(I) == 181
    # beyond the forward scattering of the truncated sum (Q r_cut < ~2 pi) the tallest feature is the (111)/(200) doublet; the window
    # resolves 2 pi / r_cut = 2.6 and the two lie 1.2 apart, so they merge into one maximum between them
    assert Q111 - 0.05 < Qm[np.argmax(I)] < Q200 + 0.05


def test_contrast_between_crystal_hot_crystal_and_random(crystal):
    pos, types, L = snapshot(0.13)
    hot = dsf.compute(pos, types, L, util.build_nlist(pos, L, R_CUT), (Q111, Q200), R_CUT, 0)["I"]
    rnd_pos = np.random.default_rng(777).random((500, 3)) * L - L / 2
    rnd = dsf.compute(rnd_pos, types, L, util.build_nlist(rnd_pos, L, R_CUT), (Q111, Q200), R_CUT, 0)["I"]
    cold = crystal["r"]["I"]
    print("I(Q111), I(Q200): crystal %.3f %.3f, hot crystal %.3f %.3f, random %.3f %.3f" % (cold[0], cold[1], hot[0], hot[1], rnd[0], rnd[1]))
    assert cold[0] > 1.8 and rnd[0] < 1.2 and rnd[1] < 1.2
    assert cold[0] > hot[0] > rnd[0] and cold[1] > hot[1] > rnd[1]
    # the reach of the list is the resolution: more contrast at r_cut 3.5
    far = dsf.compute(crystal["pos"], crystal["types"], crystal["L"], util.build_nlist(crystal["pos"], crystal["L"], 3.5), (Q111,), 3.5, 0)["I"]
    assert far[0] > cold[0] + 0.2


def test_one_dropped_or_one_stale_entry_moves_the_result(crystal):
    pos, types, L, nl, r = (crystal[k] for k in ("pos", "types", "L", "nl", "r"))
    head, nn, lst = (np.array(x).copy() for x in nl)
    top = np.abs(r["gather"]).max()
    nn2 = nn.copy()
    nn2[17] -= 1                                                         # the last entry of row 17 is lost
    a = dsf.compute(pos, types, L, (head, nn2, lst), Q3, R_CUT, 0, c=C3)
    assert abs(a["s"] - r["s"]) > 1e-6 * abs(r["s"]) and np.abs(a["gather"][17] - r["gather"][17]).max() > 1e-4 * top
    lst2 = lst.copy()
    row = set(lst[head[40]:head[40] + nn[40]].tolist())
    other = next(j for j in lst[head[int(lst[head[40]])]:][:40] if int(j) not in row and int(j) != 40)
    lst2[head[40]] = other                                               # a stale entry: a particle that is no neighbour any more
    b = dsf.compute(pos, types, L, (head, nn, lst2), Q3, R_CUT, 0, c=C3)
    assert np.abs(b["gather"][40] - r["gather"][40]).max() > 1e-4 * top and b["local"][40] != r["local"][40]


def test_no_particles_of_the_type_no_pairs_and_a_coincident_pair():
    pos, types, L = snapshot(0.05)
    nl = util.build_nlist(pos, L, R_CUT)
    r = dsf.compute(pos, types, L, nl, Q3, R_CUT, 1, c=C3)
    assert r["s"] == 0.0 and r["n_t"] == 0 and np.all(r["I"] == 0.0) and np.all(r["grad"] == 0.0) and np.all(r["local"] == 0.0)
    far = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    r = dsf.compute(far, np.zeros(3, dtype=np.int32), 20.0, util.build_nlist(far, 20.0, R_CUT), Q3, R_CUT, 0, c=C3)
    assert np.all(r["I"] == 1.0) and r["s"] == pytest.approx(sum(C3)) and np.all(r["grad"] == 0.0)
    two = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.5, 1.0, 1.0]])
    nl = (np.array([0, 2, 4]), np.array([2, 2, 2]), np.array([1, 2, 0, 2, 0, 1]))
    r = dsf.compute(two, np.zeros(3, dtype=np.int32), 20.0, nl, (Q111,), R_CUT, 0)
    assert np.isfinite(r["grad"]).all() and np.isfinite(r["s"])
    x = math.pi * 0.5 / R_CUT
    phi = math.sin(x) / x * math.sin(Q111 * 0.5) / (Q111 * 0.5)
    assert r["I"][0] == pytest.approx(1.0 + (2 * 1.0 + 4 * phi) / 3, rel=1e-14)
