"""CPU: the numpy restatement of the pair entropy (tests/pair_entropy_ref.py) that the GPU tests compare against is itself checked here:
its analytic gradient against central differences of its value, its virial against differences of the value under strained positions and
box (cubic and tilted), the additivity of the sums over complementary sets of central particles (the identity a domain-decomposed run
rests on), and the ordering crystal < hot crystal < random <= ~0."""
import numpy as np
import pytest

import pair_entropy_ref as pe
import util

PAR = (2.0, 0.1, 40, 0)              # r_max, sigma_r, n_bins, type


def snapshot(noise):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(777).normal(0, noise, pos.shape)
    return pos, np.zeros(len(pos), dtype=np.int32), L


@pytest.fixture(scope="module")
def crystal():
    pos, types, L = snapshot(0.05)
    nl = util.build_nlist(pos, L, 2.4)
    return dict(pos=pos, types=types, L=L, nl=nl, r=pe.compute(pos, types, L, nl, *PAR))


def test_known_values(crystal):
    r = crystal["r"]
    print("S = %.12g, bins above g_min: %d, entries per particle %.1f" % (r["S"], (r["g"] >= pe.G_MIN).sum(), len(crystal["nl"][2]) / 500))
    assert r["S"] == pytest.approx(-2.832, abs=5e-4)
    assert (r["g"] >= pe.G_MIN).sum() == 37 and r["n_t"] == 500
    assert np.abs(r["grad"]).max() == pytest.approx(0.089, abs=1e-3)


def test_gather_form_is_the_gradient_on_a_symmetric_list(crystal):
    r = crystal["r"]
    assert np.abs(r["gather"] - r["grad"]).max() <= 1e-14 * np.abs(r["grad"]).max()


def test_gradient_against_central_differences(crystal):
    pos, types, L, nl, r = (crystal[k] for k in ("pos", "types", "L", "nl", "r"))
    top = np.abs(r["grad"]).max()
    h, worst = 1e-5, 0.0
    for k in (0, 7, 123, 256, 499):
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[k, a] += h
            m[k, a] -= h
            fd = (pe.value(p, types, L, nl, *PAR) - pe.value(m, types, L, nl, *PAR)) / (2 * h)
            worst = max(worst, abs(fd - r["grad"][k, a]))
    print("gradient vs central differences: %.3e of max |dS/dr| %.3e" % (worst / top, top))
    assert worst <= 1e-8 * top


def _strain_check(pos, types, L, nl, tilt, par):
    """the six derivatives of S under x -> (1 + eps) x of positions and box, against -virial_sum / bias"""
    r = pe.compute(pos, types, L, nl, *par, tilt=tilt, bias=1.0)
    t = tilt or dict(xy=0.0, xz=0.0, yz=0.0)
    h = np.array([[L, t["xy"] * L, t["xz"] * L], [0, L, t["yz"] * L], [0, 0, L]])
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
            vals.append(pe.value(pos @ F.T, types, L2, nl, *par, tilt=t2))
        fd = (vals[0] - vals[1]) / (2 * e)
        worst = max(worst, abs(fd + r["virial_sum"][c6]))
        print("eps_%d%d: difference %.10g, -virial sum %.10g" % (a, b, fd, -r["virial_sum"][c6]))
    assert top > 0.1
    assert worst <= 1e-6 * top          # central differences of step 1e-6 on a value of order 1: ~1e-10 / 1e-6 rounding, O(e^2) truncation
    return r


def test_strain_derivatives_cubic_box(crystal):
    r = _strain_check(crystal["pos"], crystal["types"], crystal["L"], crystal["nl"], None, PAR)
    assert -(r["virial_sum"][[0, 3, 5]].sum()) == pytest.approx(-2.788235, abs=2e-6)


def test_strain_derivatives_tilted_box():
    pos, L = util.fcc_lattice(4)
    pos = pos + np.random.default_rng(11).normal(0, 0.05, pos.shape)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = (pos / L) @ h.T
    types = np.zeros(len(pos), dtype=np.int32)
    par = (1.6, 0.1, 32, 0)
    nl = pe.brute_nlist(pos, h, 2.0 + 0.05)
    _strain_check(pos, types, L, nl, tilt, par)


def test_sums_add_up_over_complementary_rows(crystal):
    pos, types, L, nl, r = (crystal[k] for k in ("pos", "types", "L", "nl", "r"))
    mine = np.where(pos[:, 2] < 0.3)[0]
    rest = np.setdiff1d(np.arange(len(pos)), mine)
    assert 0 < len(mine) < len(pos)
    Ha, na = pe.sums(pos, types, L, nl, *PAR, rows=mine)
    Hb, nb = pe.sums(pos, types, L, nl, *PAR, rows=rest)
    assert na + nb == r["n_t"]
    assert np.abs(Ha + Hb - r["H"]).max() <= 1e-13 * r["H"].max()
    S = pe.finalize(Ha + Hb, na + nb, L, *PAR[:3])["S"]
    assert S == pytest.approx(r["S"], rel=1e-13)
    # and the rows of one domain with the reduced sums are the single-domain rows: forces and virial
    part = pe.compute(pos, types, L, nl, *PAR, rows=mine, sums_override=(r["H"], r["n_t"]), bias=0.7)
    full = pe.compute(pos, types, L, nl, *PAR, bias=0.7)
    assert np.abs(part["gather"][mine] - full["gather"][mine]).max() <= 1e-15
    assert np.abs(part["virial"][mine] - full["virial"][mine]).max() <= 1e-15
    assert np.all(part["virial"][rest] == 0.0)


def test_ordering_of_crystal_hot_crystal_and_random(crystal):
    hot_pos, types, L = snapshot(0.13)
    hot = pe.value(hot_pos, types, L, util.build_nlist(hot_pos, L, 2.4), *PAR)
    rnd_pos = np.random.default_rng(777).random((500, 3)) * L - L / 2
    rnd = pe.value(rnd_pos, types, L, util.build_nlist(rnd_pos, L, 2.4), *PAR)
    print("S: crystal %.4f, hot crystal %.4f, random %.4f" % (crystal["r"]["S"], hot, rnd))
    assert hot == pytest.approx(-0.616, abs=5e-4)
    assert crystal["r"]["S"] < hot < rnd <= 1e-3
    assert rnd > -0.05


def test_no_particles_of_the_type_and_no_pairs():
    pos, types, L = snapshot(0.05)
    nl = util.build_nlist(pos, L, 2.4)
    r = pe.compute(pos, types, L, nl, 2.0, 0.1, 40, 1)
    assert r["S"] == 0.0 and r["n_t"] == 0 and np.all(r["grad"] == 0.0) and np.all(r["virial"] == 0.0)
    far = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    r = pe.compute(far, np.zeros(3, dtype=np.int32), 20.0, util.build_nlist(far, 20.0, 2.4), *PAR)
    c = pe.constants(*PAR[:3])
    assert np.all(r["g"] == 0.0) and np.all(r["grad"] == 0.0)
    assert r["S"] == pytest.approx(-2 * np.pi * (3 / 20.0 ** 3) * c["delta"] * (c["r_b"] ** 2).sum(), rel=1e-14)
