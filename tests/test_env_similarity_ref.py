"""CPU: the numpy restatement of the environment similarity (tests/env_similarity_ref.py) that the GPU tests compare against is itself
checked here: its analytic gradient against central differences of its value, its virial sums against differences of the value under
x_a += eps x_b of positions and box with the templates held fixed (cubic and tilted), the asymmetry of that tensor, gather = scatter on a
symmetric list, the closed-environment shortcut, known values on the common snapshots, and the additivity over complementary sets of
central particles (the identity a domain-decomposed run rests on)."""
import numpy as np
import pytest

import env_similarity_ref as es
import util
from pair_entropy_ref import brute_nlist

FCC = es.templates("fcc", np.sqrt(2.0))            # nearest-neighbour distance 1
PAR = (0.12, 1.3, 1.5, 0)                          # sigma_env, r_on, r_cut, type
SWITCH = (0.5, 6)


def rot_z(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


TWO = [FCC, FCC @ rot_z(5.0).T]                    # the unsaturated two-environment case, with lam = 20


def snapshot(noise):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(777).normal(0, noise, pos.shape)
    return pos, np.zeros(len(pos), dtype=np.int32), L


@pytest.fixture(scope="module")
def crystal():
    pos, types, L = snapshot(0.05)
    nl = util.build_nlist(pos, L, 1.5)
    return dict(pos=pos, types=types, L=L, nl=nl, r=es.compute(pos, types, L, nl, FCC, *PAR),
                two=es.compute(pos, types, L, nl, TWO, *PAR, lam=20.0, sw=SWITCH))


@pytest.fixture(scope="module")
def hot():
    pos, types, L = snapshot(0.13)
    nl = util.build_nlist(pos, L, 1.5)
    return dict(pos=pos, types=types, L=L, nl=nl, r=es.compute(pos, types, L, nl, FCC, *PAR))


def test_known_values_and_ordering(crystal, hot):
    pos, types, L, nl = (crystal[k] for k in ("pos", "types", "L", "nl"))
    rnd_pos = np.random.default_rng(777).random((500, 3)) * L - L / 2
    rnd = es.value(rnd_pos, types, L, util.build_nlist(rnd_pos, L, 1.5), FCC, *PAR)
    print("s: crystal %.12g, hot crystal %.12g, random %.12g" % (crystal["r"]["s"], hot["r"]["s"], rnd))
    assert crystal["r"]["s"] == pytest.approx(0.780942664906, abs=1e-10)
    assert hot["r"]["s"] == pytest.approx(0.301889784729, abs=1e-10)
    assert rnd == pytest.approx(0.105957224802, abs=1e-10)
    assert crystal["r"]["s"] > hot["r"]["s"] > rnd
    sw = [es.compute(c["pos"], c["types"], c["L"], c["nl"], FCC, *PAR, sw=SWITCH)["sum_v"] for c in (crystal, hot)]
    print("with the switch: s N = %.10g and %.10g" % tuple(sw))
    assert sw[0] == pytest.approx(460.290552539, abs=1e-6) and sw[1] == pytest.approx(61.1720117331, abs=1e-6)
    rotated = es.value(pos, types, L, nl, FCC @ util.random_rotation(5).T, *PAR)
    print("rotated template: %.12g" % rotated)
    assert rotated == pytest.approx(0.116682402189, abs=1e-10) and rotated < 0.5 * hot["r"]["s"]


def test_gather_form_is_the_gradient_on_a_symmetric_list(crystal):
    for r in (crystal["r"], crystal["two"]):
        assert np.abs(r["gather"] - r["grad"]).max() <= 1e-14 * np.abs(r["grad"]).max() + 1e-18
        assert np.abs(r["grad"].sum(axis=0)).max() <= 1e-13 * np.abs(r["grad"]).sum()


def test_closed_shortcut_is_the_general_formula(crystal):
    pos, types, L, nl = (crystal[k] for k in ("pos", "types", "L", "nl"))
    assert es.is_closed(FCC) and not es.is_closed(FCC[:6])
    for kw in (dict(), dict(sw=SWITCH)):
        a = es.compute(pos, types, L, nl, FCC, *PAR, **kw)
        b = es.compute(pos, types, L, nl, FCC, *PAR, closed_shortcut=True, **kw)
        assert np.abs(a["gather"] - b["gather"]).max() <= 1e-14 * np.abs(a["gather"]).max()
        assert np.abs(a["virial"] - b["virial"]).max() <= 1e-14 * np.abs(a["virial"]).max()


def test_unsaturated_weights(crystal):
    w = crystal["two"]["w"][:, 0]
    frac = ((w > 0.1) & (w < 0.9)).mean()
    print("particles with 0.1 < w < 0.9: %.3f" % frac)
    assert frac >= 0.1


def _gradient_check(c, templates, **kw):
    pos, types, L, nl = (c[k] for k in ("pos", "types", "L", "nl"))
    r = es.compute(pos, types, L, nl, templates, *PAR, **kw)
    top = np.abs(r["grad"]).max()
    h, worst = 1e-5, 0.0
    for k in (0, 7, 123, 256, 499):
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[k, a] += h
            m[k, a] -= h
            fd = (es.value(p, types, L, nl, templates, *PAR, **kw) - es.value(m, types, L, nl, templates, *PAR, **kw)) / (2 * h)
            worst = max(worst, abs(fd - r["grad"][k, a]))
    print("gradient vs central differences: %.3e of max |ds/dr| %.3e" % (worst / top, top))
    assert worst <= 1e-8 * top


def test_gradient_against_central_differences(crystal, hot):
    _gradient_check(crystal, FCC)
    _gradient_check(hot, FCC, sw=SWITCH)
    _gradient_check(crystal, FCC[:6])
    _gradient_check(crystal, TWO, lam=20.0)
    _gradient_check(crystal, TWO, lam=20.0, sw=SWITCH)


def _strain_check(pos, types, L, nl, tilt, templates, **kw):
    """the derivatives of s under x_a += eps x_b of positions and box, templates fixed, against -virial_sum / bias (a <= b) and the
    restatement's full tensor"""
    r = es.compute(pos, types, L, nl, templates, *PAR, tilt=tilt, bias=1.0, **kw)
    t = tilt or dict(xy=0.0, xz=0.0, yz=0.0)
    h = np.array([[L, t["xy"] * L, t["xz"] * L], [0, L, t["yz"] * L], [0, 0, L]])
    e, worst = 1e-6, 0.0
    top = np.abs(r["virial_sum"]).max()
    for c6, (a, b) in enumerate(es.COMPONENTS):
        vals = []
        for sgn in (1.0, -1.0):
            F = np.eye(3)
            F[a, b] += sgn * e
            h2 = F @ h
            L2 = np.array([h2[0, 0], h2[1, 1], h2[2, 2]])
            t2 = dict(xy=h2[0, 1] / L2[1], xz=h2[0, 2] / L2[2], yz=h2[1, 2] / L2[2])
            vals.append(es.value(pos @ F.T, types, L2, nl, templates, *PAR, tilt=t2, **kw))
        fd = (vals[0] - vals[1]) / (2 * e)
        worst = max(worst, abs(fd + r["virial_sum"][c6]))
        print("eps_%d%d: difference %.10g, -virial sum %.10g" % (a, b, fd, -r["virial_sum"][c6]))
        assert r["virial_sum"][c6] == pytest.approx(r["tensor"][a, b], rel=1e-12, abs=1e-15)
    assert top > 0.05
    assert worst <= 1e-6 * top
    return r


def test_strain_derivatives_cubic_box(crystal):
    pos, types, L, nl = (crystal[k] for k in ("pos", "types", "L", "nl"))
    r = _strain_check(pos, types, L, nl, None, FCC)
    _strain_check(pos, types, L, nl, None, TWO, lam=20.0, sw=SWITCH)
    T = r["tensor"]
    # the templates do not turn with the strain: the tensor is not symmetric.  On this snapshot (template aligned with the crystal) the
    # xz and yz pairs differ by 6e-2 and 5e-2 of the largest component, the xy pair by 7e-4; the tilted snapshot below asserts xy
    off = [abs(T[a, b] - T[b, a]) / np.abs(T).max() for a, b in ((0, 1), (0, 2), (1, 2))]
    print("|T_ab - T_ba| / largest: xy %.3e, xz %.3e, yz %.3e" % tuple(off))
    assert off[1] > 1e-3 and off[2] > 1e-3


def test_strain_derivatives_tilted_box():
    pos, L = util.fcc_lattice(4)
    pos = pos + np.random.default_rng(11).normal(0, 0.05, pos.shape)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = (pos / L) @ h.T
    types = np.zeros(len(pos), dtype=np.int32)
    nl = brute_nlist(pos, h, 1.55)
    T = _strain_check(pos, types, L, nl, tilt, FCC)["tensor"]
    print("T_xy %.6e, T_yx %.6e, largest %.6e" % (T[0, 1], T[1, 0], np.abs(T).max()))
    assert abs(T[0, 1] - T[1, 0]) > 1e-3 * np.abs(T).max()


def test_diamond_sublattices():
    pos, L, sub = es.diamond_lattice(3)
    assert len(pos) == 216
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.45)
    T = es.templates("diamond", 4.0 / np.sqrt(3.0))
    par = (0.12, 1.25, 1.45, 0)
    both = es.compute(pos, types, L, nl, T, *par)
    one = es.value(pos, types, L, nl, T[0], *par)
    print("diamond: s - 1 = %.3e with both environments, %.9f with one" % (both["s"] - 1.0, one))
    assert both["s"] == pytest.approx(1.0, abs=1e-6) and one == pytest.approx(0.5, abs=1e-6)
    assert both["closed"] == [False, False]
    a, b = both["ke"][sub == 0], both["ke"][sub == 1]
    assert np.allclose(a[:, 0], 1.0, atol=1e-6) and np.allclose(a[:, 1], 0.0, atol=1e-6)
    assert np.allclose(b[:, 0], 0.0, atol=1e-6) and np.allclose(b[:, 1], 1.0, atol=1e-6)


def test_sums_and_rows_add_up_over_complementary_sets(crystal):
    pos, types, L, nl, r = (crystal[k] for k in ("pos", "types", "L", "nl", "r"))
    mine = np.where(pos[:, 2] < 0.3)[0]
    rest = np.setdiff1d(np.arange(len(pos)), mine)
    assert 0 < len(mine) < len(pos)
    a = es.compute(pos, types, L, nl, FCC, *PAR, rows=mine, bias=0.7)
    b = es.compute(pos, types, L, nl, FCC, *PAR, rows=rest, bias=0.7)
    full = es.compute(pos, types, L, nl, FCC, *PAR, bias=0.7)
    assert a["sum_v"] + b["sum_v"] == pytest.approx(r["sum_v"], rel=1e-13)
    assert np.array_equal(a["k"][mine], full["k"][mine]) and np.all(a["k"][rest] == 0.0)
    assert np.abs(a["gather"][mine] - full["gather"][mine]).max() <= 1e-15
    assert np.abs(a["virial"][mine] - full["virial"][mine]).max() <= 1e-15
    assert np.all(a["virial"][rest] == 0.0) and np.all(a["gather"][rest] == 0.0)
    # with a switch the rows of one domain need beta of the other's particles: handed over, they are the single-domain rows
    fs = es.compute(pos, types, L, nl, FCC, *PAR, sw=SWITCH)
    ps = es.compute(pos, types, L, nl, FCC, *PAR, sw=SWITCH, rows=mine, beta_all=fs["beta"])
    assert np.abs(ps["gather"][mine] - fs["gather"][mine]).max() <= 1e-15


def test_other_types_and_no_pairs():
    pos, types, L = snapshot(0.05)
    nl = util.build_nlist(pos, L, 1.5)
    r = es.compute(pos, types, L, nl, FCC, 0.12, 1.3, 1.5, 1)
    assert r["s"] == 0.0 and np.all(r["grad"] == 0.0) and np.all(r["virial"] == 0.0)
    far = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    r = es.compute(far, np.zeros(3, dtype=np.int32), 20.0, util.build_nlist(far, 20.0, 1.5), FCC, *PAR)
    assert np.all(r["k"] == 0.0) and np.all(r["grad"] == 0.0) and r["s"] == 0.0
