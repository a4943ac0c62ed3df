"""CPU: the numpy restatement of the local pair entropy (tests/pair_entropy_local_ref.py) that the GPU tests compare against is itself
checked here: its analytic gradient against central differences of its value and its virial against differences of the value under
strained positions and box (all six components, cubic and tilted), for the four option sets plain / switch / average / both; the sum of
the forces; gather = scatter; the closed form for an isolated particle; an average window that catches nothing; particles of another type.

Every difference quotient first asserts that between its two displaced states no bin changes side of g_min and no entry changes its
centre bin: across either the definition itself jumps and the quotient would measure the jump.

Bounds.  Central differences with h = 1e-5 on a value of order 1 carry ~1e-16 / 1e-5 = 1e-11 of rounding and O(h^2) = 1e-10 of
truncation: 1e-8 of the largest gradient component (the bound of tests/test_pair_entropy_ref.py); strain differences with eps = 1e-6:
1e-6 of the largest component (as there).  Measured: gradient <= 6.5e-10 of the largest component in the cubic box and <= 7.9e-9 in the tilted one (with the switch, where the
largest component is 2e-2: 1.6e-10 absolute), strain <= 8.7e-10.
"""
import numpy as np
import pytest

import pair_entropy_local_ref as pel
import pair_entropy_ref as pe
import util

PAR = (2.0, 0.1, 40, 0)              # r_max, sigma_r, n_bins, type
OPTIONS = {"plain": dict(), "switch": dict(switch=(4.0, 6)), "average": dict(average=(1.2, 1.5)),
           "both": dict(switch=(4.0, 6), average=(1.2, 1.5))}


@pytest.fixture(scope="module")
def system():
    """fcc 3 (N = 108), noise 0.1, every seventh particle of another type, the list to 2.4"""
    pos, L = util.fcc_lattice(3)
    pos = pos + np.random.default_rng(777).normal(0, 0.1, pos.shape)
    types = (np.arange(len(pos)) % 7 == 3).astype(np.int32)
    return dict(pos=pos, types=types, L=L, nl=util.build_nlist(pos, L, 2.4))


@pytest.fixture(scope="module")
def tilted():
    """fcc 3 sheared into a tilted box, the list by brute force over the images"""
    pos, L = util.fcc_lattice(3)
    pos = pos + np.random.default_rng(11).normal(0, 0.05, pos.shape)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = (pos / L) @ h.T
    types = (np.arange(len(pos)) % 7 == 3).astype(np.int32)
    par = (1.6, 0.1, 32, 0)
    return dict(pos=pos, types=types, L=L, tilt=tilt, h=h, par=par, nl=pe.brute_nlist(pos, h, 2.05))


def same_side(a, b):
    """no bin on another side of g_min, no entry in another centre bin: the two states lie on one smooth piece of the definition"""
    assert np.array_equal(a["on"], b["on"])
    assert np.array_equal(a["bc"], b["bc"])


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_gradient_against_central_differences(system, opt):
    pos, types, L, nl = (system[k] for k in ("pos", "types", "L", "nl"))
    kw = OPTIONS[opt]
    r = pel.compute(pos, types, L, nl, *PAR, **kw)
    top = np.abs(r["grad"]).max()
    h, worst = 1e-5, 0.0
    for k in (0, 3, 10, 31, 57, 80, 107):                              # (3, 10, 31 and 80 are of the other type: they feel no force)
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[k, a] += h
            m[k, a] -= h
            rp, rm = pel.compute(p, types, L, nl, *PAR, **kw), pel.compute(m, types, L, nl, *PAR, **kw)
            same_side(rp, rm)
            worst = max(worst, abs((rp["cv"] - rm["cv"]) / (2 * h) - r["grad"][k, a]))
    print("%s: gradient vs central differences: %.3e of max |dCV/dr| %.3e" % (opt, worst / top, top))
    assert top > 1e-4
    assert worst <= 1e-8 * top
    assert np.all(r["grad"][types != 0] == 0.0)


def _strain_check(pos, types, L, nl, tilt, par, kw):
    r = pel.compute(pos, types, L, nl, *par, tilt=tilt, bias=1.0, **kw)
    t = tilt or dict(xy=0.0, xz=0.0, yz=0.0)
    h = np.array([[L, t["xy"] * L, t["xz"] * L], [0, L, t["yz"] * L], [0, 0, L]])
    e, worst = 1e-6, 0.0
    top = np.abs(r["virial_sum"]).max()
    for c6, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        states = []
        for sgn in (1.0, -1.0):
            # an upper-triangular strain keeps the cell in HOOMD's form: eps_ab with a <= b moves x_a by eps x_b
            F = np.eye(3)
            F[a, b] += sgn * e
            h2 = F @ h
            L2 = np.array([h2[0, 0], h2[1, 1], h2[2, 2]])
            t2 = dict(xy=h2[0, 1] / L2[1], xz=h2[0, 2] / L2[2], yz=h2[1, 2] / L2[2])
            states.append(pel.compute(pos @ F.T, types, L2, nl, *par, tilt=t2, **kw))
        same_side(*states)
        fd = (states[0]["cv"] - states[1]["cv"]) / (2 * e)
        worst = max(worst, abs(fd + r["virial_sum"][c6]), abs(fd - r["strain"][c6]))
        print("eps_%d%d: difference %.10g, -virial sum %.10g, scatter form %.10g" % (a, b, fd, -r["virial_sum"][c6], r["strain"][c6]))
    print("strain: worst %.3e of %.3e" % (worst / top, top))
    assert top > 1e-3
    assert worst <= 1e-6 * top
    return r


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_strain_derivatives_cubic_box(system, opt):
    _strain_check(system["pos"], system["types"], system["L"], system["nl"], None, PAR, OPTIONS[opt])


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_strain_derivatives_tilted_box(tilted, opt):
    """xy, xz and yz included, in a box that is tilted to begin with"""
    kw = dict(OPTIONS[opt])
    if "average" in kw:
        kw["average"] = (1.0, 1.3)
    if "switch" in kw:
        kw["switch"] = (3.0, 6)
    _strain_check(tilted["pos"], tilted["types"], tilted["L"], tilted["nl"], tilted["tilt"], tilted["par"], kw)


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_gradient_tilted_box(tilted, opt):
    pos, types, L, nl, tilt, par = (tilted[k] for k in ("pos", "types", "L", "nl", "tilt", "par"))
    kw = dict(OPTIONS[opt])
    if "average" in kw:
        kw["average"] = (1.0, 1.3)
    if "switch" in kw:
        kw["switch"] = (3.0, 6)
    r = pel.compute(pos, types, L, nl, *par, tilt=tilt, **kw)
    top = np.abs(r["grad"]).max()
    h, worst = 1e-5, 0.0
    for k in (1, 50, 106):
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[k, a] += h
            m[k, a] -= h
            rp, rm = pel.compute(p, types, L, nl, *par, tilt=tilt, **kw), pel.compute(m, types, L, nl, *par, tilt=tilt, **kw)
            same_side(rp, rm)
            worst = max(worst, abs((rp["cv"] - rm["cv"]) / (2 * h) - r["grad"][k, a]))
    print("%s, tilted: gradient vs central differences: %.3e of max |dCV/dr| %.3e" % (opt, worst / top, top))
    assert top > 1e-4 and worst <= 1e-8 * top


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_forces_add_up_to_zero_and_gather_is_scatter(system, tilted, opt):
    for s, par, tilt in ((system, PAR, None), (tilted, tilted["par"], tilted["tilt"])):
        r = pel.compute(s["pos"], s["types"], s["L"], s["nl"], *par, tilt=tilt, **OPTIONS[opt])
        top = np.abs(r["grad"]).max()
        print("%s: sum of the gradients %.3e, gather - scatter %.3e, of max %.3e" % (opt, np.abs(r["grad"].sum(axis=0)).max(),
                                                                                    np.abs(r["gather"] - r["grad"]).max(), top))
        assert np.abs(r["grad"].sum(axis=0)).max() <= 1e-13 * top * len(s["pos"])
        assert np.abs(r["gather"] - r["grad"]).max() <= 1e-13 * top
        assert np.abs(r["virial_sum"] + r["strain"]).max() <= 1e-13 * np.abs(r["strain"]).max()


def test_isolated_particle_has_the_closed_form(system):
    """a particle with no neighbour inside r_cut: every bin empty, phi = 1, s_i = -2 pi rho Delta sum_b r_b^2 exactly"""
    pos, L = util.fcc_lattice(3)
    L2 = 3.0 * L
    pos = np.vstack([pos, [[0.4 * L2, 0.4 * L2, 0.4 * L2]]])
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L2, 2.4)
    assert nl[1][-1] == 0
    r = pel.compute(pos, types, L2, nl, *PAR)
    c = pe.constants(*PAR[:3])
    want = -2 * np.pi * (len(pos) / L2 ** 3) * c["delta"] * (c["r_b"] ** 2).sum()
    assert r["s"][-1] == pytest.approx(want, rel=1e-15)
    assert np.all(r["W"][-1] == 0.0) and np.all(r["grad"][-1] == 0.0)
    assert np.all(r["s"] <= 0.0) and r["s"][0] < want                 # (ordered neighbours only lower the entropy)


def test_average_that_catches_nothing_is_the_plain_variable(system):
    pos, types, L, nl = (system[k] for k in ("pos", "types", "L", "nl"))
    d_min = min(np.sqrt((d * d).sum()) for d in pe.entries(pos, types, nl, 0, np.inf, L)[2])
    assert d_min > 0.5
    for sw in (None, (4.0, 6)):
        plain = pel.compute(pos, types, L, nl, *PAR, switch=sw)
        avg = pel.compute(pos, types, L, nl, *PAR, switch=sw, average=(0.2, 0.5))
        assert np.all(avg["n"] == 0.0)
        for key in ("s", "sbar", "v", "grad", "gather", "virial"):
            assert np.array_equal(plain[key], avg[key]), key
        assert plain["cv"] == avg["cv"]


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_particles_of_the_other_type_get_zeros(system, opt):
    pos, types, L, nl = (system[k] for k in ("pos", "types", "L", "nl"))
    r = pel.compute(pos, types, L, nl, *PAR, **OPTIONS[opt])
    other = types != 0
    assert 10 < other.sum() < 20 and r["n_t"] == (~other).sum()
    for key in ("s", "sbar", "v", "gamma", "alpha", "X"):
        assert np.all(r[key][other] == 0.0), key
    assert np.all(r["W"][other] == 0.0) and np.all(r["grad"][other] == 0.0) and np.all(r["virial"][other] == 0.0)
    assert np.all(r["s"][~other] < 0.0)
    # and with no particle of the type at all: nothing anywhere
    none = pel.compute(pos, types, L, nl, 2.0, 0.1, 40, 5, **OPTIONS[opt])
    assert none["n_t"] == 0 and none["cv"] == 0.0 and np.all(none["grad"] == 0.0) and np.all(none["virial"] == 0.0)


def test_typical_values(system):
    """the medians the snapshots of the GPU tests give (fcc 5, seed 777): -s_i ~ 3.0 at noise 0.05 and ~ 1.07 at noise 0.13 for B = 40"""
    for noise, want in ((0.05, 3.0), (0.13, 1.07)):
        pos, L = util.fcc_lattice(5)
        pos = pos + np.random.default_rng(777).normal(0, noise, pos.shape)
        types = np.zeros(len(pos), dtype=np.int32)
        r = pel.compute(pos, types, L, util.build_nlist(pos, L, 2.4), *PAR)
        med = float(np.median(-r["s"]))
        nz = r["g"][r["g"] > 0.0]
        print("noise %.2f: median -s_i %.4f, smallest non-zero g %.3e, empty bins %.1f %%" % (noise, med, nz.min(), 100.0 * (r["g"] == 0.0).mean()))
        assert med == pytest.approx(want, rel=0.05)
        assert not np.any((nz > pe.G_MIN / 2.3) & (nz < pe.G_MIN * 2.3))
