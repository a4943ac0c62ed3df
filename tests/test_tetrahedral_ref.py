"""CPU: the numpy restatement of the tetrahedral order (tests/tetrahedral_ref.py) that the GPU tests compare against is itself checked here:
its pair sum against the moment form, its analytic gradient against central differences of its value in every coordinate of a sample of
particles, its virial against differences of the value under strained positions and box (cubic and tilted), for the six option sets;
the lattice values (diamond 1, fcc 3/11); particles with no or one neighbour; the sum and the torque of the forces; and, with a gate, a
particle whose coordination lies just above n_lo."""
import numpy as np
import pytest

import tetrahedral_ref as tr
import util

R_ON, R_CUT = 0.9, 1.3
OPTIONS = {
    "plain": dict(),
    "switch": dict(switch=(0.6, 6)),
    "gate": dict(gate=(1.5, 3.5)),
    "switch+gate": dict(switch=(0.6, 6), gate=(1.5, 3.5)),
    "penalty": dict(normalise=False),
    "cos0=0": dict(cos0=0.0),
}


def noisy_diamond(n=2, sigma=0.05, seed=5):
    pos, L = tr.diamond_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


def tilted(pos, L, tilt):
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    return (pos / L) @ h.T, h


TILT = dict(xy=0.15, xz=-0.1, yz=0.2)


@pytest.fixture(scope="module")
def boxes():
    """noisy diamond 2^3 (64 particles, two interleaved types) in the cubic box and sheared into a tilted one, the list beyond r_cut"""
    pos, L = noisy_diamond()
    types = (np.arange(len(pos)) % 5 == 0).astype(np.int32)
    out = {"cubic": dict(pos=pos, L=L, types=types, tilt=None, h=np.diag([L, L, L]), nl=util.build_nlist(pos, L, R_CUT + 0.05))}
    p2, h = tilted(pos, L, TILT)
    out["tilted"] = dict(pos=p2, L=L, types=types, tilt=TILT, h=h, nl=tr.brute_nlist(p2, h, R_CUT + 0.05))
    return out


def test_pair_sum_equals_the_moment_form():
    rng = np.random.default_rng(1)
    par = tr.params(0, 1.5, 1.0)
    d = rng.normal(size=(9, 3))
    d *= (rng.uniform(0.7, 1.45, 9) / np.sqrt((d * d).sum(axis=1)))[:, None]
    r = np.sqrt((d * d).sum(axis=1))
    assert (r < 1.0).any() and (r > 1.0).any()                         # the row crosses the window
    pos = np.concatenate([np.zeros((1, 3)), d])
    nl = (np.array([0] + [9] * 9), np.array([9] + [0] * 9), np.arange(1, 10))
    for cos0 in (-1.0 / 3.0, 0.0, 0.4):
        par["cos0"] = cos0
        res = tr.compute(pos, np.zeros(10, dtype=np.int32), 40.0, nl, par)
        A_m, W_m = tr.moment_form(d, r, par)
        A_p = (1.0 - res["local"][0]) * res["W"][0] * (1.0 / 3.0 + cos0 * cos0)
        print("cos0 %.3f: W %.15g vs %.15g, A %.15g vs %.15g" % (cos0, res["W"][0], W_m, A_p, A_m))
        assert res["W"][0] == pytest.approx(W_m, rel=1e-14) and A_p == pytest.approx(A_m, rel=1e-13)
        pen = tr.compute(pos, np.zeros(10, dtype=np.int32), 40.0, nl, dict(par, normalise=False))
        assert pen["local"][0] == pytest.approx(A_m, rel=1e-14)


@pytest.mark.parametrize("box", ["cubic", "tilted"])
@pytest.mark.parametrize("name", list(OPTIONS))
def test_gradient_against_central_differences(boxes, box, name):
    b = boxes[box]
    par = tr.params(0, R_CUT, R_ON, **OPTIONS[name])
    res = tr.compute(b["pos"], b["types"], b["L"], b["nl"], par, tilt=b["tilt"])
    top = np.abs(res["grad"]).max()
    assert top > 1e-4 and res["n_t"] == 51
    h, worst = 1e-5, 0.0
    for k in (1, 7, 22, 38, 63, 5):                                      # (5: of the other type; its gradient is exactly 0)
        for a in range(3):
            p, m = b["pos"].copy(), b["pos"].copy()
            p[k, a] += h
            m[k, a] -= h
            fd = (tr.value(p, b["types"], b["L"], b["nl"], par, tilt=b["tilt"]) - tr.value(m, b["types"], b["L"], b["nl"], par, tilt=b["tilt"])) / (2 * h)
            worst = max(worst, abs(fd - res["grad"][k, a]))
    print("%s, %s: gradient vs central differences %.3e of max |ds/dr| %.3e" % (box, name, worst / top, top))
    assert worst <= 1e-7 * top                                           # rounding of a value of order 1 over 2 h, O(h^2) of the window
    assert np.all(res["grad"][b["types"] != 0] == 0.0)
    # no net force, no net torque (the pair term is not parallel to d: the torque is a statement of its own)
    d = res["grad"]
    assert np.abs(d.sum(axis=0)).max() <= 1e-13 * top * len(d)
    # every entry gives +g to one end and -g to the other, a lever arm d apart: the torque is sum_e d_e x g_e
    e = res["entries"]
    torque = np.cross(e["d"], e["g"]).sum(axis=0)
    scale = (np.sqrt((e["d"] ** 2).sum(axis=1)) * np.sqrt((e["g"] ** 2).sum(axis=1))).sum()
    print("%s, %s: torque %.3e of sum |d| |g| %.3e" % (box, name, np.abs(torque).max(), scale))
    assert scale > 0 and np.abs(torque).max() <= 1e-13 * scale
    assert np.abs(np.cross(e["d"], e["g"])).max() > 1e-3 * np.abs(e["g"]).max()      # (the single terms are NOT parallel to d)


@pytest.mark.parametrize("box", ["cubic", "tilted"])
@pytest.mark.parametrize("name", list(OPTIONS))
def test_strain_derivatives(boxes, box, name):
    """the six derivatives of s under x -> (1 + eps) x of positions and box, against -virial_sum / bias"""
    b = boxes[box]
    par = tr.params(0, R_CUT, R_ON, **OPTIONS[name])
    res = tr.compute(b["pos"], b["types"], b["L"], b["nl"], par, tilt=b["tilt"], bias=1.0)
    e, worst = 1e-6, 0.0
    top = np.abs(res["virial_sum"]).max()
    for c6, (x, y) in enumerate(tr.PAIRS6):
        vals = []
        for sgn in (1.0, -1.0):
            # an upper-triangular strain keeps the cell in HOOMD's form: eps_xy with x <= y moves x_x by eps x_y
            F = np.eye(3)
            F[x, y] += sgn * e
            h2 = F @ b["h"]
            L2 = np.array([h2[0, 0], h2[1, 1], h2[2, 2]])
            t2 = dict(xy=h2[0, 1] / L2[1], xz=h2[0, 2] / L2[2], yz=h2[1, 2] / L2[2])
            vals.append(tr.value(b["pos"] @ F.T, b["types"], L2, b["nl"], par, tilt=t2))
        fd = (vals[0] - vals[1]) / (2 * e)
        worst = max(worst, abs(fd + res["virial_sum"][c6]))
        print("%s, %s, eps_%d%d: difference %.10g, -virial sum %.10g" % (box, name, x, y, fd, -res["virial_sum"][c6]))
    assert top > 1e-3
    assert worst <= 1e-6 * top
    # the per-particle rows add up to the sum, and a particle of the other type has none
    assert np.all(res["virial"][b["types"] != 0] == 0.0)


def test_perfect_diamond_and_fcc():
    """diamond with the first shell inside r_on: t_i = 1, A_i = 0, n_i = 4; fcc: t_i = 3/11, n_i = 12; no gradient on either"""
    pos, L = tr.diamond_lattice(2)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.3)
    res = tr.compute(pos, types, L, nl, tr.params(0, 1.3, 1.1))
    assert np.abs(res["local"] - 1.0).max() <= 1e-14 and np.abs(res["coordination"] - 4.0).max() == 0.0 and res["s"] == pytest.approx(1.0, abs=1e-14)
    assert np.abs(res["grad"]).max() <= 1e-13
    pen = tr.compute(pos, types, L, nl, tr.params(0, 1.3, 1.1, normalise=False))
    assert np.abs(pen["local"]).max() <= 1e-14 and np.abs(pen["grad"]).max() <= 1e-13
    pos, L = util.fcc_lattice(3)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.25)
    res = tr.compute(pos, types, L, nl, tr.params(0, 1.25, 1.1))
    print("fcc: t %.15f (3/11 = %.15f)" % (res["local"][0], 3.0 / 11.0))
    assert np.abs(res["local"] - 3.0 / 11.0).max() <= 1e-14 and np.abs(res["coordination"] - 12.0).max() == 0.0
    assert np.abs(res["grad"]).max() <= 1e-13
    # the four diamond vectors and the twelve fcc vectors through the moment form
    tet = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) / np.sqrt(3.0)
    A, W = tr.moment_form(tet, np.ones(4), tr.params(0, 1.3, 1.1))
    assert abs(A) <= 1e-14 and W == 6.0                                 # (terms of size n^2 = 16 cancel: a few of their ulps, 3.6e-15 each)
    fcc = np.array([[a, b, 0] for a in (1, -1) for b in (1, -1)] + [[a, 0, b] for a in (1, -1) for b in (1, -1)]
                   + [[0, a, b] for a in (1, -1) for b in (1, -1)], dtype=np.float64) / np.sqrt(2.0)
    A, W = tr.moment_form(fcc, np.ones(12), tr.params(0, 1.3, 1.1))
    assert 1.0 - 2.25 * A / W == pytest.approx(3.0 / 11.0, abs=1e-15)


def test_no_or_one_neighbour():
    """a lone particle, a dimer and a particle of the other type: t_i = 0, v_i = 0, F = 0, with every option set"""
    pos = np.array([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0], [5.7, 0.6, 0.2], [0.0, 5.0, 0.0], [0.5, 5.5, 0.0], [0.0, 5.0, 0.9]])
    types = np.array([0, 0, 0, 0, 1, 0], dtype=np.int32)
    L = 20.0
    nl = util.build_nlist(pos, L, 1.4)
    assert list(nl[1]) == [0, 1, 1, 2, 2, 2]
    for name, opt in OPTIONS.items():
        res = tr.compute(pos, types, L, nl, tr.params(0, R_CUT, R_ON, **opt))
        assert np.all(res["local"] == 0.0) and np.all(res["switched"] == 0.0) and res["s"] == 0.0, name
        assert np.all(res["grad"] == 0.0) and np.all(res["virial"] == 0.0), name
        assert res["n_t"] == 5 and res["coordination"][0] == 0.0 and 0.0 < res["coordination"][1] <= 1.0
        assert res["coordination"][3] == res["coordination"][5] and res["coordination"][4] == 0.0     # (the other type is no neighbour)


def test_gate_just_above_n_lo():
    """particle 0 has one neighbour inside r_on and a second one at the outer edge of the window: n_0 = 1 + 4e-3, W_0 = 4e-3.  Without a
    gate its gradient does not vanish with the weight of the second neighbour; with the gate (n_lo = 1) it is finite, small and agrees with differences"""
    par0 = tr.params(0, 1.5, 1.0)
    out = np.array([np.cos(2.0), np.sin(2.0), 0.0])
    pos = np.array([[0.0, 0.0, 0.0], [0.8, 0.0, 0.0], 1.48 * out, [0.1, -0.9, 0.3], [-0.7, -0.5, -0.6], [0.3, 0.2, 1.1]])
    types = np.zeros(len(pos), dtype=np.int32)
    L = 30.0
    # rows by hand: particle 0 lists 1 and 2 only, everybody lists particle 0 back where it is in reach; 3, 4, 5 give the others full rows
    rows = [[1, 2], [0, 3, 4, 5], [0, 3, 4, 5], [1, 2, 4, 5], [1, 2, 3, 5], [1, 2, 3, 4]]
    import list_layouts as ll
    nl = ll.from_rows([np.array(x) for x in rows])
    plain = tr.compute(pos, types, L, nl, par0)
    assert 1.0 < plain["coordination"][0] < 1.01 and 0.0 < plain["W"][0] < 1e-2
    gated = tr.params(0, 1.5, 1.0, gate=(1.0, 3.0))
    res = tr.compute(pos, types, L, nl, gated)
    assert np.isfinite(res["grad"]).all()
    h, worst = 1e-6, 0.0
    for k in range(3):
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[k, a] += h
            m[k, a] -= h
            fd = (tr.value(p, types, L, nl, gated) - tr.value(m, types, L, nl, gated)) / (2 * h)
            worst = max(worst, abs(fd - res["grad"][k, a]))
    top = np.abs(res["grad"]).max()
    print("gate just above n_lo: n_0 %.6f, W_0 %.3e, v_0 %.3e; gradient vs differences %.3e of %.3e" % (
        res["coordination"][0], res["W"][0], res["switched"][0], worst, top))
    assert worst <= 1e-7 * top
    # what the gate removes: with two neighbours t_0 depends on their angle alone, so the ungated dv_0/dr_2 does not vanish with f_02
    # (4e-3 here); the gated one carries g ~ 3 y^2 and g' ~ 3 y, y = (n_0 - 1) / 2 = 2e-3
    big = np.abs(_grad_of_particle0(pos, types, L, nl, par0)).max()
    small = np.abs(_grad_of_particle0(pos, types, L, nl, gated)).max()
    print("|dv_0/dr_2|: %.3e without a gate, %.3e with it" % (big, small))
    assert big > 0.1 and small < 0.05 * big


def _grad_of_particle0(pos, types, L, nl, par):
    """dv_0 / dr_2 by central differences of v_0"""
    h = 1e-7
    out = np.zeros(3)
    for a in range(3):
        p, m = pos.copy(), pos.copy()
        p[2, a] += h
        m[2, a] -= h
        out[a] = (tr.compute(p, types, L, nl, par)["switched"][0] - tr.compute(m, types, L, nl, par)["switched"][0]) / (2 * h)
    return out
