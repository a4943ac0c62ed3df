"""CPU: the numpy restatement of the bond-orientational order (tests/hexatic_ref.py) that the GPU tests compare against is itself checked
here: the known answers (triangular monolayer with k = 6 and k = 3, fcc with k = 4 about each of the three axes), the three axes on
cyclically permuted coordinates, the in-plane rotation of an isolated clump, its analytic gradient against central differences of its
value in every coordinate of a sample of particles and its virial against differences of the value under strained positions and box
(cubic and tilted; both modes, switch + gate, k = 1, 4, 6), the sum of the forces, a bond exactly along the axis, and a centre whose
coordination lies below MTD_HEX_N_MIN."""
import numpy as np
import pytest

import hexatic_ref as hr
import util

R_ON, R_CUT = 0.9, 1.3
OPTIONS = {
    "k=6": dict(k=6),
    "k=4": dict(k=4),
    "k=1": dict(k=1),
    "k=6 switch+gate": dict(k=6, switch=(0.05, 2), gate=(5.0, 9.0)),
    "k=4 switch+gate": dict(k=4, switch=(0.05, 2), gate=(5.0, 9.0)),
    "k=6 global": dict(k=6, global_order=True),
    "k=4 global": dict(k=4, global_order=True),
    "k=1 global": dict(k=1, global_order=True),
    "k=4 about x": dict(k=4, axis="x"),
    "k=6 global about y": dict(k=6, axis="y", global_order=True),
}
TILT = dict(xy=0.15, xz=-0.1, yz=0.2)
PERMUTED = {"z": [0, 1, 2], "x": [1, 2, 0], "y": [2, 0, 1]}              # where old (x, y, z) go: the plane (x, y) becomes the axis' (u, v)


def tilted(pos, L, tilt):
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    return (pos / L) @ h.T, h


@pytest.fixture(scope="module")
def boxes():
    """noisy fcc 3^3 (108 particles, every fifth of another type: bonds in and out of every plane) in the cubic box and sheared into a
    tilted one, the list beyond r_cut"""
    pos, L = util.fcc_lattice(3)
    pos = pos + np.random.default_rng(5).normal(0, 0.05, pos.shape)
    types = (np.arange(len(pos)) % 5 == 0).astype(np.int32)
    out = {"cubic": dict(pos=pos, L=L, types=types, tilt=None, h=np.diag([L, L, L]), nl=util.build_nlist(pos, L, R_CUT + 0.05))}
    p2, h = tilted(pos, L, TILT)
    out["tilted"] = dict(pos=p2, L=L, types=types, tilt=TILT, h=h, nl=hr.brute_nlist(p2, h, R_CUT + 0.05))
    return out


@pytest.mark.parametrize("phi0", [0.0, 0.3, np.pi / 6])
def test_triangular_monolayer(phi0):
    """k = 6: c_i = 1 and |Psi|^2 = 1 whatever the in-plane orientation of the lattice (arg psi = 6 phi0); k = 3: 0"""
    pos, L = hr.triangular_layer(8, 8)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = hr.box_nlist(pos, L, 1.2)
    assert np.all(nl[1] == 6)
    if phi0:
        # the periodic box does not rotate: the rotated copy is isolated, and the interior particles keep their six bonds
        pos = hr.triangular_layer(8, 8, phi0=phi0)[0]
        L = np.array([40.0, 40.0, 4.0])
        nl = hr.box_nlist(pos, L, 1.2)
    full = nl[1] == 6
    assert full.sum() >= 36
    for glob in (False, True):
        res = hr.compute(pos, types, L, nl, hr.params(0, 1.2, 1.1, k=6, global_order=glob))
        assert np.abs(res["local"][full] - 1.0).max() <= 1e-13
        assert np.abs(res["psi"][full] - np.exp(6j * phi0)).max() <= 1e-13
        if not phi0:
            assert res["s"] == pytest.approx(1.0, abs=1e-13) and abs(res["Psi"] - 1.0) <= 1e-13
            assert np.abs(res["grad"]).max() <= 1e-13
        res = hr.compute(pos, types, L, nl, hr.params(0, 1.2, 1.1, k=3, global_order=glob))
        assert np.abs(res["local"][full]).max() <= 1e-13
        if not phi0:
            assert abs(res["s"]) <= 1e-13


def test_fcc_about_each_axis():
    """first shell inside r_on, k = 4: psi_i = (4 (-1) + 8 (1/4) (+1)) / 12 = -1/6, s = 1/36 in both modes, about x, y and z"""
    pos, L = util.fcc_lattice(3)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.25)
    for axis in "xyz":
        for glob in (False, True):
            res = hr.compute(pos, types, L, nl, hr.params(0, 1.25, 1.1, k=4, axis=axis, global_order=glob))
            print("fcc about %s, global %d: psi_0 %r, s %.15f (1/36 = %.15f)" % (axis, glob, res["psi"][0], res["s"], 1.0 / 36.0))
            assert np.abs(res["psi"] + 1.0 / 6.0).max() <= 1e-14 and np.all(res["coordination"] == 12.0)
            assert res["s"] == pytest.approx(1.0 / 36.0, abs=1e-14) and abs(res["Psi"] + 1.0 / 6.0) <= 1e-14
            assert np.abs(res["grad"]).max() <= 1e-13
            assert res["sums"][1] == len(pos) and res["sums"][2] == pytest.approx(-len(pos) / 6.0, abs=1e-11)


@pytest.mark.parametrize("name", ["k=6", "k=4 switch+gate", "k=1 global"])
def test_axes_on_permuted_coordinates(boxes, name):
    """the variable about x (y) on cyclically permuted coordinates is the variable about z: the same numbers, the gradient permuted"""
    b = boxes["cubic"]
    opt = dict(OPTIONS[name])
    ref = hr.compute(b["pos"], b["types"], b["L"], b["nl"], hr.params(0, R_CUT, R_ON, axis="z", **opt))
    assert np.abs(ref["grad"]).max() > 0
    for axis in "xy":
        perm = PERMUTED[axis]
        new = np.empty_like(b["pos"])
        new[:, perm] = b["pos"]                                          # new[:, perm[a]] = old[:, a]: old x -> the axis' u, old y -> its v
        res = hr.compute(new, b["types"], b["L"], b["nl"], hr.params(0, R_CUT, R_ON, axis=axis, **opt))
        assert res["s"] == pytest.approx(ref["s"], rel=1e-13)
        assert np.abs(res["psi"] - ref["psi"]).max() <= 1e-14 and np.abs(res["switched"] - ref["switched"]).max() <= 1e-14
        assert np.abs(res["grad"][:, perm] - ref["grad"]).max() <= 1e-13 * np.abs(ref["grad"]).max()


@pytest.mark.parametrize("k", [1, 4, 6])
def test_in_plane_rotation_of_a_clump(k):
    """an isolated clump rotated by phi about the axis: |psi_i|^2 unchanged, arg psi_i shifted by k phi"""
    rng = np.random.default_rng(2)
    pos = rng.uniform(-1.2, 1.2, size=(30, 3)) * np.array([1.0, 1.0, 0.3])
    types = np.zeros(len(pos), dtype=np.int32)
    L, phi = 40.0, 0.37
    par = hr.params(0, 1.3, 0.9, k=k)
    a = hr.compute(pos, types, L, util.build_nlist(pos, L, 1.3), par)
    cs, sn = np.cos(phi), np.sin(phi)
    rot = pos @ np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]]).T
    b = hr.compute(rot, types, L, util.build_nlist(rot, L, 1.3), par)
    assert (a["coordination"] > 0.5).sum() >= 20 and np.abs(a["psi"]).max() > 0.1
    assert np.abs(b["local"] - a["local"]).max() <= 1e-13
    assert np.abs(b["psi"] - a["psi"] * np.exp(1j * k * phi)).max() <= 1e-13
    assert b["s"] == pytest.approx(a["s"], rel=1e-12)


@pytest.mark.parametrize("box", ["cubic", "tilted"])
@pytest.mark.parametrize("name", list(OPTIONS))
def test_gradient_against_central_differences(boxes, box, name):
    b = boxes[box]
    par = hr.params(0, R_CUT, R_ON, **OPTIONS[name])
    res = hr.compute(b["pos"], b["types"], b["L"], b["nl"], par, tilt=b["tilt"])
    top = np.abs(res["grad"]).max()
    assert top > 1e-6 and res["n_t"] == 86
    h, worst = 1e-5, 0.0
    for k in (1, 7, 22, 38, 63, 5):                                      # (5: of the other type; its gradient is exactly 0)
        for a in range(3):
            p, m = b["pos"].copy(), b["pos"].copy()
            p[k, a] += h
            m[k, a] -= h
            fd = (hr.value(p, b["types"], b["L"], b["nl"], par, tilt=b["tilt"]) - hr.value(m, b["types"], b["L"], b["nl"], par, tilt=b["tilt"])) / (2 * h)
            worst = max(worst, abs(fd - res["grad"][k, a]))
    print("%s, %s: gradient vs central differences %.3e of max |ds/dr| %.3e" % (box, name, worst / top, top))
    assert worst <= 1e-7 * top                                           # rounding of a value of order 1 over 2 h, O(h^2) of the window
    assert np.all(res["grad"][b["types"] != 0] == 0.0)
    # no net force; the single terms are NOT parallel to d, and there IS a net torque: the variable selects the axis
    d = res["grad"]
    assert np.abs(d.sum(axis=0)).max() <= 1e-13 * top * len(d)
    e = res["entries"]
    assert np.abs(np.cross(e["d"], e["g"])).max() > 1e-3 * np.abs(e["g"]).max()


@pytest.mark.parametrize("box", ["cubic", "tilted"])
@pytest.mark.parametrize("name", list(OPTIONS))
def test_strain_derivatives(boxes, box, name):
    """the six derivatives of s under x_a -> x_a + eps x_b of positions and box, against -virial_sum / bias; the tensor is not symmetric,
    so the six stored components are the upper triangle and nothing else"""
    b = boxes[box]
    par = hr.params(0, R_CUT, R_ON, **OPTIONS[name])
    res = hr.compute(b["pos"], b["types"], b["L"], b["nl"], par, tilt=b["tilt"], bias=1.0)
    e, worst = 1e-6, 0.0
    top = np.abs(res["virial_sum"]).max()
    for c6, (x, y) in enumerate(hr.PAIRS6):
        vals = []
        for sgn in (1.0, -1.0):
            # an upper-triangular strain keeps the cell in HOOMD's form: eps_xy with x <= y moves x_x by eps x_y
            F = np.eye(3)
            F[x, y] += sgn * e
            h2 = F @ b["h"]
            L2 = np.array([h2[0, 0], h2[1, 1], h2[2, 2]])
            t2 = dict(xy=h2[0, 1] / L2[1], xz=h2[0, 2] / L2[2], yz=h2[1, 2] / L2[2])
            vals.append(hr.value(b["pos"] @ F.T, b["types"], L2, b["nl"], par, tilt=t2))
        fd = (vals[0] - vals[1]) / (2 * e)
        worst = max(worst, abs(fd + res["virial_sum"][c6]))
        print("%s, %s, eps_%d%d: difference %.10g, -virial sum %.10g" % (box, name, x, y, fd, -res["virial_sum"][c6]))
    assert top > 1e-6
    assert worst <= 1e-6 * top
    assert np.all(res["virial"][b["types"] != 0] == 0.0)


@pytest.mark.parametrize("k", [2, 4, 6])
def test_bond_along_the_axis(k):
    """a pair exactly along the axis: B = 0 for k >= 2, an ordinary point — psi = 0, finite (zero) gradient; with a third particle in
    the plane the pair's gradient is finite and agrees with differences"""
    for axis, e in (("z", [0, 0, 1.0]), ("x", [1.0, 0, 0]), ("y", [0, 1.0, 0])):
        pos = np.array([[0.0, 0.0, 0.0], e])
        types = np.zeros(2, dtype=np.int32)
        nl = util.build_nlist(pos, 20.0, 1.3)
        for glob in (False, True):
            res = hr.compute(pos, types, 20.0, nl, hr.params(0, 1.3, 0.9, k=k, axis=axis, global_order=glob))
            assert np.all(res["psi"] == 0.0) and res["s"] == 0.0 and np.all(res["coordination"] > 0.5)
            assert np.isfinite(res["grad"]).all() and np.all(res["grad"] == 0.0) and np.all(res["virial"] == 0.0)
    pos = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.95, 0.2, 0.1]])
    types = np.zeros(3, dtype=np.int32)
    nl = util.build_nlist(pos, 20.0, 1.3)
    par = hr.params(0, 1.3, 0.9, k=k)
    res = hr.compute(pos, types, 20.0, nl, par)
    assert np.isfinite(res["grad"]).all() and np.abs(res["grad"]).max() > 1e-3
    h, worst = 1e-6, 0.0
    for p_i in range(3):
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[p_i, a] += h
            m[p_i, a] -= h
            worst = max(worst, abs((hr.value(p, types, 20.0, nl, par) - hr.value(m, types, 20.0, nl, par)) / (2 * h) - res["grad"][p_i, a]))
    assert worst <= 1e-7 * np.abs(res["grad"]).max()


def test_coordination_below_n_min():
    """a centre whose only neighbour has f < 1e-12 (1e-7 inside the end of the window: f ~ (pi x)^2 / 4): psi, c, v and every
    gradient are exactly 0, in both modes and with options; a lone particle and a particle of another type likewise"""
    r_cut, r_on = 1.3, 0.9
    pos = np.array([[0.0, 0.0, 0.0], [r_cut - 1e-7 * (r_cut - r_on), 0.0, 0.0], [0.0, 6.0, 0.0], [6.0, 6.0, 0.0], [6.5, 6.5, 0.0]])
    types = np.array([0, 0, 0, 0, 1], dtype=np.int32)
    nl = util.build_nlist(pos, 20.0, r_cut)
    assert list(nl[1]) == [1, 1, 0, 1, 1]
    for opt in (dict(), dict(switch=(0.3, 2), gate=(0.0, 2.0)), dict(global_order=True)):
        res = hr.compute(pos, types, 20.0, nl, hr.params(0, r_cut, r_on, k=6, **opt))
        assert 0.0 < res["coordination"][0] < hr.N_MIN and res["n_t"] == 4
        assert np.all(res["psi"] == 0.0) and np.all(res["local"] == 0.0) and np.all(res["switched"] == 0.0) and res["s"] == 0.0
        assert np.all(res["grad"] == 0.0) and np.all(res["virial"] == 0.0)
