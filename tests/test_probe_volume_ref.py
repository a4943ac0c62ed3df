"""CPU: the restatement of the probe-volume variable (tests/probe_volume_ref.py) against what the definition demands of it — the
cumulative's end values, the volume the smoothed indicator keeps, gradient and virial against central differences, continuity across the
shell's edge and the sharp faces, and periodic images.  The GPU tests hold the kernels to this restatement."""
import math

import numpy as np
import pytest

import probe_volume_ref as pv

INF = float("inf")
TILT = dict(xy=0.3, xz=-0.2, yz=0.15)
L_TILT = (17.0, 18.5, 16.25)
COEFF = [1.0, -0.5, 0.0, 0.75]


def regions(centre, tilted=False):
    """tilted: for a box with all three tilt factors, where only an axis along z may be unbounded (the fit rule)"""
    return {
        "slab": pv.region("box", centre, 0.3, w=[INF, INF, 1.5]),
        "box": pv.region("box", centre, 0.3, w=[2.0, 1.25, 1.5]),
        "tiny box": pv.region("box", centre, 0.3, w=[0.25, 0.4, 0.2]),      # w < r_c: both shells of an axis overlap
        "sphere": pv.region("sphere", centre, 0.3, R=2.5),
        "cylinder x": pv.region("cylinder", centre, 0.3, R=2.0, w=1.0, axis=0),
        "cylinder y": pv.region("cylinder", centre, 0.05, R=2.0, w=3.0 if tilted else INF, axis=1),
        "cylinder z": pv.region("cylinder", centre, 0.3, r_c=0.75, R=2.0, w=1.5, axis=2),
    }


def particles(reg, n, seed, spread=4.0):
    """n particles of four types around the region, no further out per axis than `spread` or a little beyond the shell"""
    rng = np.random.default_rng(seed)
    reach = np.minimum(spread, np.array(pv.extents(reg)) + 0.3)
    return reg["centre"] + rng.uniform(-1.0, 1.0, (n, 3)) * reach, rng.integers(0, len(COEFF), n)


@pytest.mark.parametrize("sigma,rc", [(0.05, 0.1), (0.3, 0.6), (0.3, 1.5), (1.0, 0.5)])
def test_cumulative_end_values(sigma, rc):
    assert abs(pv.G(-rc, sigma, rc)) <= 1e-15 and abs(pv.G(rc, sigma, rc) - 1.0) <= 1e-15 and abs(pv.G(0.0, sigma, rc) - 0.5) <= 1e-15
    below, above = math.nextafter(rc, 0.0), math.nextafter(rc, INF)
    assert abs(pv.G(below, sigma, rc) - 1.0) <= 1e-15 and abs(pv.G(-below, sigma, rc)) <= 1e-15    # the formula itself, at the edge
    assert pv.G(above, sigma, rc) == 1.0 and pv.G(-above, sigma, rc) == 0.0
    assert pv.phi(rc, sigma, rc) == 0.0 and abs(pv.phi(below, sigma, rc)) <= 1e-15 * pv.phi(0.0, sigma, rc) * 1e3
    # G' = Phi
    for u in np.linspace(-0.9 * rc, 0.9 * rc, 7):
        fd = (pv.G(u + 1e-6, sigma, rc) - pv.G(u - 1e-6, sigma, rc)) / 2e-6
        assert abs(fd - pv.phi(u, sigma, rc)) <= 1e-7 * pv.phi(0.0, sigma, rc)


@pytest.mark.parametrize("w", [1.5, 0.25])
def test_smoothed_indicator_keeps_the_volume(w):
    """sum_x h(x) delta over a lattice of spacing 2^-8 across a slab is 2 w (Euler-Maclaurin: h and h' vanish at both ends, h'' is bounded)"""
    reg = pv.region("box", [0.0, 0.0, 0.0], 0.3, w=[INF, INF, w])
    delta = 2.0 ** -8
    z = np.arange(-1024, 1025) * delta                                       # [-4, 4]: beyond w + r_c = 2.1
    total = math.fsum(pv.h_grad([0.0, 0.0, x], reg)[0] for x in z) * delta
    assert abs(total - 2.0 * w) <= 1e-9, total


@pytest.mark.parametrize("name", list(regions([0, 0, 0])))
@pytest.mark.parametrize("tilted", [False, True])
def test_gradient_against_central_differences(name, tilted):
    centre = np.array([0.4, -0.3, 0.2])
    reg = regions(centre, tilted)[name]
    L, tilt = (L_TILT, TILT) if tilted else (16.0, None)
    assert pv.fits(reg, L, tilt)
    pos, types = particles(reg, 60, 7)
    pos[:6] += np.array([L if np.isscalar(L) else L[0], 0.0, 0.0])           # some through a periodic image
    r = pv.compute(pos, types, COEFF, reg, L, tilt)
    phi0 = pv.phi(0.0, reg["sigma_s"], reg["r_c"])
    step = 1e-6
    assert np.abs(r["grad"]).max() > 0.1 * phi0
    for i in range(len(pos)):
        for k in range(3):
            p, m = pos.copy(), pos.copy()
            p[i, k] += step
            m[i, k] -= step
            fd = (pv.compute(p[i:i + 1], types[i:i + 1], [1.0] * 4, reg, L, tilt)["s"] - pv.compute(m[i:i + 1], types[i:i + 1], [1.0] * 4, reg, L, tilt)["s"]) / (2 * step)
            assert abs(fd - r["grad"][i, k]) <= 1e-7 * phi0, (i, k, fd, r["grad"][i, k])


def _strained(pos, centre, L, tilt, eps):
    """positions, centre and lattice vectors under r -> (1 + eps) r; the new box as (L, tilt) — eps keeps the lattice matrix triangular"""
    A = pv.lattice(L, **(tilt or {})) @ (np.eye(3) + eps).T
    Ln = np.array([A[0, 0], A[1, 1], A[2, 2]])
    return pos @ (np.eye(3) + eps).T, centre @ (np.eye(3) + eps).T, Ln, dict(xy=A[1, 0] / Ln[1], xz=A[2, 0] / Ln[2], yz=A[2, 1] / Ln[2]), A


@pytest.mark.parametrize("name", ["box", "sphere", "cylinder x", "cylinder z", "slab"])
def test_virial_against_central_differences_of_the_strained_value(name):
    """sum_i virial_i[ab] = -bias (ds/d eps_ab + ds/d eps_ba) / 2 with positions, box and centre strained together.  Upper-triangular
    strains keep HOOMD's box form (a_1 along x, a_2 in the xy plane); the symmetrised derivative needs both eps_ab and eps_ba, and the
    value depends on d alone (all images are strained alike), so the lower ones are taken with the plain minimum image of a cubic box
    that is large against the region."""
    centre = np.array([0.4, -0.3, 0.2])
    reg = regions(centre)[name]
    L = 16.0
    pos, types = particles(reg, 80, 11, spread=3.5)                          # |d| < L / 2 - strain: no image changes under the strain
    bias = -1.7
    r = pv.compute(pos, types, COEFF, reg, L, None, bias=bias)
    a = r["a"]
    step = 1e-6
    phi0 = pv.phi(0.0, reg["sigma_s"], reg["r_c"])
    dsde = np.zeros((3, 3))
    for p in range(3):
        for q in range(3):
            vals = []
            for sign in (1.0, -1.0):
                eps = np.zeros((3, 3))
                eps[p, q] = sign * step
                M = np.eye(3) + eps
                d = (pos - centre) @ M.T                                     # strained displacement, same image
                vals.append(math.fsum(a[i] * pv.h_grad(d[i], reg)[0] for i in range(len(pos))))
            dsde[p, q] = (vals[0] - vals[1]) / (2 * step)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    want = np.array([-bias * 0.5 * (dsde[p, q] + dsde[q, p]) for p, q in pairs])
    got = r["virial"].sum(axis=1)
    scale = abs(bias) * np.abs(a).sum() * phi0 * np.abs(r["d"]).max()
    assert np.abs(got).max() > 1e-3 * scale
    assert np.abs(got - want).max() <= 1e-7 * scale, (got, want)
    # and through the box: an upper-triangular strain of positions, centre AND box gives the same value as the strained displacements
    eps = np.zeros((3, 3))
    eps[0, 1], eps[0, 0], eps[1, 2] = 2e-3, -1e-3, 1.5e-3
    pos_s, centre_s, Ln, tilt_n, _ = _strained(pos, centre, L, None, eps)
    reg_s = dict(reg, centre=centre_s)
    s_box = pv.compute(pos_s + np.array([Ln[0], 0, 0]), types, COEFF, reg_s, Ln, tilt_n)["s"]
    d = (pos - centre) @ (np.eye(3) + eps).T
    s_direct = math.fsum(a[i] * pv.h_grad(d[i], reg)[0] for i in range(len(pos)))
    assert abs(s_box - s_direct) <= 1e-12 * np.abs(a).sum()


@pytest.mark.parametrize("name", list(regions([0, 0, 0])))
def test_continuity_across_the_shell_edge_and_the_sharp_faces(name):
    """h and grad h on the two sides of |u| = r_c and of u = 0, one part in 2^40 apart: they differ by no more than the slope allows"""
    reg = regions(np.zeros(3))[name]
    s, rc = reg["sigma_s"], reg["r_c"]
    phi0 = pv.phi(0.0, s, rc)
    rel = 2.0 ** -40
    if reg["shape"] == "sphere":
        faces = [(np.array([0.6, -0.48, 0.64]), reg["R"])]                   # a unit vector, the face at R along it
    elif reg["shape"] == "box":
        faces = [(np.eye(3)[k] * sg, reg["w"][k]) for k in range(3) if reg["w"][k] != INF for sg in (1.0, -1.0)]
    else:
        ax = reg["axis"]
        perp = np.roll(np.eye(3)[ax], 1) * 0.8 + np.roll(np.eye(3)[ax], 2) * 0.6
        faces = [(perp, reg["R"])] + ([(np.eye(3)[ax] * sg, reg["w"][ax]) for sg in (1.0, -1.0)] if reg["w"][ax] != INF else [])
    checked = 0
    for n, dist in faces:
        for u0 in (0.0, rc, -rc):
            t = dist - u0                                                    # the point at signed distance u0 inside this face
            if t <= 0.0:
                continue
            lo, hi = pv.h_grad(n * t * (1 - rel), reg), pv.h_grad(n * t * (1 + rel), reg)
            step = 2 * t * rel
            assert abs(hi[0] - lo[0]) <= 2 * phi0 * step + 1e-15, (name, n, u0)
            assert np.abs(hi[1] - lo[1]).max() <= 2 * (phi0 / s + phi0 / max(t, s)) * step + 1e-15, (name, n, u0)   # |Phi'| <= Phi(0) / sigma
            checked += 1
    assert checked >= 3


@pytest.mark.parametrize("name", ["box", "sphere", "cylinder z", "slab"])
@pytest.mark.parametrize("tilted", [False, True])
def test_region_across_the_periodic_boundary(name, tilted):
    """the region centred on a corner of the box, particles wrapped into the box: the same as the configuration shifted to the middle"""
    L, tilt = (L_TILT, TILT) if tilted else ((16.0, 16.0, 16.0), None)
    A = pv.lattice(L, **(tilt or {}))
    middle = np.array([0.3, -0.2, 0.1])
    reg0 = regions(middle)[name]
    assert pv.fits(reg0, L, tilt)
    pos0, types = particles(reg0, 200, 3)
    r0 = pv.compute(pos0, types, COEFF, reg0, L, tilt, bias=0.7)
    corner = 0.5 * (A[0] + A[1] + A[2])
    shifted = pos0 - middle + corner
    f = shifted @ np.linalg.inv(A)
    wrapped = (f - np.rint(f)) @ A                                           # back into the box: the region is cut into eight pieces
    assert np.abs(wrapped - shifted).max() > 0.4 * min(L)
    r1 = pv.compute(wrapped, types, COEFF, dict(reg0, centre=corner), L, tilt, bias=0.7)
    assert abs(r1["s"] - r0["s"]) <= 1e-12 * np.abs(r0["a"]).sum() and r1["count"] == r0["count"] and r0["count"] != 0
    assert np.abs(r1["h"] - r0["h"]).max() <= 1e-12 and np.abs(r1["F"] - r0["F"]).max() <= 1e-11
    assert np.abs(r1["virial"] - r0["virial"]).max() <= 1e-10


def test_fit_rule():
    reg = pv.region("box", [0, 0, 0], 0.5, r_c=1.0, w=[7.0, INF, INF])
    assert pv.fits(reg, 16.0) and not pv.fits(dict(reg, w=[7.0 + 1e-9, INF, INF]), 16.0)
    # bounded along z only: every tilt is fine (a_3 alone has a z component and its coordinate is z / Lz)
    slab_z = pv.region("box", [0, 0, 0], 0.5, r_c=1.0, w=[INF, INF, 3.0])
    assert pv.fits(slab_z, L_TILT, TILT)
    # bounded along x only in a box tilted in xy: a_2 has an x component and its coordinate depends on y, which is unbounded
    slab_x = pv.region("box", [0, 0, 0], 0.5, r_c=1.0, w=[3.0, INF, INF])
    assert not pv.fits(slab_x, L_TILT, TILT) and pv.fits(slab_x, L_TILT, dict(xy=0.0, xz=0.0, yz=0.15))
    sphere = pv.region("sphere", [0, 0, 0], 0.5, r_c=1.0, R=4.0)
    assert pv.fits(sphere, L_TILT, TILT) and not pv.fits(dict(sphere, R=6.5), L_TILT, TILT) and pv.fits(dict(sphere, R=6.5), L_TILT, None)
