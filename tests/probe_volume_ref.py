"""fp64 restatement of the probe-volume variable (include/mtd_abi.h "Probe volume"; csrc/probe_volume.hip), straight from the definition:

    s = sum_i a_i h(d_i),  N_v = sum_i a_i [d_i inside],  d_i = min_image(r_i - c)
    Phi(u) = [exp(-u^2 / 2 sigma^2) - exp(-r_c^2 / 2 sigma^2)] / k  (|u| < r_c),  G = its cumulative
    box h = prod [G(w - d) - G(-w - d)];  sphere h = G(R - |d|);  cylinder h = G(R - d_perp) [G(w - d_ax) - G(-w - d_ax)]
    F_i = -bias a_i grad h,  virial_i[ab] = -bias a_i (g_a d_b + g_b d_a) / 2

math.erf and math.exp per particle and face, numpy for the rest.  A region is a dict(shape, centre (Cartesian), sigma_s, r_c, w (three
half-widths, inf: unbounded; cylinder: only w[axis] counts), R, axis).  The minimum image is HOOMD's BoxDim::minImage, restated."""
import math

import numpy as np

INF = float("inf")


def lattice(L, xy=0.0, xz=0.0, yz=0.0):
    """the lattice vectors a_1, a_2, a_3 of a HOOMD box as the rows of a matrix"""
    L = np.full(3, float(L)) if np.isscalar(L) else np.asarray(L, dtype=np.float64)
    return np.array([[L[0], 0.0, 0.0], [xy * L[1], L[1], 0.0], [xz * L[2], yz * L[2], L[2]]])


def region(shape, centre, sigma_s, r_c=None, w=None, R=0.0, axis=0):
    w3 = [INF] * 3
    if shape == "box":
        w3 = [float(x) for x in w]
    elif shape == "cylinder":
        w3[axis] = INF if w is None else float(w)
    return dict(shape=shape, centre=np.asarray(centre, dtype=np.float64), sigma_s=float(sigma_s), r_c=2.0 * sigma_s if r_c is None else float(r_c),
                w=w3, R=float(R), axis=int(axis))


def norm_k(sigma, rc):
    return math.sqrt(2.0 * math.pi) * sigma * math.erf(rc / (math.sqrt(2.0) * sigma)) - 2.0 * rc * math.exp(-rc * rc / (2.0 * sigma * sigma))


def phi(u, sigma, rc):
    if not abs(u) < rc:
        return 0.0
    return (math.exp(-u * u / (2.0 * sigma * sigma)) - math.exp(-rc * rc / (2.0 * sigma * sigma))) / norm_k(sigma, rc)


def G(u, sigma, rc):
    if u <= -rc:
        return 0.0
    if u >= rc:
        return 1.0
    return 0.5 + (math.sqrt(math.pi / 2.0) * sigma * math.erf(u / (math.sqrt(2.0) * sigma)) - u * math.exp(-rc * rc / (2.0 * sigma * sigma))) / norm_k(sigma, rc)


def min_image(d, L, tilt=None):
    """HOOMD BoxDim::minImage of the rows of d"""
    L = np.full(3, float(L)) if np.isscalar(L) else np.asarray(L, dtype=np.float64)
    t = dict(xy=0.0, xz=0.0, yz=0.0)
    t.update(tilt or {})
    d = np.array(d, dtype=np.float64).reshape(-1, 3)
    img = np.rint(d[:, 2] / L[2])
    d[:, 2] -= L[2] * img
    d[:, 1] -= L[2] * t["yz"] * img
    d[:, 0] -= L[2] * t["xz"] * img
    img = np.rint(d[:, 1] / L[1])
    d[:, 1] -= L[1] * img
    d[:, 0] -= L[1] * t["xy"] * img
    d[:, 0] -= L[0] * np.rint(d[:, 0] / L[0])
    return d


def _axis(w, d, s, rc):
    """f, df/dd, inside of one axis of a box"""
    if w == INF:
        return 1.0, 0.0, True
    return G(w - d, s, rc) - G(-w - d, s, rc), phi(-w - d, s, rc) - phi(w - d, s, rc), -w <= d < w


def h_grad(d, reg):
    """h, grad h (with respect to d) and [inside] of ONE displacement d (already the minimum image)"""
    s, rc, shape = reg["sigma_s"], reg["r_c"], reg["shape"]
    if shape == "box":
        f, e, inside = zip(*(_axis(reg["w"][k], d[k], s, rc) for k in range(3)))
        g = [e[0] * f[1] * f[2], e[1] * f[0] * f[2], e[2] * f[0] * f[1]]
        return f[0] * f[1] * f[2], np.array(g), all(inside)
    if shape == "sphere":
        r = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        p = phi(reg["R"] - r, s, rc)
        g = -p * np.asarray(d) / r if r > 0.0 else np.zeros(3)
        return G(reg["R"] - r, s, rc), g, r < reg["R"]
    ax = reg["axis"]
    perp = [k for k in range(3) if k != ax]
    r = math.sqrt(d[perp[0]] ** 2 + d[perp[1]] ** 2)
    Gr, Pr = G(reg["R"] - r, s, rc), phi(reg["R"] - r, s, rc)
    fa, ea, ia = _axis(reg["w"][ax], d[ax], s, rc)
    g = np.zeros(3)
    if r > 0.0:
        for k in perp:
            g[k] = -Pr * d[k] / r * fa
    g[ax] = Gr * ea
    return Gr * fa, g, (r < reg["R"]) and ia


def compute(pos, types, coeff, reg, L, tilt=None, bias=1.0):
    """dict(s, count, h[N], a[N], d[N, 3], grad[N, 3], inside[N], F[N, 3], virial[6, N]); the sums with math.fsum"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    a = np.asarray(coeff, dtype=np.float64)[np.asarray(types, dtype=np.int64)] if len(pos) else np.zeros(0)
    d = min_image(pos - reg["centre"], L, tilt)
    N = len(pos)
    h, g, inside = np.zeros(N), np.zeros((N, 3)), np.zeros(N, dtype=bool)
    for i in range(N):
        h[i], g[i], inside[i] = h_grad(d[i], reg)
    F = -bias * a[:, None] * g
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    virial = np.array([0.5 * (F[:, p] * d[:, q] + F[:, q] * d[:, p]) for p, q in pairs]).reshape(6, N)
    return dict(s=math.fsum(a * h), count=math.fsum(a[inside]), h=h, a=a, d=d, grad=g, inside=inside, F=F, virial=virial)


def value(pos, types, coeff, reg, L, tilt=None):
    return compute(pos, types, coeff, reg, L, tilt)["s"]


def extents(reg):
    """e[3]: w + r_c or R + r_c on the bounded lab axes, inf on the others"""
    rc = reg["r_c"]
    if reg["shape"] == "box":
        return [w + rc for w in reg["w"]]
    e = [reg["R"] + rc] * 3
    if reg["shape"] == "cylinder":
        e[reg["axis"]] = reg["w"][reg["axis"]] + rc
    return e


def fits(reg, L, tilt=None):
    """the fit rule of include/mtd_abi.h"""
    L = np.full(3, float(L)) if np.isscalar(L) else np.asarray(L, dtype=np.float64)
    e = extents(reg)
    if not tilt or not any(tilt.values()):
        return all(e[k] == INF or e[k] <= 0.5 * L[k] for k in range(3))
    A = lattice(L, **tilt)
    xy, xz, yz = (tilt.get(k, 0.0) for k in ("xy", "xz", "yz"))
    # row i: b_i' . a_j = delta_ij, in closed form (the zeros are exact zeros)
    B = np.array([[1.0 / L[0], -xy / L[0], (xy * yz - xz) / L[0]], [0.0, 1.0 / L[1], -yz / L[1]], [0.0, 0.0, 1.0 / L[2]]])
    for i in range(3):
        if not any(e[k] != INF and A[i, k] != 0.0 for k in range(3)):
            continue
        if any(e[k] == INF and B[i, k] != 0.0 for k in range(3)):
            return False
        if sum(abs(B[i, k]) * e[k] for k in range(3) if e[k] != INF) > 0.5 * (1.0 + 1e-12):
            return False
    return True
