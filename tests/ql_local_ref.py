"""fp64 numpy restatement of the local Steinhardt variable (cv.steinhardt_local, include/mtd_abi.h "Local Steinhardt bond order"),
vectorised over the pairs of the list, with an ANALYTIC gradient in the scatter form (every pair gives +G to its centre and -G to
its neighbour) — independent of the gather form the GPU pass uses.  Harmonics: scipy.special.sph_harm_y (Condon-Shortley phase).

    n_i = sum_j f,  A_lm(i) = sum_j f Y_lm(d_ij),  q_l^2(i) = 4 pi/(2l+1) sum_m |A_lm(i)|^2 / n_i^2,
    c_i = sum_l Ql_ref[l] q_l^2(i),  s = sum_i c_i / N_global,  F = -bias ds/dr

`frame` (a proper rotation Q, util.random_rotation): the pair vectors are rotated after the minimum image (d @ Q.T), everything angular is
done in that frame and the per-pair gradients are rotated back (G @ Q).  The variable is rotation invariant, so nothing changes — but
the spherical components below divide by sin(theta), and a bond on the z axis of the box (a column of a cubic crystal) is generic in
the rotated frame.  frame=None is the lab frame, with its NaN on the axis.
"""
import numpy as np
from scipy.special import sph_harm_y


def box_matrix(L, xy=0.0, xz=0.0, yz=0.0):
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    return L, float(xy), float(xz), float(yz)


def min_image(d, L, xy=0.0, xz=0.0, yz=0.0):
    """HOOMD BoxDim::minImage for a periodic (triclinic) box; d: (n, 3)"""
    L, xy, xz, yz = box_matrix(L, xy, xz, yz)
    d = np.array(d, dtype=np.float64)
    img = np.rint(d[:, 2] / L[2])
    d[:, 2] -= L[2] * img
    d[:, 1] -= L[2] * yz * img
    d[:, 0] -= L[2] * xz * img
    img = np.rint(d[:, 1] / L[1])
    d[:, 1] -= L[1] * img
    d[:, 0] -= L[1] * xy * img
    d[:, 0] -= L[0] * np.rint(d[:, 0] / L[0])
    return d


def smoothing(r, r_on, r_cut):
    """SteinhardtQl.cc:36-60: f and df/dr"""
    x = (r - r_on) / (r_cut - r_on)
    inside = r > r_on
    f = np.where(inside, 0.5 * (np.cos(np.pi * x) + 1.0), 1.0)
    df = np.where(inside, -0.5 * np.pi / (r_cut - r_on) * np.sin(np.pi * x), 0.0)
    return f, df


def pairs(pos, types, nl, type_id, r_cut, tilt=None, L=None, rows=None):
    """(i, j, d) of the list entries that take part: both of `type_id`, r^2 <= r_cut^2; rows: only these central particles"""
    head, nn, lst = (np.asarray(a).astype(np.int64) for a in nl)
    n_rows = len(head)
    i = np.repeat(np.arange(n_rows), nn)
    first = np.repeat(head, nn)
    k = np.arange(len(i)) - np.repeat(np.cumsum(nn) - nn, nn)
    j = lst[first + k]
    keep = (types[i] == type_id) & (types[j] == type_id)
    if rows is not None:
        mask = np.zeros(n_rows, dtype=bool)
        mask[rows] = True
        keep &= mask[i]
    i, j = i[keep], j[keep]
    d = min_image(pos[i] - pos[j], L, **(tilt or {}))
    rsq = (d * d).sum(axis=1)
    keep = rsq <= r_cut * r_cut
    return i[keep], j[keep], d[keep]


def to_frame(d, frame):
    """the pair vectors in the frame Q (None: as they are)"""
    return d if frame is None else d @ np.asarray(frame, dtype=np.float64).T


def from_frame(G, frame):
    """per-pair vectors of the frame Q back in the lab frame"""
    return G if frame is None else G @ np.asarray(frame, dtype=np.float64)


def compute(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=None, tilt=None, gradient=True, rows=None, frame=None):
    """returns dict(s, c, n, grad): c_i, n_i for every particle, grad = ds/dr (N, 3) (None when gradient=False).
    rows: restrict the CENTRAL particles to these (values of the others are 0; the gradient is then that of the partial sum)."""
    pos = np.asarray(pos, dtype=np.float64)
    types = np.asarray(types)
    N = len(pos)
    n_global = N if n_global is None else n_global
    Ql_ref = np.asarray(Ql_ref, dtype=np.float64)
    i, j, d = pairs(pos, types, nl, type_id, r_cut, tilt=tilt, L=L, rows=rows)
    d = to_frame(d, frame)
    r = np.sqrt((d * d).sum(axis=1))
    f, df = smoothing(r, r_on, r_cut)
    theta = np.arccos(np.clip(d[:, 2] / r, -1.0, 1.0))
    phi = np.arctan2(d[:, 1], d[:, 0])
    n = np.bincount(i, weights=f, minlength=N)
    inv_n = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)
    c = np.zeros(N)
    A = {}
    for l in range(lmax + 1):
        if Ql_ref[l] == 0.0:
            continue
        sq = np.zeros(N)
        for m in range(-l, l + 1):
            y = f * sph_harm_y(l, m, theta, phi)
            a = np.bincount(i, weights=y.real, minlength=N) + 1j * np.bincount(i, weights=y.imag, minlength=N)
            A[(l, m)] = a
            sq += np.abs(a) ** 2
        c += Ql_ref[l] * 4.0 * np.pi / (2 * l + 1) * sq * inv_n ** 2
    s = c.sum() / n_global
    grad = None
    if gradient:
        rhat = d / r[:, None]
        st, ct = np.sin(theta), np.cos(theta)
        cp, sp = np.cos(phi), np.sin(phi)
        e_theta = np.stack([ct * cp, ct * sp, -st], axis=1)
        e_phi = np.stack([-sp, cp, np.zeros_like(sp)], axis=1)
        # G = sum_lm Re{W_lm(i) grad(f Y_lm)} - 2 c_i / n_i grad f, per pair
        G = (-2.0 * c[i] * inv_n[i] * df)[:, None] * rhat
        for l in range(lmax + 1):
            if Ql_ref[l] == 0.0:
                continue
            gl = Ql_ref[l] * 4.0 * np.pi / (2 * l + 1) * 2.0 * inv_n ** 2
            for m in range(-l, l + 1):
                W = gl[i] * np.conj(A[(l, m)][i])
                Y = sph_harm_y(l, m, theta, phi)
                dY_dtheta = m * (ct / st) * Y
                if m < l:
                    dY_dtheta = dY_dtheta + np.sqrt((l - m) * (l + m + 1.0)) * np.exp(-1j * phi) * sph_harm_y(l, m + 1, theta, phi)
                dY_dphi = 1j * m * Y
                rad = (W * Y).real * df
                tht = (W * dY_dtheta).real * f / r
                ph = (W * dY_dphi).real * f / (r * st)
                G += rad[:, None] * rhat + tht[:, None] * e_theta + ph[:, None] * e_phi
        G = from_frame(G, frame)
        grad = np.zeros((N, 3))
        for k in range(3):
            grad[:, k] = np.bincount(i, weights=G[:, k], minlength=N) - np.bincount(j, weights=G[:, k], minlength=N)
        grad /= n_global
    return {"s": s, "c": c, "n": n, "grad": grad}


def forces(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, bias, n_global=None, tilt=None, frame=None):
    """(N, 4): F = -bias ds/dr, w = 0"""
    out = compute(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=n_global, tilt=tilt, frame=frame)
    F = np.zeros((len(pos), 4))
    F[:, :3] = -bias * out["grad"]
    return F


def issue_case():
    """the noisy two-type snapshot the known answer s = 0.253169653157423 belongs to"""
    import util
    pos, L = util.fcc_lattice(3)
    rng = np.random.default_rng(3)
    pos = pos + rng.normal(0, 0.05, pos.shape)
    types = (rng.random(108) < 0.2).astype(np.int32)
    nl = util.build_nlist(pos, L, 1.55)
    return dict(pos=pos, types=types, L=L, nl=nl, r_cut=1.4, r_on=1.2, lmax=6, type_id=0, Ql_ref=[0, 0, 0.3, 0, 1, 0, 1], n_global=108)
