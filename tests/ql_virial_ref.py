"""fp64 numpy restatement of the per-entry force of the GLOBAL Steinhardt variable (SteinhardtQl.cc:278-322) and of the VIRIAL of the
force the pass applies (include/mtd_abi.h, mtd_ql_forces_virial).  For a list entry (k centre, j neighbour) with d = minImage(r_k - r_j):

    fp_kj = -bias sum_l Ql_ref[l] 4 pi / ((2l + 1) N_global^2) 2 Re sum_m conj(Q_lm) grad_d (f Y_lm)(d)

with the Q_lm table of the oracle's ql_compute_cv (the reference's order: per degree m = 0..l, then -1..-l) and scipy's sph_harm_y
(Condon-Shortley phase).  In the scatter form, independent of the GPU pass's pipeline: an entry adds fp to F_k — and, for a half list,
-fp to F_j when j is a local particle (:328-333) — and 1/2 d_a fp_b to virial_k[ab] — and, for a half list, the same to virial_j[ab],
which is what row j of the symmetric full list forms from -d and -fp.  Components xx, xy, xz, yy, yz, zz (HOOMD's order).
Pairs, minimum image and smoothing are those of ql_local_ref; strain() is ql_local_virial_ref's.

`frame`: a rotation the angular part is done in (see ql_local_ref).  The oracle's Q_lm table belongs to the lab frame (its CV pass takes
the angles from acos / atan2 and is finite on the z axis); rotate_qlm() carries it into the frame, degree by degree, with the matrix
that maps Y_l(d) to Y_l(Q d).  fp comes back in the lab frame and the virial is formed there with the lab-frame pair vectors (Q^T V Q).
"""
import numpy as np
from scipy.special import sph_harm_y

import ql_local_ref
from ql_local_virial_ref import COMPONENTS, strain  # noqa: F401  (re-exported)


def qlm_index(l, m):
    """position of (l, m) in the reference's table: l^2 + p with m = p for p <= l, m = l - p beyond"""
    return l * l + (m if m >= 0 else l - m)


def _angles(u):
    return np.arccos(np.clip(u[:, 2], -1.0, 1.0)), np.arctan2(u[:, 1], u[:, 0])


def rotate_qlm(Qlm, lmax, frame):
    """the table Q_lm = sum w Y_lm(d) of the vectors d, restated for the vectors Q d: per degree Y_l(Q u) = D_l Y_l(u) with a
    (2l + 1)^2 matrix D_l, found here by least squares over 8 (2l + 1) seeded unit vectors (residual ~1e-15), and Q'_l = D_l Q_l"""
    frame = np.asarray(frame, dtype=np.float64)
    Qlm = np.asarray(Qlm)
    out = np.array(Qlm, dtype=np.complex128)
    rng = np.random.default_rng(20240)
    for l in range(lmax + 1):
        u = rng.normal(size=(8 * (2 * l + 1), 3))
        u /= np.sqrt((u * u).sum(axis=1))[:, None]
        ms = list(range(-l, l + 1))
        t0, p0 = _angles(u)
        t1, p1 = _angles(u @ frame.T)
        Y0 = np.stack([sph_harm_y(l, m, t0, p0) for m in ms], axis=1)
        Y1 = np.stack([sph_harm_y(l, m, t1, p1) for m in ms], axis=1)
        Dt, *_ = np.linalg.lstsq(Y0, Y1, rcond=None)                     # Y1 = Y0 @ D^T
        assert np.abs(Y0 @ Dt - Y1).max() < 1e-12
        idx = [qlm_index(l, m) for m in ms]
        out[idx] = Dt.T @ Qlm[idx]
    return out


def entry_forces(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, Qlm, bias, n_global=None, tilt=None, frame=None):
    """(i, j, d, fp): the list entries that take part, their pair vectors and the `force` of SteinhardtQl.cc:278-322"""
    pos = np.asarray(pos, dtype=np.float64)
    types = np.asarray(types)
    n_global = len(nl[0]) if n_global is None else n_global
    Ql_ref = np.asarray(Ql_ref, dtype=np.float64)
    i, j, d_lab = ql_local_ref.pairs(pos, types, nl, type_id, r_cut, tilt=tilt, L=L)
    d = ql_local_ref.to_frame(d_lab, frame)
    if frame is not None:
        Qlm = rotate_qlm(Qlm, lmax, frame)
    r = np.sqrt((d * d).sum(axis=1))
    f, df = ql_local_ref.smoothing(r, r_on, r_cut)
    theta = np.arccos(np.clip(d[:, 2] / r, -1.0, 1.0))
    phi = np.arctan2(d[:, 1], d[:, 0])
    rhat = d / r[:, None]
    st, ct = np.sin(theta), np.cos(theta)
    cp, sp = np.cos(phi), np.sin(phi)
    e_theta = np.stack([ct * cp, ct * sp, -st], axis=1)
    e_phi = np.stack([-sp, cp, np.zeros_like(sp)], axis=1)
    fp = np.zeros_like(d)
    for l in range(lmax + 1):
        if Ql_ref[l] == 0.0:
            continue
        del_Ql = np.zeros_like(d)
        for m in range(-l, l + 1):
            w = np.conj(Qlm[qlm_index(l, m)])
            y = sph_harm_y(l, m, theta, phi)
            dY_dtheta = m * (ct / st) * y
            if m < l:
                dY_dtheta = dY_dtheta + np.sqrt((l - m) * (l + m + 1.0)) * np.exp(-1j * phi) * sph_harm_y(l, m + 1, theta, phi)
            dY_dphi = 1j * m * y
            rad = (w * y).real * df
            tht = (w * dY_dtheta).real * f / r
            ph = (w * dY_dphi).real * f / (r * st)
            del_Ql += 2.0 * (rad[:, None] * rhat + tht[:, None] * e_theta + ph[:, None] * e_phi)
        fp -= bias * Ql_ref[l] * 4.0 * np.pi / (2 * l + 1) / (float(n_global) ** 2) * del_Ql
    return i, j, d_lab, ql_local_ref.from_frame(fp, frame)


def compute(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, Qlm, bias, n_global=None, tilt=None, half=False, frame=None):
    """returns dict(fp (entries, 3), virial (N, 6), W (6,) = its sums, F (N, 3) the per-particle force sums, i, j, d); N = rows of the
    list (the local particles: `pos` may hold ghost particles behind them)"""
    N = len(nl[0])
    i, j, d, fp = entry_forces(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, Qlm, bias, n_global=n_global, tilt=tilt,
                               frame=frame)
    local = j < N
    F = np.zeros((N, 3))
    virial = np.zeros((N, 6))
    for k in range(3):
        F[:, k] = np.bincount(i, weights=fp[:, k], minlength=N)
        if half:
            F[:, k] -= np.bincount(j[local], weights=fp[local, k], minlength=N)
    for c, (a, b) in enumerate(COMPONENTS):
        w = 0.5 * d[:, a] * fp[:, b]
        virial[:, c] = np.bincount(i, weights=w, minlength=N)
        if half:
            virial[:, c] += np.bincount(j[local], weights=w[local], minlength=N)
    return {"fp": fp, "virial": virial, "W": virial.sum(axis=0), "F": F, "i": i, "j": j, "d": d}


def oracle_cv(ref, pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=None, tilt=None, half=False):
    """(value, Qlm) of the oracle's ql_compute_cv"""
    import util
    Lv = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    box = ref.Box.make(Lv, **(tilt or {}))
    val, Qlm, _ = ref.ql_compute_cv(util.oracle_postype(np.asarray(pos, dtype=np.float64), types), box, *nl, r_cut, r_on, lmax, type_id, Ql_ref,
                                    half=half, n_global=n_global)
    return val, Qlm


def value(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=None, tilt=None, half=False, frame=None):
    """the CV value of SteinhardtQl.cc:62-201 restated: s = sum_l Ql_ref[l] 4 pi / ((2l + 1) N_global^2) sum_m |Q_lm|^2 with
    Q_lm = sum over the entries of f Y_lm(d) (half lists: even degrees doubled, odd ones zero), the angles taken in `frame`.  The oracle's
    value takes theta from acos: finite on the z axis, but a bond 1e-6 off the axis has lost half its digits there."""
    pos = np.asarray(pos, dtype=np.float64)
    n_global = len(nl[0]) if n_global is None else n_global
    i, j, d = ql_local_ref.pairs(pos, np.asarray(types), nl, type_id, r_cut, tilt=tilt, L=L)
    d = ql_local_ref.to_frame(d, frame)
    r = np.sqrt((d * d).sum(axis=1))
    f, _ = ql_local_ref.smoothing(r, r_on, r_cut)
    theta, phi = _angles(d / r[:, None])
    s = 0.0
    for l in range(lmax + 1):
        if Ql_ref[l] == 0.0 or (half and l % 2):
            continue
        sq = sum(abs((f * sph_harm_y(l, m, theta, phi)).sum()) ** 2 for m in range(-l, l + 1))
        s += Ql_ref[l] * 4.0 * np.pi / (2 * l + 1) * (4.0 if half else 1.0) * sq / float(n_global) ** 2
    return s


def strain_derivative(ref, pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, eps, n_global=None, tilt=None, half=False, frame=None):
    """(6,): ds / d eps_ab by central differences of the oracle's CV under an affine strain of positions and box, the list kept;
    with a frame: of value() in that frame"""
    out = np.zeros(6)
    for c, (a, b) in enumerate(COMPONENTS):
        s = []
        for sign in (1.0, -1.0):
            p2, L2, t2 = strain(pos, L, tilt, a, b, sign * eps)
            if frame is None:
                s.append(oracle_cv(ref, p2, types, L2, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=n_global, tilt=t2, half=half)[0])
            else:
                s.append(value(p2, types, L2, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=n_global, tilt=t2, half=half, frame=frame))
        out[c] = (s[0] - s[1]) / (2.0 * eps)
    return out
