"""fp64 numpy restatement of the VIRIAL of the local Steinhardt variable's bias force (include/mtd_abi.h, mtd_ql_local_forces_virial),
for the plain variable and every option, in the scatter form: an ordered list entry (i centre, j neighbour) with gradient G_ij and
pair vector d_ij = minImage(r_i - r_j) exerts -bias G_ij / N_global on i and the opposite on j, and gives

    1/2 d_ij,a (-bias G_ij,b / N_global)        to virial_i[ab] and the same to virial_j[ab]

for the six components xx, xy, xz, yy, yz, zz (HOOMD's order).  Independent of the gather form of the GPU pass, which forms the complete
pair force per entry of a row.  Pairs, smoothing, switch and gate are those of ql_local_ref / ql_local_avg_ref; the per-entry gradient G,
which those keep internal, is restated here (the value and the gradient it returns are compared with theirs in
tests/test_ql_local_virial_ref.py).

`frame`: a rotation the angular part is done in (see ql_local_ref); G comes back in the lab frame and the virial is formed there with the
lab-frame pair vectors, which is the tensor of the frame carried back (Q^T V Q).  None: the lab frame.
"""
import numpy as np
from scipy.special import sph_harm_y

import ql_local_avg_ref
import ql_local_ref

COMPONENTS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]        # xx, xy, xz, yy, yz, zz


def entry_gradients(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, tilt=None, average=False, switch=None, gate=None,
                    frame=None):
    """(i, j, d, G, v): the list entries that take part, their pair vectors and G_ij = d v_i-and-beyond / d d_ij (before 1 / N_global),
    and v_i = g(n_i) h(c_i) per particle.  N_global ds/dr_k = sum_{i = k} G - sum_{j = k} G."""
    pos = np.asarray(pos, dtype=np.float64)
    types = np.asarray(types)
    N = len(pos)
    Ql_ref = np.asarray(Ql_ref, dtype=np.float64)
    i, j, d_lab = ql_local_ref.pairs(pos, types, nl, type_id, r_cut, tilt=tilt, L=L)
    d = ql_local_ref.to_frame(d_lab, frame)
    r = np.sqrt((d * d).sum(axis=1))
    f, df = ql_local_ref.smoothing(r, r_on, r_cut)
    theta = np.arccos(np.clip(d[:, 2] / r, -1.0, 1.0))
    phi = np.arctan2(d[:, 1], d[:, 0])
    n = np.bincount(i, weights=f, minlength=N)
    inv_n = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)

    def gather(w):
        return np.bincount(i, weights=w.real, minlength=N) + 1j * np.bincount(i, weights=w.imag, minlength=N)

    lm = [(l, m) for l in range(lmax + 1) if Ql_ref[l] != 0.0 for m in range(-l, l + 1)]
    gl = {l: Ql_ref[l] * 4.0 * np.pi / (2 * l + 1) for l in range(lmax + 1)}
    Y = {k: sph_harm_y(k[0], k[1], theta, phi) for k in lm}
    q = {k: gather(f * Y[k]) * inv_n for k in lm}
    qbar = {k: (q[k] + gather(f * q[k][j])) / (1.0 + n) for k in lm} if average else q
    c = np.zeros(N)
    for k in lm:
        c += gl[k[0]] * np.abs(qbar[k]) ** 2
    h, dh = ql_local_avg_ref.switch_fn(c, switch)
    g, dg = ql_local_avg_ref.gate_fn(n, gate)
    # B = dv_i / d qbar_lm(i), carried back through the average to C; a: the coefficient of grad f from n_i and the normalisations
    B = {k: g * dh * 2.0 * gl[k[0]] * np.conj(qbar[k]) / (1.0 + n if average else 1.0) for k in lm}
    C = {k: B[k] + gather(f * B[k][j]) for k in lm} if average else B
    a = dg * h
    for k in lm:
        a = a - (C[k] * q[k]).real * inv_n
        if average:
            a = a - (B[k] * qbar[k]).real
    wf = a[i]
    if average:
        for k in lm:
            wf = wf + (B[k][i] * q[k][j]).real
    rhat = d / r[:, None]
    st, ct = np.sin(theta), np.cos(theta)
    cp, sp = np.cos(phi), np.sin(phi)
    e_theta = np.stack([ct * cp, ct * sp, -st], axis=1)
    e_phi = np.stack([-sp, cp, np.zeros_like(sp)], axis=1)
    G = (wf * df)[:, None] * rhat
    for (l, m) in lm:
        W = C[(l, m)][i] * inv_n[i]
        y = Y[(l, m)]
        dY_dtheta = m * (ct / st) * y
        if m < l:
            dY_dtheta = dY_dtheta + np.sqrt((l - m) * (l + m + 1.0)) * np.exp(-1j * phi) * sph_harm_y(l, m + 1, theta, phi)
        dY_dphi = 1j * m * y
        rad = (W * y).real * df
        tht = (W * dY_dtheta).real * f / r
        ph = (W * dY_dphi).real * f / (r * st)
        G += rad[:, None] * rhat + tht[:, None] * e_theta + ph[:, None] * e_phi
    return i, j, d_lab, ql_local_ref.from_frame(G, frame), g * h, n


def compute(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, bias, n_global=None, tilt=None, average=False, switch=None, gate=None,
            frame=None):
    """returns dict(virial (N, 6), W (6,) = its sums, tensor (3, 3) = sum over entries of d_a F_b with all nine (a, b), s, n, grad (N, 3))"""
    N = len(pos)
    n_global = N if n_global is None else n_global
    i, j, d, G, v, n = entry_gradients(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, tilt=tilt, average=average, switch=switch,
                                       gate=gate, frame=frame)
    Fp = -bias * G / n_global                                        # the force of the entry on its centre i; -Fp on its neighbour j
    virial = np.zeros((N, 6))
    for c, (a, b) in enumerate(COMPONENTS):
        w = 0.5 * d[:, a] * Fp[:, b]
        virial[:, c] = np.bincount(i, weights=w, minlength=N) + np.bincount(j, weights=w, minlength=N)
    grad = np.zeros((N, 3))
    for k in range(3):
        grad[:, k] = np.bincount(i, weights=G[:, k], minlength=N) - np.bincount(j, weights=G[:, k], minlength=N)
    return {"virial": virial, "W": virial.sum(axis=0), "tensor": d.T @ Fp, "s": v.sum() / n_global, "n": n, "grad": grad / n_global}


def strain(pos, L, tilt, a, b, eps):
    """positions and box under r -> (I + eps e_a e_b^T) r, a <= b: the box stays upper triangular, so it is a box of mtd_box again.
    Returns (pos, L (3,), tilt dict)."""
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    t = dict(xy=0.0, xz=0.0, yz=0.0)
    t.update(tilt or {})
    H = np.array([[L[0], t["xy"] * L[1], t["xz"] * L[2]], [0.0, L[1], t["yz"] * L[2]], [0.0, 0.0, L[2]]])
    S = np.eye(3)
    S[a, b] += eps
    H2 = S @ H
    L2 = np.array([H2[0, 0], H2[1, 1], H2[2, 2]])
    tilt2 = dict(xy=H2[0, 1] / L2[1], xz=H2[0, 2] / L2[2], yz=H2[1, 2] / L2[2])
    return np.asarray(pos, dtype=np.float64) @ S.T, L2, tilt2


def strain_derivative(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, eps, n_global=None, tilt=None, **opt):
    """(6,): ds / d eps_ab by central differences of ql_local_avg_ref.compute(..., gradient=False)["s"], the list kept"""
    out = np.zeros(6)
    for c, (a, b) in enumerate(COMPONENTS):
        s = []
        for sign in (1.0, -1.0):
            p2, L2, t2 = strain(pos, L, tilt, a, b, sign * eps)
            s.append(ql_local_avg_ref.compute(p2, types, L2, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=n_global, tilt=t2, gradient=False,
                                              **opt)["s"])
        out[c] = (s[0] - s[1]) / (2.0 * eps)
    return out
