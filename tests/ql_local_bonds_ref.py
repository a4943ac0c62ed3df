"""fp64 numpy restatement of the SOLID-BOND COUNT of the local Steinhardt variable (include/mtd_abi.h "Local Steinhardt bond order",
mtd_ql_local_bonds; ten Wolde, Ruiz-Montero and Frenkel): value, b_i, the per-entry products d, the gradient and the virial, in the
scatter form (every ordered list entry gives +G to its centre and -G to its neighbour, and hands its share of the back-propagated
vectors to BOTH of its ends) — independent of the gather form of the GPU passes, which rely on the list being symmetric.  Pairs and
smoothing are those of ql_local_ref, switch and gate those of ql_local_avg_ref, the per-entry gradient has the shape of
ql_local_virial_ref.entry_gradients.

    <a, b>  = sum_l g_l Re sum_m a_lm conj(b_lm),   g_l = Ql_ref[l] 4 pi / (2l + 1)
    c_i     = <q(i), q(i)>,  u(i) = q(i) / sqrt(c_i)  (0 when c_i = 0),  d_ij = <u(i), u(j)>
    sigma   = 3 t^2 - 2 t^3, t = clip((d - d_lo) / (d_hi - d_lo), 0, 1)
    b_i     = sum_j f_ij sigma(d_ij),  v_i = g(n_i) h(b_i),  s = sum_i v_i / N_global
bonds = None: v_i = g(n_i) h(c_i), the variable of ql_local_avg_ref without the average.

`frame`: a rotation the angular part is done in (see ql_local_ref); the per-entry gradients come back in the lab frame, where the virial
is formed with the lab-frame pair vectors (the tensor of the frame carried back, Q^T V Q).  None: the lab frame.
"""
import numpy as np
from scipy.special import sph_harm_y

import ql_local_avg_ref
import ql_local_ref

COMPONENTS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]        # xx, xy, xz, yy, yz, zz


def ramp_fn(d, bonds):
    """sigma(d) and d sigma / dd; bonds = (d_lo, d_hi)"""
    d_lo, d_hi = float(bonds[0]), float(bonds[1])
    t = np.clip((np.asarray(d, dtype=np.float64) - d_lo) / (d_hi - d_lo), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t), 6.0 * t * (1.0 - t) / (d_hi - d_lo)


def entry_gradients(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, tilt=None, switch=None, gate=None, bonds=None, gradient=True,
                    frame=None):
    """dict(i, j, d: the list entries that take part and their pair vectors; G: the gradient of N_global s with respect to d per entry
    (None without `gradient`); c, n, v, b per particle; dent: d_ij per entry (b and dent None without bonds)).
    N_global ds/dr_k = sum_{i = k} G - sum_{j = k} G."""
    pos = np.asarray(pos, dtype=np.float64)
    types = np.asarray(types)
    N = len(pos)
    Ql_ref = np.asarray(Ql_ref, dtype=np.float64)
    if bonds is not None and (Ql_ref < 0).any():
        raise ValueError("bonds need Ql_ref >= 0")
    i, j, d_lab = ql_local_ref.pairs(pos, types, nl, type_id, r_cut, tilt=tilt, L=L)
    d = ql_local_ref.to_frame(d_lab, frame)
    r = np.sqrt((d * d).sum(axis=1))
    f, df = ql_local_ref.smoothing(r, r_on, r_cut)
    theta = np.arccos(np.clip(d[:, 2] / r, -1.0, 1.0))
    phi = np.arctan2(d[:, 1], d[:, 0])
    n = np.bincount(i, weights=f, minlength=N)
    inv_n = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)

    def gather(w, at=i):                             # sum over the entries with end `at` of a complex weight per entry
        return np.bincount(at, weights=w.real, minlength=N) + 1j * np.bincount(at, weights=w.imag, minlength=N)

    lm = [(l, m) for l in range(lmax + 1) if Ql_ref[l] != 0.0 for m in range(-l, l + 1)]
    gl = {l: Ql_ref[l] * 4.0 * np.pi / (2 * l + 1) for l in range(lmax + 1)}
    Y = {k: sph_harm_y(k[0], k[1], theta, phi) for k in lm}
    A = {k: gather(f * Y[k]) for k in lm}
    q = {k: A[k] * inv_n for k in lm}
    c = np.zeros(N)
    for l in range(lmax + 1):
        if Ql_ref[l] == 0.0:
            continue
        sq = np.zeros(N)
        for m in range(-l, l + 1):
            sq += np.abs(A[(l, m)]) ** 2
        c += gl[l] * sq * inv_n ** 2
    g, dg = ql_local_avg_ref.gate_fn(n, gate)
    b = dent = None
    if bonds is None:
        h, dh = ql_local_avg_ref.switch_fn(c, switch)
    else:
        inv_rc = np.where(c > 0, 1.0 / np.sqrt(np.where(c > 0, c, 1.0)), 0.0)
        u = {k: q[k] * inv_rc for k in lm}
        dent = np.zeros(len(i))
        for k in lm:
            dent += gl[k[0]] * (u[k][i] * np.conj(u[k][j])).real
        sg, dsg = ramp_fn(dent, bonds)
        b = np.bincount(i, weights=f * sg, minlength=N)
        h, dh = ql_local_avg_ref.switch_fn(b, switch)
    v = g * h
    out = dict(i=i, j=j, d=d_lab, G=None, c=c, n=n, v=v, b=b, dent=dent)
    if not gradient:
        return out
    beta = g * dh
    if bonds is None:
        B = {k: beta * 2.0 * gl[k[0]] * np.conj(q[k]) for k in lm}
        wf = np.zeros(len(i))
    else:
        # the entry (i, j) moves d_ij with weight beta_i f sigma': its share of the vector T goes to i (with u(j)) and to j (with u(i))
        t = beta[i] * f * dsg
        td = np.bincount(i, weights=t * dent, minlength=N) + np.bincount(j, weights=t * dent, minlength=N)
        B = {}
        for k in lm:
            T = gather(t * u[k][j], i) + gather(t * u[k][i], j)
            B[k] = gl[k[0]] * np.conj((T - td * u[k]) * inv_rc)
        wf = beta[i] * sg
    a = dg * h
    for k in lm:
        a = a - (B[k] * q[k]).real * inv_n
    wf = wf + a[i]
    rhat = d / r[:, None]
    st, ct = np.sin(theta), np.cos(theta)
    cp, sp = np.cos(phi), np.sin(phi)
    e_theta = np.stack([ct * cp, ct * sp, -st], axis=1)
    e_phi = np.stack([-sp, cp, np.zeros_like(sp)], axis=1)
    G = (wf * df)[:, None] * rhat
    for (l, m) in lm:
        W = B[(l, m)][i] * inv_n[i]
        y = Y[(l, m)]
        dY_dtheta = m * (ct / st) * y
        if m < l:
            dY_dtheta = dY_dtheta + np.sqrt((l - m) * (l + m + 1.0)) * np.exp(-1j * phi) * sph_harm_y(l, m + 1, theta, phi)
        dY_dphi = 1j * m * y
        rad = (W * y).real * df
        tht = (W * dY_dtheta).real * f / r
        ph = (W * dY_dphi).real * f / (r * st)
        G += rad[:, None] * rhat + tht[:, None] * e_theta + ph[:, None] * e_phi
    out["G"] = ql_local_ref.from_frame(G, frame)
    return out


def compute(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=None, tilt=None, gradient=True, switch=None, gate=None,
            bonds=None, bias=None, frame=None):
    """returns dict(s, c, v, n, b, dent, i, j, grad (N, 3)); with `bias` also virial (N, 6), W (6,) = its sums and tensor (3, 3) =
    sum over the entries of d_a F_b, as ql_local_virial_ref.compute"""
    N = len(pos)
    n_global = N if n_global is None else n_global
    e = entry_gradients(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, tilt=tilt, switch=switch, gate=gate, bonds=bonds,
                        gradient=gradient, frame=frame)
    out = {k: e[k] for k in ("c", "v", "n", "b", "dent", "i", "j")}
    out["s"] = e["v"].sum() / n_global
    out["grad"] = None
    if gradient:
        i, j, d, G = e["i"], e["j"], e["d"], e["G"]
        grad = np.zeros((N, 3))
        for k in range(3):
            grad[:, k] = np.bincount(i, weights=G[:, k], minlength=N) - np.bincount(j, weights=G[:, k], minlength=N)
        out["grad"] = grad / n_global
        if bias is not None:
            Fp = -bias * G / n_global                                # the force of the entry on its centre i; -Fp on its neighbour j
            virial = np.zeros((N, 6))
            for cc, (a, bb) in enumerate(COMPONENTS):
                w = 0.5 * d[:, a] * Fp[:, bb]
                virial[:, cc] = np.bincount(i, weights=w, minlength=N) + np.bincount(j, weights=w, minlength=N)
            out.update(virial=virial, W=virial.sum(axis=0), tensor=d.T @ Fp)
    return out


def forces(bias, **case):
    """(N, 4): F = -bias ds/dr, w = 0"""
    out = compute(**case)
    F = np.zeros((len(case["pos"]), 4))
    F[:, :3] = -bias * out["grad"]
    return F


def strain_derivative(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, eps, n_global=None, tilt=None, **opt):
    """(6,): ds / d eps_ab by central differences of this module's s under ql_local_virial_ref.strain, the list kept"""
    from ql_local_virial_ref import strain
    out = np.zeros(6)
    for cc, (a, bb) in enumerate(COMPONENTS):
        s = []
        for sign in (1.0, -1.0):
            p2, L2, t2 = strain(pos, L, tilt, a, bb, sign * eps)
            s.append(compute(p2, types, L2, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=n_global, tilt=t2, gradient=False, **opt)["s"])
        out[cc] = (s[0] - s[1]) / (2.0 * eps)
    return out


def noisy_fcc(cells, sigma=0.13, seed=777):
    """the parity snapshot: fcc plus normal(0, sigma), wrapped into the box; list at 1.55, r_cut 1.4, r_on 1.2, degree 6.  At this noise
    the products d_ij spread below, inside and above the ramp (0.3, 0.8); at 0.05 every bond lies above it"""
    import util
    pos, L = util.fcc_lattice(cells)
    pos = pos + np.random.default_rng(seed).normal(0, sigma, pos.shape)
    pos = pos - L * np.rint(pos / L)
    return dict(pos=pos, types=np.zeros(len(pos), dtype=np.int32), L=L, nl=util.build_nlist(pos, L, 1.55), r_cut=1.4, r_on=1.2, lmax=6,
                type_id=0, Ql_ref=[0, 0, 0, 0, 0, 0, 1])


def dilute_case():
    """ql_local_avg_ref.dilute_case() (positions, list and degrees 4 and 6) with the bond count in place of the average"""
    case = ql_local_avg_ref.dilute_case()
    for k in ("average", "switch", "gate"):
        case.pop(k)
    return case, dict(bonds=(0.0, 0.9), switch=(4.0, 4), gate=(2, 6))


E6 = [0, 0, 0, 0, 0, 0, 1]
# the option combinations of the known answers on ql_local_ref.issue_case(); Ql_ref None: the case's own
COMBINATIONS = {
    "bonds(0.5,0.7)": (E6, dict(bonds=(0.5, 0.7))),
    "bonds": (E6, dict(bonds=(0.0, 0.9))),
    "bonds+switch": (E6, dict(bonds=(0.0, 0.9), switch=(6.5, 6))),
    "bonds+switch+gate": (E6, dict(bonds=(0.0, 0.9), switch=(6.5, 6), gate=(4, 8))),
    "own-degrees+bonds+switch": (None, dict(bonds=(0.3, 0.95), switch=(5.0, 4))),
}


def issue_case(name):
    """(case, options) of a known answer"""
    case = ql_local_ref.issue_case()
    ql, opt = COMBINATIONS[name]
    if ql is not None:
        case["Ql_ref"] = ql
    return case, opt
