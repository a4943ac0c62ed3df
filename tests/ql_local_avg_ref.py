"""fp64 numpy restatement of the local Steinhardt variable WITH its options (include/mtd_abi.h "Local Steinhardt bond order":
neighbour-averaged q_lm after Lechner and Dellago, a rational switch per particle, a smooth coordination gate), vectorised over the
pairs of the list, with an ANALYTIC gradient in the scatter form (every ordered pair gives +G to its centre and -G to its neighbour)
— independent of the gather form the GPU passes use.  Pairs and smoothing are those of ql_local_ref.

    n_i = sum_j f_ij,  q_lm(i) = sum_j f_ij Y_lm(d_ij) / n_i  (0 when n_i = 0)
    average:  qbar_lm(i) = [q_lm(i) + sum_j f_ij q_lm(j)] / (1 + n_i)                 (else qbar = q)
    c_i = sum_l Ql_ref[l] 4 pi/(2l+1) sum_m |qbar_lm(i)|^2
    switch:   h(c) = x^p / (1 + x^p), x = max(c, 0) / c0                              (else h(c) = c)
    gate:     g(n) = 3 t^2 - 2 t^3, t = clip((n - n_lo) / (n_hi - n_lo), 0, 1)        (else g = 1)
    v_i = g(n_i) h(c_i),  s = sum_i v_i / N_global,  F = -bias ds/dr

`frame`: a rotation the angular part is done in, the gradient rotated back (see ql_local_ref); None: the lab frame.
"""
import numpy as np
from scipy.special import sph_harm_y

import ql_local_ref


def switch_fn(c, switch):
    """h(c) and dh/dc; switch = (c0, p) or None"""
    c = np.asarray(c, dtype=np.float64)
    if switch is None:
        return c.copy(), np.ones_like(c)
    c0, p = float(switch[0]), int(switch[1])
    x = np.maximum(c, 0.0) / c0
    with np.errstate(over="ignore", invalid="ignore"):
        xp1 = x ** (p - 1)
        xp = xp1 * x
        big = ~(xp < np.inf)                         # x^p beyond the range of a double: h -> 1, h' -> 0
        h = np.where(big, 1.0, xp / (1.0 + xp))
        dh = np.where((c >= 0.0) & ~big, p * xp1 / ((1.0 + xp) ** 2 * c0), 0.0)
    return h, dh


def gate_fn(n, gate):
    """g(n) and dg/dn; gate = (n_lo, n_hi) or None"""
    n = np.asarray(n, dtype=np.float64)
    if gate is None:
        return np.ones_like(n), np.zeros_like(n)
    n_lo, n_hi = float(gate[0]), float(gate[1])
    t = np.clip((n - n_lo) / (n_hi - n_lo), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t), 6.0 * t * (1.0 - t) / (n_hi - n_lo)


def compute(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global=None, tilt=None, gradient=True,
            average=False, switch=None, gate=None, frame=None):
    """returns dict(s, c, v, n, grad): c_i (averaged when `average`), v_i = g h, n_i for every particle, grad = ds/dr (N, 3)"""
    pos = np.asarray(pos, dtype=np.float64)
    types = np.asarray(types)
    N = len(pos)
    n_global = N if n_global is None else n_global
    Ql_ref = np.asarray(Ql_ref, dtype=np.float64)
    i, j, d = ql_local_ref.pairs(pos, types, nl, type_id, r_cut, tilt=tilt, L=L)
    d = ql_local_ref.to_frame(d, frame)
    r = np.sqrt((d * d).sum(axis=1))
    f, df = ql_local_ref.smoothing(r, r_on, r_cut)
    theta = np.arccos(np.clip(d[:, 2] / r, -1.0, 1.0))
    phi = np.arctan2(d[:, 1], d[:, 0])
    n = np.bincount(i, weights=f, minlength=N)
    inv_n = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)

    def gather(w):                                   # sum over the pairs of centre i of a complex weight per pair
        return np.bincount(i, weights=w.real, minlength=N) + 1j * np.bincount(i, weights=w.imag, minlength=N)

    lm = [(l, m) for l in range(lmax + 1) if Ql_ref[l] != 0.0 for m in range(-l, l + 1)]
    gl = {l: Ql_ref[l] * 4.0 * np.pi / (2 * l + 1) for l in range(lmax + 1)}
    Y = {k: sph_harm_y(k[0], k[1], theta, phi) for k in lm}
    A = {k: gather(f * Y[k]) for k in lm}
    q = {k: A[k] * inv_n for k in lm}
    if average:
        qbar = {k: (q[k] + gather(f * q[k][j])) / (1.0 + n) for k in lm}
    c = np.zeros(N)
    for l in range(lmax + 1):
        if Ql_ref[l] == 0.0:
            continue
        sq = np.zeros(N)
        for m in range(-l, l + 1):
            sq += np.abs(qbar[(l, m)] if average else A[(l, m)]) ** 2
        c += gl[l] * sq if average else gl[l] * sq * inv_n ** 2
    h, dh = switch_fn(c, switch)
    g, dg = gate_fn(n, gate)
    v = g * h
    s = v.sum() / n_global
    grad = None
    if gradient:
        # B = dv_i / d qbar_lm(i) (times 2 for the conjugate pair), carried back through the average to C
        B = {k: g * dh * 2.0 * gl[k[0]] * np.conj(qbar[k] if average else q[k]) / (1.0 + n if average else 1.0) for k in lm}
        C = {k: B[k] + gather(f * B[k][j]) for k in lm} if average else B
        a = dg * h
        for k in lm:
            a = a - (C[k] * q[k]).real * inv_n
            if average:
                a = a - (B[k] * qbar[k]).real
        rhat = d / r[:, None]
        st, ct = np.sin(theta), np.cos(theta)
        cp, sp = np.cos(phi), np.sin(phi)
        e_theta = np.stack([ct * cp, ct * sp, -st], axis=1)
        e_phi = np.stack([-sp, cp, np.zeros_like(sp)], axis=1)
        wf = a[i]                                    # coefficient of grad f in the pair (i centre, j neighbour)
        if average:
            for k in lm:
                wf = wf + (B[k][i] * q[k][j]).real
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
        G = ql_local_ref.from_frame(G, frame)
        grad = np.zeros((N, 3))
        for k in range(3):
            grad[:, k] = np.bincount(i, weights=G[:, k], minlength=N) - np.bincount(j, weights=G[:, k], minlength=N)
        grad /= n_global
    return {"s": s, "c": c, "v": v, "n": n, "grad": grad}


def dilute_case():
    """a small noisy crystal in a dilute gas: 6 particles with n = 0, 41 with 0 < n < 2 and 20 inside the gate's ramp; the known
    answer s = 0.29674341030178875 and these three counts belong to the stream of default_rng(11) with the gas drawn BEFORE the
    crystal's noise (drawn in the other order the same recipe gives 11 / 31 / 17 particles and s = 0.2757...)"""
    import util
    rng = np.random.default_rng(11)
    pos, _ = util.fcc_lattice(2)
    gas = rng.uniform(-4, 4, (60, 3))
    pos = np.concatenate([pos + rng.normal(0, 0.04, pos.shape), gas])
    L = 8.0
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.6)
    return dict(pos=pos, types=types, L=L, nl=nl, r_cut=1.4, r_on=1.2, lmax=6, type_id=0, Ql_ref=[0, 0, 0, 0, 1, 0, 1],
                average=True, switch=(0.12, 3), gate=(2, 6))


# the option combinations of the known answers on ql_local_ref.issue_case()
COMBINATIONS = {
    "average": dict(average=True),
    "switch": dict(switch=(0.25, 3)),
    "average+switch": dict(average=True, switch=(0.12, 3)),
    "average+switch+gate": dict(average=True, switch=(0.12, 3), gate=(4, 8)),
    "switch+gate": dict(switch=(0.25, 3), gate=(4, 8)),
}
