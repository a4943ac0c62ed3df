"""fp64 numpy restatement of the Debye structure factor (cv.debye_structure_factor, include/mtd_abi.h "Debye structure factor"), vectorised
over the entries of the list, with an ANALYTIC gradient in the scatter form (every entry gives +u d/r to its centre and -u d/r to its
neighbour, over N_t) — independent of the gather form the GPU pass uses, which is returned beside it — the per-particle virial and the
spectrum.

    x = pi r / r_cut,  w = sin x / x,  y_p = Q_p r,  phi_p = w sin y_p / y_p          (r = 0: phi_p = 1, u = 0)
    w' = (pi / r_cut) (x cos x - sin x) / x^2,  phi_p' = w' sin y_p / y_p + w Q_p (y_p cos y_p - sin y_p) / y_p^2
    A_p = sum_entries phi_p,  N_t = central particles of the type,  I_p = 1 + A_p / N_t,  s = sum_p c_p I_p
    s_i = sum_p c_p (1 + sum_{j in row i} phi_p),  u = sum_p c_p phi_p',  ds/dr_k = (2 / N_t) sum_{j in row k} u d / r
"""
import math

import numpy as np

from pair_entropy_ref import brute_nlist, entries        # noqa: F401  (the entries that take part follow the same rule)


def _phi(r, r_cut, q):
    """phi_p and phi_p' of every entry, (len(r), len(q)) each; r = 0 gives 1 and 0"""
    q = np.asarray(q, dtype=np.float64)
    safe = np.where(r > 0.0, r, 1.0)
    x = math.pi * safe / r_cut
    w = np.sin(x) / x
    dw = (math.pi / r_cut) * (x * np.cos(x) - np.sin(x)) / (x * x)
    y = q[None, :] * safe[:, None]
    j = np.sin(y) / y
    dj = q[None, :] * (y * np.cos(y) - np.sin(y)) / (y * y)
    phi = w[:, None] * j
    dphi = dw[:, None] * j + w[:, None] * dj
    zero = (r <= 0.0)[:, None]
    return np.where(zero, 1.0, phi), np.where(zero, 0.0, dphi)


def _central(types, nl, type_id, rows):
    n_rows = len(nl[0])
    central = np.arange(n_rows) if rows is None else np.asarray(rows)
    return central[types[central] == type_id]


def sums(pos, types, L, nl, q, r_cut, type_id, tilt=None, rows=None):
    """this domain's sums: A_p [P] and N_t — what the ranks of a domain-decomposed run add up"""
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    i, j, d = entries(pos, types, nl, type_id, r_cut, L, tilt=tilt, rows=rows)
    r = np.sqrt((d * d).sum(axis=1))
    phi, _ = _phi(r, r_cut, q)
    return phi.sum(axis=0), len(_central(types, nl, type_id, rows))


def finalize(A, n_t, c):
    """(s, I_p)"""
    c = np.asarray(c, dtype=np.float64)
    if n_t == 0:
        return 0.0, np.zeros(len(c))
    I = 1.0 + np.asarray(A) / n_t
    return float((c * I).sum()), I


def compute(pos, types, L, nl, q, r_cut, type_id, c=None, tilt=None, rows=None, sums_override=None, bias=1.0):
    """returns dict(s, I, A, n_t, local, grad, gather, virial, virial_sum)
    local   (rows,): s_i (0 for particles of another type and for rows outside `rows`)
    grad    (len(pos), 3): ds/dr in the scatter form, ghosts included
    gather  (rows, 3): (2 / N_t) sum_{j in row k} u_kj d_kj / r_kj — what the force pass forms; equals grad on a symmetric full list
    virial  (rows, 6): -(bias / N_t) sum_{j in row k} u_kj d_a d_b / r_kj
    sums_override: (A, N_t) of the WHOLE system when this call sees one domain (rows / a shard) only"""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    c = np.ones(len(q)) if c is None else np.atleast_1d(np.asarray(c, dtype=np.float64))
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    n_rows = len(nl[0])
    i, j, d = entries(pos, types, nl, type_id, r_cut, L, tilt=tilt, rows=rows)
    r = np.sqrt((d * d).sum(axis=1))
    phi, dphi = _phi(r, r_cut, q)
    central = _central(types, nl, type_id, rows)
    A, n_t = phi.sum(axis=0), len(central)
    if sums_override is not None:
        A, n_t = sums_override
    s, I = finalize(A, n_t, c)
    local = np.zeros(n_rows)
    local[central] = c.sum()
    local += np.bincount(i, weights=phi @ c, minlength=n_rows)
    u = dphi @ c
    G = np.where(r > 0.0, u / np.where(r > 0.0, r, 1.0), 0.0)[:, None] * d / max(n_t, 1)
    grad = np.zeros((len(pos), 3))
    gather = np.zeros((n_rows, 3))
    for a in range(3):
        grad[:, a] = np.bincount(i, weights=G[:, a], minlength=len(pos)) - np.bincount(j, weights=G[:, a], minlength=len(pos))
        gather[:, a] = 2.0 * np.bincount(i, weights=G[:, a], minlength=n_rows)
    virial = np.zeros((n_rows, 6))
    for c6, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        virial[:, c6] = -bias * np.bincount(i, weights=d[:, a] * G[:, b], minlength=n_rows)
    return dict(s=s, I=I, A=A, n_t=n_t, local=local, grad=grad, gather=gather, virial=virial, virial_sum=virial.sum(axis=0))


def value(pos, types, L, nl, q, r_cut, type_id, c=None, tilt=None):
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    A, n_t = sums(pos, types, L, nl, q, r_cut, type_id, tilt=tilt)
    return finalize(A, n_t, np.ones(len(q)) if c is None else c)[0]


def spectrum_points(q_min, q_max, n_q):
    return q_min + np.arange(n_q) * ((q_max - q_min) / (n_q - 1) if n_q > 1 else 0.0)


def spectrum_sums(pos, types, L, nl, r_cut, type_id, q_min, q_max, n_q, tilt=None, rows=None):
    """this domain's sums of the spectrum: sum_entries w sin(Q_m r) / (Q_m r) [n_q] and N_t"""
    return sums(pos, types, L, nl, spectrum_points(q_min, q_max, n_q), r_cut, type_id, tilt=tilt, rows=rows)


def spectrum(pos, types, L, nl, r_cut, type_id, q_min, q_max, n_q, tilt=None, rows=None):
    """(Q_m, I(Q_m)): the diagnostic on n_q equally spaced wave numbers"""
    Q = spectrum_points(q_min, q_max, n_q)
    A, n_t = spectrum_sums(pos, types, L, nl, r_cut, type_id, q_min, q_max, n_q, tilt=tilt, rows=rows)
    return Q, finalize(A, n_t, np.ones(n_q))[1]
