"""fp64 numpy restatement of the local pair entropy (cv.pair_entropy_local, include/mtd_abi.h "Local pair entropy"), vectorised over the
entries of the list, with an ANALYTIC gradient in the scatter form (entry (i, j) gives +t_ij d/r to its centre and -t_ij d/r to its
neighbour, the adjoint alpha scattered over the neighbours) — independent of the gather form the GPU pass uses, which is returned beside
it — and the virial per particle with its sums.

    H_ib = sum_{j in row i} f(r) K(r_b - r),  rho = N_t / V,  g_ib = H_ib / (4 pi rho r_b^2)
    s_i = -2 pi rho Delta sum_b r_b^2 phi_ib,  phi = g ln g - g + 1 (g >= 1e-10, else 1)
    sbar_i = (s_i + sum_j f_a s_j) / (1 + n_i),  n_i = sum_j f_a,   v_i = h(-sbar_i) or sbar_i,   CV = sum_i v_i / N_global
"""
import math

import numpy as np

import pair_entropy_ref as pe
from ql_local_avg_ref import switch_fn
from ql_local_ref import smoothing

G_MIN = pe.G_MIN


def _volume(L):
    return float(np.prod(np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))))


def compute(pos, types, L, nl, r_max, sigma_r, n_bins, type_id, average=None, switch=None, tilt=None, n_global=None, bias=1.0):
    """average = (a_on, a_cut) or None, switch = (c0, p) or None.  Returns a dict:
    s, sbar, v, n, gamma, alpha, X (N,)   g, H, W, on (N, n_bins)   cv   n_t
    grad    (N, 3): dCV/dr in the scatter form
    gather  (N, 3): (1 / N_global) sum_{j in row k} (t_kj + t_jk) d_kj / r — what the force pass forms; equals grad on a symmetric list
    virial  (N, 6): -(bias / N_global) (1/2 sum_j d_a (t_kj + t_jk) d_b / r + delta_ab alpha_k X_k);  virial_sum (6,)
    strain  (6,):   dCV/d eps_ab from the scatter form (xx, xy, xz, yy, yz, zz): virial_sum = -bias strain on a symmetric list
    bc      centre bin of every list entry with both particles of the type, cut-off ignored (for the difference quotients)"""
    c = pe.constants(r_max, sigma_r, n_bins)
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    N = len(nl[0])
    n_global = N if n_global is None else n_global
    central = types[:N] == type_id
    n_t = int(central.sum())
    rho = n_t / _volume(L)
    i, j, d = pe.entries(pos, types, nl, type_id, np.inf, L, tilt=tilt)
    r = np.sqrt((d * d).sum(axis=1))
    bc = np.floor(r * (n_bins / r_max)).astype(np.int64)
    keep = (r <= c["r_cut"]) & (j < N)
    i, j, d, r = i[keep], j[keep], d[keep], r[keep]
    f, df = smoothing(r, c["r_on"], c["r_cut"])
    r2 = c["r_b"] ** 2
    H = np.zeros(N * n_bins)
    for lo in range(0, len(r), pe.CHUNK):
        K, _ = pe._window(r[lo:lo + pe.CHUNK], c, r_max, sigma_r, n_bins)
        slot = i[lo:lo + pe.CHUNK, None] * n_bins + np.arange(n_bins)[None, :]
        H += np.bincount(slot.ravel(), weights=(f[lo:lo + pe.CHUNK, None] * K).ravel(), minlength=N * n_bins)
    H = H.reshape(N, n_bins)
    if n_t:
        g = np.where(central[:, None], H / (4.0 * math.pi * rho * r2[None, :]), 0.0)
    else:
        g = np.zeros((N, n_bins))
    on = central[:, None] & (g >= G_MIN)
    lg = np.log(np.where(on, g, 1.0))
    phi = np.where(on, g * lg - g + 1.0, 1.0)
    c2 = 2.0 * math.pi * rho * c["delta"]
    s = np.where(central, -c2 * (r2[None, :] * phi).sum(axis=1), 0.0)
    W = np.where(on, -0.5 * c["delta"] * lg, 0.0)
    X = np.where(central, -(s + c2 * (r2[None, :] * g * lg * on).sum(axis=1)), 0.0)
    if average is not None:
        a_on, a_cut = float(average[0]), float(average[1])
        fa, dfa = smoothing(r, a_on, a_cut)
        inside = r <= a_cut
        fa, dfa = np.where(inside, fa, 0.0), np.where(inside, dfa, 0.0)
        n = np.bincount(i, weights=fa, minlength=N)
        sbar = np.where(central, (s + np.bincount(i, weights=fa * s[j], minlength=N)) / (1.0 + n), 0.0)
    else:
        fa, dfa = np.zeros(len(r)), np.zeros(len(r))
        n = np.zeros(N)
        sbar = s.copy()
    if switch is not None:
        h, dh = switch_fn(-sbar, switch)
        v, gamma = np.where(central, h, 0.0), np.where(central, -dh, 0.0)
    else:
        v, gamma = sbar.copy(), central.astype(np.float64)
    gn = gamma / (1.0 + n)
    alpha = gn + np.bincount(j, weights=fa * gn[i], minlength=N)[:N]          # the adjoint, scattered over the neighbours
    u_i, u_j = np.zeros(len(r)), np.zeros(len(r))                             # u_ij(W_i) and u_ij(W_j)
    for lo in range(0, len(r), pe.CHUNK):
        sl = slice(lo, lo + pe.CHUNK)
        K, x = pe._window(r[sl], c, r_max, sigma_r, n_bins)
        core = K * (df[sl, None] + f[sl, None] * x / sigma_r ** 2)
        u_i[sl] = (W[i[sl]] * core).sum(axis=1)
        u_j[sl] = (W[j[sl]] * core).sum(axis=1)
    t = alpha[i] * u_i + gn[i] * dfa * (s[j] - sbar[i])                       # t_ij
    t_mirror = alpha[j] * u_j + gn[j] * dfa * (s[i] - sbar[j])                # t_ji, evaluated at the entry (i, j)
    G = (t / r)[:, None] * d
    G2 = ((t + t_mirror) / r)[:, None] * d
    grad, gather = np.zeros((N, 3)), np.zeros((N, 3))
    for a in range(3):
        grad[:, a] = np.bincount(i, weights=G[:, a], minlength=N) - np.bincount(j, weights=G[:, a], minlength=N)[:N]
        gather[:, a] = np.bincount(i, weights=G2[:, a], minlength=N)
    virial, strain = np.zeros((N, 6)), np.zeros(6)
    for c6, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        virial[:, c6] = 0.5 * np.bincount(i, weights=d[:, a] * G2[:, b], minlength=N)
        strain[c6] = (d[:, a] * G[:, b]).sum()
        if a == b:
            virial[:, c6] += alpha * X
            strain[c6] += (alpha * X).sum()
    virial *= -bias / n_global
    return dict(s=s, sbar=sbar, v=v, n=n, gamma=gamma, alpha=alpha, X=X, g=g, H=H, W=W, on=on, cv=v.sum() / n_global, n_t=n_t,
                grad=grad / n_global, gather=gather / n_global, virial=virial, virial_sum=virial.sum(axis=0), strain=strain / n_global,
                bc=bc, r_b=c["r_b"])
