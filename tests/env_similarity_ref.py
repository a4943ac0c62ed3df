"""fp64 numpy restatement of the environment similarity (cv.environment_similarity, include/mtd_abi.h "Environment similarity"; Piaggi
and Parrinello, J. Chem. Phys. 150, 244119), vectorised over the entries of the list.  Over the entries (i, j) of a FULL list with both
particles of the type, j != i, d = minImage(r_j - r_i) and r = |d| <= r_cut:

    phi(x) = exp(-|x|^2 / (4 sigma_env^2))
    k^e_i  = (1 / M_e) sum_j f(r_ij) sum_m phi(d_ij - T^e_m)
    k_i    = k^1_i (E = 1),   (1 / lam) ln sum_e exp(lam k^e_i) (E > 1),    w^e_i = exp(lam k^e_i) / sum_e' exp(lam k^e'_i)
    v_i    = h(k_i),  h(k) = x^p / (1 + x^p), x = k / c0  (h(k) = k without a switch),      s = (1 / N_global) sum_i v_i
    B_e(d) = f'(r) (d / r) sum_m phi_m - f(r) sum_m phi_m (d - T^e_m) / (2 sigma_env^2)
    g_ij   = sum_e (beta^e_i / M_e) B_e(d_ij),   beta^e_i = h'(k_i) w^e_i                   (= d(N s) / d d_ij)

The gradient is returned in the SCATTER form (every entry gives +g to its neighbour and -g to its centre) and, independently, in the
GATHER form the GPU pass uses (row k: sum_j [-g_kj(d_kj) + g_jk(-d_kj)]); the per-particle virial is the gather form of the header.
"""
import numpy as np

from ql_local_ref import min_image, smoothing

COMPONENTS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def as_environments(templates):
    """a list of 3-vectors (one environment) or a list of such lists -> list of (M_e, 3) arrays"""
    t = [np.asarray(e, dtype=np.float64) for e in templates] if np.ndim(templates[0]) == 2 else [np.asarray(templates, dtype=np.float64)]
    for e in t:
        assert e.ndim == 2 and e.shape[1] == 3 and len(e) >= 1
    return t


def is_closed(env):
    """the environment holds -T for every T (exact comparison)"""
    have = {tuple(v) for v in np.asarray(env, dtype=np.float64) + 0.0}
    return all(tuple(-np.asarray(v) + 0.0) in have for v in have)


def entries(pos, types, nl, type_id, r_cut, L, tilt=None, rows=None):
    """(i, j, d) of the list entries that take part: i a row of the list (in `rows` when given), both of `type_id`, j != i, r <= r_cut;
    d = minImage(r_j - r_i); j may index a particle behind the rows (a ghost)"""
    head, nn, lst = (np.asarray(a).astype(np.int64) for a in nl)
    n_rows = len(head)
    i = np.repeat(np.arange(n_rows), nn)
    k = np.arange(len(i)) - np.repeat(np.cumsum(nn) - nn, nn)
    j = lst[np.repeat(head, nn) + k]
    keep = (types[i] == type_id) & (types[j] == type_id) & (i != j)
    if rows is not None:
        mask = np.zeros(n_rows, dtype=bool)
        mask[rows] = True
        keep &= mask[i]
    i, j = i[keep], j[keep]
    d = min_image(pos[j] - pos[i], L, **(tilt or {}))
    keep = np.sqrt((d * d).sum(axis=1)) <= r_cut
    return i[keep], j[keep], d[keep]


def _sums(d, env, sigma_env):
    """S = sum_m phi(d - T_m) (n,) and U = sum_m phi(d - T_m) (d - T_m) (n, 3)"""
    x = d[:, None, :] - env[None, :, :]
    phi = np.exp(-(x * x).sum(axis=2) / (4.0 * sigma_env ** 2))
    return phi.sum(axis=1), (phi[:, :, None] * x).sum(axis=1)


def _bracket(d, r, f, df, env, sigma_env):
    """B_e(d) / M_e (n, 3)"""
    S, U = _sums(d, env, sigma_env)
    return ((df * S / r)[:, None] * d - (f / (2.0 * sigma_env ** 2))[:, None] * U) / len(env)


def switch(k, sw):
    """h(k) and h'(k); sw = (c0, p) or None"""
    if sw is None:
        return k.copy(), np.ones_like(k)
    c0, p = float(sw[0]), int(sw[1])
    x = k / c0
    xp = x ** p
    return xp / (1.0 + xp), p * x ** (p - 1) / (c0 * (1.0 + xp) ** 2)


def compute(pos, types, L, nl, templates, sigma_env, r_on, r_cut, type_id, lam=100.0, sw=None, n_global=None, tilt=None, rows=None, bias=1.0,
            beta_all=None, closed_shortcut=False):
    """returns dict(s, sum_v, ke, k, v, w, beta, grad, gather, virial, virial_sum, tensor, closed)
    ke (rows, E), k, v (rows,): 0 for rows that are not central particles of the type
    grad    (len(pos), 3): ds/dr in the scatter form, ghosts included
    gather  (rows, 3): ds/dr_k as the gather over row k; equals grad on a symmetric full list
    virial  (rows, 6): -(bias / N_global) 1/2 sum_j [g_kj,a d_kj,b + g_jk,a d_jk,b] for (a, b) = xx xy xz yy yz zz
    beta_all: beta^e of EVERY particle (len(pos), E) when this call sees a subset of the central particles and E > 1 or a switch is set
    closed_shortcut: inversion-closed environments take B_e(-d) = -B_e(d) instead of the second evaluation"""
    envs = as_environments(templates)
    E = len(envs)
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    n_rows = len(nl[0])
    N = float(n_global if n_global is not None else n_rows)
    i, j, d = entries(pos, types, nl, type_id, r_cut, L, tilt=tilt, rows=rows)
    r = np.sqrt((d * d).sum(axis=1))
    f, df = smoothing(r, r_on, r_cut)
    central = np.zeros(n_rows, dtype=bool)
    central[np.arange(n_rows) if rows is None else np.asarray(rows)] = True
    central &= types[:n_rows] == type_id
    ke = np.zeros((n_rows, E))
    for e, env in enumerate(envs):
        ke[:, e] = np.bincount(i, weights=f * _sums(d, env, sigma_env)[0], minlength=n_rows) / len(env)
    if E == 1:
        k, w = ke[:, 0].copy(), np.ones((n_rows, 1))
    else:
        top = ke.max(axis=1)
        ex = np.exp(lam * (ke - top[:, None]))
        k = top + np.log(ex.sum(axis=1)) / lam
        w = ex / ex.sum(axis=1)[:, None]
    k = np.where(central, k, 0.0)
    v, dh = switch(k, sw)
    v = np.where(central, v, 0.0)
    beta = np.where(central[:, None], dh[:, None] * w, 0.0)
    if beta_all is None:
        beta_all = np.zeros((len(pos), E))
        if E == 1 and sw is None:
            beta_all[types == type_id] = 1.0                   # the plain variable: beta = 1 for every particle of the type, ghosts included
        else:
            assert rows is None and n_rows == len(pos), "beta of the particles outside the rows is needed"
            beta_all[:n_rows] = beta
    P = [_bracket(d, r, f, df, env, sigma_env) for env in envs]                                  # B_e(d) / M_e
    closed = [is_closed(env) for env in envs]
    Q = [-P[e] if closed_shortcut and closed[e] else _bracket(-d, r, f, df, env, sigma_env) for e, env in enumerate(envs)]   # B_e(-d) / M_e
    g = sum(beta[i, e][:, None] * P[e] for e in range(E))                                        # g_ij(d_ij)
    g_back = sum(beta_all[j, e][:, None] * Q[e] for e in range(E))                               # g_ji(-d_ij)
    grad = np.zeros((len(pos), 3))
    gather = np.zeros((n_rows, 3))
    for a in range(3):
        grad[:, a] = (np.bincount(j, weights=g[:, a], minlength=len(pos)) - np.bincount(i, weights=g[:, a], minlength=len(pos))) / N
        gather[:, a] = np.bincount(i, weights=g_back[:, a] - g[:, a], minlength=n_rows) / N
    virial = np.zeros((n_rows, 6))
    for c6, (a, b) in enumerate(COMPONENTS):
        virial[:, c6] = -(bias / N) * 0.5 * np.bincount(i, weights=(g[:, a] - g_back[:, a]) * d[:, b], minlength=n_rows)
    tensor = -(bias / N) * np.einsum("na,nb->ab", g, d)          # all nine -bias ds/d eps_ab (x_a += eps x_b): not symmetric
    return dict(s=v.sum() / N, sum_v=v.sum(), ke=ke * central[:, None], k=k, v=v, w=w, beta=beta, grad=grad, gather=gather, virial=virial,
                virial_sum=virial.sum(axis=0), tensor=tensor, closed=closed)


def value(pos, types, L, nl, templates, sigma_env, r_on, r_cut, type_id, lam=100.0, sw=None, n_global=None, tilt=None):
    envs = as_environments(templates)
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    n_rows = len(nl[0])
    i, j, d = entries(pos, types, nl, type_id, r_cut, L, tilt=tilt)
    r = np.sqrt((d * d).sum(axis=1))
    f, _ = smoothing(r, r_on, r_cut)
    ke = np.stack([np.bincount(i, weights=f * _sums(d, env, sigma_env)[0], minlength=n_rows) / len(env) for env in envs], axis=1)
    if len(envs) == 1:
        k = ke[:, 0]
    else:
        top = ke.max(axis=1)
        k = top + np.log(np.exp(lam * (ke - top[:, None])).sum(axis=1)) / lam
    v = np.where(types[:n_rows] == type_id, switch(k, sw)[0], 0.0)
    return v.sum() / float(n_global if n_global is not None else n_rows)


def templates(structure, a):
    """the template environments of a cubic lattice with conventional lattice constant a (what cv.environment_templates returns)"""
    a = float(a)
    perm = lambda v: sorted({p for p in [(v[0], v[1], v[2]), (v[0], v[2], v[1]), (v[1], v[0], v[2]), (v[1], v[2], v[0]), (v[2], v[0], v[1]),
                                        (v[2], v[1], v[0])]})
    signs = lambda v: sorted({(sx * v[0] + 0.0, sy * v[1] + 0.0, sz * v[2] + 0.0) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)})
    both = lambda v: sorted({s for p in perm(v) for s in signs(p)})
    if structure == "fcc":
        return np.array(both((0.5, 0.5, 0.0))) * a
    if structure == "bcc":
        return np.array(both((0.5, 0.5, 0.5)) + both((1.0, 0.0, 0.0))) * a
    if structure == "sc":
        return np.array(both((1.0, 0.0, 0.0))) * a
    if structure == "diamond":
        first = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], dtype=np.float64) * (a / 4.0)
        return [first, -first]
    raise ValueError(structure)


def diamond_lattice(n, nn_dist=1.0):
    """n^3 cubic cells x 8 particles of the diamond lattice; positions centred on 0, box length, sublattice (0 / 1) per particle"""
    a = nn_dist * 4.0 / np.sqrt(3.0)
    fcc = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    basis = np.concatenate([fcc, fcc + 0.25])
    cells = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    pos = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    L = n * a
    return pos - L / 2 + 0.125 * a, L, np.tile(np.repeat([0, 1], 4), len(cells))
