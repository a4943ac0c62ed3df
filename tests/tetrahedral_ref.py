"""fp64 numpy restatement of the tetrahedral order (cv.tetrahedral, include/mtd_abi.h "Tetrahedral order") FROM THE DEFINITION: the explicit
sum over the pairs j < k of every row, not the moment form the kernels evaluate — the GPU parity tests the identity between the two as
well.  Gradient and virial by the analytic derivatives of the pair sum, in the scatter form (an entry (i, j) gives +g_ij to r_j and -g_ij
to r_i, half of its virial to each end), independent of the gather form of the GPU pass.

    entries (i, j): both of the type, j != i, j a central particle, 0 < r = |d| <= r_cut, d = minImage(r_j - r_i), u = d / r
    f(r) = 1 (r <= r_on), (1 + cos(pi (r - r_on) / (r_cut - r_on))) / 2 beyond
    A_i = sum_{j<k} f_ij f_ik (u_ij.u_ik - cos0)^2      W_i = sum_{j<k} f_ij f_ik      n_i = sum_j f_ij
    t_i = 1 - A_i / (W_i (1/3 + cos0^2)) where W_i >= W_MIN, else 0 with zero gradient
    v_i = g(n_i) h(t_i)      (not normalised: v_i = A_i)      s = (1 / N_t) sum_i v_i
Rows are grouped by their number of entries, so that the pair sums of all rows of one length are one einsum.
"""
import numpy as np

from pair_entropy_ref import brute_nlist, min_image      # noqa: F401

PAIRS6 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
W_MIN = 1e-12


def params(type_id, r_cut, r_on, cos0=-1.0 / 3.0, normalise=True, switch=None, gate=None):
    """switch: None or (c0, p); gate: None or (n_lo, n_hi)"""
    return dict(type=int(type_id), r_cut=float(r_cut), r_on=float(r_on), cos0=float(cos0), normalise=bool(normalise), switch=switch, gate=gate)


def window(r, par):
    """f(r) and df/dr of every entry"""
    r = np.asarray(r, dtype=np.float64)
    x = (r - par["r_on"]) / (par["r_cut"] - par["r_on"])
    inside = r <= par["r_on"]
    f = np.where(inside, 1.0, 0.5 * (1.0 + np.cos(np.pi * x)))
    df = np.where(inside, 0.0, -0.5 * np.pi * np.sin(np.pi * x) / (par["r_cut"] - par["r_on"]))
    return f, df


def h_of(t, switch):
    """h(t) and h'(t): x^p / (1 + x^p), x = max(t, 0) / c0; h(t) = t without a switch"""
    if switch is None:
        return t.copy(), np.ones_like(t)
    c0, p = float(switch[0]), int(switch[1])
    x = np.maximum(t, 0.0) / c0
    xp = x ** p
    return xp / (1.0 + xp), np.where(t >= 0.0, p * x ** (p - 1) / c0 / (1.0 + xp) ** 2, 0.0)


def g_of(n, gate):
    """g(n) and g'(n): the smoothstep from n_lo to n_hi; 1 without a gate"""
    if gate is None:
        return np.ones_like(n), np.zeros_like(n)
    n_lo, n_hi = float(gate[0]), float(gate[1])
    y = np.clip((n - n_lo) / (n_hi - n_lo), 0.0, 1.0)
    return y * y * (3.0 - 2.0 * y), 6.0 * y * (1.0 - y) / (n_hi - n_lo)


def row_entries(pos, types, nl, L, par, tilt=None):
    """(i, j, d, r) of the entries that take part, in the order of the list"""
    head, nn, lst = (np.asarray(a).astype(np.int64) for a in nl)
    n_rows = len(head)
    i = np.repeat(np.arange(n_rows), nn)
    k = np.arange(len(i)) - np.repeat(np.cumsum(nn) - nn, nn)
    j = lst[np.repeat(head, nn) + k]
    keep = (i != j) & (j < n_rows)
    i, j = i[keep], j[keep]
    keep = (types[i] == par["type"]) & (types[j] == par["type"])
    i, j = i[keep], j[keep]
    d = min_image(pos[j] - pos[i], L, **(tilt or {}))
    r = np.sqrt((d * d).sum(axis=1))
    keep = (r > 0.0) & (r <= par["r_cut"])
    return i[keep], j[keep], d[keep], r[keep]


def compute(pos, types, L, nl, par, tilt=None, bias=1.0):
    """returns dict(s, n_t, local, switched, coordination, W, grad, virial, virial_sum, r, entries)
    local        (N,): t_i (A_i when not normalised; 0 for particles of another type)
    switched     (N,): v_i
    coordination (N,): n_i
    W            (N,): the pair weight W_i
    grad         (N, 3): ds/dr, the scatter form
    virial       (N, 6): -(bias / (2 N_t)) sum over the entries that end at the particle, as centre or as neighbour, of g_a d_b
    r            the distances of the entries that take part (the tests' condition on the inputs)
    entries      dict(i, j, d, g): the entries that take part and g_ij = dv_i/dd_ij of each"""
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    N = len(nl[0])
    c0 = par["cos0"]
    kappa = 1.0 / (1.0 / 3.0 + c0 * c0)
    i, j, d, r = row_entries(pos, types, nl, L, par, tilt=tilt)
    order = np.argsort(i, kind="stable")
    i, j, d, r = i[order], j[order], d[order], r[order]
    f, df = window(r, par)
    u = d / r[:, None]
    cnt = np.bincount(i, minlength=N)
    first = np.cumsum(cnt) - cnt
    A, W, n = np.zeros(N), np.zeros(N), np.zeros(N)
    dA, dW, dn = np.zeros((len(i), 3)), np.zeros((len(i), 3)), np.zeros((len(i), 3))
    for c in np.unique(cnt[cnt > 0]):
        rows = np.nonzero(cnt == c)[0]
        e = first[rows][:, None] + np.arange(c)[None, :]                 # (R, c) entry indices
        fe, dfe, ue, re = f[e], df[e], u[e], r[e]
        cosm = np.einsum("rja,rka->rjk", ue, ue)
        dev = cosm - c0
        ff = fe[:, :, None] * fe[:, None, :]
        upper = np.triu(np.ones((c, c), dtype=bool), 1)
        A[rows] = (ff * dev * dev * upper).sum(axis=(1, 2))              # the pair sum itself: j < k
        W[rows] = (ff * upper).sum(axis=(1, 2))
        n[rows] = fe.sum(axis=1)
        off = ~np.eye(c, dtype=bool)
        fk = fe[:, None, :] * off                                        # (R, j, k): f_k for k != j
        radial = (fk * dev * dev).sum(axis=2)                            # sum_{k != j} f_k (c_jk - cos0)^2
        # d(u_j.u_k)/dd_j = (u_k - c_jk u_j) / r_j
        trans = np.einsum("rjk,rka->rja", 2.0 * fk * dev, ue) - (2.0 * fk * dev * cosm).sum(axis=2)[:, :, None] * ue
        dA[e] = (dfe * radial)[:, :, None] * ue + (fe / re)[:, :, None] * trans
        dW[e] = (dfe * fk.sum(axis=2))[:, :, None] * ue
        dn[e] = dfe[:, :, None] * ue
    of_t = types[:N] == par["type"]
    n_t = int(of_t.sum())
    if par["normalise"]:
        ok = W >= W_MIN
        Ws = np.where(ok, W, 1.0)
        t = np.where(ok, 1.0 - kappa * A / Ws, 0.0)
        h, dh = h_of(t, par["switch"])
        g, dg = g_of(n, par["gate"])
        v = np.where(ok, g * h, 0.0)
        dt = -kappa * (dA * Ws[i][:, None] - A[i][:, None] * dW) / (Ws[i] ** 2)[:, None]
        ge = np.where(ok[i][:, None], (g * dh)[i][:, None] * dt + (dg * h)[i][:, None] * dn, 0.0)
        local = t
    else:
        assert par["switch"] is None and par["gate"] is None
        v, ge, local = A.copy(), dA, A.copy()
    s = float(v.sum()) / n_t if n_t else 0.0
    grad = np.zeros((N, 3))
    virial = np.zeros((N, 6))
    if n_t:
        for a in range(3):
            grad[:, a] = (np.bincount(j, weights=ge[:, a], minlength=N) - np.bincount(i, weights=ge[:, a], minlength=N)) / n_t
        for c6, (a, b) in enumerate(PAIRS6):
            w = ge[:, a] * d[:, b]
            virial[:, c6] = -0.5 * bias / n_t * (np.bincount(i, weights=w, minlength=N) + np.bincount(j, weights=w, minlength=N))
    return dict(s=s, n_t=n_t, local=local, switched=v, coordination=n, W=W, grad=grad, virial=virial, virial_sum=virial.sum(axis=0), r=r,
                entries=dict(i=i, j=j, d=d, g=ge))


def value(pos, types, L, nl, par, tilt=None):
    return compute(pos, types, L, nl, par, tilt=tilt)["s"]


def moment_form(d, r, par):
    """(A, W) of ONE row from its moments n, m, b, T: what the kernels evaluate"""
    f, _ = window(r, par)
    u = d / r[:, None]
    c0 = par["cos0"]
    n, m = f.sum(), (f * f).sum()
    b = (f[:, None] * u).sum(axis=0)
    T = np.einsum("e,ea,eb->ab", f, u, u)
    return 0.5 * (((T * T).sum() - m) - 2.0 * c0 * (b @ b - m) + c0 * c0 * (n * n - m)), 0.5 * (n * n - m)


def diamond_lattice(n, nn_dist=1.0):
    """n^3 cubic diamond cells x 8 particles, nearest-neighbour distance nn_dist; returns positions centred on 0 and box length"""
    a = nn_dist * 4.0 / np.sqrt(3.0)
    fcc = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    basis = np.concatenate([fcc, fcc + 0.25])
    cells = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    pos = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    L = n * a
    return pos - L / 2 + 0.125 * a, L
