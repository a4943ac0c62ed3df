"""fp64 numpy restatement of the pair entropy (cv.pair_entropy, include/mtd_abi.h "Pair entropy"), vectorised over the entries of the
list, with an ANALYTIC gradient in the scatter form (every entry gives +u d/r to its centre and -u d/r to its neighbour) — independent of
the gather form the GPU pass uses, which is returned beside it — and the virial (pair part per particle, explicit volume part).

    Delta = r_max / B,  r_b = (b + 1/2) Delta,  r_on = r_max + 3 sigma,  r_cut = r_max + 4 sigma,  w = ceil(6 sigma / Delta)
    K(x) = exp(-x^2 / 2 sigma^2) / (sqrt(2 pi) sigma),  b_c = floor(r B / r_max),  window |b - b_c| <= w, 0 <= b < B
    H_b = sum_entries f(r) K(r_b - r),  N_t = central particles of the type,  rho = N_t / V
    g_b = H_b / (4 pi N_t rho r_b^2),  phi_b = g ln g - g + 1 (g >= 1e-10, else 1),  S = -2 pi rho Delta sum_b r_b^2 phi_b
"""
import math

import numpy as np

from ql_local_ref import min_image, smoothing

G_MIN = 1e-10
CHUNK = 1 << 15                 # entries per slab of the (entries, bins) arrays


def _window(r, c, r_max, sigma_r, n_bins):
    """K(r_b - r) inside the window of every entry (0 outside) and x = r_b - r; (len(r), n_bins) each"""
    bc = np.floor(r * (n_bins / r_max)).astype(np.int64)
    x = c["r_b"][None, :] - r[:, None]
    K = np.exp(-x * x / (2.0 * sigma_r ** 2)) / (math.sqrt(2.0 * math.pi) * sigma_r)
    return np.where(np.abs(np.arange(n_bins)[None, :] - bc[:, None]) <= c["w"], K, 0.0), x


def constants(r_max, sigma_r, n_bins):
    delta = r_max / n_bins
    return dict(delta=delta, r_b=(np.arange(n_bins) + 0.5) * delta, r_on=r_max + 3.0 * sigma_r, r_cut=r_max + 4.0 * sigma_r,
                w=int(math.ceil(6.0 * sigma_r / delta)))


def entries(pos, types, nl, type_id, r_cut, L, tilt=None, rows=None):
    """(i, j, d) of the list entries that take part: i a central particle (a row of the list, in `rows` when given), both of `type_id`,
    j != i, r <= r_cut; j may index a particle behind the rows (a ghost)"""
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
    d = min_image(pos[i] - pos[j], L, **(tilt or {}))
    r = np.sqrt((d * d).sum(axis=1))
    keep = r <= r_cut
    return i[keep], j[keep], d[keep]


def sums(pos, types, L, nl, r_max, sigma_r, n_bins, type_id, tilt=None, rows=None):
    """this domain's sums: H_b [n_bins] and N_t — what the ranks of a domain-decomposed run add up"""
    c = constants(r_max, sigma_r, n_bins)
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    i, j, d = entries(pos, types, nl, type_id, c["r_cut"], L, tilt=tilt, rows=rows)
    r = np.sqrt((d * d).sum(axis=1))
    f, _ = smoothing(r, c["r_on"], c["r_cut"])
    H = np.zeros(n_bins)
    for lo in range(0, len(r), CHUNK):
        K, _ = _window(r[lo:lo + CHUNK], c, r_max, sigma_r, n_bins)
        H += (f[lo:lo + CHUNK, None] * K).sum(axis=0)
    n_rows = len(nl[0])
    central = np.arange(n_rows) if rows is None else np.asarray(rows)
    n_t = int((types[central] == type_id).sum())
    return H, n_t


def finalize(H, n_t, L, r_max, sigma_r, n_bins):
    """dict(S, g, W, explicit): the value, g_b, W_b = dS/dH_b and the explicit volume derivative dS/d eps_aa"""
    c = constants(r_max, sigma_r, n_bins)
    if n_t == 0:
        return dict(S=0.0, g=np.zeros(n_bins), W=np.zeros(n_bins), explicit=0.0)
    V = float(np.prod(np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))))
    rho = n_t / V
    r2 = c["r_b"] ** 2
    g = H / (4.0 * math.pi * n_t * rho * r2)
    on = g >= G_MIN
    lg = np.log(np.where(on, g, 1.0))
    phi = np.where(on, g * lg - g + 1.0, 1.0)
    S = -2.0 * math.pi * rho * c["delta"] * (r2 * phi).sum()
    W = np.where(on, -c["delta"] * lg / (2.0 * n_t), 0.0)
    explicit = -(S + 2.0 * math.pi * rho * c["delta"] * (r2 * g * lg)[on].sum())
    return dict(S=S, g=g, W=W, explicit=explicit)


def compute(pos, types, L, nl, r_max, sigma_r, n_bins, type_id, tilt=None, rows=None, sums_override=None, bias=1.0):
    """returns dict(S, g, H, n_t, W, grad, gather, virial, virial_sum, explicit)
    grad    (len(pos), 3): dS/dr in the scatter form, ghosts included
    gather  (rows, 3): 2 sum_{j in row k} u_kj d_kj / r_kj — what the force pass forms; equals grad on a symmetric full list
    virial  (rows, 6): -bias (1/2 sum_j d_a G_kj,b + explicit / N_t on the diagonal of central particles of the type)
    sums_override: (H, N_t) of the WHOLE system when this call sees one domain (rows / a shard) only"""
    c = constants(r_max, sigma_r, n_bins)
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    H, n_t = sums(pos, types, L, nl, r_max, sigma_r, n_bins, type_id, tilt=tilt, rows=rows)
    if sums_override is not None:
        H, n_t = sums_override
    fin = finalize(H, n_t, L, r_max, sigma_r, n_bins)
    i, j, d = entries(pos, types, nl, type_id, c["r_cut"], L, tilt=tilt, rows=rows)
    r = np.sqrt((d * d).sum(axis=1))
    f, df = smoothing(r, c["r_on"], c["r_cut"])
    u = np.zeros(len(r))
    for lo in range(0, len(r), CHUNK):
        K, x = _window(r[lo:lo + CHUNK], c, r_max, sigma_r, n_bins)
        u[lo:lo + CHUNK] = (fin["W"][None, :] * K * (df[lo:lo + CHUNK, None] + f[lo:lo + CHUNK, None] * x / sigma_r ** 2)).sum(axis=1)
    G = (u / r)[:, None] * d
    n_rows = len(nl[0])
    grad = np.zeros((len(pos), 3))
    gather = np.zeros((n_rows, 3))
    for a in range(3):
        grad[:, a] = np.bincount(i, weights=G[:, a], minlength=len(pos)) - np.bincount(j, weights=G[:, a], minlength=len(pos))
        gather[:, a] = 2.0 * np.bincount(i, weights=G[:, a], minlength=n_rows)
    virial = np.zeros((n_rows, 6))
    for c6, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        virial[:, c6] = -bias * np.bincount(i, weights=d[:, a] * G[:, b], minlength=n_rows)      # 1/2 d_a (2 u d_b / r)
    central = np.arange(n_rows) if rows is None else np.asarray(rows)
    central = central[types[central] == type_id]
    if n_t:
        for c6 in (0, 3, 5):
            virial[central, c6] += -bias * fin["explicit"] / n_t
    return dict(S=fin["S"], g=fin["g"], H=H, n_t=n_t, W=fin["W"], grad=grad, gather=gather, virial=virial, virial_sum=virial.sum(axis=0),
                explicit=fin["explicit"], r_b=c["r_b"])


def value(pos, types, L, nl, r_max, sigma_r, n_bins, type_id, tilt=None):
    H, n_t = sums(pos, types, L, nl, r_max, sigma_r, n_bins, type_id, tilt=tilt)
    return finalize(H, n_t, L, r_max, sigma_r, n_bins)["S"]


def brute_nlist(pos, h, r):
    """full list of a triclinic box (lattice vectors in the columns of h), O(N^2), images -1..1"""
    N = len(pos)
    shifts = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.float64) @ h.T
    rows = []
    for i in range(N):
        d = pos[i] - pos
        best = np.min(((d[:, None, :] + shifts[None, :, :]) ** 2).sum(-1), axis=1)
        rows.append(np.nonzero((best <= r * r) & (np.arange(N) != i))[0])
    nn = np.array([len(x) for x in rows], dtype=np.uint32)
    head = np.zeros(N, dtype=np.uint32)
    head[1:] = np.cumsum(nn)[:-1]
    return head, nn, np.concatenate(rows).astype(np.uint32)
