"""fp64 numpy restatement of the coordination number (cv.coordination, include/mtd_abi.h "Coordination number"), vectorised over the entries
of the list, with an ANALYTIC gradient in the scatter form (every entry (i in A, j in B) gives +g'(n_i) s~' d/r to its centre and the
opposite to its partner, over N_A) — independent of the gather form the GPU pass uses, which is returned beside it — and the
per-particle virial.

    x = max(r - d_0, 0) / r_0,  s(x) = P_n(x) / P_m(x),  P_k(x) = 1 + x + ... + x^(k-1)      (P_k and P_k' by Horner's rule)
    s~(r) = (s - s_c) / (1 - s_c),  s_c = s((r_cut - d_0) / r_0);  s~(r <= d_0) = 1 with gradient 0
    n_i = sum_{j in row i, j of type B} s~(r_ij) for i of type A,  v_i = g(n_i),  s = (1 / N_A) sum_i v_i
    g(c) = c, or h(c) = y^p / (1 + y^p) with y = c / c0, or 1 - h (less)
"""
import numpy as np

from pair_entropy_ref import brute_nlist, min_image      # noqa: F401

PAIRS6 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def params(type_a, type_b, r_0, r_cut, d_0=0.0, n=6, m=12, switch=None):
    """switch: None or (c0, p[, less])"""
    return dict(type_a=type_a, type_b=type_b, r_0=float(r_0), r_cut=float(r_cut), d_0=float(d_0), n=int(n), m=int(m), switch=switch)


def geometric(x, k):
    """P_k(x) = 1 + x + ... + x^(k-1) and P_k'(x), by Horner's rule"""
    x = np.asarray(x, dtype=np.float64)
    p, dp = np.ones_like(x), np.zeros_like(x)
    for _ in range(k - 1):
        dp = dp * x + p
        p = p * x + 1.0
    return p, dp


def rational(x, n, m):
    """s(x) = P_n / P_m and ds/dx: THE definition"""
    pn, dpn = geometric(x, n)
    pm, dpm = geometric(x, m)
    s = pn / pm
    return s, (dpn - s * dpm) / pm


def quotient(x, n, m):
    """(1 - x^n) / (1 - x^m) and its derivative as written: 0 / 0 at x = 1, digits lost beside it"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        num, den = 1.0 - x ** n, 1.0 - x ** m
        s = num / den
        ds = (-n * x ** (n - 1) * den + m * x ** (m - 1) * num) / (den * den)
    return s, ds


def switching(r, par):
    """s~(r) and ds~/dr of every entry"""
    r = np.asarray(r, dtype=np.float64)
    s_c = float(rational((par["r_cut"] - par["d_0"]) / par["r_0"], par["n"], par["m"])[0])
    over = r - par["d_0"]
    s, ds = rational(np.maximum(over, 0.0) / par["r_0"], par["n"], par["m"])
    st = (s - s_c) / (1.0 - s_c)
    dst = ds / par["r_0"] / (1.0 - s_c)
    inner = over <= 0.0
    return np.where(inner, 1.0, st), np.where(inner, 0.0, dst)


def g_of(n_i, switch):
    """v = g(n) and g'(n)"""
    if switch is None:
        return n_i.copy(), np.ones_like(n_i)
    c0, p = float(switch[0]), int(switch[1])
    less = bool(switch[2]) if len(switch) > 2 else False
    y = n_i / c0
    yp = y ** p
    h = yp / (1.0 + yp)
    dh = p * y ** (p - 1) / c0 / (1.0 + yp) ** 2
    return (1.0 - h, -dh) if less else (h, dh)


def row_entries(pos, nl, L, r_cut, tilt=None, rows=None):
    """(i, j, d, r) of the list entries with j != i and r <= r_cut, whatever the types: i a central particle (a row of the list, in `rows`
    when given); j may index a particle behind the rows (a ghost)"""
    head, nn, lst = (np.asarray(a).astype(np.int64) for a in nl)
    n_rows = len(head)
    i = np.repeat(np.arange(n_rows), nn)
    k = np.arange(len(i)) - np.repeat(np.cumsum(nn) - nn, nn)
    j = lst[np.repeat(head, nn) + k]
    keep = i != j
    if rows is not None:
        mask = np.zeros(n_rows, dtype=bool)
        mask[rows] = True
        keep &= mask[i]
    i, j = i[keep], j[keep]
    d = min_image(pos[i] - pos[j], L, **(tilt or {}))
    r = np.sqrt((d * d).sum(axis=1))
    keep = r <= r_cut
    return i[keep], j[keep], d[keep], r[keep]


def compute(pos, types, L, nl, par, tilt=None, rows=None, sums_override=None, bias=1.0):
    """returns dict(s, n_a, v_sum, local, switched, grad, gather, virial, virial_sum)
    local    (rows,): n_i (0 for particles that are not of type A and for rows outside `rows`)
    switched (rows,): v_i = g(n_i)
    grad     (len(pos), 3): ds/dr in the scatter form, ghosts included
    gather   (rows, 3): what the force pass forms (module docstring of the header); equals grad on a symmetric full list
    virial   (rows, 6): -(bias / (2 N_A)) sum_{j in row k} s~' d_a d_b / r (bracket)
    sums_override: (sum v_i, N_A) of the WHOLE system when this call sees one domain (rows / a shard) only; with ghosts the gather form
    needs g'(n_j) of a ghost and is formed for the plain variable only"""
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    A, B = par["type_a"], par["type_b"]
    n_rows = len(nl[0])
    i, j, d, r = row_entries(pos, nl, L, par["r_cut"], tilt=tilt, rows=rows)
    st, dst = switching(r, par)
    as_centre = (types[i] == A) & (types[j] == B)
    as_partner = (types[i] == B) & (types[j] == A)
    central = np.arange(n_rows) if rows is None else np.asarray(rows)
    central = central[types[central] == A]
    is_a = np.zeros(n_rows, dtype=bool)
    is_a[central] = True
    local = np.bincount(i[as_centre], weights=st[as_centre], minlength=n_rows) * is_a
    v, dv = g_of(local, par["switch"])
    v, dv = v * is_a, dv * is_a
    v_sum, n_a = float(v.sum()), len(central)
    if sums_override is not None:
        v_sum, n_a = sums_override
    s = v_sum / n_a if n_a > 0 else 0.0
    dg = np.zeros(len(pos))                                # g'(n_j): of the rows, and 1 for every A particle of the plain variable
    dg[:n_rows] = dv
    if par["switch"] is None:
        dg[:] = (types == A)
    elif len(pos) > n_rows or rows is not None:
        dg[:] = np.nan                                     # not defined: the entry points refuse it
        dg[:n_rows] = dv
    unit = np.where(r > 0.0, 1.0 / np.where(r > 0.0, r, 1.0), 0.0)[:, None] * d
    slope = (dst / max(n_a, 1))[:, None] * unit            # s~' d / r / N_A of every entry
    grad = np.zeros((len(pos), 3))
    gather = np.zeros((n_rows, 3))
    w_scatter = np.where(as_centre, dg[i], 0.0)
    w_gather = np.where(as_centre, dg[i], 0.0) + np.where(as_partner, dg[j], 0.0)
    for a in range(3):
        t = w_scatter * slope[:, a]
        grad[:, a] = np.bincount(i, weights=t, minlength=len(pos)) - np.bincount(j, weights=t, minlength=len(pos))
        gather[:, a] = np.bincount(i, weights=w_gather * slope[:, a], minlength=n_rows)
    virial = np.zeros((n_rows, 6))
    for c6, (a, b) in enumerate(PAIRS6):
        virial[:, c6] = -0.5 * bias * np.bincount(i, weights=w_gather * d[:, a] * slope[:, b], minlength=n_rows)
    return dict(s=s, n_a=n_a, v_sum=v_sum, local=local, switched=v, grad=grad, gather=gather, virial=virial, virial_sum=virial.sum(axis=0))


def value(pos, types, L, nl, par, tilt=None):
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    n_rows = len(nl[0])
    i, j, d, r = row_entries(pos, nl, L, par["r_cut"], tilt=tilt)
    keep = (types[i] == par["type_a"]) & (types[j] == par["type_b"])
    st, _ = switching(r[keep], par)
    is_a = types[:n_rows] == par["type_a"]
    local = np.bincount(i[keep], weights=st, minlength=n_rows)
    v, _ = g_of(local, par["switch"])
    n_a = int(is_a.sum())
    return float((v * is_a).sum()) / n_a if n_a else 0.0
