"""fp64 restatement of the cluster pass (include/mtd_abi.h "Clusters", csrc/cluster.hip) and of the local Steinhardt variable restricted to
the largest cluster (mtd_ql_local_accumulate_cluster, cv.steinhardt_local(cluster=)).

    nodes   particles i < N of `type_id` with v_i >= v_min (NaN is not a node)
    edges   list entries (i, j): both ends nodes, j != i, j < N, |minImage(r_i - r_j)|^2 <= r_link^2; the list need not be symmetric
    label   scipy.sparse.csgraph.connected_components, relabelled to the smallest member index; NONE for a particle that is not a node
    largest most members, a tie to the smaller root;  w_i = 1 for its members, 0 else
    s       = sum_i w_i v_i / N_global

Membership is piecewise constant: the per-entry gradient is the scatter form of ql_local_bonds_ref.entry_gradients with w_i multiplying
g h' (beta_i) and g' h (the n-dependent part of a_i).  Pairs, smoothing, switch, gate and ramp are imported from the existing restatements;
the gradient is restated here because the mask enters in its middle.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.special import sph_harm_y

import ql_local_avg_ref
import ql_local_bonds_ref
import ql_local_ref

NONE = 0xffffffff
COMPONENTS = ql_local_bonds_ref.COMPONENTS


def listed(pos, nl, L, tilt=None):
    """(i, j, rsq) of every list entry with j < N and j != i, whatever the types"""
    head, nn, lst = (np.asarray(a).astype(np.int64) for a in nl)
    N = len(pos)
    i = np.repeat(np.arange(len(head)), nn)
    k = np.arange(len(i)) - np.repeat(np.cumsum(nn) - nn, nn)
    j = lst[np.repeat(head, nn) + k]
    keep = (j < N) & (j != i) & (i < N)
    i, j = i[keep], j[keep]
    d = ql_local_ref.min_image(np.asarray(pos, dtype=np.float64)[i] - np.asarray(pos, dtype=np.float64)[j], L, **(tilt or {}))
    return i, j, (d * d).sum(axis=1)


def nodes_of(types, type_id, v, v_min):
    with np.errstate(invalid="ignore"):
        return (np.asarray(types) == type_id) & (np.asarray(v, dtype=np.float64) >= v_min)


def clusters(pos, types, L, nl, type_id, v, v_min, r_link, tilt=None):
    """dict(label (N,) uint32, size (N,) uint32, w (N,) float64, summary (4,) uint32 = root, members, clusters, nodes, node (N,) bool)"""
    N = len(pos)
    node = nodes_of(types, type_id, v, v_min)
    i, j, rsq = listed(pos, nl, L, tilt)
    keep = node[i] & node[j] & (rsq <= r_link * r_link)
    i, j = i[keep], j[keep]
    graph = coo_matrix((np.ones(len(i)), (i, j)), shape=(N, N)).tocsr()
    n_comp, comp = connected_components(graph, directed=False)
    smallest = np.full(n_comp, N, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(N))
    label = smallest[comp]
    label[~node] = NONE
    size = np.zeros(N, dtype=np.uint32)
    roots, counts = np.unique(label[node], return_counts=True)          # roots ascending: argmax takes the smallest root of a tie
    size[roots] = counts
    w = np.zeros(N)
    summary = np.array([NONE, 0, len(roots), node.sum()], dtype=np.uint32)
    if len(roots):
        best = int(np.argmax(counts))
        summary[0], summary[1] = roots[best], counts[best]
        w[label == roots[best]] = 1.0
    return dict(label=label.astype(np.uint32), size=size, w=w, summary=summary, node=node)


def margins(pos, types, L, nl, type_id, v, v_min, r_link, tilt=None):
    """(the smallest |v_i - v_min| that is not exactly 0 over the particles of the type, the smallest | r / r_link - 1 | over the listed
    pairs of the type): how far rounding is from flipping a node or an edge"""
    types = np.asarray(types)
    v = np.asarray(v, dtype=np.float64)
    dv = np.abs(v[(types == type_id) & np.isfinite(v)] - v_min)
    dv = dv[dv != 0.0]
    i, j, rsq = listed(pos, nl, L, tilt)
    same = (types[i] == type_id) & (types[j] == type_id)
    dr = np.abs(np.sqrt(rsq[same]) / r_link - 1.0)
    return (dv.min() if len(dv) else np.inf), (dr.min() if len(dr) else np.inf)


def widest_gap(values, lo, hi):
    """the middle of the widest gap between consecutive sorted values inside [lo, hi], and half its width"""
    x = np.sort(np.asarray(values, dtype=np.float64))
    x = x[(x >= lo) & (x <= hi)]
    k = int(np.argmax(np.diff(x)))
    return 0.5 * (x[k] + x[k + 1]), 0.5 * (x[k + 1] - x[k])


def entry_gradients(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, w=None, tilt=None, switch=None, gate=None, bonds=None,
                    gradient=True, frame=None):
    """ql_local_bonds_ref.entry_gradients with the mask: dict(i, j, d, G, c, n, v, b, dent); v is UNMASKED, G is the gradient of
    N_global sum_i w_i v_i per entry.  w None: all ones."""
    pos = np.asarray(pos, dtype=np.float64)
    types = np.asarray(types)
    N = len(pos)
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    Ql_ref = np.asarray(Ql_ref, dtype=np.float64)
    i, j, d_lab = ql_local_ref.pairs(pos, types, nl, type_id, r_cut, tilt=tilt, L=L)
    d = ql_local_ref.to_frame(d_lab, frame)
    r = np.sqrt((d * d).sum(axis=1))
    f, df = ql_local_ref.smoothing(r, r_on, r_cut)
    theta = np.arccos(np.clip(d[:, 2] / r, -1.0, 1.0))
    phi = np.arctan2(d[:, 1], d[:, 0])
    n = np.bincount(i, weights=f, minlength=N)
    inv_n = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)

    def gather(x, at=i):
        return np.bincount(at, weights=x.real, minlength=N) + 1j * np.bincount(at, weights=x.imag, minlength=N)

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
        sg, dsg = ql_local_bonds_ref.ramp_fn(dent, bonds)
        b = np.bincount(i, weights=f * sg, minlength=N)
        h, dh = ql_local_avg_ref.switch_fn(b, switch)
    v = g * h
    out = dict(i=i, j=j, d=d_lab, G=None, c=c, n=n, v=v, b=b, dent=dent)
    if not gradient:
        return out
    beta = w * g * dh                                                    # the mask: w_i g h'
    if bonds is None:
        B = {k: beta * 2.0 * gl[k[0]] * np.conj(q[k]) for k in lm}
        wf = np.zeros(len(i))
    else:
        t = beta[i] * f * dsg
        td = np.bincount(i, weights=t * dent, minlength=N) + np.bincount(j, weights=t * dent, minlength=N)
        B = {}
        for k in lm:
            T = gather(t * u[k][j], i) + gather(t * u[k][i], j)
            B[k] = gl[k[0]] * np.conj((T - td * u[k]) * inv_rc)
        wf = beta[i] * sg
    a = w * dg * h                                                       # the mask: w_i g' h
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


def compute(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, cluster=None, n_global=None, tilt=None, gradient=True, switch=None,
            gate=None, bonds=None, bias=None, frame=None):
    """cluster = (v_min, r_link) or None (the unmasked variable).  dict(s, c, v (unmasked), n, b, w, label, size, summary, grad (N, 3));
    with `bias` also virial (N, 6), W (6,) and tensor (3, 3), as ql_local_bonds_ref.compute"""
    N = len(pos)
    n_global = N if n_global is None else n_global
    opt = dict(tilt=tilt, switch=switch, gate=gate, bonds=bonds, frame=frame)
    out = {}
    w = np.ones(N)
    if cluster is not None:
        v0 = entry_gradients(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, gradient=False, **opt)["v"]
        cl = clusters(pos, types, L, nl, type_id, v0, cluster[0], cluster[1], tilt=tilt)
        w = cl["w"]
        out.update(label=cl["label"], size=cl["size"], summary=cl["summary"])
    e = entry_gradients(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, w=w, gradient=gradient, **opt)
    out.update({k: e[k] for k in ("c", "v", "n", "b", "dent", "i", "j")})
    out["w"] = w
    out["s"] = (w * e["v"]).sum() / n_global
    out["grad"] = None
    if gradient:
        i, j, d, G = e["i"], e["j"], e["d"], e["G"]
        grad = np.zeros((N, 3))
        for k in range(3):
            grad[:, k] = np.bincount(i, weights=G[:, k], minlength=N) - np.bincount(j, weights=G[:, k], minlength=N)
        out["grad"] = grad / n_global
        if bias is not None:
            Fp = -bias * G / n_global
            virial = np.zeros((N, 6))
            for cc, (a, bb) in enumerate(COMPONENTS):
                x = 0.5 * d[:, a] * Fp[:, bb]
                virial[:, cc] = np.bincount(i, weights=x, minlength=N) + np.bincount(j, weights=x, minlength=N)
            out.update(virial=virial, W=virial.sum(axis=0), tensor=d.T @ Fp)
    return out


def strain_derivative(pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, eps, w, n_global=None, tilt=None, **opt):
    """(6,): d(sum_i w_i v_i / N_global) / d eps_ab by central differences under ql_local_virial_ref.strain, list and mask kept"""
    from ql_local_virial_ref import strain
    n_global = len(pos) if n_global is None else n_global
    out = np.zeros(6)
    for cc, (a, bb) in enumerate(COMPONENTS):
        s = []
        for sign in (1.0, -1.0):
            p2, L2, t2 = strain(pos, L, tilt, a, bb, sign * eps)
            v = entry_gradients(p2, types, L2, nl, r_cut, r_on, lmax, type_id, Ql_ref, tilt=t2, gradient=False, **opt)["v"]
            s.append((w * v).sum() / n_global)
        out[cc] = (s[0] - s[1]) / (2.0 * eps)
    return out


def two_crystallites(seed=21, n_gas=1200, other=0.08, jitter=0.04, L=18.0):
    """a jittered fcc crystallite of 4 x 4 x 4 cells (256 particles) and one of 2 x 2 x 2 cells (32) in a random gas of the same type
    that keeps 1.0 clear of both, a second type sprinkled over everything: dict(pos, types, L, big, small (index arrays))"""
    import util
    rng = np.random.default_rng(seed)
    a, _ = util.fcc_lattice(4)
    b, _ = util.fcc_lattice(2)
    a = a - a.mean(axis=0) + np.array([-3.5, -3.5, -3.5])
    b = b - b.mean(axis=0) + np.array([4.5, 4.5, 4.5])
    crystal = np.concatenate([a, b]) + rng.normal(0, jitter, (len(a) + len(b), 3))
    gas = []
    while len(gas) < n_gas:
        p = rng.uniform(-0.5 * L, 0.5 * L, 3)
        d = crystal - p
        d -= L * np.rint(d / L)
        if (d * d).sum(axis=1).min() < 1.0:
            continue
        if gas:
            g = np.array(gas) - p
            g -= L * np.rint(g / L)
            if (g * g).sum(axis=1).min() < 0.7 ** 2:
                continue
        gas.append(p)
    pos = np.concatenate([crystal, np.array(gas)])
    order = rng.permutation(len(pos))                                    # the crystallites are not contiguous index ranges
    inverse = np.argsort(order)
    pos = pos[order]
    pos = pos - L * np.rint(pos / L)
    types = (rng.random(len(pos)) < other).astype(np.int32)
    return dict(pos=pos, types=types, L=L, big=np.sort(inverse[:len(a)]), small=np.sort(inverse[len(a):len(a) + len(b)]))


E6 = [0, 0, 0, 0, 0, 0, 1]
ARGS = dict(r_cut=1.4, r_on=1.2, lmax=6, type_id=0, Ql_ref=E6)
R_LINK_WINDOW = (1.15, 1.3)
# the option combinations of the parity tests on two_crystallites(), each with the window v_min is looked for in: below the values of the
# crystallites' particles, so that both crystallites are clusters (q6 alone does not tell a crystal from a gas particle with two
# neighbours: without the bond count or a gate much of the gas is solid too, and hangs on to whatever it touches)
COMBOS = {
    "plain": (dict(), (0.15, 0.25)),
    "switch": (dict(switch=(0.2, 6)), (0.5, 0.8)),
    "switch+gate": (dict(switch=(0.2, 6), gate=(4, 9)), (0.2, 0.4)),
    "bonds+switch": (dict(bonds=(0.5, 0.7), switch=(6.5, 12)), (0.1, 0.4)),
    "bonds+switch+gate": (dict(bonds=(0.3, 0.8), switch=(4.5, 6), gate=(6, 10)), (0.1, 0.3)),
}


def choose(pos, types, L, nl, opt, window, type_id=0, tilt=None, args=None):
    """(v_min, r_link) in the widest gap of the v_i inside `window` and of the listed pair distances inside R_LINK_WINDOW, and the
    margins() of that choice"""
    args = dict(ARGS if args is None else args, type_id=type_id)
    v = entry_gradients(pos, types, L, nl, tilt=tilt, gradient=False, **args, **opt)["v"]
    v_min, _ = widest_gap(v[np.asarray(types) == type_id], *window)
    i, j, rsq = listed(pos, nl, L, tilt)
    same = (np.asarray(types)[i] == type_id) & (np.asarray(types)[j] == type_id)
    r_link, _ = widest_gap(np.sqrt(rsq[same]), *R_LINK_WINDOW)
    return (v_min, r_link), margins(pos, types, L, nl, type_id, v, v_min, r_link, tilt=tilt)


def far_from_members(pos, L, w, reach, tilt=None):
    """(N,) bool: not a member, and no member within `reach` (minimum image)"""
    pos = np.asarray(pos, dtype=np.float64)
    members = np.nonzero(w)[0]
    far = np.asarray(w) == 0.0
    if len(members) == 0:
        return far
    for k in np.nonzero(far)[0]:
        d = ql_local_ref.min_image(pos[members] - pos[k], L, **(tilt or {}))
        far[k] = (d * d).sum(axis=1).min() > reach * reach
    return far
