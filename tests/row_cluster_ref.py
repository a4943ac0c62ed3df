"""fp64 restatement of the coordination number and of the tetrahedral order restricted to the largest cluster
(mtd_coord_accumulate_cluster, mtd_tetrahedral_accumulate_cluster; cv.coordination.set_cluster, cv.tetrahedral.set_cluster):

    s = (1 / N_type) sum_i w_i v_i          N_type the UNMASKED count (N_A, N_t)

v_i and its derivative come from the existing restatements (coordination_ref.compute / g_of, tetrahedral_ref.compute), the 0 / 1 mask
w from ql_local_cluster_ref.clusters built on these v_i with `type` = the variable's central type.  Membership is piecewise constant:
the gradient is the variable's own with the per-particle table entry of particle i times w_i —
    coordination   g'(n_i) -> w_i g'(n_i)
    tetrahedral    alpha_i -> w_i alpha_i       (g_ij = dv_i / dd_ij is linear in alpha_i: w_i g_ij)
The force and the per-particle virial with the masked table are restated HERE, in the gather form over the rows of a symmetric full list
(what the force passes form); single domain, no ghosts.
"""
import numpy as np

import coordination_ref as cn
import ql_local_cluster_ref as cl
import tetrahedral_ref as tr

NONE = cl.NONE
PAIRS6 = cn.PAIRS6


def _mask(pos, types, L, nl, type_id, v, cluster, w, tilt):
    """(w, the dict of ql_local_cluster_ref.clusters or None): cluster = (v_min, r_link) builds the mask, else `w` (None: all ones)"""
    if cluster is not None:
        c = cl.clusters(pos, types, L, nl, type_id, v, cluster[0], cluster[1], tilt=tilt)
        return c["w"], c
    return (np.ones(len(pos)) if w is None else np.asarray(w, dtype=np.float64)), None


def coordination(pos, types, L, nl, par, cluster=None, w=None, tilt=None, bias=1.0):
    """dict(s, n_a, local, switched (UNMASKED), w, label, size, summary, grad (N, 3) = ds/dr, force = -bias grad, virial (N, 6),
    virial_sum); par needs a switch.  cluster = (v_min, r_link), or a frozen mask `w`, or neither (w = 1)"""
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    N = len(nl[0])
    assert len(pos) == N and par["switch"] is not None
    A, B = par["type_a"], par["type_b"]
    base = cn.compute(pos, types, L, nl, par, tilt=tilt)
    v, n_a = base["switched"], base["n_a"]
    _, dv = cn.g_of(base["local"], par["switch"])
    dv = dv * (types == A)
    w, c = _mask(pos, types, L, nl, A, v, cluster, w, tilt)
    table = w * dv                                                       # the masked table: w_i g'(n_i)
    i, j, d, r = cn.row_entries(pos, nl, L, par["r_cut"], tilt=tilt)
    _, dst = cn.switching(r, par)
    bracket = np.where((types[i] == A) & (types[j] == B), table[i], 0.0) + np.where((types[i] == B) & (types[j] == A), table[j], 0.0)
    unit = np.where(r > 0.0, 1.0 / np.where(r > 0.0, r, 1.0), 0.0)[:, None] * d
    slope = (bracket * dst / max(n_a, 1))[:, None] * unit
    grad = np.stack([np.bincount(i, weights=slope[:, a], minlength=N) for a in range(3)], axis=1)
    virial = np.stack([-0.5 * bias * np.bincount(i, weights=d[:, a] * slope[:, b], minlength=N) for a, b in PAIRS6], axis=1)
    out = dict(s=float((w * v).sum()) / n_a if n_a else 0.0, n_a=n_a, local=base["local"], switched=v, w=w, grad=grad, force=-bias * grad,
               virial=virial, virial_sum=virial.sum(axis=0), label=None, size=None, summary=None)
    if c is not None:
        out.update(label=c["label"], size=c["size"], summary=c["summary"])
    return out


def tetrahedral(pos, types, L, nl, par, cluster=None, w=None, tilt=None, bias=1.0):
    """dict(s, n_t, local, switched (UNMASKED), coordination, w, label, size, summary, grad, force, virial (N, 6), virial_sum); par is
    normalised.  Row k of a symmetric list holds (k, j) and its mirror (j, k) is an entry too: the gather over row k,
    sum_j [-w_k g_kj + w_j g_jk], is minus the entries that start at k plus those that end there"""
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    N = len(nl[0])
    assert len(pos) == N and par["normalise"]
    base = tr.compute(pos, types, L, nl, par, tilt=tilt)
    v, n_t = base["switched"], base["n_t"]
    w, c = _mask(pos, types, L, nl, par["type"], v, cluster, w, tilt)
    e = base["entries"]
    i, j, d = e["i"], e["j"], e["d"]
    g = w[i][:, None] * e["g"]                                           # the masked table: w_i alpha_i
    grad, virial = np.zeros((N, 3)), np.zeros((N, 6))
    if n_t:
        grad = np.stack([np.bincount(j, weights=g[:, a], minlength=N) - np.bincount(i, weights=g[:, a], minlength=N) for a in range(3)], axis=1) / n_t
        virial = np.stack([-0.5 * bias / n_t * (np.bincount(i, weights=g[:, a] * d[:, b], minlength=N)
                                                + np.bincount(j, weights=g[:, a] * d[:, b], minlength=N)) for a, b in PAIRS6], axis=1)
    out = dict(s=float((w * v).sum()) / n_t if n_t else 0.0, n_t=n_t, local=base["local"], switched=v, coordination=base["coordination"], w=w,
               grad=grad, force=-bias * grad, virial=virial, virial_sum=virial.sum(axis=0), label=None, size=None, summary=None)
    if c is not None:
        out.update(label=c["label"], size=c["size"], summary=c["summary"])
    return out


def masked_value(kind, pos, types, L, nl, par, w, tilt=None):
    """sum_i w_i v_i / N_type at these positions with the mask FROZEN: what the finite differences of the tests differentiate"""
    ref, count = (cn, "n_a") if kind == "coordination" else (tr, "n_t")
    r = ref.compute(pos, types, L, nl, par, tilt=tilt)
    return float((np.asarray(w) * r["switched"]).sum()) / r[count] if r[count] else 0.0


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
R_LINK_WINDOW = cl.R_LINK_WINDOW                                         # coordination: (1.15, 1.3), on two_crystallites()
COORD_LIST = 1.55
COORD_PAR = dict(type_a=0, type_b=0, r_0=1.2, r_cut=1.5)
# option sets of the parity tests, each with the window v_min is looked for in.  `less` counts v = 1 - h: the gap of the switch, mirrored
COORD_COMBOS = {
    "switch": ((6, 8), (0.2, 0.5)),
    "switch+less": ((6, 8, True), (0.5, 0.8)),
}
TET_LIST = 1.45
TET_ARGS = dict(r_cut=1.4, r_on=1.2)
TET_R_LINK_WINDOW = (1.1, 1.35)
TET_COMBOS = {
    "plain": (dict(), (0.6, 0.95)),
    "switch": (dict(switch=(0.7, 8)), (0.2, 0.8)),
    "switch+gate": (dict(switch=(0.7, 8), gate=(1.5, 3.0)), (0.1, 0.6)),
}


def two_diamonds(seed=5, n_gas=700, other=0.08, jitter=0.03, L=18.0):
    """ql_local_cluster_ref.two_crystallites() with diamond: a jittered crystallite of 3 x 3 x 3 cells (216 particles) and one of
    2 x 2 x 2 cells (64), nearest-neighbour distance 1, in a random gas that keeps 1.5 clear of both and 0.8 clear of itself, a second
    type sprinkled over everything, indices shuffled: dict(pos, types, L, big, small (index arrays))"""
    rng = np.random.default_rng(seed)
    a, _ = tr.diamond_lattice(3)
    b, _ = tr.diamond_lattice(2)
    a = a - a.mean(axis=0) + np.array([-3.5, -3.5, -3.5])
    b = b - b.mean(axis=0) + np.array([4.5, 4.5, 4.5])
    crystal = np.concatenate([a, b]) + rng.normal(0, jitter, (len(a) + len(b), 3))
    gas = []
    while len(gas) < n_gas:
        p = rng.uniform(-0.5 * L, 0.5 * L, 3)
        d = crystal - p
        d -= L * np.rint(d / L)
        if (d * d).sum(axis=1).min() < 1.5 ** 2:
            continue
        if gas:
            g = np.array(gas) - p
            g -= L * np.rint(g / L)
            if (g * g).sum(axis=1).min() < 0.8 ** 2:
                continue
        gas.append(p)
    pos = np.concatenate([crystal, np.array(gas)])
    order = rng.permutation(len(pos))
    inverse = np.argsort(order)
    pos = pos[order]
    pos = pos - L * np.rint(pos / L)
    types = (rng.random(len(pos)) < other).astype(np.int32)
    return dict(pos=pos, types=types, L=L, big=np.sort(inverse[:len(a)]), small=np.sort(inverse[len(a):len(a) + len(b)]))


def choose(pos, types, L, nl, v, type_id, v_window, r_window):
    """(v_min, r_link) in the widest gap of the v_i of the type inside v_window and of the listed same-type pair distances inside r_window,
    and ql_local_cluster_ref.margins of that choice"""
    types = np.asarray(types)
    v_min, _ = cl.widest_gap(np.asarray(v)[types == type_id], *v_window)
    i, j, rsq = cl.listed(pos, nl, L)
    same = (types[i] == type_id) & (types[j] == type_id)
    r_link, _ = cl.widest_gap(np.sqrt(rsq[same]), *r_window)
    return (v_min, r_link), cl.margins(pos, types, L, nl, type_id, v, v_min, r_link)


_CACHE = {}


def _fixture(key, make, r_list, dtype):
    """the fixture with its positions rounded to `dtype` (the snapshot IS the rounded array) and the list built on those; built once"""
    import util
    if (key, dtype) not in _CACHE:
        if key not in _CACHE:
            _CACHE[key] = make()
        f = dict(_CACHE[key])
        f["pos"] = f["pos"].astype(dtype).astype(np.float64)
        f["nl"] = util.build_nlist(f["pos"], f["L"], r_list)
        _CACHE[(key, dtype)] = f
    return _CACHE[(key, dtype)]


def coordination_case(name, dtype=np.float64):
    """dict(pos, types, L, nl, par, cluster, margins, ref, big, small) of an option set of COORD_COMBOS on two_crystallites(), the list to
    COORD_LIST, (v_min, r_link) chosen on these positions; built once per array type"""
    if ("cn", name, dtype) not in _CACHE:
        f = _fixture("cn", cl.two_crystallites, COORD_LIST, dtype)
        switch, window = COORD_COMBOS[name]
        par = cn.params(switch=switch, **COORD_PAR)
        v = cn.compute(f["pos"], f["types"], f["L"], f["nl"], par)["switched"]
        cluster, margins = choose(f["pos"], f["types"], f["L"], f["nl"], v, 0, window, R_LINK_WINDOW)
        ref = coordination(f["pos"], f["types"], f["L"], f["nl"], par, cluster=cluster)
        _CACHE[("cn", name, dtype)] = dict(f, par=par, cluster=cluster, margins=margins, ref=ref)
    return _CACHE[("cn", name, dtype)]


def tetrahedral_case(name, dtype=np.float64):
    """the same for an option set of TET_COMBOS on two_diamonds(), the list to TET_LIST"""
    if ("tet", name, dtype) not in _CACHE:
        f = _fixture("tet", two_diamonds, TET_LIST, dtype)
        opt, window = TET_COMBOS[name]
        par = tr.params(0, TET_ARGS["r_cut"], TET_ARGS["r_on"], **opt)
        v = tr.compute(f["pos"], f["types"], f["L"], f["nl"], par)["switched"]
        cluster, margins = choose(f["pos"], f["types"], f["L"], f["nl"], v, 0, window, TET_R_LINK_WINDOW)
        ref = tetrahedral(f["pos"], f["types"], f["L"], f["nl"], par, cluster=cluster)
        _CACHE[("tet", name, dtype)] = dict(f, par=par, cluster=cluster, margins=margins, ref=ref)
    return _CACHE[("tet", name, dtype)]


def cut(case, n, r_list=COORD_LIST):
    """the n particles of the big crystallite of a case nearest to its centre (a compact blob, in index order), alone in the box, with
    their own list"""
    import util
    big = case["big"]
    d = case["pos"][big] - case["pos"][big].mean(axis=0)
    keep = np.sort(big[np.argsort((d * d).sum(axis=1), kind="stable")[:n]])
    pos, types = case["pos"][keep], case["types"][keep]
    return dict(pos=pos, types=types, L=case["L"], nl=util.build_nlist(pos, case["L"], r_list), par=case["par"])


far_from_members = cl.far_from_members
