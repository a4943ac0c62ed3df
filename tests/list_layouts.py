"""Neighbour lists in HOOMD's row layout, and rows of every length (helper, no test).

Every list entry point of include/mtd_abi.h reads the neighbours of i at nlist[head[i] .. head[i] + n_neigh[i]).  In a HOOMD list the
rows have a fixed capacity, so head is NOT the prefix sum of n_neigh and the slack behind a row holds stale entries of earlier builds.
util.build_nlist and every other list of the suite are compact (head[1:] = cumsum(n_neigh)[:-1], ascending, from 0).  relayout() stores
the same rows differently:

  compact           the identity
  slack             row i has the capacity max(n_neigh) + pad_i, pad_i in 1 .. 9; rows ascending, the first one behind a leading offset
  slack_descending  the same capacities, the rows stored in descending particle order: head decreases
  scattered         the same capacities, the rows at a random permutation of the row slots

Every slot that belongs to no row is filled, wrong but valid: the slack behind a row repeats that row's own entries cyclically (an
over-read counts a true partner inside the cut-off twice), the slack of an empty row and the leading offset hold indices of real
particles < n_positions.  A walk that leaves its row then gives a wrong number, never an access outside the position array.
`stale` (one sequence per row) goes into a row's slack ahead of the repetition: the cluster labelling is idempotent under a repeated
edge, so its lists withhold true partners and keep them in the slack (thinned()).

clumps() builds isolated clumps of 1, 2, ..., M particles: every member of clump m has exactly m - 1 partners, all inside the cut-off, so
the rows have every length 0 .. M - 1 — with G lanes per row, 0 .. 3G + 1 covers each boundary of e < cnt, e + G < cnt and e + 2G < cnt
of the two-deep look-ahead (csrc/row_walk.hpp) for every lane.  padded() adds the entries a walk must skip, split_ghosts() moves the last
member of every clump behind the central particles.

tests/test_list_layouts.py proves on the references alone that one stale entry, or one entry dropped, moves every result by far more
than the GPU tolerances; tests/test_gpu_list_layouts.py hands the lists to the kernels.
"""
import numpy as np

import util

KINDS = ("compact", "slack", "slack_descending", "scattered")
OTHER_KINDS = KINDS[1:]


def as_rows(nl):
    """the rows of a list as read through (head, n_neigh)"""
    head, nn, lst = (np.asarray(a).astype(np.int64) for a in nl)
    return [lst[head[i]:head[i] + nn[i]].copy() for i in range(len(head))]


def from_rows(rows):
    """the compact list of the given rows"""
    nn = np.array([len(r) for r in rows], dtype=np.uint32)
    head = np.zeros(len(rows), dtype=np.uint32)
    head[1:] = np.cumsum(nn)[:-1]
    flat = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if nn.sum() else np.zeros(0, dtype=np.int64)
    return head, nn, flat.astype(np.uint32)


def describe(nl, kind, seed=0, n_positions=None, stale=None):
    """dict(nl=(head, n_neigh, nlist), capacity (rows,), free: mask of the slots that belong to no row)"""
    assert kind in KINDS, kind
    rows = as_rows(nl)
    n_rows = len(rows)
    nn = np.array([len(r) for r in rows], dtype=np.int64)
    if kind == "compact":
        head, nn32, lst = from_rows(rows)
        return dict(nl=(head, nn32, lst), capacity=nn.copy(), free=np.zeros(len(lst), dtype=bool))
    n_positions = n_rows if n_positions is None else n_positions
    rng = np.random.default_rng(seed)
    capacity = int(nn.max() if n_rows else 0) + rng.integers(1, 10, n_rows)
    lead = int(rng.integers(3, 12))                                      # the first row does not start at 0
    order = {"slack": np.arange(n_rows), "slack_descending": np.arange(n_rows)[::-1], "scattered": rng.permutation(n_rows)}[kind]
    head = np.zeros(n_rows, dtype=np.int64)
    head[order] = lead + np.cumsum(capacity[order]) - capacity[order]    # order[k]: the particle whose row is stored k-th
    lst = np.full(lead + int(capacity.sum()), -1, dtype=np.int64)
    free = np.ones(len(lst), dtype=bool)
    lst[:lead] = rng.integers(0, n_positions, lead)
    for i in range(n_rows):
        a, b, c = head[i], head[i] + nn[i], head[i] + capacity[i]
        lst[a:b] = rows[i]
        free[a:b] = False
        first = np.asarray(stale[i], dtype=np.int64) if stale is not None else np.zeros(0, dtype=np.int64)
        if nn[i] or len(first):
            fill = np.concatenate([first, np.resize(rows[i], c - b)]) if nn[i] else np.resize(first, c - b)
            lst[b:c] = fill[:c - b]
        else:
            lst[b:c] = rng.integers(0, n_positions, c - b)
    assert lst.min() >= 0
    return dict(nl=(head.astype(np.uint32), nn.astype(np.uint32), lst.astype(np.uint32)), capacity=capacity, free=free)


def relayout(nl, kind, seed=0, n_positions=None, stale=None):
    """the same rows, the same entries in the same order inside each row, stored as `kind` says"""
    return describe(nl, kind, seed, n_positions, stale)["nl"]


def over_read(nl, by=1):
    """the list a walk sees that takes `by` entries too many from every non-empty row: n_neigh + by there, everything else as it is"""
    head, nn, lst = nl
    nn = np.asarray(nn).astype(np.int64)
    return head, np.where(nn > 0, nn + by, 0).astype(np.uint32), lst


def drop_last(nl):
    """the compact list without the last entry of every non-empty row"""
    return from_rows([r[:-1] for r in as_rows(nl)])


def thinned(nl, keep=lambda i, j: (i + j) % 3 != 0):
    """(list, stale): the list without the pairs that `keep` rejects — at both ends, keep is symmetric — and the withheld partners per
    row: in a row's slack they are true partners that the list does not hold"""
    rows = as_rows(nl)
    kept = [np.array([j for j in r if keep(i, j)], dtype=np.int64) for i, r in enumerate(rows)]
    stale = [np.array([j for j in r if not keep(i, j)], dtype=np.int64) for i, r in enumerate(rows)]
    return from_rows(kept), stale


_liquid = {}


def thinned_liquid(N=1000):
    """the liquid of tests/test_gpu_cluster.py (its recipe, seed = N: random positions at density 0.8, v random, v_min and r_link in the
    widest gaps) with a third of its pairs withheld from the list and kept for the slack: dict(pos, types, L, nl, v, cluster, stale,
    full); built once"""
    import ql_local_cluster_ref as cr
    if N not in _liquid:
        rng = np.random.default_rng(N)
        L = (N / 0.8) ** (1.0 / 3.0)
        pos = rng.uniform(-0.5 * L, 0.5 * L, (N, 3)).astype(np.float32).astype(np.float64)
        types = np.zeros(N, dtype=np.int32)
        full = util.build_nlist(pos, L, 1.5)
        v = rng.random(N)
        v_min, _ = cr.widest_gap(v, np.quantile(v, 0.47), np.quantile(v, 0.53))
        _, _, rsq = cr.listed(pos, full, L)
        r_link, _ = cr.widest_gap(np.sqrt(rsq), 1.0, 1.1)
        nl, stale = thinned(full)
        _liquid[N] = dict(pos=pos, types=types, L=L, nl=nl, v=v, cluster=(v_min, r_link), stale=stale, full=full)
    return _liquid[N]


# ---- rows of every length ---------------------------------------------------------------------------------------------------------

def clumps(M, half_width, dtype, seed=2024, spacing=8.0, min_dist=0.3, positions=None, sites=None, L=None):
    """clumps of 1 .. M particles of type 0 about the sites of a cubic grid with `spacing`, the members uniform in a cube of
    `half_width` and no two closer than min_dist (positions, sites, L: take these members about these sites instead), and behind them
    one particle of type 1 per clump at its site: inside the cut-off of every member, never a partner.  Returns dict(pos, types, L,
    clump, n_members, nl): nl lists, for every member, the other members of its clump (m - 1 entries); the rows of the type-1
    particles are empty."""
    if sites is None:
        side = int(np.ceil(M ** (1.0 / 3.0) - 1e-9))
        L = spacing * side
        sites = spacing * (np.array([[x, y, z] for x in range(side) for y in range(side) for z in range(side)], dtype=np.float64) - 0.5 * (side - 1))
    sites = np.asarray(sites, dtype=np.float64)
    sizes = np.arange(1, M + 1)
    clump = np.repeat(np.arange(M), sizes)
    n_members = int(sizes.sum())
    if positions is None:
        rng = np.random.default_rng(seed)
        positions = []
        for m in sizes:
            members = []
            while len(members) < m:
                x = rng.uniform(-half_width, half_width, 3)
                if np.linalg.norm(x) >= min_dist and all(np.linalg.norm(x - y) >= min_dist for y in members):
                    members.append(x)
            positions += [sites[m - 1] + x for x in members]
    pos = np.concatenate([np.asarray(positions, dtype=np.float64), sites[:M]]).astype(dtype).astype(np.float64)
    types = np.concatenate([np.zeros(n_members, dtype=np.int32), np.ones(M, dtype=np.int32)])
    rows = [np.array([j for j in np.nonzero(clump == clump[i])[0] if j != i], dtype=np.int64) for i in range(n_members)]
    rows += [np.zeros(0, dtype=np.int64)] * M
    nl = from_rows(rows)
    assert np.array_equal(nl[1][:n_members], np.repeat(sizes - 1, sizes))
    return dict(pos=pos, types=types, L=L, clump=np.concatenate([clump, np.arange(M)]), n_members=n_members, nl=nl)


def distances(case):
    """(inside, beyond, closest): the largest distance between two particles of one clump (the type-1 particle included), the smallest
    one between particles of different clumps, the smallest one at all — minimum image"""
    import ql_local_ref
    pos, clump = case["pos"], case["clump"]
    i, j = np.triu_indices(len(pos), 1)
    d = ql_local_ref.min_image(pos[i] - pos[j], case["L"])
    r = np.sqrt((d * d).sum(axis=1))
    same = clump[i] == clump[j]
    return r[same].max(), r[~same].min(), r.min()


def padded(case, ghosts, own=True, nl=None):
    """every row of a member (of case["nl"], or of `nl`) with one entry of each kind that a walk must skip, rotated between the front,
    the middle and the end by the particle index: the particle itself (`own`), the type-1 particle of its clump (inside the cut-off), a
    member of the next clump (beyond it) and, with `ghosts`, an index >= N (only for the units that skip those)"""
    N, n_members, clump = len(case["pos"]), case["n_members"], case["clump"]
    M = N - n_members
    rows = as_rows(case["nl"] if nl is None else nl)
    out = []
    for i in range(N):
        if i >= n_members:
            out.append(rows[i])
            continue
        row = list(rows[i])
        other = int(np.nonzero(clump[:n_members] == (clump[i] + 1) % M)[0][0])
        pad = ([i] if own else []) + [n_members + int(clump[i]), other]
        pad = pad[i % len(pad):] + pad[:i % len(pad)]
        mid = len(row) // 2
        out.append([pad[0]] + row[:mid] + pad[1:-1] + ([N + i % 7] if ghosts else []) + row[mid:] + [pad[-1]])
    return from_rows(out)


def split_ghosts(case):
    """the last member of every clump of two or more moved behind all other particles: dict(pos, types, L, nl, n_rows) — the first
    n_rows particles are central and own the rows, the others are ghosts that the rows index"""
    N, n_members, clump = len(case["pos"]), case["n_members"], case["clump"]
    last = np.zeros(N, dtype=bool)
    for c in range(N - n_members):
        members = np.nonzero(clump[:n_members] == c)[0]
        if len(members) >= 2:
            last[members[-1]] = True
    order = np.concatenate([np.nonzero(~last)[0], np.nonzero(last)[0]])
    new = np.empty(N, dtype=np.int64)
    new[order] = np.arange(N)
    n_rows = int((~last).sum())
    rows = as_rows(case["nl"])
    nl = from_rows([new[rows[old]] for old in order[:n_rows]])
    assert (nl[2] >= n_rows).any()
    return dict(pos=case["pos"][order], types=case["types"][order], L=case["L"], nl=nl, n_rows=n_rows)


# ---- the sweeps of tests/test_gpu_list_layouts.py, shared with the CPU checks of tests/test_list_layouts.py ---------------------------
PE_SWEEP = dict(M=26, half_width=0.65, par=(2.4, 0.1, 48))              # PE_G = 8: rows of 0 .. 25 = 3 G + 1; r_cut = r_max + 4 sigma_r = 2.8
ES_SWEEP = dict(M=14, half_width=0.42, min_dist=0.25, sigma_env=0.3, r_on=1.3, r_cut=1.5)      # ES_G = 4: rows of 0 .. 13
CL_SWEEP = dict(M=14, half_width=0.45, v_min=0.5, r_link=2.0)           # CL_G = 4
QL_SWEEP = dict(M=14, r_cut=1.4, r_on=1.2, lmax=8, Ql_ref=[0, 0, 0, 0, 1, 0, 1, 0, 0.5])       # 22 table slots: k_qll_forces

_sweeps = {}


def sweep(unit, dtype):
    """the clumps of a unit, rounded to the dtype: built once per unit and dtype, shared, never changed"""
    key = (unit, np.dtype(dtype).name)
    if key not in _sweeps:
        if unit == "pe":
            # the seed of 20 .. 39 at which the weakest last entry of a row carries most of max|F|, 2.3e-3 (the pair force u(r) changes
            # sign inside the window: at most seeds some last entry sits next to a zero), judged on the reference alone
            case = clumps(PE_SWEEP["M"], PE_SWEEP["half_width"], dtype, seed=37)
        elif unit == "es":
            case = clumps(ES_SWEEP["M"], ES_SWEEP["half_width"], dtype, seed=14, min_dist=ES_SWEEP["min_dist"])
        elif unit == "cl":
            case = clumps(CL_SWEEP["M"], CL_SWEEP["half_width"], dtype, seed=4)
            # a star: the first member of a clump lists all the others (rows of 0 .. 13), they list nothing — every entry is the only
            # edge to its leaf, which a symmetric list of a fully linked clump would not make it
            rows = as_rows(case["nl"])
            first = {int(c): int(np.nonzero(case["clump"] == c)[0][0]) for c in range(CL_SWEEP["M"])}
            case["nl"] = from_rows([r if first[int(case["clump"][i])] == i else r[:0] for i, r in enumerate(rows)])
        elif unit == "ql":
            # the members of test_gpu_ql_local_avg.cluster_case (its recipe, its seed), with the type-1 particles added
            rng = np.random.default_rng(2024)
            centres = 8.0 * (np.array([[x, y, z] for x in range(5) for y in range(5) for z in range(5)], dtype=np.float64) - 2.0)
            positions = []
            for m in range(1, 15):
                members = []
                while len(members) < m:
                    x = rng.uniform(-0.45, 0.45, 3)
                    if all(np.linalg.norm(x - y) >= 0.3 for y in members):
                        members.append(x)
                positions += [centres[m - 1] + x for x in members]
            case = clumps(14, 0.45, dtype, positions=positions, sites=centres[:14], L=40.0)
        else:
            raise ValueError(unit)
        _sweeps[key] = case
    return _sweeps[key]


def half_of(nl):
    """the half list of a symmetric full list: every pair at its lower index"""
    return from_rows([r[r > i] for i, r in enumerate(as_rows(nl))])


BIAS = 0.9
ES_SWITCH = (0.5, 6)
QL_COMBOS = {"plain": dict(), "average": dict(average=True), "bonds+switch+gate": dict(bonds=(0.0, 0.9), switch=(3.0, 4), gate=(2, 9))}
_references = {}


def es_variants():
    """name: (templates, lambda, switch) — `fcc` and `two_switch` of tests/test_gpu_env_similarity.py"""
    import env_similarity_ref as es
    fcc = es.templates("fcc", np.sqrt(2.0))
    c, s = np.cos(np.deg2rad(5.0)), np.sin(np.deg2rad(5.0))
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return {"fcc": (fcc, 100.0, None), "two_switch": ([fcc, fcc @ rot.T], 20.0, ES_SWITCH)}


def reference(unit, dtype, variant=None, split=False):
    """the restatement's answer for the CLEAN list of a sweep (split: with the last member of every clump a ghost), computed once per
    key and left unchanged.  unit: pe, es (variant fcc / two_switch), ql (variant of QL_COMBOS), cl"""
    key = (unit, np.dtype(dtype).name, variant, split)
    if key not in _references:
        case = split_ghosts(sweep(unit, dtype)) if split else sweep(unit, dtype)
        pos, types, L, nl = case["pos"], case["types"], case["L"], case["nl"]
        if unit == "pe":
            import pair_entropy_ref as pe
            r = pe.compute(pos, types, L, nl, *PE_SWEEP["par"], 0, bias=BIAS)
        elif unit == "es":
            import env_similarity_ref as es
            t, lam, sw = es_variants()[variant]
            r = es.compute(pos, types, L, nl, t, ES_SWEEP["sigma_env"], ES_SWEEP["r_on"], ES_SWEEP["r_cut"], 0, lam=lam, sw=sw,
                           n_global=len(pos), bias=BIAS)
        elif unit == "ql":
            args = (QL_SWEEP["r_cut"], QL_SWEEP["r_on"], QL_SWEEP["lmax"], 0, QL_SWEEP["Ql_ref"])
            if "bonds" in QL_COMBOS[variant]:
                import ql_local_bonds_ref
                r = ql_local_bonds_ref.compute(pos, types, L, nl, *args, bias=BIAS, **QL_COMBOS[variant])
            else:
                import ql_local_avg_ref
                r = ql_local_avg_ref.compute(pos, types, L, nl, *args, **QL_COMBOS[variant])
        elif unit == "cl":
            import ql_local_cluster_ref as cr
            r = cr.clusters(pos, types, L, nl, 0, np.ones(len(pos)), CL_SWEEP["v_min"], CL_SWEEP["r_link"])
        else:
            raise ValueError(unit)
        _references[key] = r
    return _references[key]
