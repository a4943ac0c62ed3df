"""No GPU: tests/list_layouts.py stores what it is given, and the references alone tell a walk that leaves its row.

1. relayout(): every row read back through (head, n_neigh) is the input row, the extents do not overlap, the array ends with the last
   capacity, no slot is left unfilled and every filled slot holds a stored position.
2. The fill is detectable: with n_neigh + 1 on every non-empty row (one stale entry each) ql_local_ref, pair_entropy_ref and
   env_similarity_ref move by more than 1000 x the tolerance of the matching GPU parity test, and ql_local_cluster_ref.clusters changes
   a label.  A repeated edge cannot move a label, so the cluster list withholds a third of its pairs and keeps them in the slack.
3. The sweeps over the row lengths are not vacuous: dropping the last entry of a row moves that row's value (or the force on its
   particle) by more than 1000 x the GPU tolerance; the geometry of the pads is what tests/test_gpu_list_layouts.py relies on.
"""
import numpy as np
import pytest

import env_similarity_ref as es
import list_layouts as ll
import pair_entropy_ref as pe
import ql_local_cluster_ref as cr
import ql_local_ref
import util

FACTOR = 1000.0
SEED = 7


def noisy_fcc(n, sigma=0.05, seed=777):
    pos, L = util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


@pytest.fixture(scope="module")
def crystal():
    pos, L = noisy_fcc(4)
    return dict(pos=pos, L=L, types=np.zeros(len(pos), dtype=np.int32))


def _lists(crystal):
    full = util.build_nlist(crystal["pos"], crystal["L"], 1.55)
    half = util.build_nlist(crystal["pos"], crystal["L"], 1.55, half=True)
    n_rows = 200
    rows = ll.from_rows(ll.as_rows(full)[:n_rows])                       # the trailing particles are ghosts: indexed, owning no row
    return {"full": (full, 256), "half": (half, 256), "rows": (rows, 256), "empty": (ll.from_rows([np.zeros(0, dtype=np.int64)] * 5), 5)}


# ---- 1. the helper ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ll.KINDS)
@pytest.mark.parametrize("which", ["full", "half", "rows", "empty"])
def test_relayout_keeps_the_rows_and_fills_every_other_slot(crystal, kind, which):
    nl, n_positions = _lists(crystal)[which]
    d = ll.describe(nl, kind, seed=SEED, n_positions=n_positions)
    head, nn, lst = (np.asarray(a).astype(np.int64) for a in d["nl"])
    cap, free = d["capacity"], d["free"]
    assert d["nl"][0].dtype == np.uint32 and d["nl"][1].dtype == np.uint32 and d["nl"][2].dtype == np.uint32
    want = ll.as_rows(nl)
    got = ll.as_rows(d["nl"])
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))     # the same entries in the same order
    assert np.array_equal(nn, np.asarray(nl[1]).astype(np.int64)) and (cap >= nn).all()
    order = np.argsort(head, kind="stable")
    assert (head[order][1:] >= (head + cap)[order][:-1]).all()                                # the extents do not overlap
    assert (head + cap).max() == len(lst)
    owned = np.zeros(len(lst), dtype=bool)
    for i in range(len(head)):
        assert not owned[head[i]:head[i] + nn[i]].any()
        owned[head[i]:head[i] + nn[i]] = True
    assert np.array_equal(free, ~owned)
    assert (lst[free] < n_positions).all() and (lst[~free] < n_positions).all()              # nothing but stored positions, anywhere
    if kind == "compact":
        assert all(np.array_equal(a, np.asarray(b)) for a, b in zip(d["nl"], nl)) and not free.any()
        return
    assert head.min() >= 3 and free[:head.min()].all()                                       # a leading offset, filled
    assert ((cap - nn.max() >= 1) & (cap - nn.max() <= 9)).all() and len(set(cap.tolist())) > 1
    assert free.sum() == len(lst) - nn.sum() > len(head)
    for i in range(len(head)):                                                               # the slack repeats the row's own entries
        if nn[i]:
            assert np.array_equal(lst[head[i] + nn[i]:head[i] + cap[i]], np.resize(want[i], cap[i] - nn[i]))
    steps = np.diff(head)
    if kind == "slack":
        assert (steps > 0).all()
    elif kind == "slack_descending":
        assert (steps < 0).all()
    else:
        assert (steps > 0).any() and (steps < 0).any()
    if which != "empty":
        assert not np.array_equal(head[1:], np.cumsum(nn)[:-1])
    again = ll.relayout(nl, kind, seed=SEED, n_positions=n_positions)
    assert all(np.array_equal(a, b) for a, b in zip(again, d["nl"]))                         # seeded: the same arrays every time


def test_stale_entries_go_into_the_slack_first(crystal):
    full = util.build_nlist(crystal["pos"], crystal["L"], 1.55)
    thin, stale = ll.thinned(full)
    assert 0.2 * len(full[2]) < len(full[2]) - len(thin[2]) < 0.5 * len(full[2])
    rows, kept = ll.as_rows(full), ll.as_rows(thin)
    for i in range(len(rows)):
        assert sorted(list(kept[i]) + list(stale[i])) == sorted(rows[i])
        assert all(i in kept[j] for j in kept[i])                                             # still symmetric
    for kind in ll.OTHER_KINDS:
        d = ll.describe(thin, kind, seed=SEED, stale=stale)
        head, nn, lst = (np.asarray(a).astype(np.int64) for a in d["nl"])
        assert all(np.array_equal(a, b) for a, b in zip(ll.as_rows(d["nl"]), kept))
        for i in range(len(head)):
            n = min(len(stale[i]), d["capacity"][i] - nn[i])
            assert np.array_equal(lst[head[i] + nn[i]:head[i] + nn[i] + n], stale[i][:n])


# ---- 2. one stale entry per row shows in every reference ---------------------------------------------------------------------------

def _moved(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(a)).max()


@pytest.mark.parametrize("kind", ll.OTHER_KINDS)
def test_a_stale_entry_moves_the_local_steinhardt_variable(crystal, kind):
    """tests/test_gpu_ql_local*.py: c_i and n_i to 1e-11 of their largest value, s to 1e-10 relative"""
    nl = ll.relayout(util.build_nlist(crystal["pos"], crystal["L"], 1.55), kind, seed=SEED)
    args = (crystal["pos"], crystal["types"], crystal["L"])
    par = (1.4, 1.2, 6, 0, [0, 0, 0, 0, 1, 0, 1])
    a = ql_local_ref.compute(*args, nl, *par, gradient=False)
    b = ql_local_ref.compute(*args, ll.over_read(nl), *par, gradient=False)
    same = ql_local_ref.compute(*args, ll.relayout(nl, "compact"), *par, gradient=False)
    assert a["s"] == same["s"] and np.array_equal(a["c"], same["c"])                          # the reference does index through head
    print("s %.3e relative, c %.3e, n %.3e of their largest" % (abs(b["s"] / a["s"] - 1.0), _moved(a["c"], b["c"]), _moved(a["n"], b["n"])))
    assert abs(b["s"] / a["s"] - 1.0) > FACTOR * 1e-10
    assert _moved(a["c"], b["c"]) > FACTOR * 1e-11 and _moved(a["n"], b["n"]) > FACTOR * 1e-11


@pytest.mark.parametrize("kind", ll.OTHER_KINDS)
def test_a_stale_entry_moves_the_pair_entropy(crystal, kind):
    """tests/test_gpu_pair_entropy.py: g_b to 1e-10 of max g, S to 1e-9 relative"""
    nl = ll.relayout(util.build_nlist(crystal["pos"], crystal["L"], 2.4), kind, seed=SEED)
    args = (crystal["pos"], crystal["types"], crystal["L"])
    par = (2.0, 0.1, 40, 0)
    Ha, n_t = pe.sums(*args, nl, *par)
    Hb, _ = pe.sums(*args, ll.over_read(nl), *par)
    a, b = pe.finalize(Ha, n_t, crystal["L"], *par[:3]), pe.finalize(Hb, n_t, crystal["L"], *par[:3])
    print("S %.3e relative, g %.3e of max g" % (abs(b["S"] / a["S"] - 1.0), _moved(a["g"], b["g"])))
    assert abs(b["S"] / a["S"] - 1.0) > FACTOR * 1e-9 and _moved(a["g"], b["g"]) > FACTOR * 1e-10


@pytest.mark.parametrize("kind", ll.OTHER_KINDS)
@pytest.mark.parametrize("variant", ["fcc", "two_switch"])
def test_a_stale_entry_moves_the_environment_similarity(crystal, kind, variant):
    """tests/test_gpu_env_similarity.py: k_i and v_i to 1e-10 of their maximum, s to 1e-9 relative"""
    nl = ll.relayout(util.build_nlist(crystal["pos"], crystal["L"], 1.5), kind, seed=SEED)
    t, lam, sw = ll.es_variants()[variant]
    args = (crystal["pos"], crystal["types"], crystal["L"])
    par = (t, 0.12, 1.3, 1.5, 0)
    a = es.compute(*args, nl, *par, lam=lam, sw=sw)
    b = es.compute(*args, ll.over_read(nl), *par, lam=lam, sw=sw)
    print("s %.3e relative, k %.3e, v %.3e of their maxima" % (abs(b["s"] / a["s"] - 1.0), _moved(a["k"], b["k"]), _moved(a["v"], b["v"])))
    assert abs(b["s"] / a["s"] - 1.0) > FACTOR * 1e-9
    assert _moved(a["k"], b["k"]) > FACTOR * 1e-10 and _moved(a["v"], b["v"]) > FACTOR * 1e-10


@pytest.mark.parametrize("kind", ll.OTHER_KINDS)
def test_a_stale_entry_changes_a_cluster_label(kind):
    """everything is exact in tests/test_gpu_cluster.py: one label or size that differs is a failure there"""
    case = ll.thinned_liquid()
    args = (case["pos"], case["types"], case["L"])
    nl = ll.relayout(case["nl"], kind, seed=SEED, stale=case["stale"])
    a = cr.clusters(*args, nl, 0, case["v"], *case["cluster"])
    b = cr.clusters(*args, ll.over_read(nl), 0, case["v"], *case["cluster"])
    same = cr.clusters(*args, case["nl"], 0, case["v"], *case["cluster"])
    assert np.array_equal(a["label"], same["label"]) and np.array_equal(a["summary"], same["summary"])
    print("labels that differ: %d, sizes: %d; clusters %d -> %d" % ((a["label"] != b["label"]).sum(), (a["size"] != b["size"]).sum(),
                                                                     a["summary"][2], b["summary"][2]))
    assert (a["label"] != b["label"]).any() and (a["size"] != b["size"]).any()
    assert a["summary"][2] > 10
    # the repetition of a row's own entries alone would not show: a repeated edge links nothing new
    plain = ll.relayout(case["nl"], kind, seed=SEED)
    c = cr.clusters(*args, ll.over_read(plain), 0, case["v"], *case["cluster"])
    assert np.array_equal(a["label"], c["label"])


# ---- 3. the sweeps over the row lengths -------------------------------------------------------------------------------------------

DTYPES = [np.float64, np.float32]
CUTS = {"pe": ll.PE_SWEEP["par"][0] + 4 * ll.PE_SWEEP["par"][1], "es": ll.ES_SWEEP["r_cut"], "cl": ll.CL_SWEEP["r_link"], "ql": ll.QL_SWEEP["r_cut"]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("unit", sorted(CUTS))
def test_sweep_geometry_and_pads(unit, dtype):
    """every row length 0 .. 3 G + 1; every partner inside the cut-off, the type-1 pad inside, the pad from the next clump beyond, each
    by more than 1e-3; the padded rows hold the clean rows in their order"""
    case = ll.sweep(unit, dtype)
    G = 8 if unit == "pe" else 4
    M = len(case["pos"]) - case["n_members"]
    assert M == 3 * G + 2
    nn = np.asarray(case["nl"][1]).astype(np.int64)
    assert set(nn.tolist()) == set(range(M)) and not nn[case["n_members"]:].any()
    inside, beyond, closest = ll.distances(case)
    r_in = ll.PE_SWEEP["par"][0] if unit == "pe" else CUTS[unit]         # pair entropy: inside r_max, where the bins are
    print("%s: N = %d, pairs of a clump <= %.4f, of two clumps >= %.4f, closest %.4f" % (unit, len(case["pos"]), inside, beyond, closest))
    assert inside < r_in - 1e-3 and beyond > CUTS[unit] + 1e-3 and beyond > 2 * CUTS[unit]
    if unit == "pe":
        assert len(case["pos"]) == 351 + 26 and closest >= 0.3
    for ghosts in (False, True):
        pad = ll.padded(case, ghosts)
        extra = 4 if ghosts else 3
        assert len(pad[2]) == len(case["nl"][2]) + extra * case["n_members"]
        N = len(case["pos"])
        front = set()
        for i, (row, clean) in enumerate(zip(ll.as_rows(pad), ll.as_rows(case["nl"]))):
            if i >= case["n_members"]:
                assert len(row) == 0
                continue
            rest = [j for j in row if j < case["n_members"] and j != i and case["clump"][j] == case["clump"][i]]
            assert rest == list(clean)
            skipped = [j for j in row if j not in set(clean.tolist())]
            assert len(skipped) == extra and i in skipped and (max(skipped) >= N) == ghosts
            assert sum(1 for j in skipped if j < N and case["types"][j] == 1) == 1
            front.add(row[0] == i)
            for j in skipped:
                if j < N and j != i:
                    d = ql_local_ref.min_image((case["pos"][i] - case["pos"][j])[None, :], case["L"])[0]
                    r = np.sqrt((d * d).sum())
                    assert (r < CUTS[unit] - 1e-3) if case["types"][j] == 1 else (r > CUTS[unit] + 1e-3)
        assert front == {False, True}                                   # the pads rotate
    if unit in ("pe", "es"):
        s = ll.split_ghosts(case)
        assert s["n_rows"] == len(case["pos"]) - (M - 1) and (np.asarray(s["nl"][2]) >= s["n_rows"]).sum() >= M - 1
        assert sorted(np.asarray(s["nl"][1]).tolist()) == sorted(np.delete(nn, [np.nonzero(case["clump"][:case["n_members"]] == c)[0][-1]
                                                                                  for c in range(1, M)]).tolist())


def _last_entries(nl):
    """index into the flat compact list of the last entry of every non-empty row, and those rows"""
    nn = np.asarray(nl[1]).astype(np.int64)
    rows = np.nonzero(nn)[0]
    return (np.cumsum(nn) - 1)[rows], rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropping_a_last_entry_moves_the_pair_entropy(dtype):
    """with the sums H kept, the force on particle i loses 2 u d / r of its last entry (GPU tolerance 1e-9 / 2e-7 of max|F|); the sums
    H lose that entry's window (H to 1e-10 of its largest: the bound on g_b)"""
    case = ll.sweep("pe", dtype)
    r = ll.reference("pe", dtype)
    r_max, sigma_r, n_bins = ll.PE_SWEEP["par"]
    c = pe.constants(r_max, sigma_r, n_bins)
    i, j, d = pe.entries(case["pos"], case["types"], case["nl"], 0, c["r_cut"], case["L"])
    assert len(i) == len(case["nl"][2])                                 # every entry takes part: the flat order is the list's
    rr = np.sqrt((d * d).sum(axis=1))
    f, df = ql_local_ref.smoothing(rr, c["r_on"], c["r_cut"])
    K, x = pe._window(rr, c, r_max, sigma_r, n_bins)
    u = (r["W"][None, :] * K * (df[:, None] + f[:, None] * x / sigma_r ** 2)).sum(axis=1)
    last, rows = _last_entries(case["nl"])
    assert np.array_equal(i[last], rows)
    fs = np.abs(r["gather"]).max() * ll.BIAS
    lost = np.abs(2.0 * ll.BIAS * (u / rr)[last, None] * d[last]).max(axis=1)
    lost_h = (f[last, None] * K[last]).max(axis=1)
    tol = 1e-9 if dtype == np.float64 else 2e-7
    print("max|F| %.3e; the last entry's share of F_i >= %.3e of it; of H >= %.3e of max H" % (fs, lost.min() / fs, lost_h.min() / r["H"].max()))
    assert fs > 0 and (lost > FACTOR * tol * fs).all()
    assert (lost_h > FACTOR * 1e-10 * r["H"].max()).all()
    split = ll.reference("pe", dtype, split=True)
    assert np.abs(split["gather"]).max() > 0 and split["n_t"] == ll.split_ghosts(case)["n_rows"] - ll.PE_SWEEP["M"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["fcc", "two_switch"])
def test_dropping_a_last_entry_moves_the_environment_similarity(dtype, variant):
    """k_i is a sum over row i alone: without the last entry of every row each k_i of a non-empty row moves (GPU tolerance 1e-10 of max k)"""
    case = ll.sweep("es", dtype)
    r = ll.reference("es", dtype, variant)
    t, lam, sw = ll.es_variants()[variant]
    less = es.compute(case["pos"], case["types"], case["L"], ll.drop_last(case["nl"]), t, ll.ES_SWEEP["sigma_env"], ll.ES_SWEEP["r_on"],
                      ll.ES_SWEEP["r_cut"], 0, lam=lam, sw=sw, n_global=len(case["pos"]))
    _, rows = _last_entries(case["nl"])
    moved = np.abs(r["k"] - less["k"])[rows]
    print("k: max %.3e, smallest of a non-empty row %.3e; every row moves by >= %.3e of the max; max|gather| %.3e"
          % (r["k"].max(), r["k"][rows].min(), moved.min() / r["k"].max(), np.abs(r["gather"]).max()))
    assert (moved > FACTOR * 1e-10 * r["k"].max()).all()
    assert r["k"][rows].min() > 1e-6 * r["k"].max()                     # no k_i underflowed
    assert np.abs(r["gather"]).max() > 0
    if variant == "fcc":
        assert np.abs(ll.reference("es", dtype, "fcc", split=True)["gather"]).max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("combo", sorted(ll.QL_COMBOS))
def test_dropping_a_last_entry_moves_the_local_steinhardt_variable(dtype, combo):
    """c_i and n_i are sums over row i alone (GPU tolerance 1e-11 of their largest value)"""
    case = ll.sweep("ql", dtype)
    r = ll.reference("ql", dtype, combo)
    args = (ll.QL_SWEEP["r_cut"], ll.QL_SWEEP["r_on"], ll.QL_SWEEP["lmax"], 0, ll.QL_SWEEP["Ql_ref"])
    full = ql_local_ref.compute(case["pos"], case["types"], case["L"], case["nl"], *args, gradient=False)
    less = ql_local_ref.compute(case["pos"], case["types"], case["L"], ll.drop_last(case["nl"]), *args, gradient=False)
    _, rows = _last_entries(case["nl"])
    for key in ("c", "n"):                                              # of the plain variable: what every combination is built on
        moved = np.abs(full[key] - less[key])[rows]
        print("%s: every row moves by >= %.3e of the largest" % (key, moved.min() / np.abs(full[key]).max()))
        assert (moved > FACTOR * 1e-11 * np.abs(full[key]).max()).all()
    assert np.abs(r["n"] - full["n"]).max() <= 1e-13 * full["n"].max()
    assert np.abs(r["grad"]).max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropping_a_last_entry_changes_the_cluster_labels(dtype):
    """the star lists: every entry is the only edge to its leaf, so each row, shortened alone, changes a label and a size"""
    case = ll.sweep("cl", dtype)
    r = ll.reference("cl", dtype)
    assert r["summary"].tolist() == [int(np.nonzero(case["clump"] == 13)[0][0]), 14, 14, 105]
    rows = ll.as_rows(case["nl"])
    args = (case["pos"], case["types"], case["L"])
    for i in np.nonzero(case["nl"][1])[0]:
        less = cr.clusters(*args, ll.from_rows([x[:-1] if k == i else x for k, x in enumerate(rows)]), 0, np.ones(len(case["pos"])),
                           ll.CL_SWEEP["v_min"], ll.CL_SWEEP["r_link"])
        assert (less["label"] != r["label"]).any() and (less["size"] != r["size"]).any()
    dv, dr = cr.margins(*args, ll.padded(case, False), 0, np.ones(len(case["pos"])), ll.CL_SWEEP["v_min"], ll.CL_SWEEP["r_link"])
    assert dv > 1e-6 and dr > 1e-3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("half", [False, True])
def test_dropping_a_last_entry_moves_the_global_steinhardt_force(ref, dtype, half):
    """the oracle's force on particle i (the central terms of row i) with the Q_lm of the clean list: without the last entry of row i it
    moves by more than 1000 x the GPU tolerance (1e-9 / 2e-7 of max|F|); one row at a time"""
    case = ll.sweep("ql", dtype)
    nl = ll.half_of(case["nl"]) if half else case["nl"]
    box = ref.Box.make(case["L"])
    pt = util.oracle_postype(case["pos"], case["types"])
    par = (ll.QL_SWEEP["r_cut"], ll.QL_SWEEP["r_on"], ll.QL_SWEEP["lmax"], 0, ll.QL_SWEEP["Ql_ref"])
    val, Qlm, Ql = ref.ql_compute_cv(pt, box, *nl, *par, half=half)
    F = ref.ql_compute_forces(pt, box, *nl, *par, Qlm, ll.BIAS, half=half)[:, :3]
    fs = np.abs(F).max()
    tol = 1e-9 if dtype == np.float64 else 2e-7
    rows = ll.as_rows(nl)
    worst = np.inf
    for i in np.nonzero(nl[1])[0]:
        less = ll.from_rows([x[:-1] if k == i else x for k, x in enumerate(rows)])
        Fi = ref.ql_compute_forces(pt, box, *less, *par, Qlm, ll.BIAS, half=half)[:, :3]
        worst = min(worst, np.abs(Fi[i] - F[i]).max())
    print("value %.6g, max|F| %.3e; every row's last entry moves F_i by >= %.3e of it" % (val, fs, worst / fs))
    assert fs > 0 and worst > FACTOR * tol * fs
