"""GPU: every consumer of a neighbour list on HOOMD's row layout, and every row length through the forms of the row walk.

1. Layouts (tests/list_layouts.py): each consumer runs on the compact list and on the same rows stored with slack, in descending order
   and scattered, the unused slots holding valid but wrong indices.  Particles, parameters and the helpers' scratch are the same in
   every run, and every output must be the compact run's BIT FOR BIT: all these passes sum in orders that follow the place of an entry
   in its row and the particle index, never an address; their atomics are integer ones or the exact mode of the half-list pass.  No
   consumer needed an exception.  tests/test_list_layouts.py shows on the references alone that one stale entry moves every result
   by far more than any tolerance.
2. Row lengths: isolated clumps of 1 .. M particles give rows of 0 .. M - 1 entries, every boundary of the two-deep look-ahead for each
   lane of a group, through row_walk<8> (pair entropy), row_walk<4> (environment similarity), row_walk_entries<4, .., GHOSTS = false>
   (the cluster link pass), k_qll_forces (22 table slots) and the unit feed of the global Steinhardt kernels.  Run A: the clean list
   against the unit's reference with the unit's own compare() and tolerances; run B: every row padded with the entries the walk must
   skip, against the reference of the CLEAN list; run C (pair entropy, environment similarity): the last member of every clump a ghost.
   The global variable counts entries j >= N (ghost particles behind the local ones, as SteinhardtQl.cc does) and, like the reference,
   has no rule for a self entry: its run B pads with the other type and with the partner beyond the cut-off only.

All ABI calls are on the default stream, through the run_gpu helpers of the units' own test modules."""
import numpy as np
import pytest

import list_layouts as ll
import ql_local_cluster_ref as cr
import util
from test_gpu_cluster import check as check_cluster
from test_gpu_cluster import liquid_case
from test_gpu_cluster import run_gpu as run_gpu_cluster
from test_gpu_env_similarity import compare as compare_es
from test_gpu_env_similarity import run_gpu as run_gpu_es
from test_gpu_pair_entropy import compare as compare_pe
from test_gpu_pair_entropy import run_gpu as run_gpu_pe
from test_gpu_ql_local_avg import compare as compare_avg
from test_gpu_ql_local_avg import run_gpu as run_gpu_opt
from test_gpu_ql_local_avg import snapshot as fcc_snapshot
from test_gpu_ql_local_bonds import compare as compare_bonds
from test_gpu_ql_local_bonds import run_gpu as run_gpu_bonds
from test_gpu_ql_local_cluster import run_gpu as run_gpu_ql_cluster
from test_gpu_ql_local_virial import run_gpu as run_gpu_local_virial
from test_gpu_ql_virial import run_gpu as run_gpu_ql_virial
from test_gpu_steinhardt import _symmetrize, run_gpu as run_gpu_ql, run_ref as run_ref_ql

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SEED = 11
BIAS = ll.BIAS
QL_46 = [0, 0, 0, 0, 1, 0, 1]                                            # 13 table slots: the LDS-tile force kernel
QL_468 = [0, 0, 0, 0, 1, 0, 1, 0, 0.5]                                   # 22 slots: k_qll_forces


def bits(x):
    return None if x is None else np.ascontiguousarray(x).tobytes()


def same_bits(a, b, what):
    """two results of one helper (dicts or tuples of arrays, scalars and None): every entry the same bytes"""
    items = a.items() if isinstance(a, dict) else enumerate(a)
    for key, x in items:
        assert bits(x) == bits(b[key]), (what, key)


def layouts(nl, n_positions=None, stale=None):
    """kind: the list in that layout; asserts that the others are not compact"""
    out = {kind: ll.relayout(nl, kind, seed=SEED, n_positions=n_positions, stale=stale) for kind in ll.KINDS}
    for kind in ll.OTHER_KINDS:
        head, nn, lst = (np.asarray(x).astype(np.int64) for x in out[kind])
        assert len(lst) > nn.sum() + len(head) and head.min() > 0 and not np.array_equal(head[1:], np.cumsum(nn)[:-1])
    return out


def every_layout(run, nl, what, n_positions=None, stale=None):
    """run(list) on the compact list and on the three others: the same bytes; returns the compact run's result"""
    lists = layouts(nl, n_positions, stale)
    base = run(lists["compact"])
    for kind in ll.OTHER_KINDS:
        same_bits(base, run(lists[kind]), (what, kind))
    return base


# ---- 1. layouts --------------------------------------------------------------------------------------------------------------------

_global = {}


def global_snapshot(dtype):
    """fcc 4 (N = 256), noise 0.05, rounded to the dtype, its full and half lists at 1.55"""
    key = np.dtype(dtype).name
    if key not in _global:
        pos, L, types, full = fcc_snapshot(4, dtype)
        _global[key] = (pos, L, types, full, util.build_nlist(pos, L, 1.55, half=True))
    return _global[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_global_steinhardt_on_every_layout(abi, dtype, mode):
    """mtd_ql_accumulate + mtd_ql_forces (+ mtd_ql_forces_virial on the full lists): value, Q_l, Q_lm, forces, virial.  The 64 rows of a
    chunk hold more than QL_CAP = 1024 entries, so a unit boundary falls inside a chunk and inside a row"""
    pos, L, types, full, half = global_snapshot(dtype)
    assert len(pos) == 256
    nn = np.asarray(full[1]).astype(np.int64)
    assert all(nn[c:c + 64].sum() > 1024 for c in range(0, 256, 64)) and nn.min() >= 16
    nl = half if mode == 1 else full
    args = (1.4, 1.2, 6, 0, QL_46)
    g = every_layout(lambda lists: run_gpu_ql(abi, pos, types, L, lists, *args, dtype, half=mode), nl, "ql")
    assert np.isfinite(g[3]).all() and np.abs(g[3][:, :3]).max() > 0 and g[0] > 0
    v = every_layout(lambda lists: run_gpu_ql_virial(abi, pos, types, L, lists, 6, QL_46, dtype, mode=mode, pitch=len(pos) + 3,
                                                     pass_virial=mode != 1), nl, "ql virial")
    assert np.array_equal(v["F"].astype(np.float64), g[3])
    if mode != 1:
        assert np.isfinite(v["raw"]).all() and np.abs(v["raw"][:, :len(pos)]).max() > 0


def test_symmetrize_half_list_on_every_layout(abi):
    """mtd_ql_symmetrize_half_list of a half list in each layout: the return code, the size and the three arrays of the compact one"""
    pos, L, types, full, half = global_snapshot(np.float64)
    N = len(pos)

    def run(lists):
        rc, n_full, sym = _symmetrize(abi, N, lists, capacity=2 * len(half[2]))
        return dict(rc=rc, n_full=n_full, head=sym[0], nn=sym[1], lst=sym[2])
    g = every_layout(run, half, "symmetrize")
    assert g["rc"] == 0 and g["n_full"] == len(full[2])
    assert np.array_equal(g["head"], full[0]) and np.array_equal(g["nn"], full[1]) and np.array_equal(g["lst"][:g["n_full"]], full[2])


LOCAL_SETS = {"plain": dict(), "switch+gate": dict(switch=(0.25, 3), gate=(10, 16)), "average": dict(average=True),
              "average+switch+gate": dict(average=True, switch=(0.12, 3), gate=(10, 16)),
              "bonds+switch+gate": dict(bonds=(0.3, 0.8), switch=(6.5, 6), gate=(10, 16)), "bonds+cluster": dict(bonds=(0.3, 0.8), switch=(6.5, 6))}
LOCAL_CASES = [(name, np.float64) for name in LOCAL_SETS] + [("plain", np.float32), ("average", np.float32)]


@pytest.mark.parametrize("name,dtype", LOCAL_CASES)
@pytest.mark.parametrize("lmax,Ql_ref", [(6, QL_46), (8, QL_468)], ids=["tile", "memory"])
def test_local_steinhardt_on_every_layout(abi, name, dtype, lmax, Ql_ref):
    """every option set with its force and its virial entry point, through the LDS-tile force kernel (13 table slots) and through
    k_qll_forces (22): block sums, c, n, v, b, forces, virial; with a cluster also labels, w and the summary.  The scratch of the
    `average` mode holds one slot per list ENTRY SLOT, epair[start + e]: the helpers size it with the length of the list array"""
    pos, L, types, nl = fcc_snapshot(4, dtype)
    N = len(pos)
    args = (1.4, 1.2, lmax, 0, Ql_ref)
    opt = LOCAL_SETS[name]
    if name == "bonds+cluster":
        # v_min: the median of the v_i themselves (a first run with every particle a node), so that about half the particles are nodes
        # and r_link = 1.0, the nearest-neighbour distance of the lattice: about half of the nearest pairs link
        first = run_gpu_ql_cluster(abi, pos, types, L, nl, dtype, opt=opt, cluster=(-1.0, 1.0), args=args)
        assert first["summary"][3] == N
        cluster = (float(np.median(first["v"])), 1.0)
        g = every_layout(lambda lists: run_gpu_ql_cluster(abi, pos, types, L, lists, dtype, opt=opt, cluster=cluster, args=args), nl, name)
        print("nodes %d, clusters %d, largest %d at root %d" % (g["summary"][3], g["summary"][2], g["summary"][1], g["summary"][0]))
        assert 0.3 * N < g["summary"][3] < 0.7 * N and g["summary"][2] > 1 and 1 < g["w"].sum() == g["summary"][1] < g["summary"][3]
    elif "bonds" in name:
        g = every_layout(lambda lists: run_gpu_bonds(abi, pos, types, L, lists, *args, dtype, opt=opt), nl, name)
        assert np.array_equal(g["F"], g["F_vir"]) and g["b"].max() > 0
    else:
        g = every_layout(lambda lists: run_gpu_opt(abi, pos, types, L, lists, *args, dtype, opt=opt), nl, name)
        v = every_layout(lambda lists: run_gpu_local_virial(abi, pos, types, L, lists, *args, dtype, opt=opt, pitch=N + 3), nl, name + " virial")
        assert np.array_equal(v["F"].astype(np.float64), g["F"]) and np.array_equal(v["F"], v["F_opt"])
        assert np.isfinite(v["raw"]).all() and np.abs(v["raw"][:, :N]).max() > 0
    assert np.isfinite(g["F"]).all() and np.abs(g["F"][:, :3]).max() > 0 and g["s"] > 0 and g["v"].min() >= 0
    if "gate" in name:
        assert ((g["n"] > 10) & (g["n"] < 16)).sum() > 10               # the gate's ramp is populated


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_largest_on_every_layout(abi, dtype):
    """mtd_cluster_largest alone on the liquid of tests/test_gpu_cluster.py at N = 1000.  A repeated edge links nothing new, so a third
    of the pairs is withheld from the list and sits in the slack: a walk that leaves its row links what the list does not"""
    case = ll.thinned_liquid(1000)
    theirs = liquid_case(1000)
    assert np.array_equal(case["pos"], theirs["pos"]) and np.array_equal(case["v"], theirs["v"]) and case["cluster"] == theirs["cluster"]
    assert all(np.array_equal(a, b) for a, b in zip(case["full"], theirs["nl"]))
    one = {k: case[k] for k in ("pos", "types", "L", "nl", "v", "cluster")}
    g, r = check_cluster(abi, one, dtype)                                # the compact list against the labels of the reference
    assert r["summary"][2] > 10 and 0.4 * 1000 < r["summary"][3] < 0.6 * 1000
    run = lambda lists: run_gpu_cluster(abi, case["pos"], case["types"], case["L"], lists, 0, case["v"], case["cluster"], dtype)[0]
    same_bits(g, every_layout(run, case["nl"], "cluster", stale=case["stale"]), "cluster against check()")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ghosts", [False, True], ids=["central", "ghosts"])
def test_pair_entropy_on_every_layout(abi, dtype, ghosts):
    """accumulate / finalize / forces with virial on fcc 5, all particles central and with the trailing 200 as ghosts (n_rows)"""
    pos, L, types, _ = fcc_snapshot(5, dtype)
    nl = util.build_nlist(pos, L, 2.4)
    n_rows = 300 if ghosts else None
    if ghosts:
        nl = ll.from_rows(ll.as_rows(nl)[:n_rows])
        assert (np.asarray(nl[2]) >= n_rows).any()
    g = every_layout(lambda lists: run_gpu_pe(abi, pos, types, L, lists, 2.0, 0.1, 40, 0, dtype, virial=True, n_rows=n_rows), nl, "pe",
                     n_positions=len(pos))
    assert np.isfinite(g["F"]).all() and np.abs(g["F"]).max() > 0 and np.abs(g["virial"]).max() > 0 and g["S"] < 0 and g["g"].max() > 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant,ghosts", [("fcc", False), ("two_switch", False), ("fcc", True)], ids=["fcc", "two_switch", "fcc-ghosts"])
def test_environment_similarity_on_every_layout(abi, dtype, variant, ghosts):
    """the fcc-template fused variant and the two-environment variant with a switch, with virial; the plain one once more with the
    trailing 200 particles as ghosts (n_ghost)"""
    pos, L, types, _ = fcc_snapshot(5, dtype)
    nl = util.build_nlist(pos, L, 1.5)
    t, lam, sw = ll.es_variants()[variant]
    kw = dict(lam=lam, sw=sw, virial=True)
    if ghosts:
        nl = ll.from_rows(ll.as_rows(nl)[:300])
        assert (np.asarray(nl[2]) >= 300).any()
        kw.update(n_rows=300, n_ghost=200)
    g = every_layout(lambda lists: run_gpu_es(abi, pos, types, L, lists, t, dtype, **kw), nl, "es", n_positions=len(pos))
    assert np.isfinite(g["F"]).all() and np.abs(g["F"]).max() > 0 and np.abs(g["virial"]).max() > 0 and g["s"] > 0.1


# ---- through the host classes ---------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _variable(cv, which, nl, sigma):
    if which in ("steinhardt", "steinhardt_half"):
        return cv.steinhardt(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=sigma)
    if which == "steinhardt_local":
        return cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=sigma, average=True)
    if which == "pair_entropy":
        return cv.pair_entropy(nlist=nl, type="A", sigma=sigma, r_max=1.2, sigma_r=0.08, n_bins=24)
    return cv.environment_similarity(cv.environment_templates("fcc", np.sqrt(2.0)), 0.12, 1.5, 1.3, nl, "A", sigma=sigma)


@pytest.mark.parametrize("which", ["steinhardt", "steinhardt_half", "steinhardt_local", "pair_entropy", "environment_similarity"])
def test_host_classes_on_slack_and_scattered_lists(api, which):
    """a nlist_cell fed by set_lists with a list in HOOMD's layout, two steps on a 64-point grid: the value, the bias factor and the
    force array are bitwise those of the run fed the compact list.  steinhardt_half: a half list in half storage mode, which the host
    class checks for symmetry on the host (NeighborList::setLists) and symmetrises on the device (mtd_ql_symmetrize_half_list_ws)"""
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types, full = fcc_snapshot(4, np.float64)
    half = which == "steinhardt_half"
    lists = layouts(util.build_nlist(pos, L, 1.55, half=True) if half else full)
    runs = {}
    val = None
    for kind in ("value", "compact", "slack", "scattered"):              # `value`: the compact list once before, for the grid of the three runs
        context.initialize(pos, types, ["A"], L, dtype=np.float64)
        meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
        nl = cv.nlist_cell(r_cut=1.55)
        var = _variable(cv, which, nl, 1.0 if val is None else 0.02 * abs(val))
        if half:
            nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
        nl.set_lists(*lists["compact" if kind == "value" else kind])
        if kind == "value":
            val = var.cpp_force.getCurrentValue(0)
            assert np.isfinite(val) and val != 0.0
        else:
            assert nl.cpp_nlist.getNumEntries() == len(lists[kind][2])
            var.set_grid(min(0.55 * val, 1.3 * val), max(0.55 * val, 1.3 * val), 64)
            context.run(2)
            t = context.current.system.getCurrentTimeStep()
            runs[kind] = dict(value=np.float64(var.cpp_force.getCurrentValue(t)), F=np.asarray(var.cpp_force.getForceArray()),
                              bias=np.asarray(meta.cpp_integrator.getBiasFactors(), dtype=np.float64))
        context.current = None
    assert runs["compact"]["value"] == val
    base = runs["compact"]
    assert abs(base["bias"][0]) > 0 and np.abs(base["F"][:, :3]).max() > 0 and np.isfinite(base["F"]).all()
    for kind in ("slack", "scattered"):
        same_bits(base, runs[kind], (which, kind))


def test_set_lists_refuses_a_row_that_ends_beyond_the_array(api):
    """NeighborList::setLists reads nlist[head[i] + k] on the host: a row that ends beyond the array raises before anything is replaced,
    and a valid list afterwards works"""
    context, cv, integrate = api
    pos, L, types, full = fcc_snapshot(4, np.float64)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.55)
    st = cv.steinhardt(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=1.0)
    slack = layouts(full)["scattered"]
    nl.set_lists(*slack)
    want = st.cpp_force.getCurrentValue(0)
    version = nl.cpp_nlist.getVersion()
    last = int(np.argmax(np.asarray(slack[0]).astype(np.int64) + np.asarray(slack[1]).astype(np.int64)))
    for bad in ((slack[0], slack[1], slack[2][:int(slack[0][last]) + int(slack[1][last]) - 1]),        # one entry short of the last row's end
                (full[0], full[1], full[2][:-1]), (full[0], full[1], full[2][:0]),
                (np.where(np.arange(len(pos)) == 7, 2 ** 32 - 2, full[0]).astype(np.uint32), full[1], full[2])):   # head + n_neigh wraps in 32 bits
        with pytest.raises(RuntimeError, match="ends beyond the nlist array"):
            nl.set_lists(*bad)
        assert nl.cpp_nlist.getVersion() == version and nl.cpp_nlist.getNumEntries() == len(slack[2])      # nothing was replaced
    nl.set_lists(slack[0], slack[1], slack[2][:int(slack[0][last]) + int(slack[1][last])])               # ends exactly with the array: fine
    nl.set_lists(*full)
    context.run(1)
    assert st.cpp_force.getCurrentValue(context.current.system.getCurrentTimeStep()) == want


# ---- 2. every row length -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_row_lengths_pair_entropy(abi, dtype):
    """row_walk<8>, both passes: rows of 0 .. 25 entries (A), padded with a self entry, the other type inside r_cut and a partner beyond
    it (B; an entry j >= N counts here, so none is added), and with the last member of every clump a ghost (C)"""
    case = ll.sweep("pe", dtype)
    pos, types, L = case["pos"], case["types"], case["L"]
    r = ll.reference("pe", dtype)
    for lists in (case["nl"], ll.padded(case, ghosts=False)):
        g = run_gpu_pe(abi, pos, types, L, lists, *ll.PE_SWEEP["par"], 0, dtype, virial=True)
        compare_pe(g, r, BIAS, dtype, types=types)
    s = ll.split_ghosts(case)
    g = run_gpu_pe(abi, s["pos"], s["types"], L, s["nl"], *ll.PE_SWEEP["par"], 0, dtype, virial=True, n_rows=s["n_rows"])
    compare_pe(g, ll.reference("pe", dtype, split=True), BIAS, dtype, types=s["types"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["fcc", "two_switch"])
def test_row_lengths_environment_similarity(abi, dtype, variant):
    """row_walk<4>, both passes: rows of 0 .. 13 entries (A), padded (B), and for the plain variant with ghosts (C).  sigma_env = 0.3:
    no k_i of a non-empty row is below 0.07 of the largest (tests/test_list_layouts.py)"""
    case = ll.sweep("es", dtype)
    pos, types, L = case["pos"], case["types"], case["L"]
    t, lam, sw = ll.es_variants()[variant]
    kw = dict(sigma_env=ll.ES_SWEEP["sigma_env"], r_on=ll.ES_SWEEP["r_on"], r_cut=ll.ES_SWEEP["r_cut"], lam=lam, sw=sw, virial=True)
    r = ll.reference("es", dtype, variant)
    for lists in (case["nl"], ll.padded(case, ghosts=False)):
        g = run_gpu_es(abi, pos, types, L, lists, t, dtype, **kw)
        compare_es(g, r, BIAS, dtype, types=types)
    if variant == "fcc":
        s = ll.split_ghosts(case)
        g = run_gpu_es(abi, s["pos"], s["types"], L, s["nl"], t, dtype, n_rows=s["n_rows"], n_ghost=len(pos) - s["n_rows"], **kw)
        compare_es(g, ll.reference("es", dtype, "fcc", split=True), BIAS, dtype, types=s["types"], zero_sum=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_lengths_cluster_link_pass(abi, dtype):
    """row_walk_entries<4, .., GHOSTS = false>: star lists of 0 .. 13 entries, every entry the only edge to its leaf (A), and padded with a
    self entry, the other type inside r_link, a node beyond it and an index >= N (B): labels, sizes, w and the summary exactly"""
    case = ll.sweep("cl", dtype)
    r = ll.reference("cl", dtype)
    for lists in (case["nl"], ll.padded(case, ghosts=True)):
        one = dict(pos=case["pos"], types=case["types"], L=case["L"], nl=lists, v=np.ones(len(case["pos"])),
                   cluster=(ll.CL_SWEEP["v_min"], ll.CL_SWEEP["r_link"]))
        g, r_list = check_cluster(abi, one, dtype)
        for key in ("label", "size", "w", "summary"):
            assert np.array_equal(g[key], r[key]) and np.array_equal(r_list[key], r[key]), key
    assert r["summary"].tolist()[1:] == [14, 14, 105]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("combo", sorted(ll.QL_COMBOS))
def test_row_lengths_local_steinhardt_memory_kernel(abi, dtype, combo):
    """k_qll_forces (degrees 4, 6, 8: 22 table slots) and the gather passes before it on the clumps of cluster_case: rows of 0 .. 13 (A),
    padded with a self entry, the other type, a partner beyond r_cut and an index >= N (B)"""
    case = ll.sweep("ql", dtype)
    pos, types, L = case["pos"], case["types"], case["L"]
    args = (ll.QL_SWEEP["r_cut"], ll.QL_SWEEP["r_on"], ll.QL_SWEEP["lmax"], 0, ll.QL_SWEEP["Ql_ref"])
    opt = ll.QL_COMBOS[combo]
    r = ll.reference("ql", dtype, combo)
    for lists in (case["nl"], ll.padded(case, ghosts=True)):
        if "bonds" in opt:
            compare_bonds(run_gpu_bonds(abi, pos, types, L, lists, *args, dtype, opt=opt), r, BIAS, dtype, types=types)
        else:
            compare_avg(run_gpu_opt(abi, pos, types, L, lists, *args, dtype, opt=opt), r, BIAS, dtype, types=types)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_row_lengths_global_steinhardt(abi, ref, dtype, mode):
    """QlFeed / QlUnit on rows of 0 .. 13 entries (the half list of mode 1 has them too) against the oracle, with the bounds of
    test_ql_parity: Q_lm to 1e-11 of its scale, Q_l and the value to 1e-10, forces to 1e-9 / 2e-7 of max|F|.  Run B pads with the other
    type inside r_cut and a partner beyond it (docstring of the module)"""
    case = ll.sweep("ql", dtype)
    pos, types, L = case["pos"], case["types"], case["L"]
    args = (ll.QL_SWEEP["r_cut"], ll.QL_SWEEP["r_on"], ll.QL_SWEEP["lmax"], 0, ll.QL_SWEEP["Ql_ref"])
    nl = ll.half_of(case["nl"]) if mode == 1 else case["nl"]
    assert set(np.asarray(nl[1]).tolist()) == set(range(14))
    r = run_ref_ql(ref, pos, types, L, nl, *args, half=mode == 1, bias=BIAS)
    fs, qs = np.abs(r[3][:, :3]).max(), np.abs(r[2]).max()
    assert fs > 0
    for lists in (nl, ll.padded(case, ghosts=False, own=False, nl=nl)):
        assert len(lists[2]) == len(nl[2]) + (0 if lists is nl else 2 * case["n_members"])
        g = run_gpu_ql(abi, pos, types, L, lists, *args, dtype, half=mode, bias=BIAS)
        err = np.abs(g[3][:, :3] - r[3][:, :3]).max()
        print("Q_lm %.3e of %.3e; value %.15g vs %.15g; forces %.3e of max |F| %.3e" % (np.abs(g[2] - r[2]).max(), qs, g[0], r[0], err, fs))
        assert np.abs(g[2] - r[2]).max() <= 1e-11 * qs
        assert np.allclose(g[1], r[1], rtol=1e-10, atol=1e-13 * np.abs(r[1]).max())
        assert g[0] == pytest.approx(r[0], rel=1e-10)
        assert err <= (1e-9 if dtype == np.float64 else 2e-7) * fs
        assert np.all(g[3][:, 3] == 0.0) and np.all(g[3][types == 1] == 0.0)
