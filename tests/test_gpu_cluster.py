"""GPU: mtd_cluster_largest (csrc/cluster.hip) alone against the labels of tests/ql_local_cluster_ref.py
(scipy.sparse.csgraph.connected_components, relabelled to the smallest member index).  Everything is integer or 0 / 1: every comparison
is exact.  So that rounding cannot flip a node or an edge between the two sides, every |v_i - v_min| is 0 by construction or > 1e-6 and
every listed pair distance differs from r_link by more than 1e-6 relative — asserted for every case; with fp32 arrays both sides see the
rounded positions.  The scratch starts as garbage: whatever is read back must have been written."""
import ctypes as C

import numpy as np
import pytest

import ql_local_cluster_ref as cr
import stream_gate
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

NONE = cr.NONE
DTYPES = [np.float64, np.float32]


def run_gpu(abi, pos, types, L, nl, type_id, v, cluster, dtype, tilt=None, calls=1, gate=None):
    """`calls` calls on the same scratch; returns the list of dict(label, size, w, summary) read back after each.  gate: the stream the
    calls run on and how their inputs arrive (tests/stream_gate.py; None: the NULL stream)"""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N = len(pos)
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    d_pos = gate.inp(util.pack_postype(np.asarray(pos).astype(dtype), types, dtype))
    lists = [np.asarray(x).astype(np.int64).astype(np.uint32).view(np.int32) for x in nl]
    lists[2] = np.concatenate([lists[2], np.zeros(1, dtype=np.int32)])           # never empty: a device pointer to hand over
    d_head, d_nn, d_nl = (gate.inp(x) for x in lists)
    d_v = gate.inp(np.asarray(v, dtype=np.float64))
    p = abi.ClusterParams.make(cluster)
    n_bytes = lib.mtd_cluster_scratch_bytes(N)
    scratch = torch.full((n_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    out = []
    stream = gate.arm()
    for _ in range(calls):
        ptrs = [C.c_void_p() for _ in range(4)]
        abi.check(lib.mtd_cluster_largest(N, abi.ptr(d_pos), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), type_id,
                                          abi.ptr(d_v), C.byref(p), abi.ptr(scratch), *[C.byref(x) for x in ptrs], stream))

        def read():
            raw = scratch.cpu().numpy()
            at = [x.value - scratch.data_ptr() for x in ptrs]
            assert all(0 <= a and a % 16 == 0 for a in at) and max(at) < n_bytes
            take = lambda a, n, t: raw[a:a + n * np.dtype(t).itemsize].view(t).copy()
            return dict(label=take(at[0], N, np.uint32), size=take(at[1], N, np.uint32), w=take(at[2], N, np.float64),
                        summary=take(at[3], 4, np.uint32))
        out.append(gate.done(read))
    return out


def check(abi, case, dtype, calls=1):
    """one case = dict(pos, types, L, nl, v, cluster, [type_id, tilt]): the input conditions, then every output against the ref's"""
    pos = np.asarray(case["pos"], dtype=np.float64).astype(dtype).astype(np.float64)
    types, L, nl, v, cluster = case["types"], case["L"], case["nl"], case["v"], case["cluster"]
    type_id, tilt = case.get("type_id", 0), case.get("tilt")
    dv, dr = cr.margins(pos, types, L, nl, type_id, v, *cluster, tilt=tilt)
    assert dv > 1e-6 and dr > 1e-6, (dv, dr)
    r = cr.clusters(pos, types, L, nl, type_id, v, *cluster, tilt=tilt)
    got = run_gpu(abi, pos, types, L, nl, type_id, v, cluster, dtype, tilt=tilt, calls=calls)
    g = got[0]
    print("N %d: %d nodes, %d clusters, largest %d at root %d" % (len(pos), r["summary"][3], r["summary"][2], r["summary"][1], r["summary"][0]))
    assert np.array_equal(g["summary"], r["summary"]), (g["summary"], r["summary"])
    for key in ("label", "size", "w"):
        assert np.array_equal(g[key], r[key]), key
    for other in got[1:]:
        for key in ("label", "size", "w", "summary"):
            assert g[key].tobytes() == other[key].tobytes(), key
    return g, r


def all_pairs(N):
    """every particle lists every other one: the distance test decides"""
    head = np.arange(N) * (N - 1)
    nn = np.full(N, N - 1)
    lst = np.array([j for i in range(N) for j in range(N) if j != i], dtype=np.int64)
    return head, nn, lst


def liquid(N, seed, density=0.8, r_list=1.5):
    """random positions at liquid density, v random, v_min in the widest gap about the median, r_link in the widest gap of the distances"""
    rng = np.random.default_rng(seed)
    L = (N / density) ** (1.0 / 3.0)
    pos = rng.uniform(-0.5 * L, 0.5 * L, (N, 3)).astype(np.float32).astype(np.float64)      # the same numbers for both dtypes
    types = np.zeros(N, dtype=np.int32)
    nl = util.build_nlist(pos, L, r_list)
    v = rng.random(N)
    v_min, _ = cr.widest_gap(v, np.quantile(v, 0.47), np.quantile(v, 0.53))
    _, _, rsq = cr.listed(pos, nl, L)
    r_link, _ = cr.widest_gap(np.sqrt(rsq), 1.0, 1.1)
    return dict(pos=pos, types=types, L=L, nl=nl, v=v, cluster=(v_min, r_link))


_cases = {}


def liquid_case(N, seed=None):
    seed = N if seed is None else seed
    if (N, seed) not in _cases:
        _cases[N, seed] = liquid(N, seed=seed)
    return _cases[N, seed]


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_particle(abi, dtype):
    nl = (np.zeros(1), np.zeros(1), np.zeros(0))
    g, r = check(abi, dict(pos=np.zeros((1, 3)), types=np.zeros(1, dtype=np.int32), L=10.0, nl=nl, v=np.ones(1), cluster=(0.5, 1.0)), dtype)
    assert g["summary"].tolist() == [0, 1, 1, 1] and g["w"].tolist() == [1.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_node_at_all(abi, dtype):
    case = dict(liquid_case(1000), cluster=(2.0, liquid_case(1000)["cluster"][1]))
    g, r = check(abi, case, dtype)
    assert g["summary"].tolist() == [NONE, 0, 0, 0] and not g["w"].any() and (g["label"] == NONE).all() and not g["size"].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_particles_one_cluster(abi, dtype):
    pos, L = util.fcc_lattice(3)
    N = len(pos)
    g, r = check(abi, dict(pos=pos, types=np.zeros(N, dtype=np.int32), L=L, nl=util.build_nlist(pos, L, 1.3), v=np.ones(N), cluster=(0.5, 1.1)),
                 dtype)
    assert g["summary"].tolist() == [0, N, 1, N] and g["w"].all() and g["size"][0] == N


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1000, 4099])
def test_liquid_with_v_min_at_the_median(abi, dtype, N):
    """several blocks and a ragged last chunk (4099 = 64 * 64 + 3); about half the particles are nodes; twice: the same bytes"""
    g, r = check(abi, liquid_case(N), dtype, calls=2)
    assert 0.4 * N < r["summary"][3] < 0.6 * N and r["summary"][2] > 10


# ---- the loops behind the block caps: init, flatten and mask run 1024 blocks of 256 lanes (one trip up to N = 262 144), link 4096 blocks
# of 64 rows (the same N), pick 256 blocks of 256 lanes (N = 65 536) ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_loop_liquid_past_every_cap(abi, dtype):
    """270 001 particles: 1055 chunks of 256 on 1024 blocks (flatten takes two rounds, in every lane), 4219 chunks of 64 rows on 4096
    blocks, 1055 chunks on the 256 blocks of the pick (four or five trips); about half the particles are nodes; twice: the same bytes"""
    N = 270_001
    assert (N + 255) // 256 > 1024 and (N + 63) // 64 > 4096
    g, r = check(abi, liquid_case(N, seed=3), dtype, calls=2)
    assert 0.4 * N < r["summary"][3] < 0.6 * N and r["summary"][2] > 10_000
    assert r["summary"].tolist() == [316, 100, 46090, 133917]
    assert (r["label"][262_144:] != NONE).sum() > 1000                  # nodes among the particles of the second round


def test_chunk_loop_of_the_pick_alone(abi):
    """70 001 particles: 274 chunks of 256, so only k_cluster_pick (256 blocks) takes a second trip, in blocks 0 - 17; clusters rooted at
    i >= 65 536 are counted there, by nothing else"""
    N = 70_001
    assert 256 < (N + 255) // 256 <= 1024 and (N + 63) // 64 <= 4096
    g, r = check(abi, liquid_case(N), np.float64, calls=2)
    assert 0.4 * N < r["summary"][3] < 0.6 * N and r["summary"][2] > 10_000
    assert (r["label"][65_536:] == np.arange(65_536, N)).sum() > 100     # roots that the second trip counts


@pytest.mark.parametrize("order", ["lattice", "permuted"])
def test_chunk_loop_one_cluster_spanning_the_box(abi, order):
    """simple cubic 65^3 (N = 274 625), every particle a node, linked to its six neighbours: one cluster with root 0.  4292 chunks of 64
    rows on 4096 blocks and 1073 chunks of 256 on 1024: every atomic of the link pass falls on one tree, the flatten pass counts all
    members on one word over two rounds.  In lattice order and with the indices permuted at random (deep trees, as the chain above)"""
    n = 65
    axis = np.arange(n) - 0.5 * (n - 1)
    pos = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    N = len(pos)
    assert N == 274_625 and (N + 255) // 256 > 1024 and (N + 63) // 64 > 4096
    if order == "permuted":
        pos = pos[np.random.default_rng(8).permutation(N)]
    nl = util.build_nlist(pos, float(n), 1.3)
    assert len(nl[2]) == 6 * N
    case = dict(pos=pos, types=np.zeros(N, dtype=np.int32), L=float(n), nl=nl, v=np.ones(N), cluster=(0.5, 1.1))
    g, r = check(abi, case, np.float64, calls=2)
    assert g["summary"].tolist() == [0, N, 1, N]
    assert not g["label"].any() and g["size"][0] == N and not g["size"][1:].any() and (g["w"] == 1.0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_of_4096_in_permuted_order(abi, dtype):
    """a chain whose indices are a random permutation along it: deep trees, the worst case for hooking by index"""
    N = 4096
    rng = np.random.default_rng(8)
    order = rng.permutation(N)                                           # the particle at rank k of the chain has index order[k]
    pos = np.zeros((N, 3))
    pos[order, 0] = np.arange(N) - 0.5 * N
    rows = [[] for _ in range(N)]
    for k in range(N):
        rows[order[k]] = [order[m] for m in (k - 1, k + 1) if 0 <= m < N]
    nn = np.array([len(x) for x in rows])
    head = np.concatenate([[0], np.cumsum(nn)[:-1]])
    nl = (head, nn, np.array([j for x in rows for j in x]))
    g, r = check(abi, dict(pos=pos, types=np.zeros(N, dtype=np.int32), L=2.0 * N, nl=nl, v=np.ones(N), cluster=(0.5, 1.1)), dtype, calls=2)
    assert g["summary"].tolist() == [0, N, 1, N]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tilt", [None, dict(xy=0.3, xz=-0.2, yz=0.25)])
def test_cluster_connected_only_through_the_periodic_boundary(abi, dtype, tilt):
    """six particles in a row across the y (and z) faces of the box, three on each side, and four far away: one cluster of six only
    with the minimum image, in the tilted box with its shifted images"""
    L = 20.0
    t = tilt or dict(xy=0.0, xz=0.0, yz=0.0)
    h = np.array([[L, t["xy"] * L, t["xz"] * L], [0, L, t["yz"] * L], [0, 0, L]])
    frac = [[0.1, 0.44 + 0.02 * k, 0.45 + 0.02 * k] for k in range(6)] + [[-0.3, 0.0, 0.0], [0.3, 0.1, 0.2], [0.0, -0.3, 0.1], [0.2, 0.2, -0.3]]
    frac = np.array(frac)
    frac -= np.rint(frac)                                                # wrapped into [-0.5, 0.5]: the row is cut in two
    pos = frac @ h.T
    N = len(pos)
    step = np.linalg.norm(h @ np.array([0.0, 0.02, 0.02]))
    case = dict(pos=pos, types=np.zeros(N, dtype=np.int32), L=L, nl=all_pairs(N), v=np.ones(N), cluster=(0.5, 1.2 * step), tilt=tilt)
    g, r = check(abi, case, dtype)
    assert g["summary"].tolist() == [0, 6, 5, N] and g["w"].tolist() == [1.0] * 6 + [0.0] * 4
    plain = np.sqrt(((pos[2] - pos[3]) ** 2).sum())
    assert plain > 10 * step                                             # without the minimum image 2 and 3 are far apart


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_clusters_of_equal_size_the_smaller_root_wins(abi, dtype):
    pos = np.zeros((12, 3))
    pos[:, 0] = 3.0 * np.arange(12) - 18.0
    pos[7] = pos[3] + [0, 1, 0]
    pos[9] = pos[2] + [0, 1, 0]
    pos[11] = pos[5] + [0, 0, 1]
    case = dict(pos=pos, types=np.zeros(12, dtype=np.int32), L=40.0, nl=all_pairs(12), v=np.ones(12), cluster=(0.5, 1.1))
    g, r = check(abi, case, dtype)
    assert g["summary"].tolist() == [2, 2, 9, 12]
    assert np.nonzero(g["w"])[0].tolist() == [2, 9] and g["label"][7] == 3 and g["label"][11] == 5


@pytest.mark.parametrize("dtype", DTYPES)
def test_other_types_ghost_entries_self_entries_thresholds_and_nan(abi, dtype):
    """a crystal with a second type sprinkled in (never a node, never a link), rows padded with entries j >= N (a ghost index, the
    largest unsigned) and with the particle itself at the front, in the middle and at the end; v exactly equal to v_min is a node, v just
    below is not, NaN is not"""
    pos, L = util.fcc_lattice(4)
    N = len(pos)
    rng = np.random.default_rng(3)
    types = (rng.random(N) < 0.25).astype(np.int32)
    head, nn, lst = (np.asarray(x).astype(np.int64) for x in util.build_nlist(pos, L, 1.3))
    rows = []
    for i in range(N):
        row = list(lst[head[i]:head[i] + nn[i]])
        mid = len(row) // 2
        rows.append([N + 7] + row[:mid] + [i, NONE] + row[mid:] + [N])
    nn2 = np.array([len(x) for x in rows])
    nl = (np.concatenate([[0], np.cumsum(nn2)[:-1]]), nn2, np.array([j for x in rows for j in x]))
    v = np.where(rng.random(N) < 0.5, 0.5, rng.choice([0.1, 0.9, 0.5 - 1e-5, np.nan], N))
    assert (v == 0.5).sum() > 50 and np.isnan(v).sum() > 10 and (v == 0.5 - 1e-5).sum() > 10
    for type_id in (0, 1):
        g, r = check(abi, dict(pos=pos, types=types, L=L, nl=nl, v=v, cluster=(0.5, 1.1), type_id=type_id), dtype)
        assert (g["label"][types != type_id] == NONE).all() and (g["label"][np.isnan(v)] == NONE).all()
        assert (g["label"][(v == 0.5) & (types == type_id)] != NONE).all() and (g["label"][v == 0.5 - 1e-5] == NONE).all()
        assert r["summary"][2] > 1 or type_id == 0                      # the majority type percolates through the crystal, the other cannot


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_directional_list_gives_the_labels_of_its_symmetric_closure(abi, dtype):
    case = liquid_case(1000)
    head, nn, lst = (np.asarray(x).astype(np.int64) for x in case["nl"])
    rng = np.random.default_rng(6)
    i = np.repeat(np.arange(len(head)), nn)
    lo, hi = np.minimum(i, lst), np.maximum(i, lst)
    coin = rng.random((len(head), len(head))) < 0.5                      # one coin per unordered pair: the entry of one of its ends goes
    keep = np.where(coin[lo, hi], i == lo, i == hi)
    nn2 = np.bincount(i[keep], minlength=len(head))
    one_way = (np.concatenate([[0], np.cumsum(nn2)[:-1]]), nn2, lst[keep])
    assert len(one_way[2]) * 2 == len(lst)
    sym, r_sym = check(abi, case, dtype)
    g, r = check(abi, dict(case, nl=one_way), dtype)
    for key in ("label", "size", "w", "summary"):
        assert np.array_equal(g[key], sym[key]), key
