"""Shared test helpers: seeded particle snapshots and tensor packing."""
import ctypes as C

import numpy as np

# lattice vectors of the headline config
CV1_VECTORS = [(0, 0, 3), (0, 3, 0), (3, 0, 0), (0, 0, 6), (0, 6, 0), (6, 0, 0), (3, 3, 0), (0, 3, 3)]
CV2_VECTORS = [(1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, 1, 1), (2, 2, 2), (2, -2, 2), (2, 2, -2), (-2, 2, 2)]
MODE_AB = [1.0, -1.0]


def snapshot_config0b():
    """N=4096: 16^3 simple-cubic lattice + U(-0.1,0.1) noise, lamellae of period 4a along z."""
    rng = np.random.default_rng(2024)
    n = 16
    ix, iy, iz = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    pos = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3).astype(np.float64) - n / 2  # lattice sites at lo + i*a
    pos += rng.uniform(-0.1, 0.1, size=pos.shape)
    types = (iz.reshape(-1) % 4 >= 2).astype(np.int32)  # A (0) if iz mod 4 < 2 else B (1)
    return pos, types, float(n)


def snapshot_random(N, L, seed=12345, modulated=False, dtype=np.float32):
    """config 2 style: uniform random positions, types = index parity; optional lamellar modulation
    z <- z + 1.5 sign(a) sin(2 pi 3 z / L) so that |s_1| = O(0.1)."""
    rng = np.random.default_rng(seed)
    pos = rng.random((N, 3)) * L - L / 2
    types = (np.arange(N) % 2).astype(np.int32)
    if modulated:
        a = np.where(types == 0, 1.0, -1.0)
        pos[:, 2] = pos[:, 2] + 1.5 * a * np.sin(2 * np.pi * 3 * pos[:, 2] / L)
    pos = pos.astype(dtype)  # the snapshot IS the rounded array; the oracle sees the same values
    return pos, types


def pack_postype(pos, types, dtype):
    """HOOMD Scalar4 postype as a numpy array: float32 (N,4) with the int32 type bit-cast into w,
    or float64 (N,4) with the type in the LOW 32 bits of w."""
    N = pos.shape[0]
    if dtype == np.float32:
        out = np.empty((N, 4), dtype=np.float32)
        out[:, :3] = pos
        out[:, 3] = np.asarray(types, dtype=np.int32).view(np.float32)
    else:
        out = np.empty((N, 4), dtype=np.float64)
        out[:, :3] = pos
        w = np.zeros(N, dtype=np.int64)
        w[:] = np.asarray(types, dtype=np.int64) & 0xFFFFFFFF
        out[:, 3] = w.view(np.float64)
    return out


def oracle_postype(pos, types):
    out = np.empty((pos.shape[0], 4), dtype=np.float64)
    out[:, :3] = pos.astype(np.float64)
    out[:, 3] = types
    return out


def flat_lattice(vectors):
    return (C.c_int * (3 * len(vectors)))(*[int(x) for v in vectors for x in v])


def dbl_array(values):
    return (C.c_double * len(values))(*[float(v) for v in values])


def uint_array(values):
    return (C.c_uint * len(values))(*[int(v) for v in values])


def build_nlist(pos, L, r_cut, half=False):
    """HOOMD-layout neighbour list (head_list, n_neigh, nlist) of a cubic periodic box with scipy's periodic KD-tree:
    the stand-in for hoomd.md.nlist in tests (HOOMD's NeighborList is not part of the plugin)."""
    from scipy.spatial import cKDTree
    p = np.mod(np.asarray(pos, dtype=np.float64) + L / 2, L)
    p[p >= L] -= L
    tree = cKDTree(p, boxsize=L)
    pairs = tree.query_pairs(r_cut, output_type="ndarray")
    N = len(p)
    if half:
        i, j = pairs[:, 0], pairs[:, 1]
    else:
        i = np.concatenate([pairs[:, 0], pairs[:, 1]])
        j = np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    n_neigh = np.bincount(i, minlength=N).astype(np.uint32)
    head = np.zeros(N, dtype=np.uint32)
    head[1:] = np.cumsum(n_neigh)[:-1]
    return head, n_neigh, j.astype(np.uint32)


def fcc_lattice(n, nn_dist=1.0):
    """n^3 fcc cells x 4 particles, nearest-neighbour distance nn_dist; returns positions centred on 0 and box length"""
    a = nn_dist * np.sqrt(2.0)
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    pos = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    L = n * a
    return pos - L / 2 + 0.25 * a, L


def random_rotation(seed):
    """a proper rotation (3, 3): Q of the QR decomposition of a seeded normal matrix, signs fixed so that det = +1"""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    assert abs(np.linalg.det(q) - 1.0) < 1e-12 and np.abs(q @ q.T - np.eye(3)).max() < 1e-14
    return q


# ---- crystals with bonds ON the z axis (tests/test_ql_axis_ref.py, tests/test_gpu_ql_axis.py) ------------------------------------
# Particles of one column share x and y bit for bit, so every bond inside a column has dx = dy = 0 exactly, the ones wrapped through
# the box included.  Noise: per particle in z only; every column gets one common shift in x and y.  Bonds between columns are then
# generic and no particle is an inversion centre any more (on the perfect lattice every finite gradient is 0).
COLUMNS = {
    # name: (cells per edge, basis, entries with rho == 0 among those inside r_cut)
    "bcc_columns": (4, [[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]], 256),          # 128 particles, both shells: 14 neighbours
    "sc_columns": (5, [[0.0, 0.0, 0.0]], 250),                            # 125 particles (no multiple of 64), 6 neighbours
}
COLUMNS_R_LIST, COLUMNS_R_CUT, COLUMNS_R_ON, COLUMNS_SIGMA = 1.35, 1.25, 1.05, 0.04


def axis_entries(pos, L, nl, r_cut):
    """(on, dz): mask of the list entries inside r_cut with dx = dy = 0 exactly, and dz of every entry inside r_cut"""
    import ql_local_ref
    types = np.zeros(len(pos), dtype=np.int32)
    _, _, d = ql_local_ref.pairs(np.asarray(pos, dtype=np.float64), types, nl, 0, r_cut, L=L)
    return (d[:, 0] == 0.0) & (d[:, 1] == 0.0), d[:, 2]


def _columns(name, seed, dtype, offsets):
    n, basis, want = COLUMNS[name]
    basis = np.asarray(basis)
    L = float(n)
    rng = np.random.default_rng(seed)
    col = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)          # columns of the cell grid
    xy = (col[:, None, :] + basis[None, :, :2]).reshape(-1, 2) - L / 2 + 0.25                         # one row per column
    xy = xy + rng.normal(0, COLUMNS_SIGMA, xy.shape)
    n_col = len(xy)
    z = (np.arange(n)[None, :] + np.tile(basis[:, 2], n * n)[:, None]) - L / 2 + 0.25                 # (column, place in it)
    z = z + rng.normal(0, COLUMNS_SIGMA, z.shape)
    pos = np.empty((n_col, n, 3))
    pos[:, :, :2] = xy[:, None, :]
    pos[:, :, 2] = z
    if offsets is not None:
        lo, hi = offsets
        size = np.exp(rng.uniform(np.log(lo), np.log(hi), (n_col, n)))
        size[rng.permutation(n_col)[:n_col // 4]] = 0.0                                               # a quarter of the columns stays exact
        ang = rng.uniform(0, 2 * np.pi, (n_col, n))
        pos[:, :, 0] += size * np.cos(ang)
        pos[:, :, 1] += size * np.sin(ang)
    pos = pos.reshape(-1, 3)
    if dtype == np.float32:
        pos = pos.astype(np.float32).astype(np.float64)                                               # the snapshot IS the rounded array
    nl = build_nlist(pos, L, COLUMNS_R_LIST)
    on, dz = axis_entries(pos, L, nl, COLUMNS_R_CUT)
    n_on = int(on.sum())
    if offsets is None:
        assert n_on == want, (name, n_on, want)
    else:
        assert 0 < n_on < want, (name, n_on, want)
    assert (dz[on] > 0).any() and (dz[on] < 0).any()
    return dict(pos=pos, types=np.zeros(len(pos), dtype=np.int32), L=L, nl=nl, r_cut=COLUMNS_R_CUT, r_on=COLUMNS_R_ON, type_id=0), n_on


def columns(name, seed=2024, dtype=np.float64):
    """(case, n_on): `bcc_columns` or `sc_columns`; case holds pos, types, L, nl, r_cut, r_on, type_id; n_on: entries exactly on the axis
    (asserted: 256 / 250, both signs of dz among them)"""
    return _columns(name, seed, dtype, None)


def near_axis(name, seed=2024, dtype=np.float64, lo=None, hi=1e-2):
    """the same snapshot with a further x, y offset per particle, its size log-uniform in [lo, hi] (lo: 1e-14, or one ulp of an fp32
    coordinate, 2^-23), a quarter of the columns left at exactly 0: bonds from exactly on the axis to 1e-2 off it"""
    if lo is None:
        lo = 1e-14 if dtype == np.float64 else 2.0 ** -23
    return _columns(name, seed, dtype, (lo, hi))
