"""GPU: the device neighbour-list build (mtd_nlist_*, csrc/nlist.hip) against yardsticks that are never the code under test:
tests/util.py::build_nlist (scipy's periodic KD-tree) for cubic boxes and, for everything the KD-tree cannot do, the brute-force
all-pairs minimum image in fractional coordinates of this file (N <= 3000).  Rows are compared as sorted sets, exactly.

Boundary pairs: a pair whose distance equals r_list to rounding may fall either way, so every case builds its yardstick at
r_list (1 - 1e-9), r_list and r_list (1 + 1e-9) and ASSERTS that the three are identical before it uses them — a condition on the
input (seeds are picked accordingly), not a tolerance on the result."""
import ctypes as C

import numpy as np
import pytest

import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EPS = 1e-9


# ---- reading device memory the library owns ----------------------------------------------------------------------------------------

def _download_uints(ptr, count):
    from metadynamics import _metadynamics
    return np.asarray(_metadynamics.download_uints(int(ptr or 0), int(count)), dtype=np.uint32)


class Handle:
    """stream: the HIP stream of mtd_nlist_build / mtd_nlist_check (None: the NULL stream).  The fill of a build is only stream-ordered:
    the download waits for the device on the NULL stream and for `wait` (the caller's torch stream) otherwise"""

    def __init__(self, abi, stream=None, wait=None):
        self.abi, self.lib = abi, abi.load()
        self.stream, self.wait = stream, wait
        self.h = C.c_void_p()
        abi.check(self.lib.mtd_nlist_create(C.byref(self.h)))

    def build_rc(self, postype, n_local, box, r_list, half=False, type=-1):
        """(status, lists); postype: packed Scalar4 array (fp32 or fp64) of locals followed by ghosts"""
        dt = self.abi.MTD_F32 if postype.dtype == np.float32 else self.abi.MTD_F64
        self.d_pos = torch.from_numpy(np.ascontiguousarray(postype)).cuda() if len(postype) else None
        return self.build_device(self.d_pos, dt, len(postype), n_local, box, r_list, half, type)

    def build_device(self, d_pos, dt, n_total, n_local, box, r_list, half=False, type=-1, after_build=None):
        """the same on a position array that is on the device already; after_build(): called when mtd_nlist_build has returned"""
        self.d_pos = d_pos
        head, nn, nl, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        rc = self.lib.mtd_nlist_build(self.h, n_local, n_total - n_local, self.abi.ptr(self.d_pos), dt, C.byref(box), float(r_list),
                                      int(half), int(type), C.byref(head), C.byref(nn), C.byref(nl), C.byref(n), self.stream)
        if after_build is not None:
            after_build()
        if rc != 0:
            return rc, None
        if self.stream is None:
            torch.cuda.synchronize()
        else:
            self.wait.synchronize()
        return rc, (_download_uints(head.value, n_local), _download_uints(nn.value, n_local), _download_uints(nl.value, n.value))

    def build(self, *a, **k):
        rc, lists = self.build_rc(*a, **k)
        self.abi.check(rc)
        return lists

    def check(self, postype, box, r_buff):
        dt = self.abi.MTD_F32 if postype.dtype == np.float32 else self.abi.MTD_F64
        return self.check_device(torch.from_numpy(np.ascontiguousarray(postype)).cuda(), dt, box, r_buff)

    def check_device(self, d, dt, box, r_buff):
        needs = C.c_int(-1)
        self.abi.check(self.lib.mtd_nlist_check(self.h, self.abi.ptr(d), dt, C.byref(box), float(r_buff), C.byref(needs), self.stream))
        return needs.value

    def cells(self):
        dim = (C.c_uint * 3)()
        self.abi.check(self.lib.mtd_nlist_cells(self.h, dim))
        return tuple(dim)

    def close(self):
        self.abi.check(self.lib.mtd_nlist_destroy(self.h))


@pytest.fixture()
def handle(abi):
    h = Handle(abi)
    yield h
    h.close()


# ---- yardsticks ------------------------------------------------------------------------------------------------------------------------

def lattice(L, xy=0.0, xz=0.0, yz=0.0):
    """columns a1, a2, a3 (HOOMD: a1 = (Lx, 0, 0), a2 = (xy Ly, Ly, 0), a3 = (xz Lz, yz Lz, Lz))"""
    L = [float(L)] * 3 if np.isscalar(L) else [float(x) for x in L]
    return np.array([[L[0], xy * L[1], xz * L[2]], [0.0, L[1], yz * L[2]], [0.0, 0.0, L[2]]])


def face_distances(h):
    return 1.0 / np.linalg.norm(np.linalg.inv(h), axis=1)


def min_image(d, h, periodic=(1, 1, 1)):
    f = d @ np.linalg.inv(h).T
    f -= np.round(f) * np.asarray(periodic, dtype=np.float64)
    return f @ h.T


def brute_nlist(pos, h, r, periodic=(1, 1, 1), n_local=None, half=False, types=None, type=-1):
    """all pairs, minimum image in fractional coordinates; rows of the first n_local particles, partners ascending"""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    n_local = n if n_local is None else n_local
    hinv = np.linalg.inv(h)
    f = pos @ hinv.T
    per = np.asarray(periodic, dtype=np.float64)
    rows_i, rows_j = [], []
    for lo in range(0, n_local, 256):
        df = f[lo:lo + 256, None, :] - f[None, :, :]
        df -= np.round(df) * per
        d = df @ h.T
        ok = (d * d).sum(-1) <= r * r
        i, j = np.nonzero(ok)
        i = i + lo
        keep = i != j
        if half:
            keep &= j > i
        if type >= 0:
            keep &= (types[i] == type) & (types[j] == type)
        rows_i.append(i[keep])
        rows_j.append(j[keep])
    i = np.concatenate(rows_i) if rows_i else np.zeros(0, dtype=np.int64)
    j = np.concatenate(rows_j) if rows_j else np.zeros(0, dtype=np.int64)
    order = np.lexsort((j, i))
    return _rows_to_lists(i[order], j[order], n_local)


def _rows_to_lists(i, j, n_rows):
    nn = np.bincount(i, minlength=n_rows).astype(np.uint32)
    head = np.zeros(n_rows, dtype=np.uint32)
    if n_rows:
        head[1:] = np.cumsum(nn)[:-1]
    return head, nn, j.astype(np.uint32)


def stable_yardstick(make, r):
    """the yardstick at r (1 - 1e-9), r, r (1 + 1e-9): identical, or the INPUT is unfit (pick another seed)"""
    lo, mid, hi = make(r * (1 - EPS)), make(r), make(r * (1 + EPS))
    for a, b, c in zip(lo, mid, hi):
        assert np.array_equal(a, b) and np.array_equal(b, c), "a pair sits on r_list to rounding: the input is unfit"
    return mid


def sort_rows(lists):
    head, nn, nl = lists
    rows = np.repeat(np.arange(len(nn)), nn)
    assert len(rows) == len(nl)
    return head, nn, nl[np.lexsort((nl, rows))]


def assert_same(got, want):
    got = sort_rows(got)
    assert len(got[2]) == len(want[2])                                    # n_entries
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[2], want[2])


def filter_type(lists, types, t):
    head, nn, nl = lists
    i = np.repeat(np.arange(len(nn)), nn)
    keep = (types[i] == t) & (types[nl] == t)
    return _rows_to_lists(i[keep], nl[keep], len(nn))


def config5(dtype):
    pos, L = util.fcc_lattice(40)
    pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
    return pos.astype(dtype), L


def random_box_system(seed, n, L, tilt=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    h = lattice(L, *tilt)
    f = rng.random((n, 3)) - 0.5
    return f @ h.T, h


# ---- 1. config-5 size -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_config5_full_and_half_match_kdtree(abi, handle, dtype):
    pos, L = config5(dtype)
    N = len(pos)
    types = np.zeros(N, dtype=np.int32)
    wide = pos.astype(np.float64)                                             # fp32 data is widened exactly
    want = stable_yardstick(lambda r: util.build_nlist(wide, L, r), 1.4)
    if dtype == np.float64:
        assert len(want[2]) == 3687802
    pt = util.pack_postype(pos, types, dtype)
    box = abi.Box.make(L)
    assert_same(handle.build(pt, N, box, 1.4), want)
    # half: the same pairs, each once on its smaller index (the three full lists above are identical, so are the half lists)
    want_half = util.build_nlist(wide, L, 1.4, half=True)
    assert 2 * len(want_half[2]) == len(want[2])
    assert_same(handle.build(pt, N, box, 1.4, half=True), want_half)


# ---- 2. orthorhombic and triclinic boxes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,L,tilt", [(1, (9.0, 12.5, 16.0), (0.0, 0.0, 0.0)), (2, (11.0, 12.0, 13.0), (0.4, -0.3, 0.25)),
                                         (3, (14.0, 10.0, 12.0), (-0.4, 0.4, -0.4)), (4, (12.0, 12.0, 12.0), (0.17, 0.0, -0.33))])
@pytest.mark.parametrize("half", [False, True])
def test_orthorhombic_and_triclinic_match_brute_force(abi, handle, seed, L, tilt, half):
    n, r = 2500, 1.6
    pos, h = random_box_system(seed, n, L, tilt)
    assert r <= face_distances(h).min() / 2
    types = np.zeros(n, dtype=np.int32)
    want = stable_yardstick(lambda rr: brute_nlist(pos, h, rr, half=half), r)
    assert len(want[2]) > 5 * n / (2 if half else 1)
    box = abi.Box.make(list(L), xy=tilt[0], xz=tilt[1], yz=tilt[2])
    assert_same(handle.build(util.pack_postype(pos, types, np.float64), n, box, r, half=half), want)
    assert min(handle.cells()) >= 3


# ---- 3. small boxes --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,mult,tilt", [(11, (2.05, 2.5, 2.95), (0.0, 0.0, 0.0)), (12, (2.2, 5.3, 7.3), (0.0, 0.0, 0.0)),
                                            (13, (6.1, 2.01, 4.2), (0.0, 0.0, 0.0)), (14, (2.6, 2.7, 6.5), (0.3, -0.2, 0.1)),
                                            (15, (3.4, 3.1, 2.4), (-0.25, 0.35, 0.3))])
def test_small_boxes_one_or_two_cells(abi, handle, seed, mult, tilt):
    """face distances between 2 and 3 r_list give 2 cells along that direction: the stencil must not visit a cell twice"""
    r = 1.0
    h0 = lattice((1.0, 1.0, 1.0), *tilt)
    L = tuple(m * r / d for m, d in zip(mult, face_distances(h0)))             # d_k = mult_k * r_list (tilt included)
    n = 1500
    pos, h = random_box_system(seed, n, L, tilt)
    assert np.allclose(face_distances(h), np.array(mult) * r)
    want = stable_yardstick(lambda rr: brute_nlist(pos, h, rr), r)
    box = abi.Box.make(list(L), xy=tilt[0], xz=tilt[1], yz=tilt[2])
    pt = util.pack_postype(pos, np.zeros(n, dtype=np.int32), np.float64)
    assert_same(handle.build(pt, n, box, r), want)
    assert handle.cells() == tuple(int(np.floor(m + 1e-12)) for m in mult)
    assert 2 in handle.cells()
    want_half = brute_nlist(pos, h, r, half=True)
    assert_same(handle.build(pt, n, box, r, half=True), want_half)
    # r_list just above d_k / 2 is refused
    dmin = face_distances(h).min()
    rc, _ = handle.build_rc(pt, n, box, 0.5 * dmin * (1 + 1e-9))
    assert rc == -1


def test_non_periodic_direction_one_cell(abi, handle):
    """periodic[k] == 0: no wrap, no image; a slab thinner than 2 r_list has one cell along that direction"""
    r = 1.0
    L = (7.3, 1.6, 6.2)
    n = 1200
    pos, h = random_box_system(21, n, L)
    want = stable_yardstick(lambda rr: brute_nlist(pos, h, rr, periodic=(1, 0, 0)), r)
    with_wrap = brute_nlist(pos, h, r, periodic=(1, 0, 1))
    assert len(with_wrap[2]) > len(want[2])                                   # the case does tell the two apart
    box = abi.Box.make(list(L))
    box.periodic[:] = [1, 0, 0]
    assert_same(handle.build(util.pack_postype(pos, np.zeros(n, dtype=np.int32), np.float64), n, box, r), want)
    assert handle.cells() == (7, 1, 6)


# ---- 4. ghosts ---------------------------------------------------------------------------------------------------------------------------

def test_ghosts_of_a_z_slab_shard(abi, handle):
    """a shard as bench.py builds it (owner by z, ghost layers of width r_list): the rows of the local particles are the rows of
    the whole-system list, mapped to shard indices"""
    pos, Lc = util.fcc_lattice(12)
    pos = pos + np.random.default_rng(778).normal(0, 0.05, pos.shape)
    pos = np.mod(pos + Lc / 2, Lc) - Lc / 2
    r_list, world, rank = 1.4, 3, 1
    whole = stable_yardstick(lambda r: util.build_nlist(pos, Lc, r), r_list)
    z = pos[:, 2]
    owner = np.minimum((np.mod(z + Lc / 2, Lc) / Lc * world).astype(int), world - 1)
    mine = np.where(owner == rank)[0]
    lo_z, hi_z = -Lc / 2 + rank * Lc / world, -Lc / 2 + (rank + 1) * Lc / world

    def zdist(u, v):
        d = np.abs(u - v)
        return np.minimum(d, Lc - d)

    ghosts = np.where((owner != rank) & ((zdist(z, lo_z) <= r_list) | (zdist(z, hi_z) <= r_list)))[0]
    assert len(ghosts) > 100
    shard = np.concatenate([mine, ghosts])
    to_shard = np.full(len(pos), -1, dtype=np.int64)
    to_shard[shard] = np.arange(len(shard))
    head, nn, nl = whole
    i = np.repeat(np.arange(len(nn)), nn)
    sel = owner[i] == rank
    si, sj = to_shard[i[sel]], to_shard[nl[sel]]
    assert (sj >= 0).all()                                                    # every partner of a local is local or a ghost
    order = np.lexsort((sj, si))
    want = _rows_to_lists(si[order], sj[order], len(mine))
    pt = util.pack_postype(pos[shard], np.zeros(len(shard), dtype=np.int32), np.float64)
    box = abi.Box.make(Lc)
    got = handle.build(pt, len(mine), box, r_list)
    assert_same(got, want)
    assert got[2].max() >= len(mine)                                          # entries do index ghosts
    rc, _ = handle.build_rc(pt, len(mine), box, r_list, half=True)
    assert rc == -2                                                           # MTD_ERR_UNSUPPORTED


# ---- 5. type filter ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_type_filter_on_a_mixture(abi, handle, dtype):
    pos, L = util.fcc_lattice(9)
    rng = np.random.default_rng(31)
    pos = (pos + rng.normal(0, 0.05, pos.shape)).astype(dtype)
    n = len(pos)
    types = (rng.random(n) < 0.5).astype(np.int32)
    assert 0.4 < types.mean() < 0.6
    allp = stable_yardstick(lambda r: util.build_nlist(pos.astype(np.float64), L, r), 1.5)
    pt = util.pack_postype(pos, types, dtype)
    box = abi.Box.make(L)
    for t in (0, 1):
        assert_same(handle.build(pt, n, box, 1.5, type=t), filter_type(allp, types, t))
    assert_same(handle.build(pt, n, box, 1.5, type=-1), allp)
    empty = handle.build(pt, n, box, 1.5, type=5)                             # nobody has that type
    assert len(empty[2]) == 0 and not empty[1].any()


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------------

def test_bitwise_deterministic_across_handle_states(abi):
    pos, L = util.fcc_lattice(16)
    pos = pos + np.random.default_rng(41).normal(0, 0.05, pos.shape)
    n = len(pos)
    pt = util.pack_postype(pos, np.zeros(n, dtype=np.int32), np.float64)
    box = abi.Box.make(L)
    fresh, used = Handle(abi), Handle(abi)
    try:
        other, h_other = random_box_system(42, 3000, (9.0, 14.0, 11.0), (0.2, 0.1, -0.3))
        used.build(util.pack_postype(other, np.zeros(3000, dtype=np.int32), np.float64), 3000,
                   abi.Box.make([9.0, 14.0, 11.0], xy=0.2, xz=0.1, yz=-0.3), 1.7, half=True)
        a = fresh.build(pt, n, box, 1.4)
        b = used.build(pt, n, box, 1.4)
        c = fresh.build(pt, n, box, 1.4)                                       # and the same handle twice
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)               # unsorted: bit-identical
        assert len(a[2]) > 10 * n
    finally:
        fresh.close()
        used.close()


# ---- 7. degenerate sizes ---------------------------------------------------------------------------------------------------------------

def test_empty_single_and_dilute(abi, handle):
    box = abi.Box.make(10.0)
    empty = np.zeros((0, 4), dtype=np.float64)
    head, nn, nl = handle.build(empty, 0, box, 1.0)
    assert len(head) == 0 and len(nn) == 0 and len(nl) == 0
    assert handle.check(empty, box, 0.4) == 0
    one = util.pack_postype(np.array([[0.3, -4.9, 4.99]]), np.zeros(1, dtype=np.int32), np.float64)
    head, nn, nl = handle.build(one, 1, box, 1.0)
    assert list(head) == [0] and list(nn) == [0] and len(nl) == 0
    # a gas so dilute that most rows are empty, in a box far larger than r_list
    n, L = 3000, 400.0
    pos, h = random_box_system(51, n, L)
    want = stable_yardstick(lambda r: brute_nlist(pos, h, r), 6.0)
    assert (want[1] == 0).mean() > 0.9 and len(want[2]) > 0
    big = abi.Box.make(L)
    assert_same(handle.build(util.pack_postype(pos, np.zeros(n, dtype=np.int32), np.float64), n, big, 6.0), want)


# ---- 8. displacement check -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_displacement_check(abi, handle, dtype):
    L, r_buff = 12.0, 0.4
    pos, h = random_box_system(61, 2000, L)
    pos = pos.astype(dtype).astype(np.float64)
    n = len(pos)
    types = np.zeros(n, dtype=np.int32)
    box = abi.Box.make(L)
    pack = lambda p: util.pack_postype(p.astype(dtype), types, dtype)
    assert handle.check(pack(pos), box, r_buff) == 1                          # nothing built yet
    handle.build(pack(pos), n, box, 1.4)
    assert handle.check(pack(pos), box, r_buff) == 0
    u = np.array([1.0, -2.0, 2.0]) / 3.0
    for frac, want in ((0.49, 0), (0.51, 1), (0.49, 0)):
        moved = pos.copy()
        moved[777] += frac * r_buff * u
        assert handle.check(pack(moved), box, r_buff) == want
    # across a periodic boundary: a particle close to the +x face moves out and is wrapped back in — it has not moved by L
    k = int(np.argmax(pos[:, 0]))
    gap = L / 2 - pos[k, 0]
    assert 0 <= gap < 0.05
    for frac, want in ((0.49, 0), (0.51, 1)):
        moved = pos.copy()
        moved[k, 0] += frac * r_buff
        assert moved[k, 0] > L / 2
        moved[k, 0] -= L
        assert handle.check(pack(moved), box, r_buff) == want
    # a changed box, a changed dtype: rebuild, whatever the particles did
    assert handle.check(pack(pos), abi.Box.make(L * (1 + 1e-12)), r_buff) == 1
    assert handle.check(pack(pos), abi.Box.make(L, xy=1e-9), r_buff) == 1
    other = np.float32 if dtype == np.float64 else np.float64
    assert handle.check(util.pack_postype(pos.astype(other), types, other), box, r_buff) == 1
    assert handle.check(pack(pos), box, r_buff) == 0


# ---- 9. / 10. through the API --------------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


QL_REF = [0, 0, 0, 0, 1, 0, 1]


def _api_system(seed=12):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(seed).normal(0, 0.05, pos.shape)
    return pos, L, np.zeros(len(pos), dtype=np.int32)


def _api_run(api, pos, types, L, val, device, half=False):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5, device=device)
    if not device:
        nl.update()
    st = cv.steinhardt(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_REF, nlist=nl, type="A", sigma=0.02 * val)
    if half:
        nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    st.set_grid(0.55 * val, 1.3 * val, 64)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    return meta, nl, st, st.cpp_force.getCurrentValue(t), np.array(meta.cpp_integrator.getBiasFactors()), st.cpp_force.getForceArray()


def test_through_api_device_build_and_rebuild_rule(api, ref):
    context, cv, integrate = api
    pos, L, types = _api_system()
    N = len(pos)
    rbox = ref.Box.make(L)
    r_buff = 0.4
    r_list = 1.5 + r_buff
    lists0 = stable_yardstick(lambda r: util.build_nlist(pos, L, r), r_list)
    val = ref.ql_compute_cv(util.oracle_postype(pos, types), rbox, *lists0, 1.4, 1.2, 6, 0, QL_REF)[0]
    _, _, _, cv_host, bias_host, F_host = _api_run(api, pos, types, L, val, device=False)
    context.current = None
    meta, nl, st, cv_dev, bias_dev, F_dev = _api_run(api, pos, types, L, val, device=True)     # no update() before run
    # the tolerances of test_steinhardt_through_api (the row order differs: fp64 sums may differ in the last bits)
    assert cv_dev == pytest.approx(val, rel=1e-10) and cv_dev == pytest.approx(cv_host, rel=1e-10)
    assert np.allclose(bias_dev, bias_host, rtol=1e-7)
    assert np.abs(F_dev[:, :3] - F_host[:, :3]).max() <= 1e-7 * np.abs(F_host[:, :3]).max()
    assert nl.cpp_nlist.getNumRebuilds() == 1                                 # static particles: built once in two steps
    assert_same(nl.cpp_nlist.getLists(), lists0)
    assert nl.cpp_nlist.isSymmetricFull()

    # a random walk of all particles; the rebuild rule replayed in numpy
    h = lattice(L)
    rng = np.random.default_rng(5)
    step = 0.03
    p, last, expected = pos.copy(), pos.copy(), 0
    for k in range(20):
        p = p + rng.normal(0, step, p.shape)
        dmax = np.sqrt((min_image(p - last, h) ** 2).sum(-1).max())
        assert abs(dmax - r_buff / 2) > 1e-9
        if dmax > r_buff / 2:
            expected += 1
            last = p.copy()
        context.set_positions(p, types)
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        fresh = stable_yardstick(lambda r: util.build_nlist(p, L, r), r_list)
        want = ref.ql_compute_cv(util.oracle_postype(p, types), rbox, *fresh, 1.4, 1.2, 6, 0, QL_REF)[0]
        print("step %2d: max displacement since the last build %.4f, rebuilds %d, cv %.12g (oracle %.12g)"
              % (k, dmax, nl.cpp_nlist.getNumRebuilds(), st.cpp_force.getCurrentValue(t), want))
        assert st.cpp_force.getCurrentValue(t) == pytest.approx(want, rel=1e-10)
        assert nl.cpp_nlist.getNumRebuilds() == expected + 1
    assert 2 <= expected <= 10
    # update() forces a rebuild and hands the arrays back
    before = nl.cpp_nlist.getNumRebuilds()
    assert_same(nl.update(), fresh)
    assert nl.cpp_nlist.getNumRebuilds() == before + 1
    # set_lists keeps working and switches the device build off again
    nl.set_lists(*fresh)
    assert not nl.cpp_nlist.isDeviceBuild()
    context.run(1)
    assert nl.cpp_nlist.getNumRebuilds() == before + 1


def test_through_api_half_list_built_on_device(api, ref):
    """a half list built on the device goes through SteinhardtQl's symmetrisation: the half-list value, which for even degrees
    is the full-list value of the test above"""
    pos, L, types = _api_system()
    rbox = ref.Box.make(L)
    pt = util.oracle_postype(pos, types)
    full = stable_yardstick(lambda r: util.build_nlist(pos, L, r), 1.9)
    half = util.build_nlist(pos, L, 1.9, half=True)
    val_full = ref.ql_compute_cv(pt, rbox, *full, 1.4, 1.2, 6, 0, QL_REF)[0]
    val_half, Qlm, _ = ref.ql_compute_cv(pt, rbox, *half, 1.4, 1.2, 6, 0, QL_REF, half=True)
    meta, nl, st, cv_dev, bias, F = _api_run(api, pos, types, L, val_full, device=True, half=True)
    assert cv_dev == pytest.approx(val_half, rel=1e-10) and cv_dev == pytest.approx(val_full, rel=1e-10)
    assert_same(nl.cpp_nlist.getLists(), half)
    assert nl.cpp_nlist.getNumRebuilds() == 1 and not nl.cpp_nlist.isSymmetricFull()
    F_ref = ref.ql_compute_forces(pt, rbox, *half, 1.4, 1.2, 6, 0, QL_REF, Qlm, bias[0], half=True)
    assert np.abs(F[:, :3] - F_ref[:, :3]).max() <= 1e-7 * np.abs(F_ref[:, :3]).max()


def test_changed_box_rebuilds_between_checks(api):
    """check_period > 1: the box is compared on the host at EVERY compute(), so a box changed on a step without a displacement
    check is not used with the old list for a single step; without a change no such step rebuilds"""
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types = _api_system(seed=14)
    N = len(pos)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5, r_buff=0.4, check_period=10, device=True)
    st = cv.steinhardt(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_REF, nlist=nl, type="A", sigma=1.0)
    st.set_grid(0.0, 100.0, 64)
    context.run(3)
    assert nl.cpp_nlist.getNumRebuilds() == 1
    assert_same(nl.cpp_nlist.getLists(), stable_yardstick(lambda r: brute_nlist(pos, lattice(L), r), 1.9))
    # a triclinic box of another size, set on a step that is no multiple of the period
    newL, tilt = (L * 1.07, L * 0.96, L * 1.02), (0.15, -0.1, 0.2)
    pdata = context.current.system_definition.getParticleData()
    pdata.setGlobalBox(_metadynamics.BoxDim(*newL, *tilt))
    t = context.current.system.getCurrentTimeStep()
    assert t % 10 != 0 and (t + 1) % 10 != 0
    context.run(1)
    assert nl.cpp_nlist.getNumRebuilds() == 2
    h = lattice(newL, *tilt)
    assert 1.9 <= face_distances(h).min() / 2
    want = stable_yardstick(lambda r: brute_nlist(pos, h, r), 1.9)
    assert any(not np.array_equal(a, b) for a, b in zip(want, brute_nlist(pos, lattice(L), 1.9)))     # the boxes do differ in their lists
    assert_same(nl.cpp_nlist.getLists(), want)
    context.run(3)                                                            # static again: nothing more
    assert nl.cpp_nlist.getNumRebuilds() == 2
