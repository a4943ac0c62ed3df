"""GPU parity: the local Steinhardt variable (mtd_ql_local_*, cv.steinhardt_local) against the fp64 numpy restatement of its
definition (tests/ql_local_ref.py, itself checked on the CPU in tests/test_ql_local_ref.py).  Tolerances are those
tests/test_gpu_steinhardt.py uses for the same arithmetic: c_i and n_i to 1e-11 of their largest value, s to 1e-10 relative, forces to
1e-9 of max|F| with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store)."""
import ctypes as C

import numpy as np
import pytest

import ql_local_ref
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def run_gpu(abi, pos, types, L, nl, rcut, ron, lmax, type_id, Ql_ref, dtype, n_global=None, bias=0.9, tilt=None, bias_on_device=True):
    """returns dict(s, c, n, F, partials)"""
    lib = abi.load()
    N = len(pos)
    n_global = N if n_global is None else n_global
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    d_pos = torch.from_numpy(util.pack_postype(pos.astype(dtype), types, dtype)).cuda()
    d_head, d_nn, d_nl = (torch.from_numpy(np.asarray(x).astype(np.int32)).cuda() for x in nl)
    scratch = torch.zeros(lib.mtd_ql_local_scratch_doubles(N, lmax), dtype=torch.float64, device="cuda")
    p_part, p_c, p_n = C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_part = C.c_uint()
    abi.check(lib.mtd_ql_local_accumulate(N, abi.ptr(d_pos), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), rcut, ron, lmax,
                                          type_id, util.dbl_array(Ql_ref), n_global, abi.ptr(scratch), C.byref(p_part), C.byref(n_part),
                                          C.byref(p_c), C.byref(p_n), None))
    force = torch.full((N, 4), 3.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    d_bias = torch.tensor([bias], dtype=torch.float64, device="cuda")
    abi.check(lib.mtd_ql_local_forces(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), rcut, ron,
                                      lmax, type_id, util.dbl_array(Ql_ref), n_global, abi.ptr(scratch),
                                      abi.ptr(d_bias) if bias_on_device else None, 0.0 if bias_on_device else bias, None))
    torch.cuda.synchronize()
    s = scratch.cpu().numpy()
    off = lambda p: (p.value - scratch.data_ptr()) // 8
    partials = s[off(p_part):off(p_part) + n_part.value].copy()
    return dict(s=partials.sum() / n_global, c=s[off(p_c):off(p_c) + N].copy(), n=s[off(p_n):off(p_n) + N].copy(),
                F=force.cpu().numpy().astype(np.float64), partials=partials)


def noisy_fcc(n, sigma=0.05, seed=777):
    pos, L = util.fcc_lattice(n)
    rng = np.random.default_rng(seed)
    return pos + rng.normal(0, sigma, pos.shape), L


def compare(g, r, bias, dtype, types=None, type_id=0):
    print("c_i: max |d| %.3e of %.3e; n_i: max |d| %.3e of %.3e; s %.15g vs %.15g"
          % (np.abs(g["c"] - r["c"]).max(), np.abs(r["c"]).max(), np.abs(g["n"] - r["n"]).max(), np.abs(r["n"]).max(), g["s"], r["s"]))
    F_ref = -bias * r["grad"]
    fs = np.abs(F_ref).max()
    err = np.abs(g["F"][:, :3] - F_ref).max()
    print("forces: max |d| %.3e of max |F| %.3e (%.3e relative)" % (err, fs, err / fs if fs else 0.0))
    assert np.isfinite(g["F"]).all() and np.isfinite(g["c"]).all() and np.isfinite(g["n"]).all()
    assert np.abs(g["c"] - r["c"]).max() <= 1e-11 * np.abs(r["c"]).max()
    assert np.abs(g["n"] - r["n"]).max() <= 1e-11 * np.abs(r["n"]).max()
    assert g["s"] == pytest.approx(r["s"], rel=1e-10)
    assert fs > 0
    assert err <= (1e-9 if dtype == np.float64 else 2e-7) * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        other = types != type_id
        assert np.all(g["F"][other] == 0.0) and np.all(g["c"][other] == 0.0) and np.all(g["n"][other] == 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lmax,Ql_ref", [(6, [0, 0, 0, 0, 1, 0, 1]), (4, [0.2, 0, 1.0, 0.5, 1.0]), (2, [0.5, 0.3, 1.0]),
                                         (5, [0, 0.4, 0.2, 0.6, 1, 0.7]),                      # odd and even degrees mixed
                                         (12, [0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0.5, 0.3, 0.25])])
def test_ql_local_parity(abi, dtype, lmax, Ql_ref):
    pos, L = noisy_fcc(5)
    pos = pos.astype(dtype).astype(np.float64)                          # the snapshot is the rounded array
    N = len(pos)
    types = np.zeros(N, dtype=np.int32)
    rcut, ron = 1.4, 1.2
    nl = util.build_nlist(pos, L, rcut + 0.15)
    g = run_gpu(abi, pos, types, L, nl, rcut, ron, lmax, 0, Ql_ref, dtype)
    r = ql_local_ref.compute(pos, types, L, nl, rcut, ron, lmax, 0, Ql_ref)
    compare(g, r, 0.9, dtype)


def test_ql_local_two_types_and_n_global(abi):
    pos, L = noisy_fcc(4, seed=5)
    N = len(pos)
    types = (np.random.default_rng(1).random(N) < 0.3).astype(np.int32)
    nl = util.build_nlist(pos, L, 1.6)
    args = (1.45, 1.1, 6, 0, [0.5, 0, 0.25, 0, 1, 0, 1])
    g = run_gpu(abi, pos, types, L, nl, *args, np.float64, n_global=3 * N)
    r = ql_local_ref.compute(pos, types, L, nl, *args, n_global=3 * N)
    compare(g, r, 0.9, np.float64, types=types)
    # the other type as the chosen one
    g = run_gpu(abi, pos, types, L, nl, 1.45, 1.1, 6, 1, args[4], np.float64, n_global=3 * N)
    r = ql_local_ref.compute(pos, types, L, nl, 1.45, 1.1, 6, 1, args[4], n_global=3 * N)
    assert np.abs(g["c"] - r["c"]).max() <= 1e-11 * np.abs(r["c"]).max()
    assert g["s"] == pytest.approx(r["s"], rel=1e-10)
    assert np.all(g["F"][types == 0] == 0.0)


def brute_nlist(pos, h, r):
    """full list of a triclinic box (lattice vectors in the columns of h), O(N^2), images -1..1"""
    N = len(pos)
    shifts = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.float64) @ h.T
    rows = []
    for i in range(N):
        d = pos[i] - pos
        best = np.min(((d[:, None, :] + shifts[None, :, :]) ** 2).sum(-1), axis=1)
        j = np.nonzero((best <= r * r) & (np.arange(N) != i))[0]
        rows.append(j)
    nn = np.array([len(x) for x in rows], dtype=np.uint32)
    head = np.zeros(N, dtype=np.uint32)
    head[1:] = np.cumsum(nn)[:-1]
    return head, nn, np.concatenate(rows).astype(np.uint32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ql_local_triclinic_box(abi, dtype):
    """a sheared fcc crystal in the sheared box: HOOMD's minimum image with tilt factors"""
    pos, L = noisy_fcc(4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = (pos / L) @ h.T                                               # fractional coordinates carried into the tilted cell
    pos = pos.astype(dtype).astype(np.float64)
    N = len(pos)
    types = np.zeros(N, dtype=np.int32)
    nl = brute_nlist(pos, h, 1.6)
    args = (1.45, 1.15, 6, 0, [0, 0, 0.3, 0, 1, 0, 1])
    g = run_gpu(abi, pos, types, L, nl, *args, dtype, tilt=tilt)
    r = ql_local_ref.compute(pos, types, L, nl, *args, tilt=tilt)
    assert r["n"].min() > 3
    compare(g, r, 0.9, dtype)


def test_ql_local_buffered_and_shuffled_lists(abi):
    """a list with r_list = r_cut + 0.15 gives what the list cut at r_cut gives (entries beyond r_cut are skipped); rows shuffled:
    the same values to 1e-13 (sums follow the list order); two identical calls: identical bits"""
    pos, L = noisy_fcc(5, seed=9)
    N = len(pos)
    types = (np.random.default_rng(2).random(N) < 0.15).astype(np.int32)
    args = (1.4, 1.2, 6, 0, [0, 0, 0.3, 0, 1, 0, 1])
    tight = util.build_nlist(pos, L, 1.4)
    buffered = util.build_nlist(pos, L, 1.55)
    assert len(buffered[2]) > len(tight[2])
    a = run_gpu(abi, pos, types, L, tight, *args, np.float64)
    b = run_gpu(abi, pos, types, L, buffered, *args, np.float64)
    b2 = run_gpu(abi, pos, types, L, buffered, *args, np.float64)
    r = ql_local_ref.compute(pos, types, L, buffered, *args)
    compare(b, r, 0.9, np.float64, types=types)
    for key in ("c", "n", "F", "partials"):
        assert np.array_equal(b[key], b2[key]), key                    # no atomics, fixed orders: the same bits
    fs = np.abs(a["F"]).max()
    assert np.abs(a["c"] - b["c"]).max() <= 1e-13 * np.abs(a["c"]).max() and np.abs(a["F"] - b["F"]).max() <= 1e-13 * fs
    head, nn, lst = [np.array(x).copy() for x in buffered]
    rng = np.random.default_rng(2)
    for i in range(N):
        lst[head[i]:head[i] + nn[i]] = rng.permutation(lst[head[i]:head[i] + nn[i]])
    c = run_gpu(abi, pos, types, L, (head, nn, lst), *args, np.float64)
    assert np.abs(c["c"] - b["c"]).max() <= 1e-13 * np.abs(b["c"]).max()
    assert np.abs(c["n"] - b["n"]).max() <= 1e-13 * np.abs(b["n"]).max()
    assert c["s"] == pytest.approx(b["s"], rel=1e-13)
    assert np.abs(c["F"] - b["F"]).max() <= 1e-13 * fs


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ql_local_isolated_particle(abi, dtype):
    """one particle without a neighbour in range (n_i = 0): c_i = 0, force 0, no NaN anywhere"""
    pos, L = noisy_fcc(4, seed=4)
    L2 = L + 6.0                                                        # the crystal in a larger box, one particle far from it
    pos = np.vstack([pos, [[L2 / 2 - 0.5, L2 / 2 - 0.7, L2 / 2 - 0.9]]])
    pos = pos.astype(dtype).astype(np.float64)
    N = len(pos)
    types = np.zeros(N, dtype=np.int32)
    nl = util.build_nlist(pos, L2, 1.55)
    assert nl[1][-1] == 0
    args = (1.4, 1.2, 6, 0, [0.5, 0, 0, 0, 1, 0, 1])
    g = run_gpu(abi, pos, types, L2, nl, *args, dtype)
    r = ql_local_ref.compute(pos, types, L2, nl, *args)
    compare(g, r, 0.9, dtype)
    assert g["c"][-1] == 0.0 and g["n"][-1] == 0.0 and np.all(g["F"][-1] == 0.0)


def test_ql_local_bias_from_device_and_host(abi):
    pos, L = noisy_fcc(4, seed=6)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.55)
    args = (1.4, 1.2, 6, 0, [0, 0, 0, 0, 1, 0, 1])
    dev = run_gpu(abi, pos, types, L, nl, *args, np.float64, bias=-1.7, bias_on_device=True)
    host = run_gpu(abi, pos, types, L, nl, *args, np.float64, bias=-1.7, bias_on_device=False)
    assert np.array_equal(dev["F"], host["F"])
    r = ql_local_ref.compute(pos, types, L, nl, *args)
    compare(dev, r, -1.7, np.float64)
    zero = run_gpu(abi, pos, types, L, nl, *args, np.float64, bias=0.0, bias_on_device=False)
    assert np.all(zero["F"] == 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ql_local_perfect_lattice(abi, dtype):
    """perfect fcc: n_i = 12, q_4^2 = 7/192, q_6^2 = 169/512 for every particle, whatever the size of the box; no net force"""
    for n in (3, 6):
        pos, L = util.fcc_lattice(n)
        types = np.zeros(len(pos), dtype=np.int32)
        nl = util.build_nlist(pos, L, 1.4)
        tol = 1e-11 if dtype == np.float64 else 2e-6                   # fp32 positions: the lattice itself is rounded
        for ql_ref, want in (([0, 0, 0, 0, 1, 0, 0], 7.0 / 192.0), ([0, 0, 0, 0, 0, 0, 1], 169.0 / 512.0)):
            g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, ql_ref, dtype)
            assert np.abs(g["n"] - 12.0).max() <= tol * 12
            assert np.abs(g["c"] - want).max() <= tol
            assert g["s"] == pytest.approx(want, abs=tol)
            assert np.abs(g["F"]).max() <= (1e-9 if dtype == np.float64 else 1e-4)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ql_local_config5_size(abi, dtype):
    """256 000 particles (40^3 fcc cells), lmax 6, r_cut 1.4, r_on 1.2, Ql_ref [0,0,0,0,1,0,1]: s and every c_i against the
    restatement, forces on the first and on the last 30 000 rows (a block's first and last chunks), stated tolerance 1e-5 of max|F|"""
    pos, L = noisy_fcc(40)
    N = len(pos)
    assert N == 256000
    pos = pos.astype(dtype).astype(np.float64)
    types = np.zeros(N, dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.4)
    Ql_ref = [0, 0, 0, 0, 1, 0, 1]
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, Ql_ref, dtype)
    r = ql_local_ref.compute(pos, types, L, nl, 1.4, 1.2, 6, 0, Ql_ref)
    print("s %.15g vs %.15g; c_i max |d| %.3e" % (g["s"], r["s"], np.abs(g["c"] - r["c"]).max()))
    assert g["s"] == pytest.approx(r["s"], rel=1e-10)
    assert np.abs(g["c"] - r["c"]).max() <= 1e-11 * np.abs(r["c"]).max()
    assert np.abs(g["n"] - r["n"]).max() <= 1e-11 * np.abs(r["n"]).max()
    n_sl = 30000
    F_ref = -0.9 * r["grad"][:n_sl]
    fs = np.abs(F_ref).max()
    assert fs > 0
    err = np.abs(g["F"][:n_sl, :3] - F_ref).max() / fs
    print("forces on the first %d rows: %.3e of max |F|" % (n_sl, err))
    assert err <= 1e-5, err
    # the first rows all lie in a block's first chunk (i < 1024 * 64): the last ones are written on a later trip of the chunk loop
    assert N - n_sl >= 1024 * 64 and len(r["grad"]) == N
    F_last = -0.9 * r["grad"][N - n_sl:]
    fs_last = np.abs(F_last).max()
    assert fs_last > 0
    err = np.abs(g["F"][N - n_sl:, :3] - F_last).max() / fs_last
    print("forces on the last %d rows: %.3e of max |F|" % (n_sl, err))
    assert err <= 1e-5, err
    assert np.isfinite(g["F"]).all() and np.all(g["F"][:, 3] == 0.0)
    # translation invariance of s: the forces add up to zero
    assert np.abs(g["F"][:, :3].sum(axis=0)).max() <= 1e-4 * fs * np.sqrt(N)


# ---- through the Python API -------------------------------------------------------------------------------------------------

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


def _oracle_bias(ref, kw, values, steps):
    """the oracle's grid driven with the given CV values: prepRun(0) + `steps` updates; returns the list of bias factors per call"""
    g = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    return [g.update_bias(t, values) for t in range(steps + 1)]


def test_steinhardt_local_alone_on_a_grid(api, ref, abi):
    """cv.steinhardt_local on a 512-point well-tempered grid, 6 steps, stride 1: the value the engine used, the bias factor and the
    force array against the oracle's grid driven with the restatement's value; get_local() equals the ABI's c_i"""
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    r = ql_local_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, QL_REF)
    val = r["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_REF, nlist=nl, type="A", sigma=0.02 * val)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    context.run(6)
    t = context.current.system.getCurrentTimeStep()
    assert t == 6
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-10)
    assert st.cpp_force.getLogValue("cv_steinhardt_local", t) == pytest.approx(val, rel=1e-10)
    assert "cv_steinhardt_local" in st.cpp_force.getProvidedLogQuantities()
    cvg = meta.cpp_integrator.getCurrentValues()
    assert cvg[0] == pytest.approx(val, rel=1e-10)                       # what the engine took from the block sums
    b = _oracle_bias(ref, dict(sigma=[0.02 * val], cv_min=[0.55 * val], cv_max=[1.3 * val], num_points=[512]), [val], 6)[-1]
    assert abs(b[0]) > 0
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    F = st.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert np.all(F[:, 3] == 0.0)
    g = run_gpu(abi, pos, types, L, lists, 1.4, 1.2, 6, 0, QL_REF, np.float64)
    assert np.array_equal(st.get_local(), g["c"])
    assert np.array_equal(st.get_coordination(), g["n"])
    with pytest.raises(RuntimeError):
        cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=[1, 2, 3], nlist=nl, type="A")
    with pytest.raises(RuntimeError):
        cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_REF, nlist=nl, type="Z")
    with pytest.raises(RuntimeError):
        cv.steinhardt_local(r_cut=1.2, r_on=1.4, lmax=6, Ql_ref=QL_REF, nlist=nl, type="A")


def test_steinhardt_local_with_lamellar_on_a_2d_grid(api, ref):
    """together with a cv.lamellar on a 2-d grid, 6 steps: both values, both bias factors and both force arrays against the oracle"""
    context, cv, integrate = api
    pos, L, types = _api_system(seed=13)
    types = (np.random.default_rng(4).random(len(pos)) < 0.5).astype(np.int32)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    r = ql_local_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, QL_REF)
    val = r["s"]
    rbox = ref.Box.make(L)
    opt = util.oracle_postype(pos, types)
    vec = [(0, 0, 2)]
    s_lam = ref.lamellar_cv(vec, opt, util.MODE_AB, rbox)
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_REF, nlist=nl, type="A", sigma=0.02 * val)
    st.set_grid(0.55 * val, 1.3 * val, 64)
    lam = cv.lamellar(sigma=0.05, mode=dict(A=1.0, B=-1.0), lattice_vectors=vec)
    lam.set_grid(cv_min=-1.0, cv_max=1.0, num_points=64)
    context.run(6)
    cvg = meta.cpp_integrator.getCurrentValues()
    assert cvg[0] == pytest.approx(val, rel=1e-10)
    assert cvg[1] == pytest.approx(s_lam, rel=1e-6, abs=1e-9)
    kw = dict(sigma=[0.02 * val, 0.05], cv_min=[0.55 * val, -1.0], cv_max=[1.3 * val, 1.0], num_points=[64, 64])
    b = _oracle_bias(ref, kw, [val, cvg[1]], 6)[-1]                      # the restatement's value; the lamellar value as the engine had it
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    F = st.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert np.abs(F_ref).max() > 0
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert np.all(F[types == 1] == 0.0)
    Fl = lam.cpp_force.getForceArray()
    Fl_ref = ref.lamellar_forces(vec, opt, util.MODE_AB, rbox, b[1])
    assert np.abs(Fl[:, :3] - Fl_ref[:, :3]).max() <= 1e-5 * np.abs(Fl_ref[:, :3]).max()


def test_steinhardt_local_device_list_follows_the_particles(api, ref):
    """cv.nlist_cell(device=True): particles displaced between runs by more than r_buff / 2 — the list rebuilds and the value follows"""
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5, r_buff=0.4, device=True)
    val0 = ql_local_ref.compute(pos, types, L, util.build_nlist(pos, L, 1.5), 1.4, 1.2, 6, 0, QL_REF, gradient=False)["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_REF, nlist=nl, type="A", sigma=0.02 * val0)
    st.set_grid(0.05 * val0, 1.3 * val0, 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(val0, rel=1e-10)
    assert nl.cpp_nlist.getNumRebuilds() == 1
    rng = np.random.default_rng(5)
    p = pos.copy()
    values = [val0]
    for k in range(3):
        p = p + rng.normal(0, 0.12, p.shape)                                    # far more than r_buff / 2 = 0.2 for some particle
        assert np.sqrt(((p - pos) ** 2).sum(-1)).max() > 0.2
        context.set_positions(p, types)
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        r = ql_local_ref.compute(p, types, L, util.build_nlist(p, L, 1.5), 1.4, 1.2, 6, 0, QL_REF)
        values.append(r["s"])
        assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)
        assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["s"], rel=1e-10)
        assert nl.cpp_nlist.getNumRebuilds() == 2 + k
        b = meta.cpp_integrator.getBiasFactors()[0]
        F = st.cpp_force.getForceArray()
        F_ref = -b * r["grad"]
        assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert abs(values[-1] - values[0]) > 1e-3 * values[0]                         # the value did move


def test_steinhardt_local_harmonic_umbrella_adds_to_the_bias_factor(api, ref):
    context, cv, integrate = api
    pos, L, types = _api_system(seed=15)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    r = ql_local_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, QL_REF)
    val = r["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_REF, nlist=nl, type="A", sigma=0.02 * val)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    kappa, cv0 = 35.0, 0.8 * val
    st.set_params(umbrella="harmonic", kappa=kappa, cv0=cv0)
    context.run(3)
    t = context.current.system.getCurrentTimeStep()
    b = _oracle_bias(ref, dict(sigma=[0.02 * val], cv_min=[0.55 * val], cv_max=[1.3 * val], num_points=[512]), [val], 3)[-1]
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    total = b[0] + kappa * (val - cv0)                                           # CollectiveVariable.cc:22-66
    F = st.cpp_force.getForceArray()
    F_ref = -total * r["grad"]
    assert abs(kappa * (val - cv0)) > 0.1 * abs(total)
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert st.cpp_force.getUmbrellaPotential(t) == pytest.approx(0.5 * kappa * (val - cv0) ** 2, rel=1e-9)


def test_steinhardt_local_refuses_a_half_list(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_REF, nlist=nl, type="A", sigma=1.0)
    st.set_grid(0.0, 1.0, 64)
    nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    nl.set_lists(*util.build_nlist(pos, L, 1.5, half=True))
    with pytest.raises(RuntimeError, match="full neighbour list"):
        context.run(1)
