"""GPU parity: the environment similarity (mtd_es_*, csrc/env_similarity.hip) through the C ABI against the fp64 numpy restatement of its
definition (tests/env_similarity_ref.py, itself checked on the CPU in tests/test_env_similarity_ref.py).

Tolerances, those of tests/test_gpu_pair_entropy.py for the same arithmetic: k^e_i, k_i and v_i to 1e-10 of their maximum, s to 1e-9
relative, forces to 1e-9 of max|F| with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store), the per-particle virial likewise of
max|virial_i| and its six sums of the largest sum.  Every figure is printed before it is asserted.

test_chunk_loop (simple cubic, N = 274 625 and 74 088: 4292 and 1158 chunks of 64 on the 1024 blocks the launches are capped at),
measured on an MI355X: fp64 arrays k^e, k, v <= 6e-15 of their maxima, s <= 1.5e-16 relative, forces <= 6.3e-15 of max|F|, per-particle
virial <= 1.7e-14, its sums <= 4.1e-15; fp32 arrays forces 3.5e-8, per-particle virial 3.7e-8, sums 2.4e-10.  The forces add up to
<= 2e-17 of sum|F| at 274 625 particles (the restatement's own gather: 5e-19 .. 2e-18), five orders below the 1e-12 that compare() asks:
that bound does not depend on the small shapes it was set at.  No bound had to move.
"""
import ctypes as C

import numpy as np
import pytest

import env_similarity_ref as es
import stream_gate
import util
from pair_entropy_ref import brute_nlist

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
FCC = es.templates("fcc", np.sqrt(2.0))
SIGMA_ENV, R_ON, R_CUT = 0.12, 1.3, 1.5
SWITCH = (0.5, 6)


def rot_z(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


TWO = [FCC, FCC @ rot_z(5.0).T]
# name: (templates, lambda, switch, all environments closed)
VARIANTS = {"fcc": (FCC, 100.0, None, True), "two": (TWO, 20.0, None, True), "two_switch": (TWO, 20.0, SWITCH, True),
            "half_fcc": (FCC[:6], 100.0, None, False)}


def run_gpu(abi, pos, types, L, nl, templates, dtype, sigma_env=SIGMA_ENV, r_on=R_ON, r_cut=R_CUT, type_id=0, lam=100.0, sw=None, bias=0.9,
            tilt=None, bias_on_device=True, virial=False, n_rows=None, n_ghost=0, expect=0, gate=None):
    """returns dict(s, sum_v, ke, k, v, F, virial, n_part); n_rows: the first n_rows particles are the central ones, the others ghosts;
    gate: the stream the calls run on and how their inputs arrive (tests/stream_gate.py; None: the NULL stream)"""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    envs = es.as_environments(templates)
    E = len(envs)
    N = len(nl[0]) if n_rows is None else n_rows
    n_global = len(pos)
    box = abi.Box.make(L, **(tilt or {}))
    par = abi.EsParams.make(envs, sigma_env, r_on, r_cut, lam, sw)
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    if len(nl[2]) == 0:
        d_nl = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    scratch = torch.zeros(lib.mtd_es_scratch_doubles(N), dtype=torch.float64, device="cuda")
    force = torch.full((N, 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda") if virial else None
    p_part, p_k, p_ke, p_v = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_part = C.c_uint()
    lists = (abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl))
    stream = gate.arm()
    rc = lib.mtd_es_accumulate(N, n_ghost, abi.ptr(d_pos), dt, C.byref(box), *lists, type_id, C.byref(par), n_global, abi.ptr(scratch),
                               C.byref(p_part), C.byref(n_part), C.byref(p_k), C.byref(p_ke), C.byref(p_v), stream)
    rc2 = lib.mtd_es_forces(N, n_ghost, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *lists, type_id, C.byref(par), n_global, abi.ptr(scratch),
                            abi.ptr(d_bias) if bias_on_device else None, 0.0 if bias_on_device else bias, stream,
                            abi.ptr(vir) if virial else None, pitch if virial else 0)
    if expect:
        assert rc == expect and rc2 == expect
        return None
    abi.check(rc)
    abi.check(rc2)

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        assert 1 <= n_part.value <= 1024
        sum_v = float(s[off(p_part):off(p_part) + n_part.value].sum())
        ke = s[off(p_ke):off(p_ke) + 4 * N].reshape(N, 4)
        assert np.all(ke[:, E:] == 0.0)
        out = dict(sum_v=sum_v, s=sum_v / n_global, ke=ke[:, :E].copy(), k=s[off(p_k):off(p_k) + N].copy(), v=s[off(p_v):off(p_v) + N].copy(),
                   F=force.cpu().numpy().astype(np.float64), virial=None, n_part=n_part.value)
        if virial:
            v = vir.cpu().numpy().astype(np.float64)
            assert np.all(v[:, N:] == 7.0)                                  # [n_particles, pitch) is left alone
            out["virial"] = v[:, :N].T.copy()
        return out
    return gate.done(read)


def compare(g, r, bias, dtype, types=None, type_id=0, zero_sum=True):
    """prints every figure, then asserts; r: the restatement's result (its virial formed with the same bias)"""
    n = len(g["F"])
    err = {}
    for key in ("ke", "k", "v"):
        top = np.abs(r[key][:n]).max()
        err[key] = np.abs(g[key] - r[key][:n]).max() / top if top else np.abs(g[key]).max()
    err_s = abs(g["s"] - r["s"]) / abs(r["s"]) if r["s"] else abs(g["s"])
    F_ref = -bias * r["gather"][:n]
    fs = np.abs(F_ref).max()
    err_f = np.abs(g["F"][:, :3] - F_ref).max()
    print("k^e %.3e, k %.3e, v %.3e of their maxima; s %.15g vs %.15g (%.3e rel); forces: max |d| %.3e of max |F| %.3e (%.3e rel)"
          % (err["ke"], err["k"], err["v"], g["s"], r["s"], err_s, err_f, fs, err_f / fs if fs else 0.0))
    assert np.isfinite(g["F"]).all() and np.isfinite(g["ke"]).all() and np.isfinite(g["s"])
    assert max(err.values()) <= 1e-10
    assert err_s <= 1e-9
    tol = 1e-9 if dtype == np.float64 else 2e-7
    assert fs > 0
    assert err_f <= tol * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if zero_sum and dtype == np.float64:
        tot = np.abs(g["F"][:, :3].sum(axis=0)).max() / np.abs(g["F"][:, :3]).sum()
        print("sum of the forces: %.3e of sum |F|" % tot)
        assert tot <= 1e-12
    if types is not None:
        other = types[:n] != type_id
        assert np.all(g["F"][other] == 0.0) and np.all(g["ke"][other] == 0.0) and np.all(g["k"][other] == 0.0) and np.all(g["v"][other] == 0.0)
    if g["virial"] is not None:
        top_v = np.abs(r["virial"][:n]).max()
        err_v = np.abs(g["virial"] - r["virial"][:n]).max()
        W, W_ref = g["virial"].sum(axis=0), r["virial"][:n].sum(axis=0)
        err_w = np.abs(W - W_ref).max() / np.abs(W_ref).max()
        print("virial: max |d| %.3e of max |virial_i| %.3e (%.3e rel); sums %.3e of the largest" % (err_v, top_v, err_v / top_v, err_w))
        assert top_v > 0 and err_v <= tol * top_v
        assert err_w <= tol
        if types is not None:
            assert np.all(g["virial"][types[:n] != type_id] == 0.0)


def noisy_fcc(n, sigma=0.05, seed=777):
    pos, L = util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


@pytest.fixture(scope="module")
def snapshots():
    """the common snapshot: fcc 5 (N = 500, not a multiple of 64) with noise 0.05 and 0.13, the list that reaches 1.5, and the restatement
    of every variant on the fp64 and on the fp32-rounded positions (computed once, shared, never changed)"""
    out = {}
    for noise in (0.05, 0.13):
        pos, L = noisy_fcc(5, sigma=noise)
        types = np.zeros(len(pos), dtype=np.int32)
        for dtype in (np.float64, np.float32):
            p = pos.astype(dtype).astype(np.float64)                    # the snapshot is the rounded array
            nl = util.build_nlist(p, L, R_CUT)
            refs = {name: es.compute(p, types, L, nl, t, SIGMA_ENV, R_ON, R_CUT, 0, lam=lam, sw=sw, bias=0.9)
                    for name, (t, lam, sw, _) in VARIANTS.items()}
            out[noise, dtype] = dict(pos=p, L=L, types=types, nl=nl, refs=refs)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("noise", [0.05, 0.13])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_env_similarity_parity(abi, snapshots, dtype, noise, variant):
    s = snapshots[noise, dtype]
    t, lam, sw, closed = VARIANTS[variant]
    r = s["refs"][variant]
    assert all(r["closed"]) == closed
    if variant.startswith("two"):
        w = r["w"][:, 0]
        assert ((w > 0.1) & (w < 0.9)).mean() >= 0.1                     # the smooth maximum's weights are not saturated
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], t, dtype, lam=lam, sw=sw, virial=True)
    compare(g, r, 0.9, dtype)
    plain = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], t, dtype, lam=lam, sw=sw)
    assert np.array_equal(plain["F"], g["F"])                           # the VIR call's force array is the plain call's, bit for bit
    for key in ("ke", "k", "v"):
        assert np.array_equal(plain[key], g[key])
    assert plain["sum_v"] == g["sum_v"]


def test_env_similarity_known_values(abi, snapshots):
    for noise, want, want_sw in ((0.05, 0.7809426649064931, 460.29055253872525), (0.13, 0.3018897847290363, 61.17201173307594)):
        s = snapshots[noise, np.float64]
        g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], FCC, np.float64)
        assert g["s"] == pytest.approx(want, rel=1e-9)
        g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], FCC, np.float64, sw=SWITCH)
        assert g["sum_v"] == pytest.approx(want_sw, rel=1e-9)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_env_similarity_diamond(abi, dtype):
    """216 particles, two environments that are each other's inverse (the general path), lambda = 100: saturated weights"""
    pos, L, sub = es.diamond_lattice(3)
    pos = (pos + np.random.default_rng(3).normal(0, 0.05, pos.shape)).astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    T = es.templates("diamond", 4.0 / np.sqrt(3.0))
    nl = util.build_nlist(pos, L, 1.45)
    kw = dict(sigma_env=SIGMA_ENV, r_on=1.25, r_cut=1.45)
    r = es.compute(pos, types, L, nl, T, SIGMA_ENV, 1.25, 1.45, 0, bias=0.9)
    assert r["closed"] == [False, False]
    assert np.all(r["ke"][sub == 0, 0] > 3 * r["ke"][sub == 0, 1]) and np.all(r["ke"][sub == 1, 1] > 3 * r["ke"][sub == 1, 0])
    g = run_gpu(abi, pos, types, L, nl, T, dtype, virial=True, **kw)
    compare(g, r, 0.9, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_env_similarity_long_rows(abi, dtype):
    """r_cut 2.1: ~55 entries per row, 14 trips per lane"""
    pos, L = noisy_fcc(5)
    pos = pos.astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 2.1)
    assert len(nl[2]) / len(pos) > 50
    r = es.compute(pos, types, L, nl, FCC, SIGMA_ENV, 1.9, 2.1, 0, bias=0.9)
    g = run_gpu(abi, pos, types, L, nl, FCC, dtype, r_on=1.9, r_cut=2.1, virial=True)
    compare(g, r, 0.9, dtype)
    r = es.compute(pos, types, L, nl, TWO, SIGMA_ENV, 1.9, 2.1, 0, lam=20.0, sw=SWITCH, bias=0.9)
    g = run_gpu(abi, pos, types, L, nl, TWO, dtype, r_on=1.9, r_cut=2.1, lam=20.0, sw=SWITCH, virial=True)
    compare(g, r, 0.9, dtype)


@pytest.mark.parametrize("variant", ["fcc", "two_switch", "half_fcc"])
def test_env_similarity_small_crystal(abi, variant):
    """fcc 3: N = 108, two blocks, the second one mostly empty"""
    t, lam, sw, _ = VARIANTS[variant]
    pos, L = noisy_fcc(3, seed=4)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, R_CUT)
    r = es.compute(pos, types, L, nl, t, SIGMA_ENV, R_ON, R_CUT, 0, lam=lam, sw=sw, bias=0.9)
    g = run_gpu(abi, pos, types, L, nl, t, np.float64, lam=lam, sw=sw, virial=True)
    compare(g, r, 0.9, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_env_similarity_no_pair_inside_the_cutoff(abi, dtype):
    """three particles further apart than r_cut: all k = 0, forces 0, finite; once with empty rows, once with entries beyond r_cut"""
    pos = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    types = np.zeros(3, dtype=np.int32)
    for r_list in (1.5, 4.5):
        nl = util.build_nlist(pos, 20.0, r_list)
        assert (len(nl[2]) == 0) == (r_list == 1.5)
        for sw in (None, SWITCH):
            g = run_gpu(abi, pos, types, 20.0, nl, FCC, dtype, sw=sw, virial=True)
            for key in ("ke", "k", "v", "F", "virial"):
                assert np.all(g[key] == 0.0), key
            assert g["s"] == 0.0


@pytest.mark.parametrize("type_id", [0, 1])
def test_env_similarity_two_types(abi, type_id):
    pos, L = noisy_fcc(5, seed=5)
    types = (np.random.default_rng(1).random(len(pos)) < 0.4).astype(np.int32)
    nl = util.build_nlist(pos, L, R_CUT)
    for t, lam, sw in ((FCC, 100.0, None), (TWO, 20.0, SWITCH)):
        r = es.compute(pos, types, L, nl, t, SIGMA_ENV, R_ON, R_CUT, type_id, lam=lam, sw=sw, bias=0.9)
        g = run_gpu(abi, pos, types, L, nl, t, np.float64, type_id=type_id, lam=lam, sw=sw, virial=True)
        compare(g, r, 0.9, np.float64, types=types, type_id=type_id)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_env_similarity_triclinic_box(abi, dtype):
    """a sheared fcc crystal in the sheared box: HOOMD's minimum image with tilt factors; the template stays the cubic one"""
    pos, L = noisy_fcc(4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = brute_nlist(pos, h, 1.55)
    r = es.compute(pos, types, L, nl, FCC, SIGMA_ENV, R_ON, R_CUT, 0, tilt=tilt, bias=0.9)
    g = run_gpu(abi, pos, types, L, nl, FCC, dtype, tilt=tilt, virial=True)
    compare(g, r, 0.9, dtype)


def test_env_similarity_full_capacity(abi, snapshots):
    """M_e = 32 with E = 2: all 64 slots of the table, random vectors of length 0.8 - 1.2"""
    s = snapshots[0.05, np.float64]
    rng = np.random.default_rng(64)
    v = rng.normal(size=(2, 32, 3))
    v = v / np.linalg.norm(v, axis=2)[:, :, None] * rng.uniform(0.8, 1.2, (2, 32))[:, :, None]
    T = [v[0], v[1]]
    r = es.compute(s["pos"], s["types"], s["L"], s["nl"], T, SIGMA_ENV, R_ON, R_CUT, 0, lam=20.0, sw=SWITCH, bias=0.9)
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], T, np.float64, lam=20.0, sw=SWITCH, virial=True)
    compare(g, r, 0.9, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_env_similarity_ghost_rows(abi, dtype):
    """the first 300 particles are central, the trailing 200 are ghosts: indexed by the rows, owning none.  The plain variable: the local
    rows are the single-domain rows; with a switch or two environments the call is refused"""
    pos, L = noisy_fcc(5, seed=9)
    pos = pos.astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    head, nn, lst = util.build_nlist(pos, L, R_CUT)
    n_rows = 300
    nl = (head[:n_rows], nn[:n_rows], lst[:head[n_rows]])
    assert (nl[2] >= n_rows).any()
    full = es.compute(pos, types, L, (head, nn, lst), FCC, SIGMA_ENV, R_ON, R_CUT, 0, bias=0.9)
    part = es.compute(pos, types, L, nl, FCC, SIGMA_ENV, R_ON, R_CUT, 0, n_global=len(pos), bias=0.9)
    for key in ("k", "gather", "virial"):
        assert np.abs(part[key] - full[key][:n_rows]).max() <= 1e-15
    g = run_gpu(abi, pos, types, L, nl, FCC, dtype, virial=True, n_rows=n_rows, n_ghost=len(pos) - n_rows)
    compare(g, part, 0.9, dtype, zero_sum=False)
    run_gpu(abi, pos, types, L, nl, FCC, dtype, sw=SWITCH, n_rows=n_rows, n_ghost=len(pos) - n_rows, expect=UNSUPPORTED)
    run_gpu(abi, pos, types, L, nl, TWO, dtype, lam=20.0, n_rows=n_rows, n_ghost=len(pos) - n_rows, expect=UNSUPPORTED)


@pytest.mark.parametrize("variant", ["fcc", "two_switch", "half_fcc"])
def test_env_similarity_identical_calls_and_bias_source(abi, snapshots, variant):
    """two identical calls: identical bits; the bias from the device pointer and from the host: identical bits; bias 0: zeros"""
    s = snapshots[0.13, np.float64]
    t, lam, sw, _ = VARIANTS[variant]
    kw = dict(lam=lam, sw=sw, virial=True)
    a = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], t, np.float64, bias=-1.7, **kw)
    b = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], t, np.float64, bias=-1.7, **kw)
    host = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], t, np.float64, bias=-1.7, bias_on_device=False, **kw)
    for key in ("ke", "k", "v", "F", "virial"):
        assert np.array_equal(a[key], b[key]), key
    assert a["sum_v"] == b["sum_v"]
    assert np.array_equal(a["F"], host["F"]) and np.array_equal(a["virial"], host["virial"])
    r = es.compute(s["pos"], s["types"], s["L"], s["nl"], t, SIGMA_ENV, R_ON, R_CUT, 0, lam=lam, sw=sw, bias=-1.7)
    compare(a, r, -1.7, np.float64)
    zero = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], t, np.float64, bias=0.0, bias_on_device=False, **kw)
    assert np.all(zero["F"] == 0.0) and np.all(zero["virial"] == 0.0)


def test_env_similarity_many_blocks(abi):
    """fcc 12 (N = 6912): 108 blocks, block sums across chunk boundaries"""
    pos, L = noisy_fcc(12, seed=21)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, R_CUT)
    r = es.compute(pos, types, L, nl, TWO, SIGMA_ENV, R_ON, R_CUT, 0, lam=20.0, sw=SWITCH, bias=0.9)
    g = run_gpu(abi, pos, types, L, nl, TWO, np.float64, lam=20.0, sw=SWITCH, virial=True)
    compare(g, r, 0.9, np.float64)


# ---- the chunk loops: more chunks of 64 than the 1024 blocks the launches are capped at ---------------------------------------------
SC = es.templates("sc", 1.0)
SC_R_ON, SC_R_CUT = 1.15, 1.3
SC_SWITCH = (0.5, 4)
# name: (templates, lambda, switch, all environments closed); the paths of VARIANTS on the simple cubic template
SC_VARIANTS = {"fused": (SC, 100.0, None, True),                                 # one closed environment: k_es_accumulate<FUSED> + k_es_scale
               "split_switch": ([SC[:3], SC[3:]], 20.0, SC_SWITCH, False),       # beta of the second loop read by k_es_forces<.., false, false>
               "open_single": (SC[:3], 100.0, None, False),                      # as half_fcc: CONSTB
               "two_closed": ([SC, SC @ rot_z(5.0).T], 20.0, None, True)}        # as two: k_es_forces<.., true, false>


_sc_snapshots = {}


def noisy_sc(n, dtype, sigma=0.05, seed=3):
    """n^3 particles of the simple cubic lattice with constant 1, centred on 0, with Gaussian noise, rounded to dtype; its list to 1.3
    (built once per n and dtype, shared, never changed)"""
    if (n, dtype) not in _sc_snapshots:
        axis = np.arange(n) - 0.5 * (n - 1)
        pos = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
        pos = (pos + np.random.default_rng(seed).normal(0, sigma, pos.shape)).astype(dtype).astype(np.float64)
        _sc_snapshots[n, dtype] = (pos, float(n), np.zeros(len(pos), dtype=np.int32), util.build_nlist(pos, float(n), SC_R_CUT))
    return _sc_snapshots[n, dtype]


def run_sc(abi, snap, variant, dtype):
    pos, L, types, nl = snap
    t, lam, sw, _ = SC_VARIANTS[variant]
    return run_gpu(abi, pos, types, L, nl, t, dtype, r_on=SC_R_ON, r_cut=SC_R_CUT, lam=lam, sw=sw, virial=True)


# n: (N, the restatement's s where it was worked out beforehand: 0.78544 and, with lambda = 20, 0.87823 (0.87130 is that of lambda = 100))
SC_SIZES = {65: (274625, {"fused": 0.78544, "split_switch": 0.87823}),
            42: (74088, {})}


@pytest.mark.parametrize("n,variant,dtype", [(65, "fused", np.float64), (65, "fused", np.float32), (65, "split_switch", np.float64),
                                             (42, "open_single", np.float64), (42, "two_closed", np.float64)])
def test_chunk_loop(abi, n, variant, dtype):
    """simple cubic 65^3 (N = 274 625, odd: the scratch rounds up): 4292 chunks of 64 on 1024 blocks.  Every block walks four or five
    chunks; in the second loop of k_es_accumulate all four waves of a block work and wave 0 takes the stride of 4 * gridDim.x.  The
    FUSED pair of kernels with both array types and the general path whose force pass reads the beta of that second loop.
    Simple cubic 42^3 (N = 74 088), a quarter of the cost: 1158 chunks, blocks 0 - 133 walk two chunks and their wave 1 works in the second
    loop; the two force kernels that the large snapshot does not launch (CONSTB, and CLOSED with a table of beta)"""
    snap = noisy_sc(n, dtype)
    pos, L, types, nl = snap
    N = len(pos)
    n_chunks = (N + 63) // 64
    assert N == SC_SIZES[n][0]
    assert (n_chunks > 4 * 1024 and N % 2 == 1) if n == 65 else 1024 < n_chunks <= 2 * 1024
    assert 6 <= len(nl[2]) / N <= 9
    t, lam, sw, closed = SC_VARIANTS[variant]
    r = es.compute(pos, types, L, nl, t, SIGMA_ENV, SC_R_ON, SC_R_CUT, 0, lam=lam, sw=sw, bias=0.9)
    assert all(r["closed"]) == closed
    # what the restatement's own gather adds up to: the measure for the zero-sum bound of compare() at this size
    print("restatement: sum of the gather %.3e of sum |gather|" % (np.abs(r["gather"].sum(axis=0)).max() / np.abs(r["gather"]).sum()))
    if variant in SC_SIZES[n][1]:
        assert r["s"] == pytest.approx(SC_SIZES[n][1][variant], abs=1e-5)
    if len(es.as_environments(t)) > 1:
        w = r["w"][:, 0]
        assert ((w > 0.1) & (w < 0.9)).mean() >= 0.1                     # the smooth maximum's weights are not saturated
    g = run_sc(abi, snap, variant, dtype)
    assert g["n_part"] == 1024
    compare(g, r, 0.9, dtype)
    if (n, variant, dtype) == (65, "fused", np.float64):
        again = run_sc(abi, snap, variant, dtype)
        for key in ("ke", "k", "v", "F", "virial"):
            assert np.array_equal(g[key], again[key]), key               # two identical calls: identical bits
        assert g["sum_v"] == again["sum_v"]
