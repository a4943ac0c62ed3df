"""GPU parity: the coordination number (mtd_coord_*, csrc/coordination.hip) through the C ABI against the fp64 numpy restatement of its
definition (tests/coordination_ref.py, itself checked on the CPU in tests/test_coordination_ref.py).

Tolerances, the project's for this arithmetic: value 1e-9 relative, n_i and v_i 1e-9 of their maximum; forces and per-particle virial
1e-9 of their maximum with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store).  Snapshots are rounded to the array type
first.  Every figure is printed before it is asserted.  Both routes are held to them: plain (one walk that stores every particle's
gradient and virial sums, the force call scales them) and switch (two walks, g'(n_j) from the per-particle table).

test_chunk_loop: N = 37 044 is the smallest fcc crystal whose 1158 chunks of 32 central particles (CN_PPB) exceed the 1024 blocks the
launches are capped at (CN_MAX_BLOCKS), so blocks 0 - 133 walk two chunks.
"""
import ctypes as C

import numpy as np
import pytest

import coordination_ref as cn
import stream_gate
import util
from test_gpu_ql_local import brute_nlist

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

R0, R_CUT = 1.15, 2.0
SWITCHES = {"plain": None, "switch": (5.0, 8), "less": (5.0, 8, True)}
OUTPUTS = ("s", "sums", "local", "switched", "F", "virial")
UNSUPPORTED = -2


def run_gpu(abi, pos, types, L, nl, par, dtype, bias=0.9, tilt=None, bias_on_device=True, virial=False, n_rows=None, gate=None, expect=0, compiled=True):
    """returns dict(s, sums, local, switched, F, virial); par: coordination_ref.params(...); n_rows: the first n_rows particles are the
    central ones, the others ghosts; gate: the stream the calls run on and how their inputs arrive (tests/stream_gate.py; None: the NULL
    stream); expect: the status mtd_coord_accumulate must return (then nothing else is called and None comes back); compiled: False sends
    (6, 12) through the general Horner loop (mtd_coord_set_compiled_pair)"""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N = len(nl[0]) if n_rows is None else n_rows
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    if len(nl[2]) == 0:
        d_nl = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    scratch = torch.zeros(lib.mtd_coord_scratch_doubles(N), dtype=torch.float64, device="cuda")
    force = torch.full((max(N, 1), 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda") if virial else None
    cpar = abi.CoordParams.make(par["type_a"], par["type_b"], par["r_0"], par["r_cut"], d_0=par["d_0"], n=par["n"], m=par["m"],
                                switch=par["switch"])
    p_sums, p_value, p_local, p_switched = (C.c_void_p() for _ in range(4))
    n_sums = C.c_uint()
    stream = gate.arm()
    call = abi.CoordCall(N, len(pos) - N, abi.ptr(d_pos) if len(pos) else None, dt, C.pointer(box), abi.ptr(d_head) if N else None,
                         abi.ptr(d_nn) if N else None, abi.ptr(d_nl), abi.ptr(scratch), stream)
    abi.check(lib.mtd_coord_set_compiled_pair(1 if compiled else 0))
    try:
        rc = lib.mtd_coord_accumulate(C.byref(cpar), C.byref(call), C.byref(p_sums), C.byref(n_sums))
        if expect:
            assert rc == expect
            assert lib.mtd_coord_forces(C.byref(cpar), C.byref(call), abi.ptr(force), None, bias, None, 0) == expect
            return gate.done(lambda: None)
        abi.check(rc)
        assert n_sums.value == 2
        abi.check(lib.mtd_coord_finalize(C.byref(cpar), C.byref(call), C.byref(p_value), C.byref(p_local), C.byref(p_switched)))
        abi.check(lib.mtd_coord_forces(C.byref(cpar), C.byref(call), abi.ptr(force), abi.ptr(d_bias) if bias_on_device else None,
                                       0.0 if bias_on_device else bias, abi.ptr(vir) if virial else None, pitch if virial else 0))
    finally:
        abi.check(lib.mtd_coord_set_compiled_pair(1))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        out = dict(s=float(s[off(p_value)]), sums=s[off(p_sums):off(p_sums) + 2].copy(), local=s[off(p_local):off(p_local) + N].copy(),
                   switched=s[off(p_switched):off(p_switched) + N].copy(), F=force.cpu().numpy().astype(np.float64)[:N], virial=None)
        if virial:
            v = vir.cpu().numpy().astype(np.float64)
            assert np.all(v[:, N:] == 7.0)                                  # [n_particles, pitch) is left alone
            out["virial"] = v[:, :N].T.copy()
        return out
    return gate.done(read)


def noisy_fcc(n, sigma=0.05, seed=777):
    pos, L = util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


def compare(g, r, bias, dtype, types=None, par=None, forces=True):
    """prints every figure, then asserts; r: the restatement's result (its virial formed with the same bias)"""
    n_rows = len(g["F"])
    err_s = abs(g["s"] - r["s"]) / abs(r["s"]) if r["s"] else abs(g["s"])
    top_l, top_v = max(np.abs(r["local"]).max(), 1e-300), max(np.abs(r["switched"]).max(), 1e-300)
    err_l = np.abs(g["local"] - r["local"][:n_rows]).max() / top_l
    err_v = np.abs(g["switched"] - r["switched"][:n_rows]).max() / top_v
    F_ref = -bias * r["gather"][:n_rows]
    fs = np.abs(F_ref).max()
    err_f = np.abs(g["F"][:, :3] - F_ref).max()
    print("s %.15g vs %.15g (%.3e rel); n_i %.3e of max, v_i %.3e of max; forces: max |d| %.3e of max |F| %.3e (%.3e rel)"
          % (g["s"], r["s"], err_s, err_l, err_v, err_f, fs, err_f / fs if fs else 0.0))
    assert np.isfinite(g["F"]).all() and np.isfinite(g["s"]) and np.isfinite(g["local"]).all() and np.isfinite(g["switched"]).all()
    assert g["sums"][1] == r["n_a"]
    assert err_s <= 1e-9 and err_l <= 1e-9 and err_v <= 1e-9
    tol = 1e-9 if dtype == np.float64 else 2e-7
    if forces:
        assert fs > 0
    assert err_f <= tol * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        t = types[:n_rows]
        assert np.all(g["F"][(t != par["type_a"]) & (t != par["type_b"])] == 0.0)
        assert np.all(g["local"][t != par["type_a"]] == 0.0) and np.all(g["switched"][t != par["type_a"]] == 0.0)
    if g["virial"] is not None:
        top_w = np.abs(r["virial"]).max()
        err_w = np.abs(g["virial"] - r["virial"][:n_rows]).max()
        W, W_ref = g["virial"].sum(axis=0), r["virial"][:n_rows].sum(axis=0)
        err_sum = np.abs(W - W_ref).max() / np.abs(W_ref).max() if top_w else np.abs(W).max()
        print("virial: max |d| %.3e of max |virial_i| %.3e (%.3e rel); sums %.3e rel" % (err_w, top_w, err_w / top_w if top_w else 0.0, err_sum))
        if forces:
            assert top_w > 0
        assert err_w <= tol * top_w
        assert err_sum <= tol                                          # (fp32: every stored row errs by 2^-24 of itself at most)
        if types is not None:
            assert np.all(g["virial"][(t != par["type_a"]) & (t != par["type_b"])] == 0.0)


@pytest.fixture(scope="module")
def snapshot():
    """the common snapshot: fcc 5 (N = 500, not a multiple of 64) with noise 0.05, interleaved types, the list that reaches 2.0"""
    pos, L = noisy_fcc(5)
    return dict(pos=pos, L=L, types=(np.arange(len(pos)) % 2).astype(np.int32), nl=util.build_nlist(pos, L, R_CUT))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", ["plain", "switch", "less"])
@pytest.mark.parametrize("pair", [(0, 1), (1, 0), (0, 0)])
def test_coordination_parity(abi, snapshot, dtype, mode, pair):
    s = snapshot
    par = cn.params(pair[0], pair[1], R0, R_CUT, switch=SWITCHES[mode])
    pos = s["pos"].astype(dtype).astype(np.float64)                     # the snapshot is the rounded array
    g = run_gpu(abi, pos, s["types"], s["L"], s["nl"], par, dtype, virial=True)
    r = cn.compute(pos, s["types"], s["L"], s["nl"], par, bias=0.9)
    assert r["n_a"] == 250
    compare(g, r, 0.9, dtype, types=s["types"], par=par)
    plain = run_gpu(abi, pos, s["types"], s["L"], s["nl"], par, dtype)
    assert np.array_equal(plain["F"], g["F"])                           # the call with a virial writes the plain call's force array, bit for bit
    assert plain["s"] == g["s"] and np.array_equal(plain["local"], g["local"]) and np.array_equal(plain["switched"], g["switched"])
    again = run_gpu(abi, pos, s["types"], s["L"], s["nl"], par, dtype, virial=True)
    for key in OUTPUTS:
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits
    fs, N = np.abs(g["F"]).max(), len(pos)
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N


def test_coordination_known_values(abi, snapshot):
    """the figures of the issue's table, from the CPU prototype of the restatement: 1e-8 absolute on the restatement and on the GPU"""
    s = snapshot
    for pair, mean_n, switched in (((0, 1), 6.165718608, 0.839369040), ((0, 0), 4.322091307, 0.241907792)):
        for switch, want in ((None, mean_n), ((5.0, 8), switched)):
            par = cn.params(pair[0], pair[1], R0, R_CUT, switch=switch)
            r = cn.compute(s["pos"], s["types"], s["L"], s["nl"], par)
            g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64)
            print("pair %s switch %s: restatement %.10f, GPU %.10f, table %.9f" % (pair, switch, r["s"], g["s"], want))
            assert abs(r["s"] - want) <= 1e-8 and abs(g["s"] - want) <= 1e-8
            assert g["switched"].sum() / 250 == pytest.approx(g["s"], rel=1e-12)


@pytest.mark.parametrize("d_0", [0.0, 0.1])
@pytest.mark.parametrize("n,m", [(6, 12), (5, 9), (1, 2), (12, 24), (31, 32)])
def test_coordination_exponents(abi, snapshot, n, m, d_0):
    s = snapshot
    for switch in (None, (5.0, 8)):
        par = cn.params(0, 1, R0, R_CUT, d_0=d_0, n=n, m=m, switch=switch)
        g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, virial=True)
        r = cn.compute(s["pos"], s["types"], s["L"], s["nl"], par, bias=0.9)
        compare(g, r, 0.9, np.float64, types=s["types"], par=par)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", ["plain", "switch"])
def test_both_forms_of_the_default_pair(abi, snapshot, dtype, mode):
    """(6, 12) through the general Horner loop (mtd_coord_set_compiled_pair(0)) meets the same tolerances as its compiled form
    1 / (1 + x^6), which every other test of (6, 12) runs; the two agree far inside them"""
    s = snapshot
    pos = s["pos"].astype(dtype).astype(np.float64)
    par = cn.params(0, 1, R0, R_CUT, d_0=0.1, switch=SWITCHES[mode])
    r = cn.compute(pos, s["types"], s["L"], s["nl"], par, bias=0.9)
    a = run_gpu(abi, pos, s["types"], s["L"], s["nl"], par, dtype, virial=True, compiled=True)
    b = run_gpu(abi, pos, s["types"], s["L"], s["nl"], par, dtype, virial=True, compiled=False)
    compare(a, r, 0.9, dtype, types=s["types"], par=par)
    compare(b, r, 0.9, dtype, types=s["types"], par=par)
    tol = 1e-13 if dtype == np.float64 else 2.0 ** -23                   # (fp32: the last bit of a stored component may differ)
    assert abs(a["s"] - b["s"]) <= 1e-13 * abs(a["s"]) and np.abs(a["local"] - b["local"]).max() <= 1e-13 * np.abs(a["local"]).max()
    assert np.abs(a["F"] - b["F"]).max() <= tol * np.abs(a["F"]).max()
    assert np.abs(a["virial"] - b["virial"]).max() <= tol * np.abs(a["virial"]).max()


def dimers(separations, L=40.0):
    """isolated A-B dimers on the x axis, far from each other, with the hand-made list of each particle's one partner"""
    k = len(separations)
    pos = np.zeros((2 * k, 3))
    side = int(np.ceil(k ** 0.5))
    for d, sep in enumerate(separations):
        origin = np.array([0.0, -15.0 + 6.0 * (d % side), -15.0 + 6.0 * (d // side)])      # x = 0: the separation is exactly `sep`
        pos[2 * d] = origin
        pos[2 * d + 1] = origin + np.array([sep, 0.0, 0.0])
    types = (np.arange(2 * k) % 2).astype(np.int32)
    nl = (np.arange(2 * k), np.ones(2 * k, dtype=np.int64), np.arange(2 * k) ^ 1)
    return pos, types, L, nl


@pytest.mark.parametrize("n,m", [(6, 12), (5, 9)])
def test_removable_singularity(abi, n, m):
    """separations exactly 1 and 1 +- 1e-12, 1e-9, 1e-6 with r_0 = 1, d_0 = 0: x AT and AROUND 1, where the quotient form is 0 / 0 and
    loses digits.  s~ and the force are finite and meet the tolerance at every one of them"""
    seps = [1.0] + [1.0 + sg * e for e in (1e-12, 1e-9, 1e-6) for sg in (1.0, -1.0)]
    pos, types, L, nl = dimers(seps)
    for switch, compiled in ((None, True), ((0.5, 3), True), (None, False), ((0.5, 3), False)):
        if not compiled and (n, m) != (6, 12):
            continue                                                     # (only the default pair has a compiled form beside the loop)
        par = cn.params(0, 1, 1.0, 2.0, n=n, m=m, switch=switch)
        g = run_gpu(abi, pos, types, L, nl, par, np.float64, virial=True, compiled=compiled)
        r = cn.compute(pos, types, L, nl, par, bias=0.9)
        compare(g, r, 0.9, np.float64, types=types, par=par)
        F_ref = -0.9 * r["gather"]
        for d, sep in enumerate(seps):
            rel_n = abs(g["local"][2 * d] - r["local"][2 * d]) / r["local"][2 * d]
            rel_f = np.abs(g["F"][2 * d:2 * d + 2, :3] - F_ref[2 * d:2 * d + 2]).max() / np.abs(F_ref[2 * d]).max()
            print("separation 1 %+.0e: s~ %.15g (%.3e rel), force %.3e rel" % (sep - 1.0, g["local"][2 * d], rel_n, rel_f))
            assert rel_n <= 1e-9 and rel_f <= 1e-9                       # every dimer on its own, not only against the maximum
            assert np.array_equal(g["F"][2 * d, :3], -g["F"][2 * d + 1, :3])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_inner_region_and_coincident_pair(abi, dtype):
    """entries with r <= d_0 count 1 with no force; two particles in one place (r = 0 exactly) give finite results with d_0 = 0 and 0.1"""
    pos, types, L, nl = dimers([0.05, 0.15, 0.3, 0.0, 1.0])
    pos = pos.astype(dtype).astype(np.float64)
    for d_0 in (0.0, 0.1, 0.4):
        for switch in (None, (0.5, 3)):
            par = cn.params(0, 1, 1.0, 2.0, d_0=d_0, switch=switch)
            g = run_gpu(abi, pos, types, L, nl, par, dtype, virial=True)
            r = cn.compute(pos, types, L, nl, par, bias=0.9)
            compare(g, r, 0.9, dtype, types=types, par=par)
            inside = [d for d, sep in enumerate((0.05, 0.15, 0.3, 0.0, 1.0)) if np.linalg.norm(pos[2 * d + 1] - pos[2 * d]) <= d_0]
            assert 3 in inside                                           # the coincident pair always is
            for d in inside:
                assert g["local"][2 * d] == 1.0 and np.all(g["F"][2 * d:2 * d + 2] == 0.0) and np.all(g["virial"][2 * d:2 * d + 2] == 0.0)


def test_unequal_counts_and_the_pair_sum_identity(abi, snapshot):
    s = snapshot
    types = (np.random.default_rng(2).random(len(s["pos"])) < 0.3).astype(np.int32)
    out = {}
    for pair in ((0, 1), (1, 0)):
        par = cn.params(pair[0], pair[1], R0, R_CUT)
        g = run_gpu(abi, s["pos"], types, s["L"], s["nl"], par, np.float64, virial=True)
        r = cn.compute(s["pos"], types, s["L"], s["nl"], par, bias=0.9)
        compare(g, r, 0.9, np.float64, types=types, par=par)
        out[pair] = g
    assert out[(0, 1)]["sums"][1] == 340 and out[(1, 0)]["sums"][1] == 160
    lhs, rhs = 340 * out[(0, 1)]["s"], 160 * out[(1, 0)]["s"]
    print("N_A s_AB = %.12f, N_B s_BA = %.12f" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert abs(lhs - 1151.7367242932) <= 1e-8


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ghosts(abi, dtype):
    """the first 300 particles are central, the trailing 200 are ghosts: indexed by the rows, owning none.  The plain variable forms the
    gather over the rows with the sums of the rows; with a switch the same call is refused"""
    pos, L = noisy_fcc(5, seed=9)
    pos = pos.astype(dtype).astype(np.float64)
    types = (np.arange(len(pos)) % 2).astype(np.int32)
    head, nn, lst = util.build_nlist(pos, L, R_CUT)
    n_rows = 300
    nl = (head[:n_rows], nn[:n_rows], lst[:head[n_rows]])
    assert (nl[2] >= n_rows).any()
    for pair in ((0, 1), (0, 0)):
        par = cn.params(pair[0], pair[1], R0, R_CUT)
        g = run_gpu(abi, pos, types, L, nl, par, dtype, virial=True, n_rows=n_rows)
        r = cn.compute(pos, types, L, nl, par, bias=0.9)
        assert r["n_a"] == 150
        compare(g, r, 0.9, dtype, types=types, par=par)
        assert run_gpu(abi, pos, types, L, nl, cn.params(pair[0], pair[1], R0, R_CUT, switch=(5.0, 8)), dtype, n_rows=n_rows,
                       expect=UNSUPPORTED) is None


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_triclinic_box(abi, dtype):
    """a sheared fcc crystal in the sheared box: HOOMD's minimum image with tilt factors"""
    pos, L = noisy_fcc(4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = (np.arange(len(pos)) % 2).astype(np.int32)
    nl = brute_nlist(pos, h, R_CUT + 0.05)
    for switch in (None, (5.0, 8)):
        par = cn.params(0, 1, R0, R_CUT, switch=switch)
        g = run_gpu(abi, pos, types, L, nl, par, dtype, tilt=tilt, virial=True)
        r = cn.compute(pos, types, L, nl, par, tilt=tilt, bias=0.9)
        compare(g, r, 0.9, dtype, types=types, par=par)


def test_list_beyond_the_cutoff(abi):
    """a list that reaches 2.4 gives what the list cut at r_cut = 2.0 gives: entries beyond the cut-off are skipped"""
    pos, L = noisy_fcc(5, seed=9)
    types = (np.random.default_rng(2).random(len(pos)) < 0.3).astype(np.int32)
    tight = util.build_nlist(pos, L, R_CUT)
    wide = util.build_nlist(pos, L, 2.4)
    assert len(wide[2]) > 1.3 * len(tight[2])
    for switch in (None, (5.0, 8)):
        par = cn.params(0, 1, R0, R_CUT, switch=switch)
        a = run_gpu(abi, pos, types, L, tight, par, np.float64, virial=True)
        b = run_gpu(abi, pos, types, L, wide, par, np.float64, virial=True)
        r = cn.compute(pos, types, L, wide, par, bias=0.9)
        compare(b, r, 0.9, np.float64, types=types, par=par)
        fs = np.abs(a["F"]).max()
        assert abs(a["s"] - b["s"]) <= 1e-12 * abs(a["s"]) and np.abs(a["F"] - b["F"]).max() <= 1e-12 * fs
        assert np.abs(a["virial"] - b["virial"]).max() <= 1e-12 * np.abs(a["virial"]).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nothing_to_sum(abi, dtype):
    """no particle of type A: everything 0; A without a B in reach (empty rows, and entries that all lie beyond r_cut): n_i = 0, plain
    s = 0, switch s = 0, `less` s = 1, forces exactly 0; no particle at all: success, s = 0"""
    pos = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0], [4.0, 4.0, 4.0]])
    types = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    L = 20.0
    for r_list in (2.0, 4.5):
        nl = util.build_nlist(pos, L, r_list)
        assert (len(nl[2]) == 0) == (r_list == 2.0)
        for mode, want in (("plain", 0.0), ("switch", 0.0), ("less", 1.0)):
            g = run_gpu(abi, pos, types, L, nl, cn.params(0, 1, R0, R_CUT, switch=SWITCHES[mode]), dtype, virial=True)
            assert g["s"] == want and g["sums"][1] == 3 and np.all(g["local"] == 0.0)
            assert np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
            g = run_gpu(abi, pos, types, L, nl, cn.params(2, 1, R0, R_CUT, switch=SWITCHES[mode]), dtype, virial=True)      # no A
            assert g["s"] == 0.0 and np.all(g["sums"] == 0.0) and np.all(g["local"] == 0.0) and np.all(g["switched"] == 0.0)
            assert np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    for mode in SWITCHES:
        g = run_gpu(abi, np.zeros((0, 3)), np.zeros(0, dtype=np.int32), L, empty, cn.params(0, 1, R0, R_CUT, switch=SWITCHES[mode]), dtype,
                    virial=True)
        assert g["s"] == 0.0 and np.all(g["sums"] == 0.0)


def test_bias_from_device_and_host(abi, snapshot):
    s = snapshot
    for switch in (None, (5.0, 8)):
        par = cn.params(0, 1, R0, R_CUT, switch=switch)
        dev = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=-1.7, bias_on_device=True, virial=True)
        host = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=-1.7, bias_on_device=False, virial=True)
        assert np.array_equal(dev["F"], host["F"]) and np.array_equal(dev["virial"], host["virial"])
        r = cn.compute(s["pos"], s["types"], s["L"], s["nl"], par, bias=-1.7)
        compare(dev, r, -1.7, np.float64, types=s["types"], par=par)
        zero = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=0.0, bias_on_device=False, virial=True)
        assert np.all(zero["F"] == 0.0) and np.all(zero["virial"] == 0.0)


@pytest.mark.parametrize("dtype,two_types,mode", [(np.float64, False, "plain"), (np.float32, False, "plain"), (np.float64, True, "plain"),
                                                  (np.float64, False, "switch"), (np.float64, True, "switch")])
def test_chunk_loop(abi, dtype, two_types, mode):
    """fcc 21 (N = 37 044): 1158 chunks of 32 on 1024 blocks, so blocks 0 - 133 walk two chunks.  The list reaches r_cut = 1.5 only (~17
    entries per row): the restatement stays cheap.  With a second type on ~30 % of the particles the role test decides in second-trip
    chunks too"""
    pos, L = noisy_fcc(21, sigma=0.05, seed=1)
    N = len(pos)
    n_chunks = (N + 31) // 32
    assert N == 37044 and n_chunks > 1024 and n_chunks < 2 * 1024
    pos = pos.astype(dtype).astype(np.float64)                          # the snapshot is the rounded array
    types = (np.random.default_rng(4).random(N) < 0.3).astype(np.int32) if two_types else np.zeros(N, dtype=np.int32)
    par = cn.params(0, 1 if two_types else 0, R0, 1.5, switch=(3.0, 8) if mode == "switch" else None)
    nl = util.build_nlist(pos, L, 1.5)
    assert 15 < len(nl[2]) / N < 20
    g = run_gpu(abi, pos, types, L, nl, par, dtype, virial=True)
    r = cn.compute(pos, types, L, nl, par, bias=0.9)
    if two_types:
        assert 0.6 * N < r["n_a"] < 0.8 * N and (types[1024 * 32:] == 1).sum() > 100       # the other type inside the second-trip chunks
    compare(g, r, 0.9, dtype, types=types, par=par)
    again = run_gpu(abi, pos, types, L, nl, par, dtype, virial=True)
    for key in OUTPUTS:
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits
    fs = np.abs(g["F"]).max()
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N
