"""GPU parity: the tetrahedral order (mtd_tet_*, csrc/tetrahedral.hip) through the C ABI against the fp64 numpy restatement of its
definition (tests/tetrahedral_ref.py: the explicit sum over the pairs of every row, itself checked on the CPU in
tests/test_tetrahedral_ref.py).  The kernels evaluate the moment form: the parity holds the identity between the two as well.

Tolerances, the project's for this arithmetic: value 1e-9 relative; n_i, t_i and v_i 1e-9 of their maximum; forces and per-particle
virial 1e-9 of their maximum with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store).  Snapshots are rounded to the array
type first.  Every figure is printed before it is asserted.

Condition on the inputs, asserted on the restatement before any GPU call (condition()): every pair weight W_i is 0 or >= 1e-3 — t_i is a
quotient by W_i, and the moment form of W_i cancels terms of size n_i^2 — and no distance lies within 1e-9 of r_on or r_cut, where the
rounding of r decides whether an entry counts.

test_chunk_loop: N = 37 044 is the smallest fcc crystal whose 1158 chunks of 32 central particles exceed the 1024 blocks the launches
are capped at, so blocks 0 - 133 walk two chunks.
"""
import ctypes as C

import numpy as np
import pytest

import stream_gate
import tetrahedral_ref as tr
import util
from test_gpu_ql_local import brute_nlist

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OUTPUTS = ("s", "sums", "local", "switched", "coordination", "F", "virial")
UNSUPPORTED = -2
# the window crosses the first shell (distance 1 +- noise) and ends below the second (diamond 1.63, fcc 1.41)
LATTICES = {
    "diamond": dict(r_on=0.9, r_cut=1.3, switch=(0.6, 6), gate=(1.5, 3.5)),
    "fcc": dict(r_on=0.9, r_cut=1.25, switch=(0.25, 4), gate=(5.0, 9.0)),
}
OPTION_SETS = ("plain", "switch", "gate", "switch+gate", "penalty", "cos0=0")


def params(lattice, name, type_id=0):
    k = LATTICES[lattice]
    opt = {"plain": dict(), "switch": dict(switch=k["switch"]), "gate": dict(gate=k["gate"]),
           "switch+gate": dict(switch=k["switch"], gate=k["gate"]), "penalty": dict(normalise=False), "cos0=0": dict(cos0=0.0)}[name]
    return tr.params(type_id, k["r_cut"], k["r_on"], **opt)


def run_gpu(abi, pos, types, L, nl, par, dtype, bias=0.9, tilt=None, bias_on_device=True, virial=False, n_ghost=0, gate=None, expect=0):
    """returns dict(s, sums, local, switched, coordination, F, virial); par: tetrahedral_ref.params(...); gate: the stream the calls run on
    and how their inputs arrive (tests/stream_gate.py; None: the NULL stream); expect: the status mtd_tet_accumulate must return (then
    nothing else is launched and None comes back)"""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N = len(nl[0])
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    if len(nl[2]) == 0:
        d_nl = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    scratch = torch.zeros(lib.mtd_tet_scratch_doubles(N), dtype=torch.float64, device="cuda")
    force = torch.full((max(N, 1), 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda") if virial else None
    cpar = abi.TetParams.make(par["type"], par["r_cut"], par["r_on"], cos0=par["cos0"], normalise=par["normalise"], switch=par["switch"],
                              gate=par["gate"])
    p_sums, p_value, p_local, p_switched, p_coord = (C.c_void_p() for _ in range(5))
    n_sums = C.c_uint()
    stream = gate.arm()
    call = abi.TetCall(N, n_ghost, abi.ptr(d_pos) if len(pos) else None, dt, C.pointer(box), abi.ptr(d_head) if N else None,
                       abi.ptr(d_nn) if N else None, abi.ptr(d_nl), abi.ptr(scratch), stream)
    rc = lib.mtd_tet_accumulate(C.byref(cpar), C.byref(call), C.byref(p_sums), C.byref(n_sums))
    if expect:
        assert rc == expect
        assert lib.mtd_tet_forces(C.byref(cpar), C.byref(call), abi.ptr(force), None, bias, None, 0) == expect
        return gate.done(lambda: None)
    abi.check(rc)
    assert n_sums.value == 2
    abi.check(lib.mtd_tet_finalize(C.byref(cpar), C.byref(call), C.byref(p_value), C.byref(p_local), C.byref(p_switched), C.byref(p_coord)))
    abi.check(lib.mtd_tet_forces(C.byref(cpar), C.byref(call), abi.ptr(force), abi.ptr(d_bias) if bias_on_device else None,
                                 0.0 if bias_on_device else bias, abi.ptr(vir) if virial else None, pitch if virial else 0))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        per = lambda p: s[off(p):off(p) + N].copy()
        out = dict(s=float(s[off(p_value)]), sums=s[off(p_sums):off(p_sums) + 2].copy(), local=per(p_local), switched=per(p_switched),
                   coordination=per(p_coord), F=force.cpu().numpy().astype(np.float64)[:N], virial=None)
        if virial:
            v = vir.cpu().numpy().astype(np.float64)
            assert np.all(v[:, N:] == 7.0)                                  # [n_particles, pitch) is left alone
            out["virial"] = v[:, :N].T.copy()
        return out
    return gate.done(read)


def noisy(lattice, n, sigma=0.05, seed=777):
    pos, L = tr.diamond_lattice(n) if lattice == "diamond" else util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


def condition(r, par):
    """what the tolerances presuppose (module docstring), asserted on the restatement's result"""
    W = r["W"]
    assert np.all((W == 0.0) | (W >= 1e-3)), W[(W != 0.0) & (W < 1e-3)]
    assert np.abs(r["r"] - par["r_on"]).min() > 1e-9 and np.abs(r["r"] - par["r_cut"]).min() > 1e-9


def compare(g, r, bias, dtype, types=None, par=None, forces=True):
    """prints every figure, then asserts; r: the restatement's result (its virial formed with the same bias)"""
    err_s = abs(g["s"] - r["s"]) / abs(r["s"]) if r["s"] else abs(g["s"])
    top = {k: max(np.abs(r[k]).max(), 1e-300) if len(r[k]) else 1.0 for k in ("local", "switched", "coordination")}
    err = {k: np.abs(g[k] - r[k]).max() / top[k] if len(r[k]) else 0.0 for k in top}
    F_ref = -bias * r["grad"]
    fs = np.abs(F_ref).max() if len(F_ref) else 0.0
    err_f = np.abs(g["F"][:, :3] - F_ref).max() if len(F_ref) else 0.0
    print("s %.15g vs %.15g (%.3e rel); n_i %.3e, t_i %.3e, v_i %.3e of their maxima; forces: max |d| %.3e of max |F| %.3e (%.3e rel)"
          % (g["s"], r["s"], err_s, err["coordination"], err["local"], err["switched"], err_f, fs, err_f / fs if fs else 0.0))
    for k in ("F", "local", "switched", "coordination"):
        assert np.isfinite(g[k]).all(), k
    assert np.isfinite(g["s"])
    assert g["sums"][1] == r["n_t"]
    assert err_s <= 1e-9 and err["coordination"] <= 1e-9 and err["local"] <= 1e-9 and err["switched"] <= 1e-9
    tol = 1e-9 if dtype == np.float64 else 2e-7
    if forces:
        assert fs > 0
    assert err_f <= tol * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        other = types != par["type"]
        assert np.all(g["F"][other] == 0.0)
        assert np.all(g["local"][other] == 0.0) and np.all(g["switched"][other] == 0.0) and np.all(g["coordination"][other] == 0.0)
    if g["virial"] is not None:
        top_w = np.abs(r["virial"]).max() if len(r["virial"]) else 0.0
        err_w = np.abs(g["virial"] - r["virial"]).max() if len(r["virial"]) else 0.0
        W, W_ref = g["virial"].sum(axis=0), r["virial"].sum(axis=0)
        err_sum = np.abs(W - W_ref).max() / np.abs(W_ref).max() if top_w else np.abs(W).max()
        print("virial: max |d| %.3e of max |virial_i| %.3e (%.3e rel); sums %.3e rel" % (err_w, top_w, err_w / top_w if top_w else 0.0, err_sum))
        if forces:
            assert top_w > 0
        assert err_w <= tol * top_w
        assert err_sum <= tol                                          # (fp32: every stored row errs by 2^-24 of itself at most)
        if types is not None:
            assert np.all(g["virial"][types != par["type"]] == 0.0)


_snapshots = {}


def snapshot(lattice, dtype):
    """noisy diamond 3^3 (216 particles) or noisy fcc 3^3 (108), rounded to the dtype, every fourth particle of another type, the list to
    the end of the window; built once, never changed"""
    key = (lattice, np.dtype(dtype).name)
    if key not in _snapshots:
        pos, L = noisy(lattice, 3)
        pos = pos.astype(dtype).astype(np.float64)                       # the snapshot is the rounded array
        types = (np.arange(len(pos)) % 4 == 3).astype(np.int32)
        _snapshots[key] = dict(pos=pos, L=L, types=types, nl=util.build_nlist(pos, L, LATTICES[lattice]["r_cut"]), ref={})
    return _snapshots[key]


def reference(s, par, name, bias=0.9, tilt=None):
    """the restatement's answer for a snapshot and an option set, computed once and shared"""
    key = (name, bias)
    if key not in s["ref"]:
        s["ref"][key] = tr.compute(s["pos"], s["types"], s["L"], s["nl"], par, bias=bias, tilt=tilt)
        condition(s["ref"][key], par)
    return s["ref"][key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", OPTION_SETS)
@pytest.mark.parametrize("lattice", ["diamond", "fcc"])
def test_tetrahedral_parity(abi, lattice, name, dtype):
    s = snapshot(lattice, dtype)
    assert len(s["pos"]) == (216 if lattice == "diamond" else 108)
    par = params(lattice, name)
    r = reference(s, par, name)
    assert r["n_t"] == len(s["pos"]) * 3 // 4
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, dtype, virial=True)
    compare(g, r, 0.9, dtype, types=s["types"], par=par)
    plain = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, dtype)
    assert np.array_equal(plain["F"], g["F"])                           # the call with a virial writes the plain call's force array, bit for bit
    for key in ("s", "local", "switched", "coordination"):
        assert np.array_equal(plain[key], g[key]), key
    again = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, dtype, virial=True)
    for key in OUTPUTS:
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits
    fs, N = np.abs(g["F"]).max(), len(s["pos"])
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N
    # the virial's sum is symmetric although a particle's own six are not those of a symmetric matrix: xy against the restatement's
    # holds that already; here the lattice values the noise leaves in sight
    t = g["local"][s["types"] == 0]
    if name == "plain":
        print("mean t_i %.4f" % t.mean())
        assert (t.mean() > 0.7) if lattice == "diamond" else (0.1 < t.mean() < 0.45)


@pytest.mark.parametrize("lattice,want", [("diamond", 1.0), ("fcc", 3.0 / 11.0)])
def test_perfect_lattices(abi, lattice, want):
    """first shell inside r_on: t_i = 1 (diamond, A_i = 0) and 3/11 (fcc) on the device, no force"""
    pos, L = tr.diamond_lattice(3) if lattice == "diamond" else util.fcc_lattice(3)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.25)
    par = tr.params(0, 1.25, 1.1)
    g = run_gpu(abi, pos, types, L, nl, par, np.float64, virial=True)
    print("%s: t_i in [%.15f, %.15f], s %.15f, max |F| %.3e" % (lattice, g["local"].min(), g["local"].max(), g["s"], np.abs(g["F"]).max()))
    assert np.abs(g["local"] - want).max() <= 1e-9 and abs(g["s"] - want) <= 1e-9
    assert np.all(g["coordination"] == (4.0 if lattice == "diamond" else 12.0))
    assert np.abs(g["F"]).max() <= 1e-9
    pen = run_gpu(abi, pos, types, L, nl, tr.params(0, 1.25, 1.1, normalise=False), np.float64)
    want_a = (1.0 - want) * (6.0 if lattice == "diamond" else 66.0) * 4.0 / 9.0      # A = (1 - t) W / kappa, W = n (n - 1) / 2
    assert np.abs(pen["local"] - want_a).max() <= 1e-9 * max(want_a, 1.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", OPTION_SETS)
def test_triclinic_box(abi, dtype, name):
    """a sheared diamond crystal in the sheared box: HOOMD's minimum image with tilt factors"""
    pos, L = noisy("diamond", 3, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = (np.arange(len(pos)) % 4 == 3).astype(np.int32)
    key = ("tilted", np.dtype(dtype).name)
    if key not in _snapshots:
        _snapshots[key] = brute_nlist(pos, h, LATTICES["diamond"]["r_cut"] + 0.05)
    nl = _snapshots[key]
    par = params("diamond", name)
    r = tr.compute(pos, types, L, nl, par, tilt=tilt, bias=0.9)
    condition(r, par)
    g = run_gpu(abi, pos, types, L, nl, par, dtype, tilt=tilt, virial=True)
    compare(g, r, 0.9, dtype, types=types, par=par)


@pytest.mark.parametrize("name", ["plain", "switch+gate", "penalty"])
def test_bias_from_device_and_host(abi, name):
    s = snapshot("diamond", np.float64)
    par = params("diamond", name)
    dev = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=-1.7, bias_on_device=True, virial=True)
    host = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=-1.7, bias_on_device=False, virial=True)
    assert np.array_equal(dev["F"], host["F"]) and np.array_equal(dev["virial"], host["virial"])
    compare(dev, reference(s, par, name, bias=-1.7), -1.7, np.float64, types=s["types"], par=par)
    zero = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=0.0, bias_on_device=False, virial=True)
    assert np.all(zero["F"] == 0.0) and np.all(zero["virial"] == 0.0)


def test_the_other_type_as_the_variable(abi):
    """type 1 on a random 40 % of the diamond sites: rows of 0, 1, 2, 3 and 4 partners — t_i = 0 with no or one, exactly"""
    s = snapshot("diamond", np.float64)
    types = (np.random.default_rng(3).random(len(s["pos"])) < 0.4).astype(np.int32)
    for name in ("plain", "switch+gate", "penalty"):
        par = params("diamond", name, type_id=1)
        r = tr.compute(s["pos"], types, s["L"], s["nl"], par, bias=0.9)
        condition(r, par)
        partners = np.bincount(r["entries"]["i"], minlength=len(types))[types == 1]
        assert r["n_t"] == (types == 1).sum() and all((partners == k).sum() >= 3 for k in range(5)), np.bincount(partners)
        g = run_gpu(abi, s["pos"], types, s["L"], s["nl"], par, np.float64, virial=True)
        compare(g, r, 0.9, np.float64, types=types, par=par)
        alone = np.bincount(r["entries"]["i"], minlength=len(types)) <= 1
        if name != "penalty":
            assert np.all(g["local"][alone] == 0.0) and np.all(g["switched"][alone] == 0.0)
        else:
            assert np.abs(g["local"][alone]).max() <= 1e-14               # (the moment form of one neighbour: the rounding of f^2 (u.u)^2 - f^2)


def test_list_beyond_the_cutoff(abi):
    """a list that reaches 1.7 gives what the list cut at r_cut gives: entries beyond the cut-off are skipped"""
    s = snapshot("diamond", np.float64)
    wide = util.build_nlist(s["pos"], s["L"], 1.7)
    assert len(wide[2]) > 1.3 * len(s["nl"][2])
    for name in ("plain", "penalty"):
        par = params("diamond", name)
        a = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, virial=True)
        b = run_gpu(abi, s["pos"], s["types"], s["L"], wide, par, np.float64, virial=True)
        compare(b, reference(s, par, name), 0.9, np.float64, types=s["types"], par=par)
        fs = np.abs(a["F"]).max()
        assert abs(a["s"] - b["s"]) <= 1e-12 * abs(a["s"]) and np.abs(a["F"] - b["F"]).max() <= 1e-12 * fs
        assert np.abs(a["virial"] - b["virial"]).max() <= 1e-12 * np.abs(a["virial"]).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_empty_list_no_particles_and_ghosts(abi, dtype):
    """rows that are all empty, and entries that all lie beyond r_cut: n_i = t_i = v_i = 0, s = 0, N_t counted, forces exactly 0; no
    particle of the type: everything 0; no particle at all: success, s = 0; ghosts: refused"""
    pos = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0], [4.0, 4.0, 4.0]])
    types = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    L = 20.0
    for r_list in (2.0, 6.0):
        nl = util.build_nlist(pos, L, r_list)
        assert (len(nl[2]) == 0) == (r_list == 2.0)
        for name in OPTION_SETS:
            g = run_gpu(abi, pos, types, L, nl, params("diamond", name), dtype, virial=True)
            assert g["s"] == 0.0 and g["sums"][1] == 3 and np.all(g["local"] == 0.0) and np.all(g["switched"] == 0.0)
            assert np.all(g["coordination"] == 0.0) and np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
            g = run_gpu(abi, pos, types, L, nl, params("diamond", name, type_id=2), dtype, virial=True)      # no particle of the type
            assert g["s"] == 0.0 and np.all(g["sums"] == 0.0) and np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    for name in OPTION_SETS:
        g = run_gpu(abi, np.zeros((0, 3)), np.zeros(0, dtype=np.int32), L, empty, params("diamond", name), dtype, virial=True)
        assert g["s"] == 0.0 and np.all(g["sums"] == 0.0)
    nl = util.build_nlist(pos, L, 6.0)
    assert run_gpu(abi, pos, types, L, (nl[0][:3], nl[1][:3], nl[2]), params("diamond", "plain"), dtype, n_ghost=2, expect=UNSUPPORTED) is None


@pytest.mark.parametrize("dtype,name", [(np.float64, "plain"), (np.float32, "plain"), (np.float64, "switch+gate"), (np.float64, "penalty")])
def test_chunk_loop(abi, dtype, name):
    """fcc 21 (N = 37 044): 1158 chunks of 32 on 1024 blocks, so blocks 0 - 133 walk two chunks.  The list reaches the first shell only
    (~12 entries per row): the restatement stays cheap.  A second type on ~30 % of the particles, also inside the second-trip chunks"""
    pos, L = noisy("fcc", 21, sigma=0.05, seed=1)
    N = len(pos)
    n_chunks = (N + 31) // 32
    assert N == 37044 and n_chunks > 1024 and n_chunks < 2 * 1024
    pos = pos.astype(dtype).astype(np.float64)                          # the snapshot is the rounded array
    types = (np.random.default_rng(4).random(N) < 0.3).astype(np.int32)
    par = params("fcc", name)
    key = ("chunks", np.dtype(dtype).name)
    if key not in _snapshots:
        _snapshots[key] = util.build_nlist(pos, L, LATTICES["fcc"]["r_cut"])
    nl = _snapshots[key]
    assert 10 < len(nl[2]) / N < 15
    r = tr.compute(pos, types, L, nl, par, bias=0.9)
    condition(r, par)
    assert 0.6 * N < r["n_t"] < 0.8 * N and (types[1024 * 32:] == 1).sum() > 100       # the other type inside the second-trip chunks
    g = run_gpu(abi, pos, types, L, nl, par, dtype, virial=True)
    compare(g, r, 0.9, dtype, types=types, par=par)
    again = run_gpu(abi, pos, types, L, nl, par, dtype, virial=True)
    for key in OUTPUTS:
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits
    fs = np.abs(g["F"]).max()
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N
