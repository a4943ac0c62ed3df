"""GPU parity: the bond-orientational order (mtd_hex_*, csrc/hexatic.hip) through the C ABI against the fp64 numpy restatement of its
definition (tests/hexatic_ref.py: explicit complex sums per row, the closed-form gradient in the scatter form, itself checked on the
CPU in tests/test_hexatic_ref.py).  The kernels gather both ends of an entry with the parity of z^k: the parity holds that identity too.

Tolerances, the project's for this arithmetic: value 1e-9 relative; n_i, c_i, v_i and psi_i 1e-9 of their maximum; forces and
per-particle virial 1e-9 of their maximum with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store); virial sums to the same.
Snapshots are rounded to the array type first.  Every figure is printed before it is asserted.

Condition on the inputs, asserted on the restatement before any GPU call (condition()): every n_i is 0 or >= 1e-3 — psi_i is a quotient
by n_i — and no distance lies within 1e-9 of r_on or r_cut, where the rounding of r decides whether an entry counts.

Snapshots: a noisy triangular monolayer (12 x 12 = 144 particles in the box (12, 6 sqrt 3, 4), window 0.9 .. 1.35, k = 6) and noisy
fcc (n = 3, 108 particles, window 0.9 .. 1.25, k = 4 and 6 about each of the three axes: out-of-plane bonds), noise 0.05, seed 777,
every fourth particle of another type.

test_chunk_loop: a 182 x 182 monolayer, N = 33 124, is the smallest even-sided square layer whose 1036 chunks of 32 central particles
exceed the 1024 blocks the launches are capped at, so blocks 0 - 11 walk two chunks.
"""
import ctypes as C

import numpy as np
import pytest

import hexatic_ref as hr
import stream_gate
import util
from test_gpu_ql_local import brute_nlist

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OUTPUTS = ("s", "sums", "local", "switched", "coordination", "psi", "Psi", "F", "virial")
UNSUPPORTED = -2
SNAPSHOTS = {
    "layer": dict(r_on=0.9, r_cut=1.35, switch=(0.5, 4), gate=(2.0, 5.0)),
    "fcc": dict(r_on=0.9, r_cut=1.25, switch=(0.03, 2), gate=(5.0, 9.0)),
}
OPTION_SETS = ("plain", "switch", "gate", "switch+gate", "global", "k=1")


def params(snap, name, type_id=0, k=None, axis="z"):
    w = SNAPSHOTS[snap]
    opt = {"plain": dict(), "switch": dict(switch=w["switch"]), "gate": dict(gate=w["gate"]),
           "switch+gate": dict(switch=w["switch"], gate=w["gate"]), "global": dict(global_order=True), "k=1": dict(k=1)}[name]
    opt.setdefault("k", k if k is not None else (6 if snap == "layer" else 4))
    return hr.params(type_id, w["r_cut"], w["r_on"], axis=axis, **opt)


def run_gpu(abi, pos, types, L, nl, par, dtype, bias=0.9, tilt=None, bias_on_device=True, virial=False, n_ghost=0, gate=None, expect=0):
    """returns dict(s, sums, local, switched, coordination, psi, Psi, F, virial); par: hexatic_ref.params(...); gate: the stream the calls
    run on and how their inputs arrive (tests/stream_gate.py; None: the NULL stream); expect: the status mtd_hex_accumulate must return
    (then nothing else is launched and None comes back)"""
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
    scratch = torch.zeros(lib.mtd_hex_scratch_doubles(N), dtype=torch.float64, device="cuda")
    force = torch.full((max(N, 1), 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda") if virial else None
    cpar = abi.HexParams.make(par["type"], par["r_cut"], par["r_on"], k=par["k"], axis=par["axis"], global_order=par["global_order"],
                              switch=par["switch"], gate=par["gate"])
    p_sums, p_value, p_local, p_switched, p_coord, p_psi = (C.c_void_p() for _ in range(6))
    n_sums = C.c_uint()
    stream = gate.arm()
    call = abi.HexCall(N, n_ghost, abi.ptr(d_pos) if len(pos) else None, dt, C.pointer(box), abi.ptr(d_head) if N else None,
                       abi.ptr(d_nn) if N else None, abi.ptr(d_nl), abi.ptr(scratch), stream)
    rc = lib.mtd_hex_accumulate(C.byref(cpar), C.byref(call), C.byref(p_sums), C.byref(n_sums))
    if expect:
        assert rc == expect
        assert lib.mtd_hex_forces(C.byref(cpar), C.byref(call), abi.ptr(force), None, bias, None, 0) == expect
        return gate.done(lambda: (scratch.cpu().numpy(), force.cpu().numpy()))
    abi.check(rc)
    assert n_sums.value == 4
    abi.check(lib.mtd_hex_finalize(C.byref(cpar), C.byref(call), C.byref(p_value), C.byref(p_local), C.byref(p_switched), C.byref(p_coord),
                                   C.byref(p_psi)))
    abi.check(lib.mtd_hex_forces(C.byref(cpar), C.byref(call), abi.ptr(force), abi.ptr(d_bias) if bias_on_device else None,
                                 0.0 if bias_on_device else bias, abi.ptr(vir) if virial else None, pitch if virial else 0))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        per = lambda p: s[off(p):off(p) + N].copy()
        psi = s[off(p_psi):off(p_psi) + 2 * N].reshape(N, 2)
        value = s[off(p_value):off(p_value) + 4]
        out = dict(s=float(value[0]), sums=s[off(p_sums):off(p_sums) + 4].copy(), local=per(p_local), switched=per(p_switched),
                   coordination=per(p_coord), psi=psi[:, 0] + 1j * psi[:, 1], Psi=complex(value[2], value[3]),
                   F=force.cpu().numpy().astype(np.float64)[:N], virial=None)
        assert value[1] == out["sums"][1]                                 # N_t behind the value
        if virial:
            v = vir.cpu().numpy().astype(np.float64)
            assert np.all(v[:, N:] == 7.0)                                  # [n_particles, pitch) is left alone
            out["virial"] = v[:, :N].T.copy()
        return out
    return gate.done(read)


def noisy(snap, n, sigma=0.05, seed=777):
    """layer: n x n particles in the box (n, n sqrt(3) / 2, 4); fcc: n^3 cells in the cubic box"""
    pos, L = hr.triangular_layer(n, n) if snap == "layer" else util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


def condition(r, par):
    """what the tolerances presuppose (module docstring), asserted on the restatement's result"""
    n = r["coordination"]
    assert np.all((n == 0.0) | (n >= 1e-3)), n[(n != 0.0) & (n < 1e-3)]
    if len(r["r"]):
        assert np.abs(r["r"] - par["r_on"]).min() > 1e-9 and np.abs(r["r"] - par["r_cut"]).min() > 1e-9


def compare(g, r, bias, dtype, types=None, par=None, forces=True):
    """prints every figure, then asserts; r: the restatement's result (its virial formed with the same bias)"""
    err_s = abs(g["s"] - r["s"]) / abs(r["s"]) if r["s"] else abs(g["s"])
    top = {k: max(np.abs(r[k]).max(), 1e-300) if len(r[k]) else 1.0 for k in ("local", "switched", "coordination", "psi")}
    err = {k: np.abs(g[k] - r[k]).max() / top[k] if len(r[k]) else 0.0 for k in top}
    err_P = abs(g["Psi"] - r["Psi"]) / top["psi"]
    F_ref = -bias * r["grad"]
    fs = np.abs(F_ref).max() if len(F_ref) else 0.0
    err_f = np.abs(g["F"][:, :3] - F_ref).max() if len(F_ref) else 0.0
    print("s %.15g vs %.15g (%.3e rel); n_i %.3e, c_i %.3e, v_i %.3e, psi_i %.3e of their maxima, Psi %.3e; forces: max |d| %.3e of max |F| "
          "%.3e (%.3e rel)" % (g["s"], r["s"], err_s, err["coordination"], err["local"], err["switched"], err["psi"], err_P, err_f, fs,
                               err_f / fs if fs else 0.0))
    for k in ("F", "local", "switched", "coordination", "psi"):
        assert np.isfinite(g[k]).all(), k
    assert np.isfinite(g["s"])
    assert g["sums"][1] == r["n_t"]
    sums_top = max(np.abs(r["sums"]).max(), 1.0)
    assert np.abs(g["sums"] - r["sums"]).max() <= 1e-9 * sums_top
    assert err_s <= 1e-9 and err["coordination"] <= 1e-9 and err["local"] <= 1e-9 and err["switched"] <= 1e-9 and err["psi"] <= 1e-9
    assert err_P <= 1e-9
    tol = 1e-9 if dtype == np.float64 else 2e-7
    if forces:
        assert fs > 0
    assert err_f <= tol * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        other = types != par["type"]
        assert np.all(g["F"][other] == 0.0) and np.all(g["psi"][other] == 0.0)
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


def snapshot(snap, dtype):
    """the noisy monolayer 12 x 12 (144 particles) or noisy fcc 3^3 (108), rounded to the dtype, every fourth particle of another type,
    the list to the end of the window; built once, never changed"""
    key = (snap, np.dtype(dtype).name)
    if key not in _snapshots:
        pos, L = noisy(snap, 12 if snap == "layer" else 3)
        pos = pos.astype(dtype).astype(np.float64)                       # the snapshot is the rounded array
        types = (np.arange(len(pos)) % 4 == 3).astype(np.int32)
        _snapshots[key] = dict(pos=pos, L=L, types=types, nl=hr.box_nlist(pos, L, SNAPSHOTS[snap]["r_cut"]), ref={})
    return _snapshots[key]


def reference(s, par, name, bias=0.9, tilt=None):
    """the restatement's answer for a snapshot and an option set, computed once and shared"""
    key = (name, par["k"], par["axis"], bias)
    if key not in s["ref"]:
        s["ref"][key] = hr.compute(s["pos"], s["types"], s["L"], s["nl"], par, bias=bias, tilt=tilt)
        condition(s["ref"][key], par)
    return s["ref"][key]


def _parity(abi, s, par, name, dtype):
    r = reference(s, par, name)
    assert r["n_t"] == len(s["pos"]) * 3 // 4
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, dtype, virial=True)
    compare(g, r, 0.9, dtype, types=s["types"], par=par)
    plain = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, dtype)
    assert np.array_equal(plain["F"], g["F"])                           # the call with a virial writes the plain call's force array, bit for bit
    for key in ("s", "local", "switched", "coordination", "psi", "Psi"):
        assert np.array_equal(plain[key], g[key]), key
    again = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, dtype, virial=True)
    for key in OUTPUTS:
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits
    fs, N = np.abs(g["F"]).max(), len(s["pos"])
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N
    return g


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", OPTION_SETS)
def test_monolayer_parity(abi, name, dtype):
    s = snapshot("layer", dtype)
    assert len(s["pos"]) == 144 and np.allclose(s["L"], [12.0, 6.0 * np.sqrt(3.0), 4.0])
    par = params("layer", name)
    g = _parity(abi, s, par, name, dtype)
    c = g["local"][s["types"] == 0]
    if name == "plain":
        print("mean c_i %.4f" % c.mean())
        assert c.mean() > 0.3                                            # the hexagonal order the noise leaves in sight
    if name == "global":
        assert g["s"] > 0.3 and np.array_equal(g["local"], g["switched"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("axis", ["x", "y", "z"])
@pytest.mark.parametrize("k", [4, 6])
@pytest.mark.parametrize("name", ["plain", "switch+gate", "global"])
def test_fcc_parity_about_each_axis(abi, name, k, axis, dtype):
    """out-of-plane bonds about every axis: the sectoral weight and the gradient terms along e_u, e_v and d"""
    s = snapshot("fcc", dtype)
    assert len(s["pos"]) == 108
    par = params("fcc", name, k=k, axis=axis)
    _parity(abi, s, par, name, dtype)


def test_perfect_lattices(abi):
    """first shell inside r_on: c_i = 1 and |Psi|^2 = 1 on the monolayer with k = 6, 0 with k = 3; psi_i = -1/6 and s = 1/36 on fcc with
    k = 4 about every axis, in both modes; no force"""
    pos, L = hr.triangular_layer(12, 12)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = hr.box_nlist(pos, L, 1.2)
    for glob in (False, True):
        g = run_gpu(abi, pos, types, L, nl, hr.params(0, 1.2, 1.1, k=6, global_order=glob), np.float64, virial=True)
        print("layer, global %d: c_i in [%.15f, %.15f], s %.15f, max |F| %.3e" % (glob, g["local"].min(), g["local"].max(), g["s"],
                                                                                 np.abs(g["F"]).max()))
        assert np.abs(g["local"] - 1.0).max() <= 1e-9 and abs(g["s"] - 1.0) <= 1e-9 and abs(g["Psi"] - 1.0) <= 1e-9
        assert np.all(g["coordination"] == 6.0) and np.abs(g["F"]).max() <= 1e-9
        g = run_gpu(abi, pos, types, L, nl, hr.params(0, 1.2, 1.1, k=3, global_order=glob), np.float64)
        assert np.abs(g["local"]).max() <= 1e-9 and abs(g["s"]) <= 1e-9
    pos, L = util.fcc_lattice(3)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.25)
    for axis in "xyz":
        for glob in (False, True):
            g = run_gpu(abi, pos, types, L, nl, hr.params(0, 1.25, 1.1, k=4, axis=axis, global_order=glob), np.float64, virial=True)
            print("fcc about %s, global %d: psi_0 %r, s %.15f" % (axis, glob, g["psi"][0], g["s"]))
            assert np.abs(g["psi"] + 1.0 / 6.0).max() <= 1e-9 and abs(g["s"] - 1.0 / 36.0) <= 1e-9 * (1.0 / 36.0)
            assert np.all(g["coordination"] == 12.0) and np.abs(g["F"]).max() <= 1e-9


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", OPTION_SETS)
def test_triclinic_box(abi, dtype, name):
    """a sheared fcc crystal in the sheared box: HOOMD's minimum image with tilt factors; brute-force list"""
    pos, L = noisy("fcc", 3, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = (np.arange(len(pos)) % 4 == 3).astype(np.int32)
    key = ("tilted", np.dtype(dtype).name)
    if key not in _snapshots:
        _snapshots[key] = brute_nlist(pos, h, SNAPSHOTS["fcc"]["r_cut"] + 0.05)
    nl = _snapshots[key]
    par = params("fcc", name)
    r = hr.compute(pos, types, L, nl, par, tilt=tilt, bias=0.9)
    condition(r, par)
    g = run_gpu(abi, pos, types, L, nl, par, dtype, tilt=tilt, virial=True)
    compare(g, r, 0.9, dtype, types=types, par=par)


@pytest.mark.parametrize("name", ["plain", "switch+gate", "global"])
def test_bias_from_device_and_host(abi, name):
    s = snapshot("layer", np.float64)
    par = params("layer", name)
    dev = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=-1.7, bias_on_device=True, virial=True)
    host = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=-1.7, bias_on_device=False, virial=True)
    assert np.array_equal(dev["F"], host["F"]) and np.array_equal(dev["virial"], host["virial"])
    compare(dev, reference(s, par, name, bias=-1.7), -1.7, np.float64, types=s["types"], par=par)
    zero = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], par, np.float64, bias=0.0, bias_on_device=False, virial=True)
    assert np.all(zero["F"] == 0.0) and np.all(zero["virial"] == 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pair_exactly_along_the_axis(abi, dtype):
    """two particles exactly along the axis: B = 0 for k >= 2, an ordinary point — finite everything, psi = 0, zero force and virial;
    k = 1: psi = 0 as well (z = 0) but the gradient is not, and it agrees with the restatement"""
    for axis, e in (("z", [0.0, 0.0, 1.0]), ("x", [1.0, 0.0, 0.0]), ("y", [0.0, 1.0, 0.0])):
        pos = np.array([[0.0, 0.0, 0.0], e])
        types = np.zeros(2, dtype=np.int32)
        nl = util.build_nlist(pos, 20.0, 1.3)
        for k in (2, 3, 6, 12):
            for glob in (False, True):
                par = hr.params(0, 1.3, 0.9, k=k, axis=axis, global_order=glob)
                g = run_gpu(abi, pos, types, 20.0, nl, par, dtype, virial=True)
                for key in ("F", "virial", "psi", "local", "switched", "coordination"):
                    assert np.isfinite(g[key]).all(), (axis, k, key)
                assert np.all(g["psi"] == 0.0) and g["s"] == 0.0 and np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
                assert np.all(g["coordination"] > 0.5)
    # with a third particle in the plane the on-axis entry stays an ordinary term of a non-zero force
    pos = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.953125, 0.203125, 0.109375]])
    types = np.zeros(3, dtype=np.int32)
    nl = util.build_nlist(pos, 20.0, 1.3)
    for k in (1, 2, 6):
        par = hr.params(0, 1.3, 0.9, k=k)
        r = hr.compute(pos, types, 20.0, nl, par, bias=0.9)
        condition(r, par)
        compare(run_gpu(abi, pos, types, 20.0, nl, par, dtype, virial=True), r, 0.9, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_empty_list_no_particles_and_ghosts(abi, dtype):
    """rows that are all empty, and entries that all lie beyond r_cut: n_i = c_i = v_i = 0, s = 0, N_t counted, forces exactly 0; no
    particle of the type: everything 0; no particle at all: success, s = 0; ghosts: MTD_ERR_UNSUPPORTED and nothing launched"""
    pos = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0], [4.0, 4.0, 4.0]])
    types = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    L = 20.0
    for r_list in (2.0, 6.0):
        nl = util.build_nlist(pos, L, r_list)
        assert (len(nl[2]) == 0) == (r_list == 2.0)
        for name in OPTION_SETS:
            g = run_gpu(abi, pos, types, L, nl, params("layer", name), dtype, virial=True)
            assert g["s"] == 0.0 and g["sums"][1] == 3 and np.all(g["local"] == 0.0) and np.all(g["switched"] == 0.0)
            assert np.all(g["psi"] == 0.0) and g["Psi"] == 0.0
            assert np.all(g["coordination"] == 0.0) and np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
            g = run_gpu(abi, pos, types, L, nl, params("layer", name, type_id=2), dtype, virial=True)      # no particle of the type
            assert g["s"] == 0.0 and np.all(g["sums"] == 0.0) and np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    for name in OPTION_SETS:
        g = run_gpu(abi, np.zeros((0, 3)), np.zeros(0, dtype=np.int32), L, empty, params("layer", name), dtype, virial=True)
        assert g["s"] == 0.0 and np.all(g["sums"] == 0.0)
    nl = util.build_nlist(pos, L, 6.0)
    for name in ("plain", "global"):
        scratch, force = run_gpu(abi, pos, types, L, (nl[0][:3], nl[1][:3], nl[2]), params("layer", name), dtype, n_ghost=2, expect=UNSUPPORTED)
        assert np.all(scratch == 0.0) and np.all(force == 3.0)           # nothing was launched: scratch and force array as they were


@pytest.mark.parametrize("dtype,name", [(np.float64, "plain"), (np.float32, "plain"), (np.float64, "global"), (np.float32, "global")])
def test_chunk_loop(abi, dtype, name):
    """a 182 x 182 monolayer (N = 33 124): 1036 chunks of 32 on 1024 blocks, so blocks 0 - 11 walk two chunks.  About six entries per
    row: the restatement stays cheap.  A second type on ~30 % of the particles, also inside the second-trip chunks"""
    pos, L = noisy("layer", 182, sigma=0.05, seed=1)
    N = len(pos)
    n_chunks = (N + 31) // 32
    assert N == 33124 and n_chunks == 1036 and ((180 * 180 + 31) // 32) <= 1024
    pos = pos.astype(dtype).astype(np.float64)                          # the snapshot is the rounded array
    types = (np.random.default_rng(4).random(N) < 0.3).astype(np.int32)
    par = params("layer", name)
    key = ("chunks", np.dtype(dtype).name)
    if key not in _snapshots:
        nl = hr.box_nlist(pos, L, SNAPSHOTS["layer"]["r_cut"])
        r = {}
        _snapshots[key] = (nl, r)
    nl, refs = _snapshots[key]
    assert 5 < len(nl[2]) / N < 8
    if name not in refs:
        refs[name] = hr.compute(pos, types, L, nl, par, bias=0.9)
    r = refs[name]
    condition(r, par)
    assert 0.6 * N < r["n_t"] < 0.8 * N and (types[1024 * 32:] == 1).sum() > 50        # the other type inside the second-trip chunks
    g = run_gpu(abi, pos, types, L, nl, par, dtype, virial=True)
    compare(g, r, 0.9, dtype, types=types, par=par)
    again = run_gpu(abi, pos, types, L, nl, par, dtype, virial=True)
    for key in OUTPUTS:
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits
    fs = np.abs(g["F"]).max()
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N
