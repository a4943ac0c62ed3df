"""GPU parity: the Debye structure factor (mtd_dsf_*, csrc/debye.hip) through the C ABI against the fp64 numpy restatement of its
definition (tests/debye_ref.py, itself checked on the CPU in tests/test_debye_ref.py).

Tolerances, the project's for this arithmetic: value and I_p 1e-9 relative; forces and per-particle virial 1e-9 of their maximum with
fp64 arrays and 2e-7 with fp32 arrays (one rounding on store); the spectrum 1e-10 of its maximum at n_q = 1, 64 and 256.  Every figure is
printed before it is asserted.  Both routes of the force call are held to them: the default (the first pass stores every particle's
gradient and virial sums, the force call scales them) and the second walk (mtd_dsf_set_store_gradient(0)).

test_chunk_loop: N = 37 044 is the smallest fcc crystal whose 1158 chunks of 32 central particles exceed the 1024 blocks the launches are
capped at, so blocks 0 - 133 walk two chunks.
"""
import ctypes as C

import numpy as np
import pytest

import debye_ref as dsf
import stream_gate
import util
from test_gpu_ql_local import brute_nlist

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

Q111, Q200 = 7.695, 8.886
PEAKS = {1: ((Q111,), (1.0,)),
         3: ((Q111, Q200, 12.57), (1.0, -0.5, 0.25)),
         8: ((Q111, Q200, 12.57, 14.74, 3.1, 5.2, 17.77, 10.4), (1.0, -0.5, 0.25, 0.3, -0.2, 0.1, 0.7, -1.1))}
OUTPUTS = ("s", "I", "sums", "local", "F", "virial")


def run_gpu(abi, pos, types, L, nl, q, c, r_cut, type_id, dtype, bias=0.9, tilt=None, bias_on_device=True, virial=False, n_rows=None, gate=None,
            spectrum=None, store=True):
    """returns dict(s, I, sums, local, F, virial[, spectrum, spectrum_sums]); n_rows: the first n_rows particles are the central ones, the
    others ghosts; gate: the stream the calls run on and how their inputs arrive (tests/stream_gate.py; None: the NULL stream);
    spectrum: (q_min, q_max, n_q) runs the two spectrum calls behind the step; store: the route of the force call"""
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
    scratch = torch.zeros(lib.mtd_dsf_scratch_doubles(N), dtype=torch.float64, device="cuda")
    force = torch.full((max(N, 1), 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda") if virial else None
    par = abi.DsfParams.make(type_id, r_cut, q, c=c)
    P = len(q)
    p_sums, p_value, p_I, p_local, p_ssums, p_spec = (C.c_void_p() for _ in range(6))
    n_sums, n_ssums = C.c_uint(), C.c_uint()
    stream = gate.arm()
    call = abi.DsfCall(N, len(pos) - N, abi.ptr(d_pos) if len(pos) else None, dt, C.pointer(box), abi.ptr(d_head) if N else None,
                       abi.ptr(d_nn) if N else None, abi.ptr(d_nl), abi.ptr(scratch), stream)
    abi.check(lib.mtd_dsf_set_store_gradient(1 if store else 0))
    try:
        abi.check(lib.mtd_dsf_accumulate(C.byref(par), C.byref(call), C.byref(p_sums), C.byref(n_sums)))
        assert n_sums.value == P + 1
        abi.check(lib.mtd_dsf_finalize(C.byref(par), C.byref(call), C.byref(p_value), C.byref(p_I), C.byref(p_local)))
        abi.check(lib.mtd_dsf_forces(C.byref(par), C.byref(call), abi.ptr(force), abi.ptr(d_bias) if bias_on_device else None,
                                     0.0 if bias_on_device else bias, abi.ptr(vir) if virial else None, pitch if virial else 0))
        if spectrum is not None:
            abi.check(lib.mtd_dsf_spectrum(C.byref(par), C.byref(call), spectrum[0], spectrum[1], spectrum[2], C.byref(p_ssums), C.byref(n_ssums)))
            assert n_ssums.value == spectrum[2] + 1
            abi.check(lib.mtd_dsf_spectrum_finalize(C.byref(call), spectrum[0], spectrum[1], spectrum[2], C.byref(p_spec)))
    finally:
        abi.check(lib.mtd_dsf_set_store_gradient(1))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        out = dict(s=float(s[off(p_value)]), I=s[off(p_I):off(p_I) + P].copy(), sums=s[off(p_sums):off(p_sums) + P + 1].copy(),
                   local=s[off(p_local):off(p_local) + N].copy(), F=force.cpu().numpy().astype(np.float64)[:N], virial=None)
        if virial:
            v = vir.cpu().numpy().astype(np.float64)
            assert np.all(v[:, N:] == 7.0)                                  # [n_particles, pitch) is left alone
            out["virial"] = v[:, :N].T.copy()
        if spectrum is not None:
            out["spectrum"] = s[off(p_spec):off(p_spec) + spectrum[2]].copy()
            out["spectrum_sums"] = s[off(p_ssums):off(p_ssums) + spectrum[2] + 1].copy()
        return out
    return gate.done(read)


def noisy_fcc(n, sigma=0.05, seed=777):
    pos, L = util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


def compare(g, r, bias, dtype, types=None, type_id=0):
    """prints every figure, then asserts; r: the restatement's result (its virial formed with the same bias)"""
    n_rows = len(g["F"])
    err_s = abs(g["s"] - r["s"]) / abs(r["s"]) if r["s"] else abs(g["s"])
    err_i = (np.abs(g["I"] - r["I"]) / np.where(r["I"] != 0, np.abs(r["I"]), 1.0)).max()
    top_l = max(np.abs(r["local"]).max(), 1e-300)
    err_l = np.abs(g["local"] - r["local"][:n_rows]).max() / top_l
    F_ref = -bias * r["gather"][:n_rows]
    fs = np.abs(F_ref).max()
    err_f = np.abs(g["F"][:, :3] - F_ref).max()
    print("s %.15g vs %.15g (%.3e rel); I_p %.3e rel; s_i %.3e of max; forces: max |d| %.3e of max |F| %.3e (%.3e rel)"
          % (g["s"], r["s"], err_s, err_i, err_l, err_f, fs, err_f / fs if fs else 0.0))
    assert np.isfinite(g["F"]).all() and np.isfinite(g["I"]).all() and np.isfinite(g["s"]) and np.isfinite(g["local"]).all()
    assert g["sums"][-1] == r["n_t"]
    assert err_s <= 1e-9 and err_i <= 1e-9 and err_l <= 1e-9
    tol = 1e-9 if dtype == np.float64 else 2e-7
    assert fs > 0
    assert err_f <= tol * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        assert np.all(g["F"][types[:n_rows] != type_id] == 0.0) and np.all(g["local"][types[:n_rows] != type_id] == 0.0)
    if g["virial"] is not None:
        top_v = np.abs(r["virial"]).max()
        err_v = np.abs(g["virial"] - r["virial"][:n_rows]).max()
        W, W_ref = g["virial"].sum(axis=0), r["virial"][:n_rows].sum(axis=0)
        err_w = np.abs(W - W_ref).max() / np.abs(W_ref).max()
        print("virial: max |d| %.3e of max |virial_i| %.3e (%.3e rel); sums %.3e rel" % (err_v, top_v, err_v / top_v, err_w))
        assert top_v > 0 and err_v <= tol * top_v
        assert err_w <= tol                                            # (fp32: every stored row errs by 2^-24 of itself at most)
        if types is not None:
            assert np.all(g["virial"][types[:n_rows] != type_id] == 0.0)


@pytest.fixture(scope="module")
def snapshots():
    """the common snapshot: fcc 5 (N = 500, not a multiple of 64) with noise 0.05 and 0.13, and the list that reaches 2.4"""
    out = {}
    for noise in (0.05, 0.13):
        pos, L = noisy_fcc(5, sigma=noise)
        out[noise] = dict(pos=pos, L=L, types=np.zeros(len(pos), dtype=np.int32), nl=util.build_nlist(pos, L, 2.4))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("noise", [0.05, 0.13])
@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("store", [True, False])
def test_debye_parity(abi, snapshots, dtype, noise, P, store):
    s = snapshots[noise]
    q, c = PEAKS[P]
    pos = s["pos"].astype(dtype).astype(np.float64)                     # the snapshot is the rounded array
    g = run_gpu(abi, pos, s["types"], s["L"], s["nl"], q, c, 2.4, 0, dtype, virial=True, store=store)
    r = dsf.compute(pos, s["types"], s["L"], s["nl"], q, 2.4, 0, c=c, bias=0.9)
    compare(g, r, 0.9, dtype)
    plain = run_gpu(abi, pos, s["types"], s["L"], s["nl"], q, c, 2.4, 0, dtype, store=store)
    assert np.array_equal(plain["F"], g["F"])                           # the call with a virial writes the plain call's force array, bit for bit
    assert np.array_equal(plain["I"], g["I"]) and plain["s"] == g["s"] and np.array_equal(plain["local"], g["local"])
    again = run_gpu(abi, pos, s["types"], s["L"], s["nl"], q, c, 2.4, 0, dtype, virial=True, store=store)
    for key in OUTPUTS:
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits


def test_debye_known_values(abi, snapshots):
    """the figures of the issue's table: I(Q111), I(Q200) of the noisy crystals"""
    for noise, want in ((0.05, (2.026, 1.546)), (0.13, (1.376, 1.209))):
        s = snapshots[noise]
        g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], (Q111, Q200), (1.0, 1.0), 2.4, 0, np.float64)
        print("noise %.2f: I = %s" % (noise, g["I"]))
        assert g["I"][0] == pytest.approx(want[0], abs=2e-3) and g["I"][1] == pytest.approx(want[1], abs=2e-3)
        assert g["s"] == pytest.approx(g["I"].sum(), rel=1e-14)
        assert g["local"].mean() == pytest.approx(g["s"], rel=1e-12)


def test_both_routes_of_the_force_call_agree(abi, snapshots):
    s = snapshots[0.05]
    q, c = PEAKS[3]
    a = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], q, c, 2.4, 0, np.float64, virial=True, store=True)
    b = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], q, c, 2.4, 0, np.float64, virial=True, store=False)
    assert a["s"] == b["s"] and np.array_equal(a["I"], b["I"]) and np.array_equal(a["local"], b["local"])
    assert np.abs(a["F"] - b["F"]).max() <= 1e-13 * np.abs(a["F"]).max()
    assert np.abs(a["virial"] - b["virial"]).max() <= 1e-13 * np.abs(a["virial"]).max()


@pytest.mark.parametrize("type_id", [0, 1])
def test_debye_two_types(abi, type_id):
    pos, L = noisy_fcc(5, seed=5)
    types = (np.arange(len(pos)) % 2).astype(np.int32)                  # interleaved
    nl = util.build_nlist(pos, L, 2.4)
    q, c = PEAKS[3]
    g = run_gpu(abi, pos, types, L, nl, q, c, 2.4, type_id, np.float64, virial=True)
    r = dsf.compute(pos, types, L, nl, q, 2.4, type_id, c=c, bias=0.9)
    assert r["n_t"] == 250
    compare(g, r, 0.9, np.float64, types=types, type_id=type_id)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("store", [True, False])
def test_debye_rows_fewer_than_positions(abi, dtype, store):
    """the first 300 particles are central, the trailing 200 are ghosts: indexed by the rows, owning none.  What the pass forms is the
    gather over the rows with the sums of the rows"""
    pos, L = noisy_fcc(5, seed=9)
    pos = pos.astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    head, nn, lst = util.build_nlist(pos, L, 2.4)
    n_rows = 300
    nl = (head[:n_rows], nn[:n_rows], lst[:head[n_rows]])
    assert (nl[2] >= n_rows).any()
    q, c = PEAKS[3]
    g = run_gpu(abi, pos, types, L, nl, q, c, 2.4, 0, dtype, virial=True, n_rows=n_rows, store=store)
    r = dsf.compute(pos, types, L, nl, q, 2.4, 0, c=c, bias=0.9)
    assert r["n_t"] == n_rows
    compare(g, r, 0.9, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_debye_triclinic_box(abi, dtype):
    """a sheared fcc crystal in the sheared box: HOOMD's minimum image with tilt factors"""
    pos, L = noisy_fcc(4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    q, c = PEAKS[3]
    nl = brute_nlist(pos, h, 2.05)
    g = run_gpu(abi, pos, types, L, nl, q, c, 2.0, 0, dtype, tilt=tilt, virial=True)
    r = dsf.compute(pos, types, L, nl, q, 2.0, 0, c=c, tilt=tilt, bias=0.9)
    compare(g, r, 0.9, dtype)


def test_debye_list_beyond_the_cutoff(abi):
    """a list that reaches 2.8 gives what the list cut at r_cut = 2.4 gives: entries beyond the cut-off are skipped"""
    pos, L = noisy_fcc(5, seed=9)
    types = (np.random.default_rng(2).random(len(pos)) < 0.15).astype(np.int32)
    q, c = PEAKS[3]
    tight = util.build_nlist(pos, L, 2.4)
    wide = util.build_nlist(pos, L, 2.8)
    assert len(wide[2]) > 1.3 * len(tight[2])
    a = run_gpu(abi, pos, types, L, tight, q, c, 2.4, 0, np.float64, virial=True)
    b = run_gpu(abi, pos, types, L, wide, q, c, 2.4, 0, np.float64, virial=True)
    r = dsf.compute(pos, types, L, wide, q, 2.4, 0, c=c, bias=0.9)
    compare(b, r, 0.9, np.float64, types=types)
    fs = np.abs(a["F"]).max()
    assert abs(a["s"] - b["s"]) <= 1e-12 * abs(a["s"]) and np.abs(a["F"] - b["F"]).max() <= 1e-12 * fs
    assert np.abs(a["virial"] - b["virial"]).max() <= 1e-12 * np.abs(a["virial"]).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_debye_nothing_to_sum(abi, dtype):
    """empty rows and entries that all lie beyond r_cut: I_p = 1, s = sum c_p, forces exactly 0; no particle of the type: all 0;
    no particle at all: success, s = 0"""
    pos = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0], [4.0, 4.0, 4.0]])
    types = np.zeros(len(pos), dtype=np.int32)
    L = 20.0
    q, c = PEAKS[3]
    for r_list in (2.4, 4.5):
        nl = util.build_nlist(pos, L, r_list)
        assert (len(nl[2]) == 0) == (r_list == 2.4)
        for store in (True, False):
            g = run_gpu(abi, pos, types, L, nl, q, c, 2.4, 0, dtype, virial=True, store=store)
            assert np.all(g["I"] == 1.0) and np.all(g["sums"][:-1] == 0.0) and g["sums"][-1] == len(pos)
            assert g["s"] == pytest.approx(sum(c), rel=1e-15) and np.all(g["local"] == pytest.approx(sum(c), rel=1e-15))
            assert np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
    for store in (True, False):
        g = run_gpu(abi, pos, types, L, util.build_nlist(pos, L, 4.5), q, c, 2.4, 1, dtype, virial=True, store=store)
        assert g["s"] == 0.0 and np.all(g["I"] == 0.0) and np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0) and np.all(g["local"] == 0.0)
        empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
        g = run_gpu(abi, np.zeros((0, 3)), np.zeros(0, dtype=np.int32), L, empty, q, c, 2.4, 0, dtype, virial=True, store=store,
                    spectrum=(2.0, 12.0, 9))
        assert g["s"] == 0.0 and np.all(g["I"] == 0.0) and np.all(g["sums"] == 0.0) and np.all(g["spectrum"] == 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("store", [True, False])
def test_debye_coincident_pair(abi, dtype, store):
    """two particles in one place (r = 0 exactly): phi_p = 1, no gradient from that entry, everything finite"""
    pos, L = noisy_fcc(3, seed=4)
    pos = pos.astype(dtype).astype(np.float64)
    pos[40] = pos[7]
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 2.0)
    assert 40 in nl[2][nl[0][7]:nl[0][7] + nl[1][7]]
    q, c = PEAKS[3]
    g = run_gpu(abi, pos, types, L, nl, q, c, 2.0, 0, dtype, virial=True, store=store, spectrum=(2.0, 12.0, 64))
    r = dsf.compute(pos, types, L, nl, q, 2.0, 0, c=c, bias=0.9)
    compare(g, r, 0.9, dtype)
    Q, I = dsf.spectrum(pos, types, L, nl, 2.0, 0, 2.0, 12.0, 64)
    assert np.isfinite(g["spectrum"]).all() and np.abs(g["spectrum"] - I).max() <= 1e-10 * np.abs(I).max()


def test_debye_bias_from_device_and_host(abi, snapshots):
    s = snapshots[0.13]
    q, c = PEAKS[3]
    for store in (True, False):
        dev = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], q, c, 2.4, 0, np.float64, bias=-1.7, bias_on_device=True, virial=True, store=store)
        host = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], q, c, 2.4, 0, np.float64, bias=-1.7, bias_on_device=False, virial=True, store=store)
        assert np.array_equal(dev["F"], host["F"]) and np.array_equal(dev["virial"], host["virial"])
        r = dsf.compute(s["pos"], s["types"], s["L"], s["nl"], q, 2.4, 0, c=c, bias=-1.7)
        compare(dev, r, -1.7, np.float64)
        zero = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], q, c, 2.4, 0, np.float64, bias=0.0, bias_on_device=False, virial=True, store=store)
        assert np.all(zero["F"] == 0.0) and np.all(zero["virial"] == 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_q", [1, 64, 256])
def test_debye_spectrum(abi, snapshots, dtype, n_q):
    s = snapshots[0.05]
    pos = s["pos"].astype(dtype).astype(np.float64)
    q, c = PEAKS[1]
    lo, hi = (Q111, Q111) if n_q == 1 else (1.5, 20.0)
    g = run_gpu(abi, pos, s["types"], s["L"], s["nl"], q, c, 2.4, 0, dtype, spectrum=(lo, hi, n_q))
    Q, I = dsf.spectrum(pos, s["types"], s["L"], s["nl"], 2.4, 0, lo, hi, n_q)
    top = np.abs(I).max()
    err = np.abs(g["spectrum"] - I).max()
    print("spectrum n_q = %d: max |d| %.3e of max I %.3e (%.3e rel)" % (n_q, err, top, err / top))
    assert g["spectrum_sums"][-1] == 500
    assert err <= 1e-10 * top
    if n_q == 1:
        assert abs(g["spectrum"][0] - g["I"][0]) <= 1e-12 * g["I"][0]    # the spectrum at a peak is the peak
    again = run_gpu(abi, pos, s["types"], s["L"], s["nl"], q, c, 2.4, 0, dtype, spectrum=(lo, hi, n_q))
    assert np.array_equal(again["spectrum"], g["spectrum"]) and np.array_equal(again["spectrum_sums"], g["spectrum_sums"])


@pytest.mark.parametrize("dtype,two_types,store", [(np.float64, False, True), (np.float32, False, True), (np.float64, True, True),
                                                   (np.float64, True, False)])
def test_chunk_loop(abi, dtype, two_types, store):
    """fcc 21 (N = 37 044): 1158 chunks of 32 on 1024 blocks, so blocks 0 - 133 walk two chunks.  The list reaches r_cut = 1.5 only (~17
    entries per row): the restatement stays cheap.  With a second type on ~30 % of the particles the type test decides in second-trip
    chunks too"""
    pos, L = noisy_fcc(21, sigma=0.05, seed=1)
    N = len(pos)
    n_chunks = (N + 31) // 32
    assert N == 37044 and n_chunks > 1024 and n_chunks < 2 * 1024
    pos = pos.astype(dtype).astype(np.float64)                          # the snapshot is the rounded array
    types = (np.random.default_rng(4).random(N) < 0.3).astype(np.int32) if two_types else np.zeros(N, dtype=np.int32)
    q, c = PEAKS[3]
    nl = util.build_nlist(pos, L, 1.5)
    assert 15 < len(nl[2]) / N < 20
    g = run_gpu(abi, pos, types, L, nl, q, c, 1.5, 0, dtype, virial=True, store=store, spectrum=(2.0, 12.0, 11))
    r = dsf.compute(pos, types, L, nl, q, 1.5, 0, c=c, bias=0.9)
    if two_types:
        assert 0.6 * N < r["n_t"] < 0.8 * N and (types[1024 * 32:] == 1).sum() > 100      # the other type inside the second-trip chunks
    compare(g, r, 0.9, dtype, types=types if two_types else None)
    Q, I = dsf.spectrum(pos, types, L, nl, 1.5, 0, 2.0, 12.0, 11)
    assert np.abs(g["spectrum"] - I).max() <= 1e-10 * np.abs(I).max()
    again = run_gpu(abi, pos, types, L, nl, q, c, 1.5, 0, dtype, virial=True, store=store, spectrum=(2.0, 12.0, 11))
    for key in OUTPUTS + ("spectrum",):
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits
    fs = np.abs(g["F"]).max()
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N
