"""GPU parity: the local pair entropy (mtd_pel_*, csrc/pair_entropy_local.hip) through the C ABI against the fp64 numpy restatement of its
definition (tests/pair_entropy_local_ref.py, itself checked on the CPU in tests/test_pair_entropy_local_ref.py).

Tolerances, the project's own for this arithmetic (tests/test_gpu_pair_entropy.py, tests/test_gpu_ql_local*.py): s_i, sbar_i and v_i to
1e-10 of their maximum, the CV to 1e-9 relative, forces and per-particle virials to 1e-9 of their maximum with fp64 arrays and 2e-7 with
fp32 arrays (one rounding on store), the six virial sums likewise.  The fixed-point accumulation's worst case is below 1e-12 of s_i
(header of csrc/pair_entropy_local.hip).

Before anything is compared the REFERENCE must show that the snapshot lies on a smooth piece of the definition: no non-zero g_ib within
1e-6 relative of g_min, no entry with r B / r_max within 1e-9 of an integer.  Across either the definition jumps, and a legitimate
difference of one rounding could pass as, or hide, an error.

Every figure is printed before it is asserted.  Measured on an MI355X, worst over every case of this file and of
tests/test_gpu_pair_entropy_local_layouts.py: fp64 arrays s_i, sbar_i, v_i <= 9.4e-15 of their maximum, CV <= 8.9e-16 relative, forces
<= 1.3e-14 of max|F|, per-particle virial <= 1.4e-14 of max|virial_i|, the six sums <= 4.6e-14; fp32 arrays forces <= 5.2e-8, per-particle
virial <= 4.8e-8, sums <= 3e-8.  test_chunk_loop (N = 37 044): forces 5e-15 (fp64 arrays) and 2.6e-8 (fp32 arrays) of max|F|, their sum
1.7e-18 and 5.7e-11 of N max|F|.  No bound had to move.
"""
import ctypes as C

import numpy as np
import pytest

import pair_entropy_local_ref as pel
import pair_entropy_ref as pe
import stream_gate
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

PPB, MAX_BLOCKS = 32, 1024                                               # PEL_PPB, PEL_MAX_BLOCKS of csrc/pair_entropy_local.hip
OUTPUTS = ("partials", "s", "sbar", "v", "F", "virial")


def run_gpu(abi, pos, types, L, nl, r_max, sigma_r, n_bins, type_id, dtype, average=None, switch=None, bias=0.9, tilt=None,
            bias_on_device=True, virial=False, n_global=None, gate=None):
    """accumulate + forces; returns dict(partials, cv, s, sbar, v, F, virial).  gate: the stream the calls run on and how their inputs
    arrive (tests/stream_gate.py; None: the NULL stream)"""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N = len(nl[0])
    n_global = N if n_global is None else n_global
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    if len(nl[2]) == 0:
        d_nl = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    scratch = torch.zeros(lib.mtd_pel_scratch_doubles(N, n_bins), dtype=torch.float64, device="cuda")
    force = torch.full((N, 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda") if virial else None
    par = abi.PelParams.make(r_max, sigma_r, n_bins, type_id, average=average, switch=switch)
    p_part, p_s, p_sbar, p_v = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_part = C.c_uint()
    stream = gate.arm()
    call = abi.PelCall(N, n_global, abi.ptr(d_pos), dt, C.pointer(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), abi.ptr(scratch), stream)
    abi.check(lib.mtd_pel_accumulate(C.byref(par), C.byref(call), C.byref(p_part), C.byref(n_part), C.byref(p_s), C.byref(p_sbar), C.byref(p_v)))
    abi.check(lib.mtd_pel_forces(C.byref(par), C.byref(call), abi.ptr(force), abi.ptr(d_bias) if bias_on_device else None,
                                 0.0 if bias_on_device else bias, abi.ptr(vir) if virial else None, pitch if virial else 0))
    assert n_part.value == min(max((N + PPB - 1) // PPB, 1), MAX_BLOCKS)

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        part = s[off(p_part):off(p_part) + n_part.value].copy()
        out = dict(partials=part, cv=float(part.sum()) / n_global, s=s[off(p_s):off(p_s) + N].copy(), sbar=s[off(p_sbar):off(p_sbar) + N].copy(),
                   v=s[off(p_v):off(p_v) + N].copy(), F=force.cpu().numpy().astype(np.float64), virial=None)
        if virial:
            v = vir.cpu().numpy().astype(np.float64)
            assert np.all(v[:, N:] == 7.0)                                  # [n_particles, pitch) is left alone
            out["virial"] = v[:, :N].T.copy()
        return out
    return gate.done(read)


def on_a_smooth_piece(r, r_max, n_bins):
    """what the reference must show before it is compared (module docstring); prints the margins"""
    g = r["g"][r["g"] > 0.0]
    near = np.abs(g / pe.G_MIN - 1.0).min() if len(g) else np.inf
    x = r["bc_x"]
    edge = np.abs(x - np.rint(x)).min() if len(x) else np.inf
    print("smallest non-zero g %.3e; closest to g_min %.3e relative; closest r B / r_max to an integer %.3e; empty bins %.1f %%"
          % (g.min() if len(g) else 0.0, near, edge, 100.0 * (r["g"] == 0.0).mean()))
    assert near > 1e-6
    assert edge > 1e-9


def reference(pos, types, L, nl, r_max, sigma_r, n_bins, type_id, tilt=None, **kw):
    r = pel.compute(pos, types, L, nl, r_max, sigma_r, n_bins, type_id, tilt=tilt, **kw)
    i, j, d = pe.entries(np.asarray(pos, dtype=np.float64), np.asarray(types), nl, type_id, r_max + 4.0 * sigma_r, L, tilt=tilt)
    r["bc_x"] = np.sqrt((d * d).sum(axis=1)) * (n_bins / r_max)
    on_a_smooth_piece(r, r_max, n_bins)
    return r


def compare(g, r, bias, dtype, types=None, type_id=0):
    """prints every figure, then asserts; r: the restatement's result (its virial formed with the same bias)"""
    for key in ("s", "sbar", "v"):
        top = np.abs(r[key]).max()
        err = np.abs(g[key] - r[key]).max()
        print("%-4s: max |d| %.3e of max %.3e (%.3e rel)" % (key, err, top, err / top if top else 0.0))
        assert np.isfinite(g[key]).all()
        assert err <= 1e-10 * top
    err_cv = abs(g["cv"] - r["cv"]) / abs(r["cv"]) if r["cv"] else abs(g["cv"])
    F_ref = -bias * r["gather"]
    fs = np.abs(F_ref).max()
    err_f = np.abs(g["F"][:, :3] - F_ref).max()
    print("CV %.15g vs %.15g (%.3e rel); forces: max |d| %.3e of max |F| %.3e (%.3e rel)" % (g["cv"], r["cv"], err_cv, err_f, fs, err_f / fs if fs else 0.0))
    assert np.isfinite(g["F"]).all()
    assert err_cv <= 1e-9
    tol = 1e-9 if dtype == np.float64 else 2e-7
    assert fs > 0
    assert err_f <= tol * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        other = types[:len(g["F"])] != type_id
        assert np.all(g["F"][other] == 0.0)
        for key in ("s", "sbar", "v"):
            assert np.all(g[key][other] == 0.0)
    if g["virial"] is not None:
        top_v = np.abs(r["virial"]).max()
        err_v = np.abs(g["virial"] - r["virial"]).max()
        W, W_ref = g["virial"].sum(axis=0), r["virial"].sum(axis=0)
        err_w = np.abs(W - W_ref).max() / np.abs(W_ref).max()
        print("virial: max |d| %.3e of max |virial_i| %.3e (%.3e rel); sums %.3e rel" % (err_v, top_v, err_v / top_v, err_w))
        assert top_v > 0 and err_v <= tol * top_v
        assert err_w <= tol
        if types is not None:
            assert np.all(g["virial"][types[:len(g["F"])] != type_id] == 0.0)


def same_bits(a, b):
    for key in OUTPUTS:
        assert (a[key] is None and b[key] is None) or np.array_equal(a[key], b[key]), key


def noisy_fcc(n, sigma=0.05, seed=777):
    pos, L = util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


@pytest.fixture(scope="module")
def snapshots():
    """the snapshots of tests/test_gpu_pair_entropy.py: fcc 5 (N = 500) with noise 0.05 and 0.13, and the list that reaches 2.4"""
    out = {}
    for noise in (0.05, 0.13):
        pos, L = noisy_fcc(5, sigma=noise)
        out[noise] = dict(pos=pos, L=L, types=np.zeros(len(pos), dtype=np.int32), nl=util.build_nlist(pos, L, 2.4))
    return out


CASES = [(2.0, 0.1, 40), (2.0, 0.1, 37), (2.0, 0.05, 128),       # B = 128: w = 20, windows clipped at both ends
         (1.0, 0.35, 3)]                                         # B = 3: w = 7 > B, every window covers all bins
OPTIONS = ["none", "switch", "average", "both"]
AVERAGE = (1.2, 1.5)


def option_set(name, pos, s, par):
    """the keyword arguments of an option set; c0 = the reference's median of -sbar_i: the switch is in its steep part"""
    kw = {}
    if name in ("average", "both"):
        kw["average"] = AVERAGE
    if name in ("switch", "both"):
        base = pel.compute(pos, s["types"], s["L"], s["nl"], *par, 0, **kw)
        kw["switch"] = (float(np.median(-base["sbar"])), 6)
        assert kw["switch"][0] > 0
    return kw


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("noise", [0.05, 0.13])
@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("r_max,sigma_r,n_bins", CASES)
def test_parity(abi, snapshots, dtype, noise, option, r_max, sigma_r, n_bins):
    """the four histograms x the four option sets x two noise levels x fp64 / fp32 arrays; measured figures: module docstring"""
    s = snapshots[noise]
    pos = s["pos"].astype(dtype).astype(np.float64)                     # the snapshot is the rounded array
    par = (r_max, sigma_r, n_bins)
    c = pe.constants(*par)
    assert c["r_cut"] <= 2.4 + 1e-12
    if n_bins == 3:
        assert c["w"] > n_bins
    if n_bins == 128:
        assert c["w"] == 20
    kw = option_set(option, pos, s, par)
    assert "average" not in kw or kw["average"][1] <= c["r_cut"]
    r = reference(pos, s["types"], s["L"], s["nl"], *par, 0, bias=0.9, **kw)
    g = run_gpu(abi, pos, s["types"], s["L"], s["nl"], *par, 0, dtype, virial=True, **kw)
    compare(g, r, 0.9, dtype)
    plain = run_gpu(abi, pos, s["types"], s["L"], s["nl"], *par, 0, dtype, **kw)
    for key in ("partials", "s", "sbar", "v", "F"):
        assert np.array_equal(plain[key], g[key]), key                  # the VIR call's force array is the plain call's, bit for bit
    again = run_gpu(abi, pos, s["types"], s["L"], s["nl"], *par, 0, dtype, virial=True, **kw)
    same_bits(g, again)                                                 # two identical calls: identical bits


def test_known_values(abi, snapshots):
    """pinned from the restatement (tests/pair_entropy_local_ref.py) at rel 1e-9"""
    s = snapshots[0.05]
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], 2.0, 0.1, 40, 0, np.float64)
    print("CV %.15g, s_0 %.15g, min s %.15g" % (g["cv"], g["s"][0], g["s"].min()))
    assert g["cv"] == pytest.approx(KNOWN["cv"], rel=1e-9)
    assert g["s"][0] == pytest.approx(KNOWN["s0"], rel=1e-9)
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], 2.0, 0.1, 40, 0, np.float64, average=AVERAGE, switch=(3.0, 6))
    print("CV %.15g" % g["cv"])
    assert g["cv"] == pytest.approx(KNOWN["cv_both"], rel=1e-9)


KNOWN = dict(cv=-2.97716617715964, s0=-3.53941632933475, cv_both=0.484925744853362)


def small_system(dtype):
    """fcc 3 (N = 108, not a multiple of the 32 particles of a block) in a tilted box three times its size, every seventh particle of
    another type; particle 105 far from all others (an empty row), 106 and 107 a pair on their own (rows of length 1)"""
    pos, L0 = util.fcc_lattice(3)
    pos = pos + np.random.default_rng(5).normal(0, 0.05, pos.shape)
    L = 3.0 * L0
    pos[105] = [0.3 * L, 0.3 * L, 0.3 * L]
    pos[106] = [-0.3 * L, 0.3 * L, -0.3 * L]
    pos[107] = pos[106] + [0.7, 0.5, -0.4]
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = (np.arange(len(pos)) % 7 == 3).astype(np.int32)
    nl = pe.brute_nlist(pos, h, 2.4)
    assert nl[1][105] == 0 and nl[1][106] == 1 and nl[1][107] == 1 and len(pos) % PPB != 0
    return pos, types, L, tilt, nl


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("option", OPTIONS)
def test_small_system_tilted_two_types(abi, dtype, option):
    pos, types, L, tilt, nl = small_system(dtype)
    par = (2.0, 0.1, 40)
    kw = {}
    if option in ("average", "both"):
        kw["average"] = AVERAGE
    if option in ("switch", "both"):
        base = pel.compute(pos, types, L, nl, *par, 0, tilt=tilt, **kw)
        kw["switch"] = (float(np.median(-base["sbar"][types == 0])), 6)
    r = reference(pos, types, L, nl, *par, 0, tilt=tilt, bias=-1.7, **kw)
    c = pe.constants(*par)
    rho = r["n_t"] / L ** 3
    assert r["s"][105] == pytest.approx(-2 * np.pi * rho * c["delta"] * (c["r_b"] ** 2).sum(), rel=1e-14)
    for on_device in (True, False):
        g = run_gpu(abi, pos, types, L, nl, *par, 0, dtype, tilt=tilt, virial=True, bias=-1.7, bias_on_device=on_device, **kw)
        compare(g, r, -1.7, dtype, types=types)
        assert np.all(g["F"][105] == 0.0)
    # the other type as the variable's: 16 particles, most rows empty
    r1 = reference(pos, types, L, nl, *par, 1, tilt=tilt, bias=0.9, **kw)
    g1 = run_gpu(abi, pos, types, L, nl, *par, 1, dtype, tilt=tilt, virial=True, **kw)
    for key in ("s", "sbar", "v"):
        assert np.abs(g1[key] - r1[key]).max() <= 1e-10 * np.abs(r1[key]).max()
    assert abs(g1["cv"] - r1["cv"]) <= 1e-9 * abs(r1["cv"])
    # no particle of the type at all, and a bias of zero: nothing anywhere
    g2 = run_gpu(abi, pos, types, L, nl, *par, 5, dtype, tilt=tilt, virial=True, **kw)
    assert g2["cv"] == 0.0 and np.all(g2["F"] == 0.0) and np.all(g2["virial"] == 0.0) and np.all(g2["s"] == 0.0)
    g3 = run_gpu(abi, pos, types, L, nl, *par, 0, dtype, tilt=tilt, virial=True, bias=0.0, bias_on_device=False, **kw)
    assert np.all(g3["F"] == 0.0) and np.all(g3["virial"] == 0.0)


def test_n_global_scales_value_forces_and_virial(abi, snapshots):
    s = snapshots[0.13]
    par = (2.0, 0.1, 40, 0)
    a = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], *par, np.float64, virial=True, average=AVERAGE)
    b = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], *par, np.float64, virial=True, average=AVERAGE, n_global=1000)
    assert np.array_equal(a["partials"], b["partials"])
    assert np.abs(b["F"] * 2.0 - a["F"]).max() <= 1e-15 * np.abs(a["F"]).max()
    assert np.abs(b["virial"] * 2.0 - a["virial"]).max() <= 1e-15 * np.abs(a["virial"]).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_chunk_loop(abi, dtype):
    """fcc 21 (N = 37 044): 1158 chunks of 32 on the 1024 blocks the launches are capped at, so blocks 0 - 133 walk two chunks in every
    pass: the image is zeroed and read twice, the centre rows of the force pass are loaded twice, the block sums hold two chunks.  The
    list reaches r_cut = 1.5 only (~17 entries per row): the restatement stays cheap.  Average on: all five launches"""
    pos, L = noisy_fcc(21, sigma=0.05, seed=1)
    N = len(pos)
    n_chunks = (N + PPB - 1) // PPB
    assert N == 37044 and n_chunks == 1158 and MAX_BLOCKS < n_chunks < 2 * MAX_BLOCKS
    pos = pos.astype(dtype).astype(np.float64)
    types = (np.random.default_rng(4).random(N) < 0.3).astype(np.int32)
    par = (1.1, 0.1, 22)
    assert pe.constants(*par)["r_cut"] <= 1.5 + 1e-12
    nl = util.build_nlist(pos, L, 1.5)
    kw = dict(average=(1.0, 1.3), switch=(1.4, 6))                         # (the median of -sbar_i is 1.37)
    r = reference(pos, types, L, nl, *par, 0, bias=0.9, **kw)
    assert (types[MAX_BLOCKS * PPB:] == 1).sum() > 100                    # the other type inside the second-trip chunks
    g = run_gpu(abi, pos, types, L, nl, *par, 0, dtype, virial=True, **kw)
    assert len(g["partials"]) == MAX_BLOCKS
    compare(g, r, 0.9, dtype, types=types)
    again = run_gpu(abi, pos, types, L, nl, *par, 0, dtype, virial=True, **kw)
    same_bits(g, again)
    fs = np.abs(g["F"]).max()
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N
