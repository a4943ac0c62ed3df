"""GPU parity: the pair entropy (mtd_pe_*, csrc/pair_entropy.hip) through the C ABI against the fp64 numpy restatement of its definition
(tests/pair_entropy_ref.py, itself checked on the CPU in tests/test_pair_entropy_ref.py).

Tolerances: forces to 1e-9 of max|F| with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store), virials likewise of
max|virial_i| — the bounds of tests/test_gpu_ql_local*.py for the same arithmetic; g_b to 1e-10 of max g and S to 1e-9 relative.  The
fixed-point accumulation's worst case at these shapes is below 1e-11 of H (header of csrc/pair_entropy.hip).

Measured on an MI355X (every figure is printed before it is asserted): fp64 arrays g_b <= 1.2e-14 of max g (H_b <= 1.4e-14), S <= 2.8e-14
relative, forces <= 2.7e-14 of max|F|, per-particle virial <= 2e-14 of max|virial_i|, the six sums <= 8e-14; fp32 arrays forces <= 4.6e-8,
per-particle virial <= 5.5e-8, sums <= 3.6e-8.  No bound had to move.

test_chunk_loop (N = 37 044, 1158 chunks of 32 on the 1024 blocks the launches are capped at).  The header's bound at this shape: a block
walks one or two chunks, E_blk <= 1121 entries, sum_blocks E_blk^2 K(0) 2^-62 = 3.8e-10 absolute, and 1024 blocks added in doubles give
1.1e-13 relative, on H up to 1.4e6: below 4e-13 relative, the bound of 1e-10 is not a small-shape accident.  Measured on an MI355X: fp64
arrays g_b <= 4.7e-15 of max g (H_b <= 3.7e-15), S <= 3e-15 relative, forces <= 3.6e-15 of max|F|, per-particle virial <= 5.9e-15, the six
sums <= 7.1e-15; fp32 arrays forces 3.8e-8, per-particle virial 3.6e-8, sums 4e-10.  No bound had to move here either.
"""
import ctypes as C

import numpy as np
import pytest

import pair_entropy_ref as pe
import stream_gate
import util
from test_gpu_ql_local import brute_nlist

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def run_gpu(abi, pos, types, L, nl, r_max, sigma_r, n_bins, type_id, dtype, bias=0.9, tilt=None, bias_on_device=True, virial=False, n_rows=None,
            gate=None):
    """returns dict(S, g, sums, F, virial); n_rows: the first n_rows particles are the central ones, the others ghosts; gate: the
    stream the calls run on and how their inputs arrive (tests/stream_gate.py; None: the NULL stream)"""
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
    scratch = torch.zeros(lib.mtd_pe_scratch_doubles(n_bins), dtype=torch.float64, device="cuda")
    force = torch.full((N, 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda") if virial else None
    p_sums, p_value, p_g = C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_sums = C.c_uint()
    lists = (abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl))
    stream = gate.arm()
    abi.check(lib.mtd_pe_accumulate(N, abi.ptr(d_pos), dt, C.byref(box), *lists, r_max, sigma_r, n_bins, type_id, abi.ptr(scratch),
                                    C.byref(p_sums), C.byref(n_sums), stream))
    assert n_sums.value == n_bins + 1
    abi.check(lib.mtd_pe_finalize(C.byref(box), r_max, sigma_r, n_bins, abi.ptr(scratch), C.byref(p_value), C.byref(p_g), stream))
    abi.check(lib.mtd_pe_forces(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *lists, r_max, sigma_r, n_bins, type_id, abi.ptr(scratch),
                                abi.ptr(d_bias) if bias_on_device else None, 0.0 if bias_on_device else bias, stream,
                                abi.ptr(vir) if virial else None, pitch if virial else 0))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        out = dict(S=float(s[off(p_value)]), g=s[off(p_g):off(p_g) + n_bins].copy(), sums=s[off(p_sums):off(p_sums) + n_bins + 1].copy(),
                   F=force.cpu().numpy().astype(np.float64), virial=None)
        if virial:
            v = vir.cpu().numpy().astype(np.float64)
            assert np.all(v[:, N:] == 7.0)                                  # [n_particles, pitch) is left alone
            out["virial"] = v[:, :N].T.copy()
        return out
    return gate.done(read)


def noisy_fcc(n, sigma=0.05, seed=777):
    pos, L = util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), L


def compare(g, r, bias, dtype, types=None, type_id=0, rows=None):
    """prints every figure, then asserts; r: the restatement's result (its virial formed with the same bias)"""
    n_rows = len(g["F"])
    top_g = np.abs(r["g"]).max()
    err_g = np.abs(g["g"] - r["g"]).max()
    err_h = np.abs(g["sums"][:-1] - r["H"]).max() / max(np.abs(r["H"]).max(), 1e-300)
    err_s = abs(g["S"] - r["S"]) / abs(r["S"]) if r["S"] else abs(g["S"])
    F_ref = -bias * r["gather"][:n_rows]
    fs = np.abs(F_ref).max()
    err_f = np.abs(g["F"][:, :3] - F_ref).max()
    print("g_b: max |d| %.3e of max g %.3e (%.3e rel; H %.3e rel); S %.15g vs %.15g (%.3e rel); forces: max |d| %.3e of max |F| %.3e (%.3e rel)"
          % (err_g, top_g, err_g / top_g if top_g else 0.0, err_h, g["S"], r["S"], err_s, err_f, fs, err_f / fs if fs else 0.0))
    assert np.isfinite(g["F"]).all() and np.isfinite(g["g"]).all() and np.isfinite(g["S"])
    assert g["sums"][-1] == r["n_t"]
    assert err_g <= 1e-10 * top_g
    assert err_s <= 1e-9
    tol = 1e-9 if dtype == np.float64 else 2e-7
    assert fs > 0
    assert err_f <= tol * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        assert np.all(g["F"][types[:n_rows] != type_id] == 0.0)
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


CASES = [(2.0, 0.1, 40), (2.0, 0.1, 37), (2.0, 0.05, 256),       # B = 256: w = 39, windows clipped at both ends
         (1.0, 0.35, 3)]                                         # B = 3: w = 7 > B, every window covers all bins


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("noise", [0.05, 0.13])
@pytest.mark.parametrize("r_max,sigma_r,n_bins", CASES)
def test_pair_entropy_parity(abi, snapshots, dtype, noise, r_max, sigma_r, n_bins):
    s = snapshots[noise]
    pos = s["pos"].astype(dtype).astype(np.float64)                     # the snapshot is the rounded array
    assert pe.constants(r_max, sigma_r, n_bins)["r_cut"] <= 2.4 + 1e-12
    if n_bins == 3:
        assert pe.constants(r_max, sigma_r, n_bins)["w"] > n_bins
    g = run_gpu(abi, pos, s["types"], s["L"], s["nl"], r_max, sigma_r, n_bins, 0, dtype, virial=True)
    r = pe.compute(pos, s["types"], s["L"], s["nl"], r_max, sigma_r, n_bins, 0, bias=0.9)
    compare(g, r, 0.9, dtype)
    plain = run_gpu(abi, pos, s["types"], s["L"], s["nl"], r_max, sigma_r, n_bins, 0, dtype)
    assert np.array_equal(plain["F"], g["F"])                           # the VIR call's force array is the plain call's, bit for bit
    assert np.array_equal(plain["g"], g["g"]) and plain["S"] == g["S"]


def test_pair_entropy_known_value(abi, snapshots):
    s = snapshots[0.05]
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], 2.0, 0.1, 40, 0, np.float64)
    assert g["S"] == pytest.approx(-2.8320192288734845, rel=1e-9)
    assert (g["g"] >= pe.G_MIN).sum() == 37


@pytest.mark.parametrize("type_id", [0, 1])
def test_pair_entropy_two_types(abi, type_id):
    pos, L = noisy_fcc(5, seed=5)
    types = (np.random.default_rng(1).random(len(pos)) < 0.4).astype(np.int32)
    nl = util.build_nlist(pos, L, 2.4)
    g = run_gpu(abi, pos, types, L, nl, 2.0, 0.1, 40, type_id, np.float64, virial=True)
    r = pe.compute(pos, types, L, nl, 2.0, 0.1, 40, type_id, bias=0.9)
    assert 0 < r["n_t"] < len(pos)
    compare(g, r, 0.9, np.float64, types=types, type_id=type_id)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pair_entropy_rows_fewer_than_positions(abi, dtype):
    """the first 300 particles are central, the trailing 200 are ghosts: indexed by the rows, owning none.  What the pass forms is the
    gather over the rows with the sums of the rows"""
    pos, L = noisy_fcc(5, seed=9)
    pos = pos.astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    head, nn, lst = util.build_nlist(pos, L, 2.4)
    n_rows = 300
    nl = (head[:n_rows], nn[:n_rows], lst[:head[n_rows]])
    assert (nl[2] >= n_rows).any()
    g = run_gpu(abi, pos, types, L, nl, 2.0, 0.1, 40, 0, dtype, virial=True, n_rows=n_rows)
    r = pe.compute(pos, types, L, nl, 2.0, 0.1, 40, 0, bias=0.9)
    assert r["n_t"] == n_rows
    compare(g, r, 0.9, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pair_entropy_triclinic_box(abi, dtype):
    """a sheared fcc crystal in the sheared box: HOOMD's minimum image with tilt factors"""
    pos, L = noisy_fcc(4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    par = (1.6, 0.1, 32)
    nl = brute_nlist(pos, h, 2.05)
    g = run_gpu(abi, pos, types, L, nl, *par, 0, dtype, tilt=tilt, virial=True)
    r = pe.compute(pos, types, L, nl, *par, 0, tilt=tilt, bias=0.9)
    compare(g, r, 0.9, dtype)


def test_pair_entropy_buffered_and_shuffled_lists(abi):
    """a list buffered by 0.15 gives what the list cut at r_cut gives (entries beyond r_cut are skipped); rows shuffled: the same values
    (g exactly where the blocks' scales agree, forces to 1e-13: their sums follow the list order); two identical calls: identical bits"""
    pos, L = noisy_fcc(5, seed=9)
    types = (np.random.default_rng(2).random(len(pos)) < 0.15).astype(np.int32)
    par = (2.0, 0.1, 40, 0)
    tight = util.build_nlist(pos, L, 2.4)
    buffered = util.build_nlist(pos, L, 2.55)
    assert len(buffered[2]) > len(tight[2])
    a = run_gpu(abi, pos, types, L, tight, *par, np.float64, virial=True)
    b = run_gpu(abi, pos, types, L, buffered, *par, np.float64, virial=True)
    b2 = run_gpu(abi, pos, types, L, buffered, *par, np.float64, virial=True)
    r = pe.compute(pos, types, L, buffered, *par, bias=0.9)
    compare(b, r, 0.9, np.float64, types=types)
    for key in ("g", "sums", "F", "virial"):
        assert np.array_equal(b[key], b2[key]), key
    assert b["S"] == b2["S"]
    fs, gs = np.abs(a["F"]).max(), np.abs(a["g"]).max()
    assert np.abs(a["g"] - b["g"]).max() <= 1e-12 * gs and np.abs(a["F"] - b["F"]).max() <= 1e-12 * fs
    head, nn, lst = [np.array(x).copy() for x in buffered]
    rng = np.random.default_rng(2)
    for i in range(len(pos)):
        lst[head[i]:head[i] + nn[i]] = rng.permutation(lst[head[i]:head[i] + nn[i]])
    c = run_gpu(abi, pos, types, L, (head, nn, lst), *par, np.float64, virial=True)
    assert np.array_equal(c["sums"], b["sums"]) and c["S"] == b["S"]    # integer adds inside a block: the order inside a row does not count
    assert np.abs(c["F"] - b["F"]).max() <= 1e-13 * fs
    assert np.abs(c["virial"] - b["virial"]).max() <= 1e-13 * np.abs(b["virial"]).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pair_entropy_no_pair_inside_the_cutoff(abi, dtype):
    """all g = 0, S = -2 pi rho Delta sum r_b^2, forces exactly 0; once with empty rows, once with entries that all lie beyond r_cut"""
    pos = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0], [4.0, 4.0, 4.0]])
    types = np.zeros(len(pos), dtype=np.int32)
    L = 20.0
    c = pe.constants(2.0, 0.1, 40)
    want = -2 * np.pi * (len(pos) / L ** 3) * c["delta"] * (c["r_b"] ** 2).sum()
    for r_list in (2.4, 4.5):
        nl = util.build_nlist(pos, L, r_list)
        assert (len(nl[2]) == 0) == (r_list == 2.4)
        g = run_gpu(abi, pos, types, L, nl, 2.0, 0.1, 40, 0, dtype, virial=True)
        assert np.all(g["g"] == 0.0) and np.all(g["sums"][:-1] == 0.0) and g["sums"][-1] == len(pos)
        assert g["S"] == pytest.approx(want, rel=1e-13)
        assert np.all(g["F"] == 0.0)
        r = pe.compute(pos, types, L, nl, 2.0, 0.1, 40, 0, bias=0.9)
        assert np.abs(g["virial"] - r["virial"]).max() <= (1e-12 if dtype == np.float64 else 2e-7) * np.abs(r["virial"]).max()
    # no particle of the type at all: S = 0, nothing anywhere
    g = run_gpu(abi, pos, types, L, util.build_nlist(pos, L, 4.5), 2.0, 0.1, 40, 1, dtype, virial=True)
    assert g["S"] == 0.0 and np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0) and np.all(g["g"] == 0.0)


def test_pair_entropy_many_blocks(abi):
    """fcc 12 (N = 6912): 216 blocks, block sums across chunk boundaries"""
    pos, L = noisy_fcc(12, seed=21)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 2.4)
    g = run_gpu(abi, pos, types, L, nl, 2.0, 0.1, 40, 0, np.float64, virial=True)
    r = pe.compute(pos, types, L, nl, 2.0, 0.1, 40, 0, bias=0.9)
    compare(g, r, 0.9, np.float64)
    fs = np.abs(g["F"]).max()
    assert np.abs(g["F"][:, :3].sum(axis=0)).max() <= 1e-12 * fs * len(pos)      # translation invariance: the forces add up to zero


@pytest.mark.parametrize("dtype,two_types", [(np.float64, False), (np.float32, False), (np.float64, True)])
def test_chunk_loop(abi, dtype, two_types):
    """fcc 21 (N = 37 044): 1158 chunks of 32 on 1024 blocks, so blocks 0 - 133 walk two chunks in both passes and take their fixed-point
    scale from the entries of two chunks, the others from one.  The list reaches r_cut = 1.5 only (~17 entries per row): the restatement
    stays cheap.  With a second type on ~30 % of the particles the type test decides in second-trip chunks too"""
    pos, L = noisy_fcc(21, sigma=0.05, seed=1)
    N = len(pos)
    n_chunks = (N + 31) // 32
    assert N == 37044 and n_chunks > 1024 and n_chunks < 2 * 1024
    pos = pos.astype(dtype).astype(np.float64)                          # the snapshot is the rounded array
    types = (np.random.default_rng(4).random(N) < 0.3).astype(np.int32) if two_types else np.zeros(N, dtype=np.int32)
    par = (1.1, 0.1, 22)
    assert pe.constants(*par)["r_cut"] <= 1.5 + 1e-12
    nl = util.build_nlist(pos, L, 1.5)
    assert 15 < len(nl[2]) / N < 20
    g = run_gpu(abi, pos, types, L, nl, *par, 0, dtype, virial=True)
    r = pe.compute(pos, types, L, nl, *par, 0, bias=0.9)
    if two_types:
        assert 0.6 * N < r["n_t"] < 0.8 * N and (types[1024 * 32:] == 1).sum() > 100      # the other type inside the second-trip chunks
    else:
        assert r["S"] == pytest.approx(-1.74991, abs=1e-5) and (r["g"] >= pe.G_MIN).sum() == 20
    compare(g, r, 0.9, dtype, types=types if two_types else None)
    again = run_gpu(abi, pos, types, L, nl, *par, 0, dtype, virial=True)
    for key in ("g", "sums", "F", "virial"):
        assert np.array_equal(g[key], again[key]), key                  # two identical calls: identical bits
    assert g["S"] == again["S"]
    # translation invariance: the forces add up to zero, as in test_pair_entropy_many_blocks (fp32 arrays: every stored component errs
    # by half a unit in the last place, 2^-25 of itself, at most)
    fs = np.abs(g["F"]).max()
    total = np.abs(g["F"][:, :3].sum(axis=0)).max()
    print("sum of the forces: %.3e of N max |F|" % (total / (fs * N)))
    assert total <= (1e-12 + (0.0 if dtype == np.float64 else 2.0 ** -25)) * fs * N


def test_pair_entropy_bias_from_device_and_host(abi, snapshots):
    s = snapshots[0.13]
    par = (2.0, 0.1, 40, 0)
    dev = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], *par, np.float64, bias=-1.7, bias_on_device=True, virial=True)
    host = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], *par, np.float64, bias=-1.7, bias_on_device=False, virial=True)
    assert np.array_equal(dev["F"], host["F"]) and np.array_equal(dev["virial"], host["virial"])
    r = pe.compute(s["pos"], s["types"], s["L"], s["nl"], *par, bias=-1.7)
    compare(dev, r, -1.7, np.float64)
    zero = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], *par, np.float64, bias=0.0, bias_on_device=False, virial=True)
    assert np.all(zero["F"] == 0.0) and np.all(zero["virial"] == 0.0)
