"""GPU parity: the Bragg intensity (mtd_bragg_*, csrc/bragg.hip) through the C ABI against the fp64 numpy restatement of its definition
(tests/bragg_ref.py, itself checked on the CPU in tests/test_bragg_ref.py).

Bounds: the project's lamellar bounds carried through (tests/test_gpu_lamellar.py), with N the particle count and max |a| = 1 here:
    each amplitude   |d rho_k| <= 1e-6 max(max_k |rho_k|, sqrt N) max |a|                  (test_dropin_fourier_modes_and_sq_forces)
    value, default   |d s|     <= 2e-6 sum_k |w_k| |rho_k| max(|rho_k|, sqrt N) / A1^2      (|rho|^2 errs by 2 |rho| |d rho|)
    value, modulus   |d s|     <= 1e-6 sum_k |w_k| max(|rho_k|, sqrt N) / A1
    forces           1e-5 of max |F|
Snapshots are rounded to the array type first.  Every figure is printed before it is asserted.

Conditions on the inputs, asserted on the restatement before any GPU call:
  * Miller indices with |h| + |k| + |l| <= 4.  The kernels round the phase in turns to fp32 once: half an ulp of |t| <= 2 is 6e-8 turns or
    4e-7 rad per particle at the very most, 1.5e-7 rad rms at typical |t| < 1; over N particles that is about 1.5e-7 sqrt(N / 2) in an
    amplitude, a sixth of the bound and less.  (The lamellar tests hold the same bound with indices up to 6.)
  * Force parity in the modulus form: every |rho_k| >= 0.05 sqrt A2.  There the coefficients are the DIRECTION of rho_k, which an error
    d rho turns by |d rho| / |rho_k|: a peak far below its random-walk size sqrt A2 has full-size forces (w_k |q_k| |a_j| / A1 per particle)
    whose direction no fp32 sum can give to 1e-5.  test_modulus_form_where_a_peak_vanishes covers that side: finite and bounded.
"""
import ctypes as C

import numpy as np
import pytest

import bragg_ref as br
import stream_gate
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OUTPUTS = ("s", "sums", "S", "grad", "F")
HARDWARE, ACCURATE = 1, 2
# sixteen vectors, |h| + |k| + |l| <= 4; (0, 0, 3) is the one the ordered snapshots are modulated along
VECTORS = [(0, 0, 3), (1, -1, 0), (2, 1, -1), (1, 0, 0), (0, 2, 0), (1, 1, 1), (-1, 1, 1), (2, 0, -2), (0, 1, -2), (3, 0, 1), (1, 2, 0),
           (0, 0, 1), (1, -2, 1), (2, 2, 0), (0, 3, -1), (1, 0, -3)]
# sixteen types, four of them without an amplitude; all exact in fp32, max |a| = 1
COEFF16 = [1.0, -1.0, 0.5, -0.5, 0.0, 0.25, -0.75, 0.0, 1.0, -0.125, 0.625, 0.0, -1.0, 0.375, -0.25, 0.0]
BOXES = {"cubic": ((12.0, 12.0, 12.0), None), "triclinic": ((11.0, 13.5, 9.25), dict(xy=0.3, xz=-0.2, yz=0.15))}
SIZES = (1, 63, 64, 65, 2047, 2049, 4097)


def make_snapshot(N, kind, box, dtype, seed=0):
    """N particles of sixteen types inside the box, fractional coordinates in [-1/2, 1/2); kind "ordered": layers along (0, 0, 3), the
    fractional z moved by 0.05 sign(a) sin(2 pi 3 z) as util.snapshot_random(modulated=True) does; rounded to the dtype"""
    L, tilt = BOXES[box]
    rng = np.random.default_rng(1000 * N + seed)
    f = rng.random((N, 3)) - 0.5
    types = rng.integers(0, 16, N).astype(np.int32)
    types[0] = 0                                                         # (a single particle has an amplitude)
    if kind == "ordered":
        f[:, 2] += 0.05 * np.sign(np.array(COEFF16)[types]) * np.sin(2 * np.pi * 3 * f[:, 2])
        f[:, 2] -= np.rint(f[:, 2])
    pos = (f @ br.lattice(L, **(tilt or {}))).astype(dtype).astype(np.float64)
    return dict(pos=pos, types=types, L=L, tilt=tilt, f=f)


_cache = {}


def case(N, kind, box, dtype, K, modulus, bias=0.9, weights=None):
    """the snapshot and the restatement's answer, computed once and shared, never changed"""
    key = (N, kind, box, np.dtype(dtype).name, K, modulus, bias, None if weights is None else tuple(weights))
    if key not in _cache:
        s = make_snapshot(N, kind, box, dtype)
        ref = br.compute(s["pos"], s["types"], COEFF16, VECTORS[:K], s["L"], weights, modulus, s["tilt"], bias=bias)
        _cache[key] = (s, ref)
    return _cache[key]


def run_gpu(abi, pos, types, L, hkl, coeff, dtype, weights=None, modulus=False, trig=ACCURATE, bias=0.9, tilt=None, bias_on_device=True,
            n_global=None, gate=None):
    """one step through the three entry points; returns dict(s, sums, S, grad, F).  gate: the stream the calls run on and how their
    inputs arrive (tests/stream_gate.py; None: the NULL stream)"""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N, K = len(pos), len(hkl)
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(np.asarray(pos).reshape(-1, 3).astype(dtype), types, dtype))
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    scratch = torch.full((lib.mtd_bragg_scratch_doubles(N),), 5.0, dtype=torch.float64, device="cuda")
    force = torch.full((max(N, 1), 4), 3.0, dtype=tdt, device="cuda")
    par = abi.BraggParams.make(hkl, coeff, weights, modulus, trig)
    p_sums, p_value, p_S, p_rho, p_grad = (C.c_void_p() for _ in range(5))
    n_sums = C.c_uint()
    stream = gate.arm()
    call = abi.BraggCall(N, abi.ptr(d_pos) if N else None, dt, C.pointer(box), N if n_global is None else n_global, abi.ptr(scratch), stream)
    abi.check(lib.mtd_bragg_accumulate(C.byref(par), C.byref(call), C.byref(p_sums), C.byref(n_sums)))
    assert n_sums.value == 2 * K + 2
    abi.check(lib.mtd_bragg_finalize(C.byref(par), C.byref(call), C.byref(p_value), C.byref(p_S), C.byref(p_rho), C.byref(p_grad)))
    assert p_rho.value == p_sums.value
    abi.check(lib.mtd_bragg_forces(C.byref(par), C.byref(call), abi.ptr(force), abi.ptr(d_bias) if bias_on_device else None,
                                   0.0 if bias_on_device else bias))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        return dict(s=float(s[off(p_value)]), sums=s[off(p_sums):off(p_sums) + 2 * K + 2].copy(), S=s[off(p_S):off(p_S) + K].copy(),
                    grad=s[off(p_grad):off(p_grad) + 2 * K].reshape(K, 2).copy(), F=force.cpu().numpy().astype(np.float64)[:N])
    return gate.done(read)


def value_bound(r, N, modulus):
    m = np.sqrt((r["rho"] ** 2).sum(axis=1))
    floor = np.maximum(m, np.sqrt(N))
    if modulus:
        return 1e-6 * (np.abs(r["w"]) * floor).sum() / r["A1"]
    return 2e-6 * (np.abs(r["w"]) * m * floor).sum() / r["A1"] ** 2


def compare(g, r, N, modulus, what=""):
    """prints every figure, then asserts; r: the restatement's result"""
    K = len(r["rho"])
    rho = g["sums"][:2 * K].reshape(K, 2)
    m_ref = np.sqrt((r["rho"] ** 2).sum(axis=1))
    err_rho = np.sqrt(((rho - r["rho"]) ** 2).sum(axis=1)).max()
    tol_rho = 1e-6 * max(m_ref.max(), np.sqrt(N)) * max(np.abs(COEFF16))
    err_s, tol_s = abs(g["s"] - r["s"]), value_bound(r, N, modulus)
    fs = np.abs(r["F"]).max()
    err_f = np.abs(g["F"][:, :3] - r["F"]).max()
    print("%s s %.12g vs %.12g: |ds| %.3e of bound %.3e; max |d rho| %.3e of bound %.3e (max |rho| %.3e, sqrt N %.1f); forces max |d| %.3e of"
          " max |F| %.3e (%.3e rel)" % (what, g["s"], r["s"], err_s, tol_s, err_rho, tol_rho, m_ref.max(), np.sqrt(N), err_f, fs,
                                       err_f / fs if fs else 0.0))
    for k in ("sums", "S", "grad", "F"):
        assert np.isfinite(g[k]).all(), k
    assert np.isfinite(g["s"])
    assert g["sums"][-2] == r["A1"] and g["sums"][-1] == r["A2"]           # amplitudes exact in fp32, sums of a few thousand: exact
    assert err_rho <= tol_rho
    assert err_s <= tol_s
    assert np.abs(g["S"] - r["S"]).max() <= 2e-6 * (m_ref * np.maximum(m_ref, np.sqrt(N))).max() / r["A2"]
    assert fs > 0
    assert err_f <= 1e-5 * fs
    assert np.all(g["F"][:, 3] == 0.0)
    # translation invariance: the net force vanishes, within the force bound times N
    assert np.abs(g["F"][:, :3].sum(axis=0)).max() <= 1e-5 * fs * N


def condition(r, modulus):
    if modulus:
        m = np.sqrt((r["rho"] ** 2).sum(axis=1))
        assert m.min() >= 0.05 * np.sqrt(r["A2"]), (m / np.sqrt(r["A2"])).round(3)


@pytest.mark.parametrize("trig", [HARDWARE, ACCURATE])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("modulus", [False, True])
@pytest.mark.parametrize("kind", ["random", "ordered"])
@pytest.mark.parametrize("N", SIZES[1:])
def test_parity_over_sizes(abi, N, kind, modulus, dtype, trig):
    """one lane short of a wave, a wave, one lane more; one particle short of a block of 2048 and one more; three blocks.  Nine modes in
    the sixteen-mode kernel, sixteen types, the triclinic box"""
    s, r = case(N, kind, "triclinic", dtype, 9, modulus)
    condition(r, modulus)
    g = run_gpu(abi, s["pos"], s["types"], s["L"], VECTORS[:9], COEFF16, dtype, None, modulus, trig, tilt=s["tilt"])
    compare(g, r, N, modulus, "N=%d %s" % (N, kind))
    if kind == "ordered" and N >= 2047:
        assert g["S"][0] > 20 * np.median(g["S"])                        # the peak the snapshot was built with stands out


@pytest.mark.parametrize("trig", [HARDWARE, ACCURATE])
@pytest.mark.parametrize("modulus", [False, True])
@pytest.mark.parametrize("box", ["cubic", "triclinic"])
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 16])
def test_parity_over_mode_counts(abi, K, box, modulus, trig):
    """every compiled capacity of the sums kernel full (2, 8, 16) and partly filled (1, 3, 9), orthorhombic and general projection, given
    weights of both signs, the bias as a host scalar"""
    N = 2049
    w = [(-1.0) ** k * (1.0 + 0.25 * k) for k in range(K)]
    s, r = case(N, "ordered", box, np.float32, K, modulus, bias=-1.7, weights=w)
    condition(r, modulus)
    g = run_gpu(abi, s["pos"], s["types"], s["L"], VECTORS[:K], COEFF16, np.float32, w, modulus, trig, bias=-1.7, tilt=s["tilt"],
                bias_on_device=False)
    compare(g, r, N, modulus, "K=%d %s" % (K, box))


@pytest.mark.parametrize("trig", [HARDWARE, ACCURATE])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("modulus", [False, True])
def test_one_particle(abi, modulus, dtype, trig):
    """|rho_k| = |a| = A1 whatever the position: s = sum_k w_k to 1e-6; the force on a single particle vanishes with the net force"""
    s = make_snapshot(1, "random", "triclinic", dtype)
    w = [0.5, 0.25, 1.0, 0.125]
    g = run_gpu(abi, s["pos"], s["types"], s["L"], VECTORS[:4], COEFF16, dtype, w, modulus, trig, tilt=s["tilt"])
    print("s = %.12g, F = %s" % (g["s"], g["F"]))
    assert abs(g["s"] - sum(w)) <= 1e-6
    assert np.abs(g["S"] - 1.0).max() <= 1e-6
    q = np.abs(br.wave_vectors(VECTORS[:4], s["L"], s["tilt"])).max()
    assert np.abs(g["F"]).max() <= 1e-5 * 0.9 * q * 2 * sum(w)            # (1e-5 of the force a lone mode would give, w |q| |bias| |alpha| scale)


@pytest.mark.parametrize("modulus", [False, True])
def test_identical_calls_give_identical_bits(abi, modulus):
    s, _ = case(4097, "ordered", "triclinic", np.float32, 9, modulus)
    a, b = (run_gpu(abi, s["pos"], s["types"], s["L"], VECTORS[:9], COEFF16, np.float32, None, modulus, HARDWARE, tilt=s["tilt"]) for _ in range(2))
    stream_gate.assert_same_bits(a, b, "second call", keys=OUTPUTS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("modulus", [False, True])
def test_no_amplitudes_give_zeros(abi, modulus, dtype):
    """A1 = 0: value, S_k, coefficients and forces are 0, nothing NaN; and a rank without particles of a system that has some"""
    s = make_snapshot(2049, "random", "cubic", dtype)
    types = np.where(np.arange(2049) % 2 == 0, 4, 7).astype(np.int32)     # both types without an amplitude
    g = run_gpu(abi, s["pos"], types, s["L"], VECTORS[:8], COEFF16, dtype, None, modulus, HARDWARE)
    for k in OUTPUTS:
        assert np.all(np.asarray(g[k]) == 0.0), k
    g = run_gpu(abi, np.zeros((0, 3)), np.zeros(0, dtype=np.int32), s["L"], VECTORS[:8], COEFF16, dtype, None, modulus, HARDWARE, n_global=5)
    assert g["s"] == 0.0 and not g["sums"].any() and not g["S"].any() and not g["grad"].any()


@pytest.mark.parametrize("trig", [HARDWARE, ACCURATE])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("z0", [0.25, 0.3])
def test_modulus_form_where_a_peak_vanishes(abi, z0, dtype, trig):
    """two particles half a period apart: rho = 0 exactly where the phases are dyadic (z0 = 0.25: the coefficients must be 0, not 0 / 0),
    and rounding noise with a direction nobody chose where they are not (z0 = 0.3).  No parity is asked; every force must be finite and
    within w |q| |a_j| |bias| / A1 (one part in 10^6 for the fp32 roundings of the coefficient and of sine and cosine)"""
    L, hkl, w, bias = (8.0, 8.0, 8.0), [(0, 0, 2)], [1.5], -2.5
    pos = np.array([[0.3, -1.1, z0], [0.3, -1.1, z0 + 8.0 / 4.0]])
    g = run_gpu(abi, pos, np.array([0, 0], dtype=np.int32), L, hkl, [1.0], dtype, w, True, trig, bias=bias)
    q = np.linalg.norm(br.wave_vectors(hkl, L)[0])
    top = w[0] * q * 1.0 * abs(bias) / 2.0
    print("rho = %s, s = %.3e, coefficients %s, |F| = %s of at most %.6g" % (g["sums"][:2], g["s"], g["grad"], np.linalg.norm(g["F"][:, :3], axis=1), top))
    assert np.isfinite(g["F"]).all() and np.isfinite(g["grad"]).all() and np.isfinite(g["s"])
    assert 0.0 <= g["s"] <= 1e-6
    assert np.linalg.norm(g["F"][:, :3], axis=1).max() <= top * (1 + 1e-6)
    assert np.hypot(*g["grad"][0]) <= w[0] / 2.0 * (1 + 1e-12)


@pytest.mark.parametrize("trig", [HARDWARE, ACCURATE])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("modulus", [False, True])
def test_shifted_and_rewrapped_snapshot(abi, modulus, dtype, trig):
    """all particles shifted together and wrapped back into the box: the same s within the value bound — what cv.lamellar cannot do"""
    N = 4097
    s, r = case(N, "ordered", "triclinic", dtype, 9, modulus)
    f = s["f"] + np.array([0.25 / 3.0, 0.31, -0.47])                     # a quarter period of (0, 0, 3) along z
    f -= np.rint(f)
    shifted = (f @ br.lattice(s["L"], **s["tilt"])).astype(dtype).astype(np.float64)
    g0 = run_gpu(abi, s["pos"], s["types"], s["L"], VECTORS[:9], COEFF16, dtype, None, modulus, trig, tilt=s["tilt"])
    g1 = run_gpu(abi, shifted, s["types"], s["L"], VECTORS[:9], COEFF16, dtype, None, modulus, trig, tilt=s["tilt"])
    lam0, lam1 = (br.lamellar_value(p, s["types"], COEFF16, [(0, 0, 3)], s["L"], s["tilt"]) for p in (s["pos"], shifted))
    print("s %.12g -> %.12g (|d| %.3e of bound %.3e); cv.lamellar's restatement %.6f -> %.6f" % (g0["s"], g1["s"], abs(g1["s"] - g0["s"]),
                                                                                                  value_bound(r, N, modulus), lam0, lam1))
    assert abs(g1["s"] - g0["s"]) <= value_bound(r, N, modulus)
    assert abs(lam1 - lam0) > 0.01
