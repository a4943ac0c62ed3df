"""GPU parity: the probe volume (mtd_probe_*, csrc/probe_volume.hip) through the C ABI against the fp64 restatement of its definition
(tests/probe_volume_ref.py, itself checked on the CPU in tests/test_probe_volume_ref.py).

Bounds, from fp64 rounding with about a hundredfold margin (boxes have L <= 20, sigma_s >= 0.05: the error of u is at most four roundings
x 2^-53 x 20 = 1e-14, times Phi(0) <= 8, plus a few ulp of erf):
    h_i                |h_i - ref| <= 1e-12
    value              |s - ref|   <= 1e-12 sum_{h_ref > 0} |a_i|
    forces, virial     every component within 1e-12 |bias| max|a| Phi(0), times max|d| for the virial
    N_v                equal to the restatement's, after the particles within 1e-9 of a sharp face are taken out of the input
Force and virial arrays have the scalar type of the positions.  With fp32 arrays the kernel's fp64 result is rounded once more when it is
stored, by up to 2^-24 of its size (up to 2^-126 for values below that, the smallest normal fp32 number): that storage rounding, taken
at the restatement's own value, is added to the bound of the component (nothing is added for fp64 arrays).  Every figure is printed before it is asserted.

A snapshot is built once per (region, box, array type): 4097 particles, the hand-placed ones in front, then a half close to the region
and a half anywhere in the box.  The sizes 1, 4095, 4096, 4097 (= 2 x 512 x 4 + 1: one group, the tail of the grid-stride loop, the
re-read slot of the unrolled load) take its first N particles; the restatement is evaluated once and sliced."""
import ctypes as C
import math

import numpy as np
import pytest

import probe_volume_ref as pv
import stream_gate
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

INF = float("inf")
OUTPUTS = ("s", "count", "h", "F", "virial")
# sixteen types, four of them with weight zero, both signs; all exact in fp32, max |a| = 1
COEFF16 = [1.0, -1.0, 0.5, -0.5, 0.0, 0.25, -0.75, 0.0, 1.0, -0.125, 0.625, 0.0, -1.0, 0.375, -0.25, 0.0]
BOXES = {"cubic": ((16.0, 16.0, 16.0), None), "orthorhombic": ((16.0, 18.5, 15.0), None),
         "tilted": ((17.0, 18.5, 16.25), dict(xy=0.3, xz=-0.2, yz=0.15))}
SHAPES = ("box", "slab", "sphere", "cylinder")
SIZES = (1, 4095, 4096, 4097)
N_MAX = 4097
CENTRE = np.array([0.4, -0.3, 0.2])


def make_region(shape, sigma_s, centre=CENTRE):
    if shape == "box":
        return pv.region("box", centre, sigma_s, w=[2.0, 1.25, 1.5])
    if shape == "slab":
        return pv.region("box", centre, sigma_s, w=[INF, INF, 1.5])          # bounded along z: fits every box, tilted ones too
    if shape == "sphere":
        return pv.region("sphere", centre, sigma_s, R=2.5)
    return pv.region("cylinder", centre, sigma_s, R=2.0, w=1.5, axis=1)


def hand_placed(reg):
    """displacements from the centre: on every face at u = 0, +-r_c, +-r_c (1 +- 2^-20); the sphere's centre; on the cylinder's axis;
    the corner of a box where three shells overlap"""
    rc = reg["r_c"]
    us = [0.0, rc, -rc] + [sg * rc * (1.0 + e) for sg in (1.0, -1.0) for e in (2.0 ** -20, -2.0 ** -20)]
    out = []
    if reg["shape"] == "box":
        for k in range(3):
            if reg["w"][k] == INF:
                continue
            for sg in (1.0, -1.0):
                for u in us:
                    d = np.array([0.11, -0.07, 0.05])
                    d[k] = sg * (reg["w"][k] - u)
                    out.append(d)
        out.append(np.array([reg["w"][k] - f * rc if reg["w"][k] != INF else 0.37 for k, f in enumerate((0.3, -0.2, 0.5))]))
    elif reg["shape"] == "sphere":
        n = np.array([0.6, -0.48, 0.64])
        out += [n * (reg["R"] - u) for u in us] + [np.zeros(3)]
    else:
        ax = reg["axis"]
        e_ax = np.eye(3)[ax]
        perp = np.roll(e_ax, 1) * 0.8 - np.roll(e_ax, 2) * 0.6
        out += [perp * (reg["R"] - u) + 0.2 * e_ax for u in us]
        out += [e_ax * sg * (reg["w"][ax] - u) + perp * 0.3 * reg["R"] for sg in (1.0, -1.0) for u in us]
        out += [e_ax * (reg["w"][ax] - 0.4 * rc), e_ax * 0.7, np.zeros(3)]                      # on the axis: in a cap's shell, inside, at the centre
    return np.array(out)


def make_snapshot(shape, sigma_s, box, dtype, centre=CENTRE, seed=0):
    """N_MAX particles of sixteen types, rounded to the dtype and wrapped into the box"""
    L, tilt = BOXES[box]
    reg = make_region(shape, sigma_s, centre)
    assert pv.fits(reg, L, tilt)
    rng = np.random.default_rng(seed + 17 * SHAPES.index(shape) + 1000 * list(BOXES).index(box))
    A = pv.lattice(L, **(tilt or {}))
    hand = hand_placed(reg)
    n_near = (N_MAX - len(hand)) // 2
    reach = np.minimum(7.0, np.array(pv.extents(reg)) + 0.5)
    near = rng.uniform(-1.0, 1.0, (n_near, 3)) * reach
    far = (rng.random((N_MAX - len(hand) - n_near, 3)) - 0.5) @ A - reg["centre"]
    pos = np.concatenate([hand, near, far]) + reg["centre"]
    f = pos @ np.linalg.inv(A)
    pos = (f - np.rint(f)) @ A                                               # into the box: regions near a face are cut in pieces
    pos = pos.astype(dtype).astype(np.float64)
    types = rng.integers(0, 16, N_MAX).astype(np.int32)
    types[0] = 0
    return dict(pos=pos, types=types, L=L, tilt=tilt, reg=reg, n_hand=len(hand))


_cache = {}


def case(shape, sigma_s, box, dtype, bias=0.9, centre=CENTRE):
    """the snapshot and the restatement's answer for all N_MAX particles, computed once and shared, never changed"""
    key = (shape, sigma_s, box, np.dtype(dtype).name, bias, tuple(centre))
    if key not in _cache:
        s = make_snapshot(shape, sigma_s, box, dtype, centre)
        _cache[key] = (s, pv.compute(s["pos"], s["types"], COEFF16, s["reg"], s["L"], s["tilt"], bias=bias))
    return _cache[key]


def sliced(r, N, keep=None):
    """the restatement's result for the first N particles (keep: a mask over them)"""
    idx = np.arange(N) if keep is None else np.flatnonzero(keep[:N])
    return dict(s=math.fsum(r["a"][idx] * r["h"][idx]), count=math.fsum(r["a"][idx][r["inside"][idx]]), h=r["h"][idx], a=r["a"][idx], d=r["d"][idx],
                F=r["F"][idx], virial=r["virial"][:, idx], inside=r["inside"][idx])


def probe_params(abi, reg, box, coeff):
    shapes = {"box": abi.MTD_PROBE_BOX, "sphere": abi.MTD_PROBE_SPHERE, "cylinder": abi.MTD_PROBE_CYLINDER}
    return abi.ProbeParams.make(shapes[reg["shape"]], abi.ProbeParams.fractional(reg["centre"], box), reg["sigma_s"], reg["r_c"], reg["w"],
                                reg["R"], reg["axis"], coeff)


def run_gpu(abi, pos, types, L, reg, coeff, dtype, bias=0.9, tilt=None, virial=True, bias_on_device=True, n_global=None, gate=None, local=True,
            reduce=None):
    """one step through the entry points; returns dict(s, count, h, F, virial).  gate: the stream the calls run on and how their inputs
    arrive (tests/stream_gate.py; None: the NULL stream); reduce: called with the two sums (a view of the scratch) between accumulate and
    finalize, where a domain-decomposed run adds the ranks' sums"""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N = len(pos)
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(np.asarray(pos).reshape(-1, 3).astype(dtype), types, dtype))
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    scratch = torch.full((lib.mtd_probe_scratch_doubles(N),), 5.0, dtype=torch.float64, device="cuda")
    force = torch.full((max(N, 1), 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3                                                             # rows [N, pitch) must be left alone
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda")
    h = torch.full((max(N, 1),), -1.0, dtype=torch.float64, device="cuda")
    par = probe_params(abi, reg, box, coeff)
    p_sums, p_value, p_count = (C.c_void_p() for _ in range(3))
    n_sums = C.c_uint()
    stream = gate.arm()
    call = abi.ProbeCall(N, abi.ptr(d_pos) if N else None, dt, C.pointer(box), N if n_global is None else n_global, abi.ptr(scratch), stream)
    abi.check(lib.mtd_probe_accumulate(C.byref(par), C.byref(call), C.byref(p_sums), C.byref(n_sums)))
    assert n_sums.value == 2
    if reduce is not None:
        first = (p_sums.value - scratch.data_ptr()) // 8
        reduce(scratch[first:first + 2])
    abi.check(lib.mtd_probe_finalize(C.byref(par), C.byref(call), C.byref(p_value), C.byref(p_count)))
    abi.check(lib.mtd_probe_forces(C.byref(par), C.byref(call), abi.ptr(force), abi.ptr(d_bias) if bias_on_device else None,
                                   0.0 if bias_on_device else bias, abi.ptr(vir) if virial else None, pitch if virial else 0))
    if local:
        abi.check(lib.mtd_probe_local(C.byref(par), C.byref(call), abi.ptr(h)))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        v = vir.cpu().numpy().astype(np.float64)
        assert np.all(v[:, N:] == 7.0)
        return dict(s=float(s[off(p_value)]), count=float(s[off(p_count)]), h=h.cpu().numpy()[:N].copy(),
                    F=force.cpu().numpy().astype(np.float64)[:N], virial=v[:, :N].copy())
    return gate.done(read)


def storage(ref, dtype):
    """what rounding the restatement's value to the array type may cost: for fp32 arrays 2^-24 of its size, and below the smallest
    normal fp32 number, 2^-126, up to that number (subnormals have a fixed spacing, or are flushed); nothing for fp64 arrays"""
    return np.maximum(np.abs(ref) * 2.0 ** -24, 2.0 ** -126) if dtype == np.float32 else 0.0


def compare(g, r, reg, dtype, bias, what="", n_hand=0):
    """prints the worst fraction of every bound, then asserts; r: the restatement's result for the same particles"""
    phi0 = pv.phi(0.0, reg["sigma_s"], reg["r_c"])
    amax = max(np.abs(COEFF16))
    err_h = np.abs(g["h"] - r["h"]).max() if len(r["h"]) else 0.0
    tol_s = 1e-12 * np.abs(r["a"][r["h"] > 0]).sum()
    err_s = abs(g["s"] - r["s"])
    tol_f = 1e-12 * abs(bias) * amax * phi0 + storage(r["F"], dtype)
    frac_f = (np.abs(g["F"][:, :3] - r["F"]) / tol_f).max()
    dmax = np.abs(r["d"]).max()
    tol_v = 1e-12 * abs(bias) * amax * phi0 * dmax + storage(r["virial"], dtype)
    frac_v = (np.abs(g["virial"] - r["virial"]) / tol_v).max()
    print("%s s %.15g vs %.15g; fractions of the bounds: h %.3g, s %.3g, forces %.3g, virial %.3g (Phi(0) %.3f, max |d| %.2f, max |F| %.3e)"
          % (what, g["s"], r["s"], err_h / 1e-12, err_s / tol_s if tol_s else 0.0, frac_f, frac_v, phi0, dmax, np.abs(r["F"]).max()))
    for k in ("h", "F", "virial"):
        assert np.isfinite(g[k]).all(), k
    assert err_h <= 1e-12
    assert err_s <= tol_s
    assert frac_f <= 1.0
    assert frac_v <= 1.0
    assert np.all(g["F"][:, 3] == 0.0)
    # outside region and shell: exactly nothing.  The hand-placed particles are left out: one of them sits ON the shell's edge, where the
    # last bit of u decides between 0 and a G of 1e-40
    outside = (r["h"] == 0.0) & (np.abs(r["F"]).max(axis=1) == 0.0)
    outside[:n_hand] = False
    assert np.all(g["F"][outside] == 0.0) and np.all(g["virial"][:, outside] == 0.0) and np.all(g["h"][outside] == 0.0)


def near_a_sharp_face(r, reg, eps=1e-9):
    """mask: particles within eps of a sharp face of the region (in the restatement's displacements)"""
    d = r["d"]
    if reg["shape"] == "box":
        dist = [np.abs(np.abs(d[:, k]) - reg["w"][k]) for k in range(3) if reg["w"][k] != INF]
    elif reg["shape"] == "sphere":
        dist = [np.abs(np.sqrt((d * d).sum(axis=1)) - reg["R"])]
    else:
        ax = reg["axis"]
        perp = [k for k in range(3) if k != ax]
        dist = [np.abs(np.sqrt(d[:, perp[0]] ** 2 + d[:, perp[1]] ** 2) - reg["R"])]
        if reg["w"][ax] != INF:
            dist.append(np.abs(np.abs(d[:, ax]) - reg["w"][ax]))
    return np.min(dist, axis=0) < eps


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("sigma_s", [0.05, 0.3])
@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity(abi, shape, dtype, box, sigma_s, N):
    s, full = case(shape, sigma_s, box, dtype)
    r = sliced(full, N)
    g = run_gpu(abi, s["pos"][:N], s["types"][:N], s["L"], s["reg"], COEFF16, dtype, tilt=s["tilt"])
    compare(g, r, s["reg"], dtype, 0.9, "%s %s %s sigma_s=%g N=%d:" % (shape, np.dtype(dtype).name, box, sigma_s, N), s["n_hand"])
    if N > 1000:
        assert (r["h"] == 1.0).sum() > 50 and ((r["h"] > 0) & (r["h"] < 1)).sum() > 50 and (r["h"] == 0.0).sum() > 500
        assert np.abs(r["F"]).max() > 0.1 * pv.phi(0.0, sigma_s, 2 * sigma_s)
    # the sharp count, on the input without the particles that sit on a sharp face to 1e-9: those are hand-placed ones only
    near = near_a_sharp_face(full, s["reg"])
    assert not near[s["n_hand"]:].any()
    keep = ~near
    rk = sliced(full, N, keep)
    idx = np.flatnonzero(keep[:N])
    if len(idx):
        gk = run_gpu(abi, s["pos"][idx], s["types"][idx], s["L"], s["reg"], COEFF16, dtype, tilt=s["tilt"], n_global=N_MAX, local=False)
        print("N_v %.17g vs %.17g (%d particles taken out)" % (gk["count"], rk["count"], N - len(idx)))
        assert gk["count"] == rk["count"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_region_across_the_periodic_boundary(abi, shape, dtype):
    """the region centred close to a corner of the tilted box: particles reach it through up to seven images"""
    L, tilt = BOXES["tilted"]
    A = pv.lattice(L, **tilt)
    corner = 0.5 * (A[0] + A[1] + A[2]) - np.array([0.3, 0.2, 0.1])
    s, r = case(shape, 0.3, "tilted", dtype, bias=-1.7, centre=corner)
    images = np.abs(np.rint((s["pos"] - corner - r["d"]) @ np.linalg.inv(A))).sum(axis=1)
    assert (images[r["h"] > 0] > 0).sum() > 100
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["reg"], COEFF16, dtype, bias=-1.7, tilt=s["tilt"], bias_on_device=False)
    compare(g, r, s["reg"], dtype, -1.7, "%s %s across the boundary:" % (shape, np.dtype(dtype).name), s["n_hand"])


@pytest.mark.parametrize("axis", [0, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cylinder_axes_and_an_unbounded_cylinder(abi, dtype, axis):
    """the other two axes, without caps, in the orthorhombic box; r_c = 2.5 sigma_s, not the default"""
    L, tilt = BOXES["orthorhombic"]
    reg = pv.region("cylinder", CENTRE, 0.2, r_c=0.5, R=2.0, w=INF, axis=axis)
    assert pv.fits(reg, L, tilt)
    rng = np.random.default_rng(5 + axis)
    hand = hand_placed(dict(reg, w=[1.0] * 3)) + CENTRE                     # (the cap points are ordinary points of this one)
    anywhere = (rng.random((3000, 3)) - 0.5) * np.array(L)
    anywhere[:, [k for k in range(3) if k != axis]] *= 0.45                  # towards the cylinder
    pos = np.concatenate([hand, anywhere]).astype(dtype).astype(np.float64)
    types = rng.integers(0, 16, len(pos)).astype(np.int32)
    r = pv.compute(pos, types, COEFF16, reg, L, tilt, bias=0.9)
    assert r["inside"].sum() > 100
    g = run_gpu(abi, pos, types, L, reg, COEFF16, dtype, tilt=tilt)
    compare(g, r, reg, dtype, 0.9, "cylinder along %d %s:" % (axis, np.dtype(dtype).name), len(hand))


@pytest.mark.parametrize("shape", SHAPES)
def test_identical_calls_give_identical_bits(abi, shape):
    s, _ = case(shape, 0.3, "tilted", np.float32)
    a, b = (run_gpu(abi, s["pos"], s["types"], s["L"], s["reg"], COEFF16, np.float32, tilt=s["tilt"]) for _ in range(2))
    stream_gate.assert_same_bits(a, b, "second call", keys=OUTPUTS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_forces_are_the_same_bits_without_a_virial(abi, shape, dtype):
    """with a NULL virial pointer the kernel is the one without the virial; the force array must not notice"""
    s, _ = case(shape, 0.3, "tilted", dtype)
    a = run_gpu(abi, s["pos"], s["types"], s["L"], s["reg"], COEFF16, dtype, tilt=s["tilt"], virial=True)
    b = run_gpu(abi, s["pos"], s["types"], s["L"], s["reg"], COEFF16, dtype, tilt=s["tilt"], virial=False)
    stream_gate.assert_same_bits(a, b, "without a virial", keys=("s", "count", "h", "F"))
    assert np.all(b["virial"] == 7.0) and np.abs(a["virial"]).max() > 0    # nothing written without the pointer


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_rank_without_particles_and_weights_of_zero(abi, dtype):
    """n_particles = 0 with n_global > 0: both sums 0; every particle of a type with weight 0: value, count and forces 0, h_i not"""
    s, r = case("sphere", 0.3, "cubic", dtype)
    g = run_gpu(abi, np.zeros((0, 3)), np.zeros(0, dtype=np.int32), s["L"], s["reg"], COEFF16, dtype, n_global=5)
    assert g["s"] == 0.0 and g["count"] == 0.0
    types = np.where(np.arange(N_MAX) % 2 == 0, 4, 7).astype(np.int32)
    g = run_gpu(abi, s["pos"], types, s["L"], s["reg"], COEFF16, dtype)
    assert g["s"] == 0.0 and g["count"] == 0.0 and np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
    assert np.abs(g["h"] - r["h"]).max() <= 1e-12 and g["h"].max() == 1.0
