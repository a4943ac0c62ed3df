"""GPU parity: the solid-bond count of the local Steinhardt variable (mtd_ql_local_*_bonds, cv.steinhardt_local(bonds=)) against the fp64
numpy restatement of its definition in the scatter form (tests/ql_local_bonds_ref.py, itself checked on the CPU in
tests/test_ql_local_bonds_ref.py).  Tolerances are the project's own for this arithmetic (tests/test_gpu_ql_local_avg.py,
tests/test_gpu_ql_local_virial.py): c_i, n_i, b_i and v_i to 1e-11 of their largest value, s to 1e-10 relative, forces to 1e-9 of
max|F| with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store), the per-particle virial to the same two bounds of
max|virial_i|, its six sums to 1e-9 of max|W| with fp64 arrays; w == 0 and particles of another type exactly 0.  The fp32 snapshot is
the rounded array, on both sides.  Every call runs the force pass with and without the virial: the two force arrays must agree bit
for bit.  The parity snapshot is noisy fcc at sigma = 0.13, where the products d_ij populate all three parts of the ramp (0.3, 0.8):
at 0.05 every bond lies above it and the q-dependent part of the gradient would go untested."""
import ctypes as C

import numpy as np
import pytest

import ql_local_bonds_ref as bonds_ref
import stream_gate
import util
from test_gpu_ql_local_avg import brute_nlist, cluster_case
from test_gpu_ql_local_avg import run_gpu as run_gpu_opt
from test_gpu_ql_local_virial import run_gpu as run_gpu_virial

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

E6 = [0, 0, 0, 0, 0, 0, 1]
QL_12 = [0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0.5, 0.3, 0.25]
BONDS = (0.3, 0.8)
COMBOS = {
    "bonds": dict(bonds=BONDS),
    "bonds+switch": dict(bonds=BONDS, switch=(6.5, 6)),
    "bonds+switch+gate": dict(bonds=BONDS, switch=(6.5, 6), gate=(10, 13)),
}
SENTINEL = -7.25
BIAS = 0.9


def run_gpu(abi, pos, types, L, nl, rcut, ron, lmax, type_id, Ql_ref, dtype, opt=None, n_global=None, bias=BIAS, tilt=None, bias_on_device=True,
            entry="bonds", gate=None):
    """opt: dict(switch=, gate=, bonds=, average=); pass 1 through mtd_ql_local_accumulate_bonds, then mtd_ql_local_forces_bonds without
    and with a virial array on the same table.  entry = "null": bonds == NULL, "zero": an all-zero struct.  Returns dict(s, c, n, v, b,
    F, F_vir, raw, partials); b is None with bonds off.  The scratch starts as NaN: whatever the passes read they must have written.
    gate: the stream the calls run on and how their inputs arrive (tests/stream_gate.py; None: the NULL stream)."""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    opt = dict(opt or {})
    bonds = opt.pop("bonds", None)
    N = len(pos)
    n_global = N if n_global is None else n_global
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    assert int(np.asarray(nl[0]).astype(np.int64)[-1] + np.asarray(nl[1]).astype(np.int64)[-1]) <= len(nl[2])
    o = abi.QlLocalOptions.make(**opt)
    bd = abi.QlLocalBonds.make(bonds if entry == "bonds" else None)
    p_bd = None if entry == "null" else C.byref(bd)
    n_doubles = lib.mtd_ql_local_scratch_doubles_bonds(N, lmax, len(nl[2]), C.byref(o), p_bd)
    scratch = torch.full((n_doubles,), float("nan"), dtype=torch.float64, device="cuda")
    p_part, p_c, p_n, p_v, p_b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_part = C.c_uint()
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    common = (abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), rcut, ron, lmax, type_id, util.dbl_array(Ql_ref), n_global, abi.ptr(scratch))
    force = torch.full((N, 4), 3.0, dtype=tdt, device="cuda")
    f_vir = torch.full((N, 4), 5.0, dtype=tdt, device="cuda")
    virial = torch.full((6, N + 3), SENTINEL, dtype=tdt, device="cuda")
    stream = gate.arm()
    b_args = (abi.ptr(d_bias) if bias_on_device else None, 0.0 if bias_on_device else bias, stream)
    abi.check(lib.mtd_ql_local_accumulate_bonds(N, abi.ptr(d_pos), dt, C.byref(box), *common, C.byref(p_part), C.byref(n_part), C.byref(p_c),
                                                C.byref(p_n), stream, C.byref(o), C.byref(p_v), p_bd, C.byref(p_b)))
    abi.check(lib.mtd_ql_local_forces_bonds(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *common, *b_args, C.byref(o), None, 0, p_bd))
    abi.check(lib.mtd_ql_local_forces_bonds(N, abi.ptr(d_pos), abi.ptr(f_vir), dt, C.byref(box), *common, *b_args, C.byref(o), abi.ptr(virial),
                                            N + 3, p_bd))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        partials = s[off(p_part):off(p_part) + n_part.value].copy()
        take = lambda p: s[off(p):off(p) + N].copy()
        assert (p_b.value is None) == (bonds is None or entry != "bonds")
        return dict(s=partials.sum() / n_global, c=take(p_c), n=take(p_n), v=take(p_v), b=take(p_b) if p_b.value else None,
                    F=force.cpu().numpy().astype(np.float64), F_vir=f_vir.cpu().numpy().astype(np.float64), raw=virial.cpu().numpy(),
                    partials=partials)
    return gate.done(read)


def compare(g, r, bias, dtype, types=None, type_id=0):
    """value, per-particle arrays, forces and virial against the restatement (computed with bias=`bias`)"""
    top = lambda x: np.abs(x).max()
    N = len(r["c"])
    print("c_i: max |d| %.3e of %.3e; n_i: %.3e of %.3e; b_i: %.3e of %.3e; v_i: %.3e of %.3e; s %.15g vs %.15g (%.2e relative)"
          % (top(g["c"] - r["c"]), top(r["c"]), top(g["n"] - r["n"]), top(r["n"]), top(g["b"] - r["b"]), top(r["b"]), top(g["v"] - r["v"]),
             top(r["v"]), g["s"], r["s"], abs(g["s"] / r["s"] - 1.0)))
    F_ref = -bias * r["grad"]
    fs = top(F_ref)
    err = top(g["F"][:, :3] - F_ref)
    vg = g["raw"][:, :N].astype(np.float64).T
    v_top, v_err = top(r["virial"]), top(vg - r["virial"])
    w_top, w_err = top(r["W"]), top(vg.sum(axis=0) - r["W"])
    print("forces: max |d| %.3e of max |F| %.3e (%.3e relative); virial: %.3e of max |virial_i| %.3e (%.3e relative); sums: %.3e of max |W| "
          "%.3e (%.3e relative)" % (err, fs, err / fs if fs else 0.0, v_err, v_top, v_err / v_top if v_top else 0.0, w_err, w_top,
                                    w_err / w_top if w_top else 0.0))
    for key in ("F", "F_vir", "raw", "c", "n", "v", "b", "partials"):
        assert np.isfinite(g[key]).all(), key
    for key in ("c", "n", "b", "v"):
        assert top(g[key] - r[key]) <= 1e-11 * top(r[key]), key
    assert g["s"] == pytest.approx(r["s"], rel=1e-10)
    tol = 1e-9 if dtype == np.float64 else 2e-7
    assert fs > 0 and v_top > 0
    assert err <= tol * fs
    assert v_err <= tol * v_top
    if dtype == np.float64:
        assert w_err <= 1e-9 * w_top
    assert np.array_equal(g["F"], g["F_vir"])                          # the virial must not perturb the force sums
    assert np.all(g["F"][:, 3] == 0.0)
    assert np.all(g["raw"][:, N:] == SENTINEL)                          # the padding of every component is left alone
    if types is not None:
        other = types != type_id
        assert other.sum() > 0
        assert np.all(g["F"][other] == 0.0) and np.all(vg[other] == 0.0)
        for key in ("c", "n", "b", "v"):
            assert np.all(g[key][other] == 0.0), key


_snapshots = {}
_refs = {}


def snapshot(cells, dtype):
    """the parity snapshot, rounded to the dtype, with its list at r_cut + 0.15: built once per size and dtype"""
    key = (cells, np.dtype(dtype).name)
    if key not in _snapshots:
        case = bonds_ref.noisy_fcc(cells)
        pos = case["pos"].astype(dtype).astype(np.float64)
        _snapshots[key] = (pos, case["L"], case["types"], util.build_nlist(pos, case["L"], 1.55))
    return _snapshots[key]


def reference(key, *args, **kw):
    """the restatement's answer, computed once per key and left unchanged"""
    if key not in _refs:
        _refs[key] = bonds_ref.compute(*args, **kw)
    return _refs[key]


def ramp_is_populated(r, bonds=BONDS, parts=(0, 1, 2)):
    """from the REFERENCE's per-entry d: each of the named parts (0 below, 1 inside, 2 above the ramp) holds at least 5 % of the entries.
    Inside the ramp sigma' != 0: the part of the gradient that goes through the q vectors is exercised"""
    d = r["dent"]
    got = ((d <= bonds[0]).sum(), ((d > bonds[0]) & (d < bonds[1])).sum(), (d >= bonds[1]).sum())
    print("entries below / inside / above the ramp: %d / %d / %d of %d" % (*got, len(d)))
    assert min(got[k] for k in parts) >= 0.05 * len(d)
    return got


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cells", [3, 5])                               # N = 108: one full chunk of 64 and a partial one; N = 500
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_bonds_parity(abi, dtype, cells, combo):
    pos, L, types, nl = snapshot(cells, dtype)
    opt = COMBOS[combo]
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, E6, dtype, opt=opt)
    r = reference(("parity", cells, np.dtype(dtype).name, combo), pos, types, L, nl, 1.4, 1.2, 6, 0, E6, bias=BIAS, **opt)
    got = ramp_is_populated(r)
    if dtype == np.float64:
        assert got == {3: (426, 1006, 180), 5: (2000, 4952, 548)}[cells]
    if "gate" in combo:
        assert ((r["n"] > 10) & (r["n"] < 13)).sum() > 10               # the gate's ramp is populated
    compare(g, r, BIAS, dtype)


# ---- 2. other degrees: one, two and four gather windows, both force kernels -----------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lmax,Ql_ref,bonds", [(4, [0.2, 0, 1.0, 0.5, 1.0], (0.3, 0.8)),      # l = 0 in use, an odd degree
                                               (5, [0, 0.4, 0.2, 0.6, 1, 0.7], (-0.2, 0.5)),  # odd and even mixed; 20 slots: two windows
                                               (8, [0, 0, 0, 0, 1, 0, 1, 0, 0.5], (0.0, 0.6)),  # the compiled bound 8: pass 1 scales the row it wrote
                                               (12, QL_12, (0.0, 0.6))])                      # 49 slots: four windows, the direct force pass
def test_bonds_other_degrees(abi, dtype, lmax, Ql_ref, bonds):
    pos, L, types, nl = snapshot(3, dtype)
    opt = dict(bonds=bonds, switch=(8.0, 4))
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, opt=opt)
    r = reference(("degrees", np.dtype(dtype).name, lmax), pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, bias=BIAS, **opt)
    ramp_is_populated(r, bonds=bonds, parts=(1,))
    compare(g, r, BIAS, dtype)


# ---- 3. other inputs ------------------------------------------------------------------------------------------------------------

def test_two_types_and_n_global(abi):
    case = bonds_ref.noisy_fcc(4, seed=5)
    pos, L = case["pos"], case["L"]
    N = len(pos)
    types = (np.random.default_rng(1).random(N) < 0.3).astype(np.int32)
    nl = util.build_nlist(pos, L, 1.6)
    opt = dict(bonds=BONDS, switch=(4.0, 6), gate=(4, 8))
    for type_id in (0, 1):
        args = (1.45, 1.1, 6, type_id, [0.5, 0, 0.25, 0, 1, 0, 1])
        g = run_gpu(abi, pos, types, L, nl, *args, np.float64, opt=opt, n_global=3 * N)
        r = bonds_ref.compute(pos, types, L, nl, *args, n_global=3 * N, bias=BIAS, **opt)
        if type_id == 0:
            assert 0 < ((r["n"] > 4) & (r["n"] < 8)).sum()              # some particles inside the gate's ramp
        compare(g, r, BIAS, np.float64, types=types, type_id=type_id)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_triclinic_box(abi, dtype):
    """a sheared noisy crystal in the sheared box: HOOMD's minimum image with tilt factors in all four passes"""
    pos, L = util.fcc_lattice(4)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = (((pos + np.random.default_rng(11).normal(0, 0.1, pos.shape)) / L) @ h.T).astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = brute_nlist(pos, h, 1.6)
    args = (1.45, 1.15, 6, 0, [0, 0, 0.3, 0, 1, 0, 1])
    opt = COMBOS["bonds+switch"]
    g = run_gpu(abi, pos, types, L, nl, *args, dtype, opt=opt, tilt=tilt)
    r = bonds_ref.compute(pos, types, L, nl, *args, tilt=tilt, bias=BIAS, **opt)
    ramp_is_populated(r)
    compare(g, r, BIAS, dtype)


@pytest.mark.parametrize("combo", ["bonds", "bonds+switch+gate"])
def test_buffered_and_shuffled_lists(abi, combo):
    """a list built at r_cut + 0.6 (most of its entries are out of range) with every row's order permuted gives what the tight list gives:
    values within their tolerance, forces within the force tolerance (the sums follow the list order)"""
    case = bonds_ref.noisy_fcc(5, seed=9)
    pos, L = case["pos"], case["L"]
    N = len(pos)
    types = (np.random.default_rng(2).random(N) < 0.15).astype(np.int32)
    args = (1.4, 1.2, 6, 0, [0, 0, 0.3, 0, 1, 0, 1])
    opt = COMBOS[combo]
    tight = util.build_nlist(pos, L, 1.4)
    head, nn, lst = [np.array(x).copy() for x in util.build_nlist(pos, L, 2.0)]
    assert len(lst) > 2 * len(tight[2])
    rng = np.random.default_rng(2)
    for i in range(N):
        lst[head[i]:head[i] + nn[i]] = rng.permutation(lst[head[i]:head[i] + nn[i]])
    a = run_gpu(abi, pos, types, L, tight, *args, np.float64, opt=opt)
    b = run_gpu(abi, pos, types, L, (head, nn, lst), *args, np.float64, opt=opt)
    r = bonds_ref.compute(pos, types, L, (head, nn, lst), *args, bias=BIAS, **opt)
    compare(b, r, BIAS, np.float64, types=types)
    for key in ("c", "n", "b", "v"):
        assert np.abs(a[key] - b[key]).max() <= 1e-11 * np.abs(a[key]).max(), key
    assert a["s"] == pytest.approx(b["s"], rel=1e-10)
    assert np.abs(a["F"] - b["F"]).max() <= 1e-9 * np.abs(a["F"]).max()
    assert np.abs(a["raw"] - b["raw"]).max() <= 1e-9 * np.abs(a["raw"][:, :N]).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dilute_edge_case(abi, dtype):
    """particles with n_i = 0, with 0 < n_i < 2 and inside the gate's ramp, products d from -0.30 to 1: everything finite and as the
    restatement has it; with fp64 arrays the known answer"""
    case, opt = bonds_ref.dilute_case()
    pos = case["pos"].astype(dtype).astype(np.float64)
    nl = util.build_nlist(pos, case["L"], 1.6)
    args = (case["r_cut"], case["r_on"], case["lmax"], 0, case["Ql_ref"])
    g = run_gpu(abi, pos, case["types"], case["L"], nl, *args, dtype, opt=opt)
    r = bonds_ref.compute(pos, case["types"], case["L"], nl, *args, bias=BIAS, **opt)
    lonely = r["n"] == 0
    assert lonely.sum() >= 5 and ((r["n"] > 2) & (r["n"] < 6)).sum() >= 15
    compare(g, r, BIAS, dtype)
    for key in ("v", "c", "b", "F"):
        assert np.all(g[key][lonely] == 0.0), key
    if dtype == np.float64:
        assert g["s"] == pytest.approx(0.24648936191120521, rel=1e-10)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("combo", ["bonds", "bonds+gate"])
def test_row_lengths_0_to_13_and_skipped_entries(abi, dtype, combo):
    """the walk over a row at every row length 0 .. 13 (run A), and the same rows with a self entry and two entries >= N each, at the
    front, in the middle and at the end (run B): both give what the restatement gives for the clean list"""
    pos, L, types, nl, padded, _ = cluster_case(dtype)
    opt = dict(bonds=(0.0, 0.9), switch=(3.0, 4))
    if combo == "bonds+gate":
        opt["gate"] = (2, 9)
    args = (1.4, 1.2, 6, 0, [0, 0, 0, 0, 1, 0, 1])
    r = reference(("clusters", np.dtype(dtype).name, combo), pos, types, L, nl, *args, bias=BIAS, **opt)
    ramp_is_populated(r, bonds=(0.0, 0.9), parts=(0, 1))
    assert len(padded[2]) == len(nl[2]) + 3 * len(pos)
    for lists in (nl, padded):
        g = run_gpu(abi, pos, types, L, lists, *args, dtype, opt=opt)
        compare(g, r, BIAS, dtype)


def test_chunk_loop(abi):
    """70 304 particles: more than 1024 chunks of 64, so every block walks several chunks in all four passes"""
    case = bonds_ref.noisy_fcc(26)
    pos, L = case["pos"], case["L"]
    N = len(pos)
    assert N == 70304 and (N + 63) // 64 > 1024
    types = np.zeros(N, dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.4)
    opt = dict(bonds=BONDS, switch=(3.0, 4))
    Ql_ref = [0, 0, 0, 0, 1]
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 4, 0, Ql_ref, np.float64, opt=opt)
    assert len(g["partials"]) == 1024
    r = bonds_ref.compute(pos, types, L, nl, 1.4, 1.2, 4, 0, Ql_ref, bias=BIAS, **opt)
    ramp_is_populated(r, parts=(0, 1))
    compare(g, r, BIAS, np.float64)


# ---- 4. bits --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("entry", ["null", "zero"])
def test_bonds_off_is_the_opt_and_virial_entry_points_bit_for_bit(abi, dtype, entry):
    pos, L, types, nl = snapshot(5, dtype)
    for lmax, Ql_ref in ((6, [0, 0, 0, 0, 1, 0, 1]), (12, QL_12)):
        for opt in (dict(), dict(switch=(0.25, 3), gate=(10, 13)), dict(average=True, switch=(0.12, 3))):
            old = run_gpu_opt(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, opt=opt)
            old_v = run_gpu_virial(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, opt=opt, pitch=len(pos) + 3)
            new = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, opt=opt, entry=entry)
            for key in ("c", "n", "v", "partials", "F"):
                assert np.array_equal(old[key], new[key]), key
            assert np.array_equal(old_v["F"].astype(np.float64), new["F_vir"]) and np.array_equal(old_v["raw"], new["raw"])
            assert new["b"] is None


def test_reproducible_bits(abi):
    """no atomics, fixed orders: two identical calls give identical bits"""
    pos, L, types, nl = snapshot(5, np.float64)
    for lmax, Ql_ref in ((6, E6), (12, QL_12)):
        opt = COMBOS["bonds+switch+gate"]
        a = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, np.float64, opt=opt)
        b = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, np.float64, opt=opt)
        for key in ("c", "n", "v", "b", "partials", "F", "raw"):
            assert np.array_equal(a[key], b[key]), key


def test_bias_from_device_and_host(abi):
    pos, L, types, nl = snapshot(5, np.float64)
    opt = COMBOS["bonds+switch"]
    dev = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, E6, np.float64, opt=opt, bias=-1.7, bias_on_device=True)
    host = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, E6, np.float64, opt=opt, bias=-1.7, bias_on_device=False)
    assert np.array_equal(dev["F"], host["F"]) and np.array_equal(dev["raw"], host["raw"])
    r = bonds_ref.compute(pos, types, L, nl, 1.4, 1.2, 6, 0, E6, bias=-1.7, **opt)
    compare(dev, r, -1.7, np.float64)
    zero = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, E6, np.float64, opt=opt, bias=0.0, bias_on_device=False)
    assert np.all(zero["F"] == 0.0)


# ---- 5. through the Python API --------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


API_BONDS, API_SWITCH, API_GATE = dict(d_lo=0.3, d_hi=0.8), dict(c0=6.5, p=6), dict(n_lo=10, n_hi=13)
OPT = dict(bonds=BONDS, switch=(6.5, 6))
API_TOL = 1e-7                                                          # the bias factor from the oracle's grid is known to 1e-7 only


def _api_system(seed=12):
    case = bonds_ref.noisy_fcc(5, seed=seed)
    return case["pos"], case["L"], case["types"]


def _oracle_bias(ref, kw, values, steps):
    """the oracle's grid driven with the given CV values: prepRun(0) + `steps` updates; returns the list of bias factors per call"""
    g = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    return [g.update_bias(t, values) for t in range(steps + 1)]


def test_bonds_alone_on_a_grid(api, ref):
    """cv.steinhardt_local(bonds, switch) on a 512-point well-tempered grid, 5 steps: the value the engine used, c_i, b_i, v_i, the bias
    factor and the force array against the oracle's grid driven with the restatement's value"""
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    r = bonds_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, E6, **OPT)
    val = r["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=E6, nlist=nl, type="A", sigma=0.02 * val, bonds=API_BONDS, switch=API_SWITCH)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    context.run(5)
    t = context.current.system.getCurrentTimeStep()
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-10)
    assert st.cpp_force.getLogValue("cv_steinhardt_local", t) == pytest.approx(val, rel=1e-10)
    assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(val, rel=1e-10)      # what the engine took from the block sums
    assert np.abs(st.get_local() - r["c"]).max() <= 1e-11 * np.abs(r["c"]).max()
    assert np.abs(st.get_bonds() - r["b"]).max() <= 1e-11 * np.abs(r["b"]).max()
    assert np.abs(st.get_switched() - r["v"]).max() <= 1e-11 * np.abs(r["v"]).max()
    assert np.abs(st.get_coordination() - r["n"]).max() <= 1e-11 * np.abs(r["n"]).max()
    b = _oracle_bias(ref, dict(sigma=[0.02 * val], cv_min=[0.55 * val], cv_max=[1.3 * val], num_points=[512]), [val], 5)[-1]
    assert abs(b[0]) > 0
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    F = st.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert np.all(F[:, 3] == 0.0)


def test_invalid_bonds_raise(api):
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    kw = dict(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=E6, nlist=nl, type="A")
    for bad in (dict(bonds=dict(d_lo=-1.5, d_hi=0.5)), dict(bonds=dict(d_lo=0.5, d_hi=0.5)), dict(bonds=dict(d_lo=0.7, d_hi=0.5)),
                dict(bonds=dict(d_lo=0.5, d_hi=1.5)), dict(bonds=dict(d_lo=float("nan"), d_hi=0.5)), dict(bonds=dict(d_lo=0.5)),
                dict(bonds=(0.5, 0.7)), dict(bonds=dict(d_lo=0.5, d_hi=0.7, d_mid=0.6)), dict(bonds=API_BONDS, average=True),
                dict(bonds=API_BONDS, switch=dict(c0=0.0, p=3))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.steinhardt_local(**kw, **bad)
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.steinhardt_local(**{**kw, "Ql_ref": [0, 0, 0, 0, -0.5, 0, 1]}, bonds=API_BONDS)
    st = cv.steinhardt_local(**kw)
    with pytest.raises(RuntimeError):
        st.cpp_force.setBonds(0.7, 0.5)
    with pytest.raises(RuntimeError):
        st.get_bonds()                                                 # no bond count without the option
    st.cpp_force.setBonds(0.5, 0.7)
    with pytest.raises(RuntimeError):
        st.cpp_force.setAverage(True)
    st.cpp_force.clearBonds()
    st.cpp_force.setAverage(True)
    with pytest.raises(RuntimeError):
        st.cpp_force.setBonds(0.5, 0.7)


def test_changing_options_between_runs_takes_effect(api):
    """a change of options invalidates the cached step and grows the scratch: plain -> bonds -> average -> bonds + switch + gate -> plain"""
    context, cv, integrate = api
    pos, L, types = _api_system(seed=14)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=E6, nlist=nl, type="A", sigma=1.0)
    st.set_grid(0.0, 13.0, 64)
    seen = []
    for kw, opt in ((dict(), dict()), (dict(bonds=API_BONDS), dict(bonds=BONDS)), (dict(average=True), None),
                    (dict(bonds=API_BONDS, switch=API_SWITCH, gate=API_GATE), dict(bonds=BONDS, switch=(6.5, 6), gate=(10, 13))), (dict(), dict())):
        st.set_options(**kw)
        if opt is None:                                                 # the average in between: only that it runs and bonds are gone
            context.run(1)
            with pytest.raises(RuntimeError):
                st.get_bonds()
            continue
        r = bonds_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, E6, gradient=False, **opt)
        t = context.current.system.getCurrentTimeStep()
        assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)         # the same time step: the cache must have gone
        assert np.abs(st.get_switched() - r["v"]).max() <= 1e-11 * np.abs(r["v"]).max()
        if "bonds" in opt:
            assert np.abs(st.get_bonds() - r["b"]).max() <= 1e-11 * np.abs(r["b"]).max()
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)
        seen.append(r["s"])
    assert seen[0] == seen[3] and len({round(s, 6) for s in seen[:3]}) == 3


def test_bonds_on_a_device_list_follow_the_particles(api):
    """cv.nlist_cell(device=True): particles displaced between runs — the list rebuilds (and may grow: so does the scratch), value and
    forces follow"""
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5, r_buff=0.4, device=True)
    val0 = bonds_ref.compute(pos, types, L, util.build_nlist(pos, L, 1.5), 1.4, 1.2, 6, 0, E6, gradient=False, **OPT)["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=E6, nlist=nl, type="A", sigma=0.02 * val0, bonds=API_BONDS, switch=API_SWITCH)
    st.set_grid(0.05 * val0, 1.3 * val0, 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(val0, rel=1e-10)
    rng = np.random.default_rng(5)
    p = pos.copy()
    values = [val0]
    for k in range(2):
        p = p + rng.normal(0, 0.12, p.shape)                                    # far more than r_buff / 2 = 0.2 for some particle
        context.set_positions(p, types)
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        r = bonds_ref.compute(p, types, L, util.build_nlist(p, L, 1.5), 1.4, 1.2, 6, 0, E6, **OPT)
        values.append(r["s"])
        assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)
        assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["s"], rel=1e-10)
        assert nl.cpp_nlist.getNumRebuilds() == 2 + k
        b = meta.cpp_integrator.getBiasFactors()[0]
        F = st.cpp_force.getForceArray()
        F_ref = -b * r["grad"]
        assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert abs(values[-1] - values[0]) > 1e-3 * values[0]                         # the value did move


def test_harmonic_umbrella_and_virial(api, ref):
    """a harmonic umbrella adds to the bias factor; with the pressure flag set get_virial() is the restatement's for that factor"""
    context, cv, integrate = api
    pos, L, types = _api_system(seed=15)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(True)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    val = bonds_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, E6, gradient=False, **OPT)["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=E6, nlist=nl, type="A", sigma=0.02 * val, bonds=API_BONDS, switch=API_SWITCH)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    kappa, cv0 = 35.0, 0.8 * val
    st.set_params(umbrella="harmonic", kappa=kappa, cv0=cv0)
    context.run(3)
    t = context.current.system.getCurrentTimeStep()
    b = _oracle_bias(ref, dict(sigma=[0.02 * val], cv_min=[0.55 * val], cv_max=[1.3 * val], num_points=[512]), [val], 3)[-1]
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    total = b[0] + kappa * (val - cv0)
    assert abs(kappa * (val - cv0)) > 0.1 * abs(total)
    r = bonds_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, E6, bias=total, **OPT)
    F = st.cpp_force.getForceArray()
    F_ref = -total * r["grad"]
    assert np.abs(F[:, :3] - F_ref).max() <= API_TOL * np.abs(F_ref).max()
    assert st.cpp_force.getUmbrellaPotential(t) == pytest.approx(0.5 * kappa * (val - cv0) ** 2, rel=1e-9)
    per, W = st.get_virial(per_particle=True), st.get_virial()
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["W"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["W"]).max(), w_top))
    assert per.shape == (6, len(pos)) and w_top > 0
    assert np.abs(per.T - r["virial"]).max() <= API_TOL * top
    assert np.abs(W - r["W"]).max() <= API_TOL * w_top
