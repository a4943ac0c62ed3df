"""GPU parity: the virial of the local Steinhardt variable's bias force (mtd_ql_local_forces_virial, cv.steinhardt_local.get_virial)
against the fp64 numpy restatement in the scatter form (tests/ql_local_virial_ref.py, itself checked on the CPU against strain
differences in tests/test_ql_local_virial_ref.py).  Tolerances are the project's own for the force of this variable — the virial is
the same arithmetic plus one product and one halving: per-particle virial within 1e-9 of max|virial_i| with fp64 arrays and 2e-7 with
fp32 arrays (one rounding on store; the fp32 snapshot is the rounded array, on both sides), the six sums in fp64 within 1e-9 of max|W|.
Through the Python API the bias factor is known from the oracle's grid to 1e-7 only (tests/test_gpu_ql_local_avg.py holds the force
array to 1e-7 there for that reason): the same 1e-7 holds for the virial there.
Every call also runs mtd_ql_local_forces_opt on the same table: the force array of the virial call must be that one bit for bit."""
import ctypes as C

import numpy as np
import pytest

import ql_local_avg_ref as avg_ref
import ql_local_virial_ref as vir_ref
import stream_gate
import util
from test_gpu_ql_local_avg import brute_nlist, noisy_fcc, snapshot

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

QL_46 = [0, 0, 0, 0, 1, 0, 1]
QL_12 = [0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0.5, 0.3, 0.25]
COMBOS = dict(avg_ref.COMBINATIONS)
COMBOS["plain"] = dict()
COMBOS["average+switch+gate(10,16)"] = dict(average=True, switch=(0.12, 3), gate=(10, 16))   # the ramp is populated on the dense crystal
SENTINEL = -7.25
BIAS = 0.9


def run_gpu(abi, pos, types, L, nl, rcut, ron, lmax, type_id, Ql_ref, dtype, opt=None, n_global=None, bias=BIAS, tilt=None, bias_on_device=True,
            pitch=None, pass_virial=True, gate=None):
    """pass 1, then mtd_ql_local_forces_opt and mtd_ql_local_forces_virial on the same table.  Returns dict(F_opt, F, raw): the two force
    arrays (N, 4) as stored and the whole virial buffer (6, pitch), which starts as SENTINEL.  The scratch starts as NaN.  gate: the
    stream the calls run on and how their inputs arrive (tests/stream_gate.py; None: the NULL stream)."""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N = len(pos)
    n_global = N if n_global is None else n_global
    pitch = N if pitch is None else pitch
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    assert int(np.asarray(nl[0]).astype(np.int64)[-1] + np.asarray(nl[1]).astype(np.int64)[-1]) <= len(nl[2])
    o = abi.QlLocalOptions.make(**(opt or {}))
    scratch = torch.full((lib.mtd_ql_local_scratch_doubles_opt(N, lmax, len(nl[2]), C.byref(o)),), float("nan"), dtype=torch.float64, device="cuda")
    p_part, p_c, p_n, p_v = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_part = C.c_uint()
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    common = (abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), rcut, ron, lmax, type_id, util.dbl_array(Ql_ref), n_global, abi.ptr(scratch))
    f_opt = torch.full((N, 4), 3.0, dtype=tdt, device="cuda")
    f_vir = torch.full((N, 4), 5.0, dtype=tdt, device="cuda")
    virial = torch.full((6, pitch), SENTINEL, dtype=tdt, device="cuda")
    stream = gate.arm()
    b_args = (abi.ptr(d_bias) if bias_on_device else None, 0.0 if bias_on_device else bias, stream)
    abi.check(lib.mtd_ql_local_accumulate_opt(N, abi.ptr(d_pos), dt, C.byref(box), *common, C.byref(p_part), C.byref(n_part), C.byref(p_c),
                                              C.byref(p_n), stream, C.byref(o), C.byref(p_v)))
    abi.check(lib.mtd_ql_local_forces_opt(N, abi.ptr(d_pos), abi.ptr(f_opt), dt, C.byref(box), *common, *b_args, C.byref(o)))
    abi.check(lib.mtd_ql_local_forces_virial(N, abi.ptr(d_pos), abi.ptr(f_vir), dt, C.byref(box), *common, *b_args, C.byref(o),
                                             abi.ptr(virial) if pass_virial else None, pitch))
    return gate.done(lambda: dict(F_opt=f_opt.cpu().numpy(), F=f_vir.cpu().numpy(), raw=virial.cpu().numpy()))


_refs = {}


def reference(key, *args, **kw):
    """the restatement's answer, computed once per key and left unchanged"""
    if key not in _refs:
        _refs[key] = vir_ref.compute(*args, **kw)
    return _refs[key]


def compare(g, r, dtype, N, types=None, type_id=0):
    """per-particle virial (the first N columns of the buffer) and, with fp64 arrays, the six sums against the restatement; the force
    array against that of mtd_ql_local_forces_opt, bit for bit"""
    vg = g["raw"][:, :N].astype(np.float64).T                           # (N, 6) like the reference
    top = np.abs(r["virial"]).max()
    err = np.abs(vg - r["virial"]).max()
    w_top = np.abs(r["W"]).max()
    w_err = np.abs(vg.sum(axis=0) - r["W"]).max()
    print("virial: max |d| %.3e of max |virial_i| %.3e (%.3e relative); sums: %.3e of max |W| %.3e (%.3e relative)"
          % (err, top, err / top if top else 0.0, w_err, w_top, w_err / w_top if w_top else 0.0))
    assert np.isfinite(g["raw"]).all() and np.isfinite(g["F"]).all()
    assert top > 0
    assert err <= (1e-9 if dtype == np.float64 else 2e-7) * top
    if dtype == np.float64:
        assert w_err <= 1e-9 * w_top
    assert np.array_equal(g["F"], g["F_opt"])                          # the virial must not perturb the force sums
    assert np.abs(g["F"][:, :3]).max() > 0 and np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        assert np.all(vg[types != type_id] == 0.0)
    return vg


# ---- 1. parity and force bits ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cells", [3, 5])                               # N = 108: one full chunk of 64 and a partial one; N = 500
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_virial_parity(abi, dtype, cells, combo):
    pos, L, types, nl = snapshot(cells, dtype)
    opt = COMBOS[combo]
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, dtype, opt=opt)
    r = reference(("parity", cells, np.dtype(dtype).name, combo), pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, BIAS, **opt)
    if "(10,16)" in combo:
        assert ((r["n"] > 10) & (r["n"] < 16)).sum() > 0
    compare(g, r, dtype, len(pos))


# ---- 2. both force kernels ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("average", [False, True])
@pytest.mark.parametrize("lmax,Ql_ref", [(6, QL_46),                    # rows of 208 bytes: the pass through LDS tiles
                                         (12, QL_12)])                  # rows of 784 bytes: the direct pass
def test_tile_and_direct_force_pass(abi, dtype, average, lmax, Ql_ref):
    pos, L, types, nl = snapshot(5, dtype)
    opt = dict(average=True, switch=(0.12, 3)) if average else dict()
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, opt=opt)
    r = reference(("kernels", np.dtype(dtype).name, average, lmax), pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, BIAS, **opt)
    compare(g, r, dtype, len(pos))


# ---- 3. d_virial == NULL --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lmax,Ql_ref", [(6, QL_46), (12, QL_12)])
def test_null_virial_is_the_opt_entry_point(abi, dtype, lmax, Ql_ref):
    """the same kernels, the same bits; the virial buffer is never passed and stays as it was"""
    pos, L, types, nl = snapshot(5, dtype)
    for opt in (dict(), COMBOS["average+switch+gate"]):
        g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, opt=opt, pass_virial=False)
        assert np.array_equal(g["F"], g["F_opt"])
        assert np.abs(g["F"][:, :3]).max() > 0
        assert np.all(g["raw"] == SENTINEL)


# ---- 4. pitch -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pitch_beyond_the_particles(abi, dtype):
    pos, L, types, nl = snapshot(3, dtype)
    N = len(pos)
    opt = COMBOS["average+switch"]
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, dtype, opt=opt, pitch=N + 37)
    r = reference(("parity", 3, np.dtype(dtype).name, "average+switch"), pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, BIAS, **opt)
    compare(g, r, dtype, N)
    assert g["raw"].shape == (6, N + 37)
    assert np.all(g["raw"][:, N:] == SENTINEL)                          # the padding of every component is left alone


# ---- 5. two types and n_global --------------------------------------------------------------------------------------------------

def test_two_types_and_n_global(abi):
    pos, L = noisy_fcc(4, seed=5)
    N = len(pos)
    types = (np.random.default_rng(1).random(N) < 0.3).astype(np.int32)
    nl = util.build_nlist(pos, L, 1.6)
    opt = COMBOS["average+switch+gate"]
    seen = []
    for type_id in (0, 1):
        args = (1.45, 1.1, 6, type_id, [0.5, 0, 0.25, 0, 1, 0, 1])
        g3 = run_gpu(abi, pos, types, L, nl, *args, np.float64, opt=opt, n_global=3 * N)
        r3 = reference(("types", type_id), pos, types, L, nl, *args, BIAS, n_global=3 * N, **opt)
        v3 = compare(g3, r3, np.float64, N, types=types, type_id=type_id)
        seen.append(v3)
        if type_id == 0:
            assert 0 < ((r3["n"] > 4) & (r3["n"] < 8)).sum()             # some particles inside the gate's ramp
    g1 = run_gpu(abi, pos, types, L, nl, *args, np.float64, opt=opt)     # N_global = N: three times the values
    v1 = g1["raw"].T
    assert np.abs(v1 - 3.0 * seen[1]).max() <= 1e-9 * np.abs(v1).max()


# ---- 6. triclinic box -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_triclinic_box(abi, dtype):
    """a sheared fcc crystal in the sheared box: d_kj is HOOMD's minimum image with tilt factors"""
    pos, L = noisy_fcc(4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = brute_nlist(pos, h, 1.6)
    args = (1.45, 1.15, 6, 0, [0, 0, 0.3, 0, 1, 0, 1])
    opt = COMBOS["average+switch"]
    g = run_gpu(abi, pos, types, L, nl, *args, dtype, opt=opt, tilt=tilt)
    r = vir_ref.compute(pos, types, L, nl, *args, BIAS, tilt=tilt, **opt)
    assert r["n"].min() > 3
    compare(g, r, dtype, len(pos))
    # the pair vectors did cross the tilted faces: without the tilt in the minimum image the restatement gives another virial
    flat = vir_ref.compute(pos, types, L, nl, *args, BIAS, **opt)
    assert np.abs(flat["virial"] - r["virial"]).max() > 1e-3 * np.abs(r["virial"]).max()


# ---- 7. lists -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", ["average+switch+gate", "switch+gate"])
def test_buffered_and_shuffled_lists(abi, combo):
    """a list built at r_cut + 0.4 with every row's order permuted gives what the tight list gives (the sums follow the list order)"""
    pos, L = noisy_fcc(5, seed=9)
    N = len(pos)
    types = (np.random.default_rng(2).random(N) < 0.15).astype(np.int32)
    args = (1.4, 1.2, 6, 0, [0, 0, 0.3, 0, 1, 0, 1])
    opt = COMBOS[combo]
    tight = util.build_nlist(pos, L, 1.4)
    head, nn, lst = [np.array(x).copy() for x in util.build_nlist(pos, L, 1.8)]
    assert len(lst) > 2 * len(tight[2])
    rng = np.random.default_rng(2)
    for i in range(N):
        lst[head[i]:head[i] + nn[i]] = rng.permutation(lst[head[i]:head[i] + nn[i]])
    a = run_gpu(abi, pos, types, L, tight, *args, np.float64, opt=opt)
    b = run_gpu(abi, pos, types, L, (head, nn, lst), *args, np.float64, opt=opt)
    r = vir_ref.compute(pos, types, L, (head, nn, lst), *args, BIAS, **opt)
    compare(b, r, np.float64, N, types=types)
    compare(a, r, np.float64, N, types=types)
    assert np.abs(a["raw"] - b["raw"]).max() <= 1e-9 * np.abs(a["raw"]).max()


# ---- 8. dilute case -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dilute_edge_case(abi, dtype):
    """particles with n_i = 0, with 0 < n_i < 2 and inside the gate's ramp: everything finite, rows without a neighbour exactly 0"""
    case = avg_ref.dilute_case()
    opt = {k: case.pop(k) for k in ("average", "switch", "gate")}
    pos = case["pos"].astype(dtype).astype(np.float64)
    nl = util.build_nlist(pos, case["L"], 1.6)
    args = (case["r_cut"], case["r_on"], case["lmax"], 0, case["Ql_ref"])
    g = run_gpu(abi, pos, case["types"], case["L"], nl, *args, dtype, opt=opt)
    r = vir_ref.compute(pos, case["types"], case["L"], nl, *args, BIAS, **opt)
    lonely = r["n"] == 0
    assert lonely.sum() >= 5 and ((r["n"] > 2) & (r["n"] < 6)).sum() >= 15
    vg = compare(g, r, dtype, len(pos))
    assert np.all(vg[lonely] == 0.0)


# ---- 9. bias --------------------------------------------------------------------------------------------------------------------

def test_bias_from_device_and_host_zero_bias_and_reproducible_bits(abi):
    pos, L, types, nl = snapshot(5, np.float64)
    opt = COMBOS["average+switch"]
    call = lambda **kw: run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, np.float64, opt=opt, **kw)
    dev = call(bias=-1.7, bias_on_device=True)
    host = call(bias=-1.7, bias_on_device=False)
    again = call(bias=-1.7, bias_on_device=True)
    assert np.array_equal(dev["raw"], host["raw"]) and np.array_equal(dev["F"], host["F"])
    assert np.array_equal(dev["raw"], again["raw"]) and np.array_equal(dev["F"], again["F"])     # no atomics, fixed orders
    r = vir_ref.compute(pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, -1.7, **opt)
    compare(dev, r, np.float64, len(pos))
    zero = call(bias=0.0, bias_on_device=False)
    assert np.all(zero["raw"] == 0.0) and np.all(zero["F"] == 0.0)


# ---- 10. chunk loop -------------------------------------------------------------------------------------------------------------

def test_chunk_loop(abi):
    """70 304 particles: more than 1024 chunks of 64, so every block walks several chunks"""
    pos, L = noisy_fcc(26)
    N = len(pos)
    assert N == 70304 and (N + 63) // 64 > 1024
    types = np.zeros(N, dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.4)
    opt = COMBOS["average+switch"]
    Ql_ref = [0, 0, 0, 0, 1]
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 4, 0, Ql_ref, np.float64, opt=opt)
    r = vir_ref.compute(pos, types, L, nl, 1.4, 1.2, 4, 0, Ql_ref, BIAS, **opt)
    compare(g, r, np.float64, N)


# ---- 11. through the Python API -------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


SWITCH, GATE = dict(c0=0.12, p=3), dict(n_lo=4, n_hi=8)
OPT = dict(average=True, switch=(0.12, 3), gate=(4, 8))
API_TOL = 1e-7                                                          # the bias factor from the oracle's grid: see the module docstring


def _api_system(seed=12):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(seed).normal(0, 0.05, pos.shape)
    return pos, L, np.zeros(len(pos), dtype=np.int32)


def _umbrella_run(api, pressure, steps=3):
    """the set-up of test_harmonic_umbrella_adds_to_the_bias_factor; returns (st, meta, pos, types, L, lists, val, kappa, cv0)"""
    context, cv, integrate = api
    pos, L, types = _api_system(seed=15)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    val = avg_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, QL_46, gradient=False, **OPT)["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=0.02 * val, average=True, switch=SWITCH, gate=GATE)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    kappa, cv0 = 35.0, 0.8 * val
    st.set_params(umbrella="harmonic", kappa=kappa, cv0=cv0)
    context.run(steps)
    return st, meta, pos, types, L, lists, val, kappa, cv0


def test_api_virial_with_umbrella_and_flag_off(api, ref):
    """(a) pressure flag set: get_virial() and cpp_force.getVirial() against the restatement, the bias factor being the grid's plus the
    umbrella's kappa (s - cv0); (b) flag off: get_virial() raises and the force array is that of (a) bit for bit"""
    context, cv, integrate = api
    st, meta, pos, types, L, lists, val, kappa, cv0 = _umbrella_run(api, True)
    g = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", sigma=[0.02 * val], cv_min=[0.55 * val], cv_max=[1.3 * val],
                  num_points=[512])
    b = [g.update_bias(t, [val]) for t in range(4)][-1]
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    total = b[0] + kappa * (val - cv0)
    assert abs(kappa * (val - cv0)) > 0.1 * abs(total)
    r = vir_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, QL_46, total, **OPT)
    N = len(pos)
    per = st.get_virial(per_particle=True)
    raw = st.cpp_force.getVirial()
    W = st.get_virial()
    assert per.shape == (6, N) and per.dtype == np.float64 and W.shape == (6,) and W.dtype == np.float64
    assert raw.shape == (6, st.cpp_force.getVirialPitch()) and np.array_equal(raw[:, :N], per)
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["W"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["W"]).max(), w_top))
    assert w_top > 0.05
    assert np.abs(per.T - r["virial"]).max() <= API_TOL * top
    assert np.abs(W - r["W"]).max() <= API_TOL * w_top
    F_on = st.cpp_force.getForceArray().copy()
    assert np.abs(F_on[:, :3] + total * r["grad"]).max() <= API_TOL * np.abs(total * r["grad"]).max()
    context.current = None
    # (b)
    st, meta = _umbrella_run(api, False)[:2]
    with pytest.raises(RuntimeError):
        st.get_virial()
    with pytest.raises(RuntimeError):
        st.get_virial(per_particle=True)
    assert np.array_equal(st.cpp_force.getForceArray(), F_on)


def test_api_flag_on_then_off_leaves_no_stale_virial(api):
    """(c) flag on for one run, off for the next: the array the first run filled is all zeros after the second"""
    context, cv, integrate = api
    st = _umbrella_run(api, True, steps=2)[0]
    assert np.abs(st.cpp_force.getVirial()).max() > 0
    context.current.system_definition.getParticleData().setPressureFlag(False)
    context.run(1)
    assert np.all(st.cpp_force.getVirial() == 0.0)
    with pytest.raises(RuntimeError):
        st.get_virial()
    context.current.system_definition.getParticleData().setPressureFlag(True)
    context.run(1)
    assert np.abs(st.get_virial()).max() > 0


def test_api_virial_on_a_device_list_follows_the_particles(api):
    """(d) cv.nlist_cell(device=True): the particles are displaced between two runs, the list rebuilds, the virial follows"""
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(True)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5, r_buff=0.4, device=True)
    val0 = avg_ref.compute(pos, types, L, util.build_nlist(pos, L, 1.5), 1.4, 1.2, 6, 0, QL_46, gradient=False, **OPT)["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=0.02 * val0, average=True, switch=SWITCH, gate=GATE)
    st.set_grid(0.05 * val0, 1.3 * val0, 512)
    p = pos
    seen = []
    for k in range(2):
        if k:
            p = p + np.random.default_rng(5).normal(0, 0.12, p.shape)  # far more than r_buff / 2 = 0.2 for some particle
            context.set_positions(p, types)
        context.run(2 if k == 0 else 1)
        b = meta.cpp_integrator.getBiasFactors()[0]
        assert abs(b) > 0
        r = vir_ref.compute(p, types, L, util.build_nlist(p, L, 1.5), 1.4, 1.2, 6, 0, QL_46, b, **OPT)
        per, W = st.get_virial(per_particle=True), st.get_virial()
        top, w_top = np.abs(r["virial"]).max(), np.abs(r["W"]).max()
        print("run %d: per particle %.3e of %.3e; sums %.3e of %.3e" % (k, np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["W"]).max(), w_top))
        assert np.abs(per.T - r["virial"]).max() <= API_TOL * top
        assert np.abs(W - r["W"]).max() <= API_TOL * w_top
        F = st.cpp_force.getForceArray()
        assert np.abs(F[:, :3] + b * r["grad"]).max() <= API_TOL * np.abs(b * r["grad"]).max()
        seen.append(W / b)
    assert nl.cpp_nlist.getNumRebuilds() == 2
    assert np.abs(seen[1] - seen[0]).max() > 1e-3 * np.abs(seen[0]).max()   # the virial did move
