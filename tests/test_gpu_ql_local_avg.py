"""GPU parity: the options of the local Steinhardt variable (mtd_ql_local_*_opt, cv.steinhardt_local(average=, switch=, gate=)) against
the fp64 numpy restatement of their definition (tests/ql_local_avg_ref.py, itself checked on the CPU in tests/test_ql_local_avg_ref.py).
Tolerances are those tests/test_gpu_ql_local.py uses for the same arithmetic: c_i, n_i and v_i to 1e-11 of their largest value, s to
1e-10 relative, forces to 1e-9 of max|F| with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store); w == 0 and particles of
another type exactly 0.  The fp32 snapshot is the rounded array."""
import ctypes as C

import numpy as np
import pytest

import ql_local_avg_ref as avg_ref
import stream_gate
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

COMBOS = avg_ref.COMBINATIONS
QL_46 = [0, 0, 0, 0, 1, 0, 1]


def run_gpu(abi, pos, types, L, nl, rcut, ron, lmax, type_id, Ql_ref, dtype, opt=None, n_global=None, bias=0.9, tilt=None, bias_on_device=True,
            entry="opt", gate=None):
    """opt: dict(average=, switch=, gate=) -> the _opt entry points with that struct; entry = "null": the _opt entry points with
    opt == NULL; "zero": with an all-zero struct; "old": the entry points without options.  Returns dict(s, c, n, v, F, partials).
    The scratch starts as NaN: whatever the passes read they must have written.  gate: the stream the calls run on and how their inputs
    arrive (tests/stream_gate.py; None: the NULL stream)."""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N = len(pos)
    n_global = N if n_global is None else n_global
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    assert int(np.asarray(nl[0]).astype(np.int64)[-1] + np.asarray(nl[1]).astype(np.int64)[-1]) <= len(nl[2])
    o = abi.QlLocalOptions.make(**(opt or {}))
    p_opt = None if entry in ("null", "old") else C.byref(o)
    n_doubles = lib.mtd_ql_local_scratch_doubles(N, lmax) if entry == "old" else lib.mtd_ql_local_scratch_doubles_opt(N, lmax, len(nl[2]), p_opt)
    scratch = torch.full((n_doubles,), float("nan"), dtype=torch.float64, device="cuda")
    p_part, p_c, p_n, p_v = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_part = C.c_uint()
    force = torch.full((N, 4), 3.0, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    common = (abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), rcut, ron, lmax, type_id, util.dbl_array(Ql_ref), n_global, abi.ptr(scratch))
    stream = gate.arm()
    b_args = (abi.ptr(d_bias) if bias_on_device else None, 0.0 if bias_on_device else bias, stream)
    if entry == "old":
        abi.check(lib.mtd_ql_local_accumulate(N, abi.ptr(d_pos), dt, C.byref(box), *common, C.byref(p_part), C.byref(n_part), C.byref(p_c),
                                              C.byref(p_n), stream))
        abi.check(lib.mtd_ql_local_forces(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *common, *b_args))
        p_v = p_c
    else:
        abi.check(lib.mtd_ql_local_accumulate_opt(N, abi.ptr(d_pos), dt, C.byref(box), *common, C.byref(p_part), C.byref(n_part), C.byref(p_c),
                                                  C.byref(p_n), stream, p_opt, C.byref(p_v)))
        abi.check(lib.mtd_ql_local_forces_opt(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *common, *b_args, p_opt))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        partials = s[off(p_part):off(p_part) + n_part.value].copy()
        take = lambda p: s[off(p):off(p) + N].copy()
        return dict(s=partials.sum() / n_global, c=take(p_c), n=take(p_n), v=take(p_v), F=force.cpu().numpy().astype(np.float64), partials=partials)
    return gate.done(read)


def noisy_fcc(n, sigma=0.05, seed=777):
    pos, L = util.fcc_lattice(n)
    rng = np.random.default_rng(seed)
    return pos + rng.normal(0, sigma, pos.shape), L


def compare(g, r, bias, dtype, types=None, type_id=0):
    top = lambda x: np.abs(x).max()
    print("c_i: max |d| %.3e of %.3e; n_i: %.3e of %.3e; v_i: %.3e of %.3e; s %.15g vs %.15g (%.2e relative)"
          % (top(g["c"] - r["c"]), top(r["c"]), top(g["n"] - r["n"]), top(r["n"]), top(g["v"] - r["v"]), top(r["v"]), g["s"], r["s"],
             abs(g["s"] / r["s"] - 1.0)))
    F_ref = -bias * r["grad"]
    fs = top(F_ref)
    err = top(g["F"][:, :3] - F_ref)
    print("forces: max |d| %.3e of max |F| %.3e (%.3e relative)" % (err, fs, err / fs if fs else 0.0))
    for key in ("F", "c", "n", "v", "partials"):
        assert np.isfinite(g[key]).all(), key
    assert top(g["c"] - r["c"]) <= 1e-11 * top(r["c"])
    assert top(g["n"] - r["n"]) <= 1e-11 * top(r["n"])
    assert top(g["v"] - r["v"]) <= 1e-11 * top(r["v"])
    assert g["s"] == pytest.approx(r["s"], rel=1e-10)
    assert fs > 0
    assert err <= (1e-9 if dtype == np.float64 else 2e-7) * fs
    assert np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        other = types != type_id
        assert np.all(g["F"][other] == 0.0) and np.all(g["c"][other] == 0.0) and np.all(g["n"][other] == 0.0) and np.all(g["v"][other] == 0.0)


_snapshots = {}


def snapshot(cells, dtype):
    """noisy fcc, rounded to the dtype, with its list at r_cut + 0.15: built once per size and dtype"""
    key = (cells, np.dtype(dtype).name)
    if key not in _snapshots:
        pos, L = noisy_fcc(cells)
        pos = pos.astype(dtype).astype(np.float64)
        _snapshots[key] = (pos, L, np.zeros(len(pos), dtype=np.int32), util.build_nlist(pos, L, 1.55))
    return _snapshots[key]


def parity(abi, cells, dtype, lmax, Ql_ref, opt):
    pos, L, types, nl = snapshot(cells, dtype)
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, opt=opt)
    r = avg_ref.compute(pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, **opt)
    compare(g, r, 0.9, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cells", [3, 5])                               # N = 108: one full chunk of 64 and a partial one; N = 500
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_options_parity(abi, dtype, cells, combo):
    parity(abi, cells, dtype, 6, QL_46, COMBOS[combo])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cells", [3, 5])
@pytest.mark.parametrize("lmax,Ql_ref", [(4, [0.2, 0, 1.0, 0.5, 1.0]),                          # l = 0 in use, an odd degree
                                         (5, [0, 0.4, 0.2, 0.6, 1, 0.7]),                      # odd and even degrees mixed; 20 slots: two windows
                                         (12, [0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0.5, 0.3, 0.25])])  # 49 slots: four windows, the direct force pass
def test_average_and_switch_other_degrees(abi, dtype, cells, lmax, Ql_ref):
    parity(abi, cells, dtype, lmax, Ql_ref, COMBOS["average+switch"])


def test_two_types_and_n_global(abi):
    pos, L = noisy_fcc(4, seed=5)
    N = len(pos)
    types = (np.random.default_rng(1).random(N) < 0.3).astype(np.int32)
    nl = util.build_nlist(pos, L, 1.6)
    opt = COMBOS["average+switch+gate"]
    args = (1.45, 1.1, 6, 0, [0.5, 0, 0.25, 0, 1, 0, 1])
    g = run_gpu(abi, pos, types, L, nl, *args, np.float64, opt=opt, n_global=3 * N)
    r = avg_ref.compute(pos, types, L, nl, *args, n_global=3 * N, **opt)
    assert 0 < ((r["n"] > 4) & (r["n"] < 8)).sum()                      # some particles inside the gate's ramp
    compare(g, r, 0.9, np.float64, types=types)
    # the other type as the chosen one
    args = (1.45, 1.1, 6, 1, [0.5, 0, 0.25, 0, 1, 0, 1])
    g = run_gpu(abi, pos, types, L, nl, *args, np.float64, opt=opt, n_global=3 * N)
    r = avg_ref.compute(pos, types, L, nl, *args, n_global=3 * N, **opt)
    compare(g, r, 0.9, np.float64, types=types, type_id=1)


def brute_nlist(pos, h, r):
    """full list of a triclinic box (lattice vectors in the columns of h), O(N^2), images -1..1"""
    N = len(pos)
    shifts = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.float64) @ h.T
    rows = []
    for i in range(N):
        d = pos[i] - pos
        best = np.min(((d[:, None, :] + shifts[None, :, :]) ** 2).sum(-1), axis=1)
        rows.append(np.nonzero((best <= r * r) & (np.arange(N) != i))[0])
    nn = np.array([len(x) for x in rows], dtype=np.uint32)
    head = np.zeros(N, dtype=np.uint32)
    head[1:] = np.cumsum(nn)[:-1]
    return head, nn, np.concatenate(rows).astype(np.uint32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_triclinic_box(abi, dtype):
    """a sheared fcc crystal in the sheared box: HOOMD's minimum image with tilt factors in all four passes"""
    pos, L = noisy_fcc(4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = brute_nlist(pos, h, 1.6)
    args = (1.45, 1.15, 6, 0, [0, 0, 0.3, 0, 1, 0, 1])
    opt = COMBOS["average+switch"]
    g = run_gpu(abi, pos, types, L, nl, *args, dtype, opt=opt, tilt=tilt)
    r = avg_ref.compute(pos, types, L, nl, *args, tilt=tilt, **opt)
    assert r["n"].min() > 3
    compare(g, r, 0.9, dtype)


@pytest.mark.parametrize("combo", ["average+switch+gate", "switch+gate"])
def test_buffered_and_shuffled_lists(abi, combo):
    """a list built at r_cut + 0.4 (most of its entries are out of range) with every row's order permuted gives what the tight list gives:
    values within their tolerance, forces within the force tolerance (the sums follow the list order)"""
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
    r = avg_ref.compute(pos, types, L, (head, nn, lst), *args, **opt)
    compare(b, r, 0.9, np.float64, types=types)
    for key in ("c", "n", "v"):
        assert np.abs(a[key] - b[key]).max() <= 1e-11 * np.abs(a[key]).max(), key
    assert a["s"] == pytest.approx(b["s"], rel=1e-10)
    assert np.abs(a["F"] - b["F"]).max() <= 1e-9 * np.abs(a["F"]).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dilute_edge_case(abi, dtype):
    """particles with n_i = 0, with 0 < n_i < 2 and inside the gate's ramp: everything finite and as the restatement has it"""
    case = avg_ref.dilute_case()
    opt = {k: case.pop(k) for k in ("average", "switch", "gate")}
    pos = case["pos"].astype(dtype).astype(np.float64)
    nl = util.build_nlist(pos, case["L"], 1.6)
    args = (case["r_cut"], case["r_on"], case["lmax"], 0, case["Ql_ref"])
    g = run_gpu(abi, pos, case["types"], case["L"], nl, *args, dtype, opt=opt)
    r = avg_ref.compute(pos, case["types"], case["L"], nl, *args, **opt)
    lonely = r["n"] == 0
    assert lonely.sum() >= 5 and ((r["n"] > 2) & (r["n"] < 6)).sum() >= 15
    compare(g, r, 0.9, dtype)
    assert np.all(g["v"][lonely] == 0.0) and np.all(g["c"][lonely] == 0.0) and np.all(g["F"][lonely] == 0.0)
    if dtype == np.float64:
        assert g["s"] == pytest.approx(0.29674341030178875, rel=1e-10)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("entry", ["null", "zero"])
def test_options_off_is_the_old_entry_point_bit_for_bit(abi, dtype, entry):
    pos, L, types, nl = snapshot(5, dtype)
    for lmax, Ql_ref in ((6, QL_46), (12, [0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0.5, 0.3, 0.25])):
        old = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, entry="old")
        new = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, lmax, 0, Ql_ref, dtype, entry=entry)
        for key in ("c", "n", "v", "partials", "F"):
            assert np.array_equal(old[key], new[key]), key
        assert np.array_equal(new["v"], new["c"])                       # without options v_i is c_i


def test_reproducible_bits(abi):
    """no atomics, fixed orders: two identical calls give identical bits"""
    pos, L, types, nl = snapshot(5, np.float64)
    opt = COMBOS["average+switch+gate"]
    a = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, np.float64, opt=opt)
    b = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, np.float64, opt=opt)
    for key in ("c", "n", "v", "partials", "F"):
        assert np.array_equal(a[key], b[key]), key


def test_bias_from_device_and_host(abi):
    pos, L, types, nl = snapshot(5, np.float64)
    opt = COMBOS["average+switch"]
    dev = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, np.float64, opt=opt, bias=-1.7, bias_on_device=True)
    host = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, np.float64, opt=opt, bias=-1.7, bias_on_device=False)
    assert np.array_equal(dev["F"], host["F"])
    r = avg_ref.compute(pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, **opt)
    compare(dev, r, -1.7, np.float64)
    zero = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, np.float64, opt=opt, bias=0.0, bias_on_device=False)
    assert np.all(zero["F"] == 0.0)


def test_chunk_loop(abi):
    """70 304 particles: more than 1024 chunks of 64, so every block walks several chunks in all four passes"""
    pos, L = noisy_fcc(26)
    N = len(pos)
    assert N == 70304 and (N + 63) // 64 > 1024
    types = np.zeros(N, dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.4)
    opt = COMBOS["average+switch"]
    Ql_ref = [0, 0, 0, 0, 1]
    g = run_gpu(abi, pos, types, L, nl, 1.4, 1.2, 4, 0, Ql_ref, np.float64, opt=opt)
    assert len(g["partials"]) == 1024
    r = avg_ref.compute(pos, types, L, nl, 1.4, 1.2, 4, 0, Ql_ref, **opt)
    compare(g, r, 0.9, np.float64)


# ---- through the Python API -------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


SWITCH, GATE = dict(c0=0.12, p=3), dict(n_lo=4, n_hi=8)
OPT = dict(average=True, switch=(0.12, 3), gate=(4, 8))


def _api_system(seed=12):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(seed).normal(0, 0.05, pos.shape)
    return pos, L, np.zeros(len(pos), dtype=np.int32)


def _oracle_bias(ref, kw, values, steps):
    """the oracle's grid driven with the given CV values: prepRun(0) + `steps` updates; returns the list of bias factors per call"""
    g = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    return [g.update_bias(t, values) for t in range(steps + 1)]


def test_options_alone_on_a_grid(api, ref):
    """cv.steinhardt_local(average, switch, gate) on a 512-point well-tempered grid, 5 steps: the value the engine used, c_i, v_i, the bias
    factor and the force array against the oracle's grid driven with the restatement's value"""
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    r = avg_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, QL_46, **OPT)
    val = r["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=0.02 * val, average=True, switch=SWITCH, gate=GATE)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    context.run(5)
    t = context.current.system.getCurrentTimeStep()
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-10)
    assert st.cpp_force.getLogValue("cv_steinhardt_local", t) == pytest.approx(val, rel=1e-10)
    assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(val, rel=1e-10)      # what the engine took from the block sums
    assert np.abs(st.get_local() - r["c"]).max() <= 1e-11 * np.abs(r["c"]).max()
    assert np.abs(st.get_switched() - r["v"]).max() <= 1e-11 * np.abs(r["v"]).max()
    assert np.abs(st.get_coordination() - r["n"]).max() <= 1e-11 * np.abs(r["n"]).max()
    b = _oracle_bias(ref, dict(sigma=[0.02 * val], cv_min=[0.55 * val], cv_max=[1.3 * val], num_points=[512]), [val], 5)[-1]
    assert abs(b[0]) > 0
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    F = st.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert np.all(F[:, 3] == 0.0)


def test_invalid_options_raise(api):
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    kw = dict(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A")
    for bad in (dict(switch=dict(c0=0.0, p=3)), dict(switch=dict(c0=-1.0, p=3)), dict(switch=dict(c0=0.1, p=0)), dict(switch=dict(c0=0.1, p=2.5)),
                dict(switch=dict(c0=0.1)), dict(switch=(0.1, 3)), dict(gate=dict(n_lo=-1, n_hi=4)), dict(gate=dict(n_lo=4, n_hi=4)),
                dict(gate=dict(n_lo=6, n_hi=2)), dict(gate=dict(n_lo=1)), dict(gate=dict(n_lo=1, n_hi=2, n_mid=1.5))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.steinhardt_local(**kw, **bad)
    with pytest.raises(RuntimeError):
        cv.steinhardt_local(**kw).cpp_force.setSwitch(0.0, 3)
    with pytest.raises(RuntimeError):
        cv.steinhardt_local(**kw).cpp_force.setGate(3.0, 1.0)


def test_changing_options_between_runs_takes_effect(api):
    """a change of options invalidates the cached step and grows the scratch: plain -> switch -> average + switch + gate -> plain"""
    context, cv, integrate = api
    pos, L, types = _api_system(seed=14)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=1.0)
    st.set_grid(0.0, 1.0, 64)
    seen = []
    for kw, opt in ((dict(), dict()), (dict(switch=dict(c0=0.25, p=3)), dict(switch=(0.25, 3))),
                    (dict(average=True, switch=SWITCH, gate=GATE), OPT), (dict(), dict())):
        st.set_options(**kw)
        r = avg_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, QL_46, gradient=False, **opt)
        t = context.current.system.getCurrentTimeStep()
        assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)         # the same time step: the cache must have gone
        assert np.abs(st.get_switched() - r["v"]).max() <= 1e-11 * np.abs(r["v"]).max()
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)
        seen.append(r["s"])
    assert seen[0] == seen[3] and len({round(s, 6) for s in seen[:3]}) == 3


def test_options_on_a_device_list_follow_the_particles(api):
    """cv.nlist_cell(device=True): particles displaced between runs — the list rebuilds (and may grow: so does the scratch), value and
    forces follow"""
    context, cv, integrate = api
    pos, L, types = _api_system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5, r_buff=0.4, device=True)
    val0 = avg_ref.compute(pos, types, L, util.build_nlist(pos, L, 1.5), 1.4, 1.2, 6, 0, QL_46, gradient=False, **OPT)["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=0.02 * val0, average=True, switch=SWITCH, gate=GATE)
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
        r = avg_ref.compute(p, types, L, util.build_nlist(p, L, 1.5), 1.4, 1.2, 6, 0, QL_46, **OPT)
        values.append(r["s"])
        assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)
        assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["s"], rel=1e-10)
        assert nl.cpp_nlist.getNumRebuilds() == 2 + k
        b = meta.cpp_integrator.getBiasFactors()[0]
        F = st.cpp_force.getForceArray()
        F_ref = -b * r["grad"]
        assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert abs(values[-1] - values[0]) > 1e-3 * values[0]                         # the value did move


def test_harmonic_umbrella_adds_to_the_bias_factor(api, ref):
    context, cv, integrate = api
    pos, L, types = _api_system(seed=15)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = nl.update()
    r = avg_ref.compute(pos, types, L, lists, 1.4, 1.2, 6, 0, QL_46, **OPT)
    val = r["s"]
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=0.02 * val, average=True, switch=SWITCH, gate=GATE)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    kappa, cv0 = 35.0, 0.8 * val
    st.set_params(umbrella="harmonic", kappa=kappa, cv0=cv0)
    context.run(3)
    t = context.current.system.getCurrentTimeStep()
    b = _oracle_bias(ref, dict(sigma=[0.02 * val], cv_min=[0.55 * val], cv_max=[1.3 * val], num_points=[512]), [val], 3)[-1]
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    total = b[0] + kappa * (val - cv0)
    F = st.cpp_force.getForceArray()
    F_ref = -total * r["grad"]
    assert abs(kappa * (val - cv0)) > 0.1 * abs(total)
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert st.cpp_force.getUmbrellaPotential(t) == pytest.approx(0.5 * kappa * (val - cv0) ** 2, rel=1e-9)


# ---- rows of every length 0 .. 13, and entries the passes must skip -------------------------------------------------------------

_clusters = {}


def cluster_case(dtype):
    """14 clusters of 1, 2, ..., 14 particles (N = 105: one full chunk of 64 and a partial one) far apart in a box of L = 40: every member
    of cluster m has m - 1 neighbours, all inside r_cut = 1.4, so the rows have every length 0 .. 13 — each boundary of e < cnt,
    e + 4 < cnt and e + 8 < cnt of the two-deep look-ahead, for each of the four lanes of a quad.  Returns the system, its list (A), the
    list with one self entry and two entries >= N added to every row (B), and the restatement's answer for list A per option set."""
    key = np.dtype(dtype).name
    if key not in _clusters:
        rng = np.random.default_rng(2024)
        L, pos = 40.0, []
        centres = 8.0 * (np.array([[x, y, z] for x in range(5) for y in range(5) for z in range(5)], dtype=np.float64) - 2.0)
        for m in range(1, 15):
            members = []
            while len(members) < m:
                x = rng.uniform(-0.45, 0.45, 3)
                if all(np.linalg.norm(x - y) >= 0.3 for y in members):
                    members.append(x)
            pos += [centres[m - 1] + x for x in members]
        pos = np.array(pos).astype(dtype).astype(np.float64)
        N = len(pos)
        types = np.zeros(N, dtype=np.int32)
        head, nn, lst = (np.asarray(x).astype(np.int64) for x in util.build_nlist(pos, L, 1.55))
        sizes = np.repeat(np.arange(1, 15), np.arange(1, 15))
        assert N == 105 and np.array_equal(nn, sizes - 1)
        rows = []
        for i in range(N):
            row = list(lst[head[i]:head[i] + nn[i]])
            assert all(np.linalg.norm(pos[i] - pos[j]) < 1.4 for j in row)
            pad = [i, N, N + 7]
            pad = pad[i % 3:] + pad[:i % 3]                                 # which of the three goes to the front, the middle, the end
            mid = len(row) // 2
            rows.append([pad[0]] + row[:mid] + [pad[1]] + row[mid:] + [pad[2]])
        nn_b = np.array([len(r) for r in rows], dtype=np.uint32)
        head_b = np.zeros(N, dtype=np.uint32)
        head_b[1:] = np.cumsum(nn_b)[:-1]
        padded = (head_b, nn_b, np.concatenate(rows).astype(np.uint32))
        nl = (head.astype(np.uint32), nn.astype(np.uint32), lst.astype(np.uint32))
        ref = {c: avg_ref.compute(pos, types, L, nl, 1.4, 1.2, 6, 0, QL_46, **SKIP_COMBOS[c]) for c in SKIP_COMBOS}
        _clusters[key] = (pos, L, types, nl, padded, ref)
    return _clusters[key]


SKIP_COMBOS = {"plain": {}, "average": COMBOS["average"], "average+switch+gate": COMBOS["average+switch+gate"]}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("combo", sorted(SKIP_COMBOS))
def test_row_lengths_0_to_13_and_skipped_entries(abi, dtype, combo):
    """the walk over a row at every row length 0 .. 13 (run A), and the same rows with a self entry and two entries >= N each, at the
    front, in the middle and at the end (run B): both give what the restatement gives for the clean list.  (The padding moves entries
    between lanes, so the sums of B are taken in another order than those of A: no bits are compared.)"""
    pos, L, types, nl, padded, ref = cluster_case(dtype)
    assert len(padded[2]) == len(nl[2]) + 3 * len(pos)
    for lists in (nl, padded):
        g = run_gpu(abi, pos, types, L, lists, 1.4, 1.2, 6, 0, QL_46, dtype, opt=SKIP_COMBOS[combo])
        compare(g, ref[combo], 0.9, dtype)
