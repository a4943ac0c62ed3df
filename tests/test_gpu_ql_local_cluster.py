"""GPU parity: the local Steinhardt variable restricted to the largest cluster of solid particles (mtd_ql_local_accumulate_cluster,
cv.steinhardt_local(cluster=)) against tests/ql_local_cluster_ref.py, itself checked on the CPU in tests/test_ql_local_cluster_ref.py.
The configuration is that module's two_crystallites(): a jittered fcc crystallite of 4 x 4 x 4 cells and one of 2 x 2 x 2 cells in a random
gas of the same type, a second type sprinkled in, 1488 particles; v_min and r_link sit in the widest gaps of the v_i and of the pair
distances (asserted: rounding cannot flip a node or an edge), so mask and labels are compared exactly.  The arithmetic downstream of the
mask is that of the kernels tests/test_gpu_ql_local_bonds.py checks, and the tolerances are that file's: per-particle values to 1e-11 of
their largest, s to 1e-10 relative, forces and per-particle virial to 1e-9 of max|F| / max|virial_i| with fp64 arrays and 2e-7 with fp32
arrays, the six virial sums to 1e-9 of max|W| (fp64).  Forces and virial of non-members with no member within 2 r_cut are exactly 0."""
import ctypes as C

import numpy as np
import pytest

import ql_local_cluster_ref as cr
import stream_gate
import util
from test_gpu_ql_local_bonds import API_TOL, SENTINEL, _oracle_bias
from test_gpu_ql_local_bonds import run_gpu as run_gpu_bonds

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

BIAS = 0.9
NONE = cr.NONE
UNSUPPORTED = -2
ARGS = (cr.ARGS["r_cut"], cr.ARGS["r_on"], cr.ARGS["lmax"], cr.ARGS["type_id"], cr.ARGS["Ql_ref"])


def run_gpu(abi, pos, types, L, nl, dtype, opt=None, cluster=None, entry="cluster", bias=BIAS, expect=0, args=ARGS, gate=None):
    """pass 1 through mtd_ql_local_accumulate_cluster, then mtd_ql_local_forces_bonds without and with a virial array on the same table.
    opt: dict(switch=, gate=, bonds=, average=); cluster: (v_min, r_link) or None; entry = "null": cluster == NULL, "zero": an all-zero
    struct; args: (r_cut, r_on, lmax, type_id, Ql_ref).  Both scratches start as garbage.  Returns dict(s, c, n, v, b, F, F_vir, raw,
    partials, w, label, summary).  gate: the stream the calls run on and how their inputs arrive (tests/stream_gate.py; None: the NULL
    stream)."""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    opt = dict(opt or {})
    bonds = opt.pop("bonds", None)
    r_cut, r_on, lmax, type_id, Ql_ref = args
    N = len(pos)
    box = abi.Box.make(L)
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    o = abi.QlLocalOptions.make(**opt)
    bd = abi.QlLocalBonds.make(bonds)
    cl = abi.ClusterParams.make(cluster if entry == "cluster" else None)
    p_cl = None if entry == "null" else C.byref(cl)
    n_doubles = lib.mtd_ql_local_scratch_doubles_bonds(N, lmax, len(nl[2]), C.byref(o), C.byref(bd))
    scratch = torch.full((n_doubles,), float("nan"), dtype=torch.float64, device="cuda")
    c_scratch = torch.full((lib.mtd_cluster_scratch_bytes(N),), 0xA5, dtype=torch.uint8, device="cuda")
    p_part, p_c, p_n, p_v, p_b, p_w, p_label, p_sum = (C.c_void_p() for _ in range(8))
    n_part = C.c_uint()
    common = (abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), r_cut, r_on, lmax, type_id, util.dbl_array(Ql_ref), N, abi.ptr(scratch))
    force = torch.full((N, 4), 3.0, dtype=tdt, device="cuda")
    f_vir = torch.full((N, 4), 5.0, dtype=tdt, device="cuda")
    virial = torch.full((6, N + 3), SENTINEL, dtype=tdt, device="cuda")
    stream = gate.arm()
    rc = lib.mtd_ql_local_accumulate_cluster(N, abi.ptr(d_pos), dt, C.byref(box), *common, C.byref(p_part), C.byref(n_part), C.byref(p_c),
                                             C.byref(p_n), stream, C.byref(o), C.byref(p_v), C.byref(bd), C.byref(p_b), p_cl, abi.ptr(c_scratch),
                                             C.byref(p_w), C.byref(p_label), C.byref(p_sum))
    if expect:
        assert rc == expect
        return None
    abi.check(rc)
    b_args = (None, bias, stream)
    abi.check(lib.mtd_ql_local_forces_bonds(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *common, *b_args, C.byref(o), None, 0, C.byref(bd)))
    abi.check(lib.mtd_ql_local_forces_bonds(N, abi.ptr(d_pos), abi.ptr(f_vir), dt, C.byref(box), *common, *b_args, C.byref(o), abi.ptr(virial), N + 3,
                                            C.byref(bd)))

    def read():
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        partials = s[off(p_part):off(p_part) + n_part.value].copy()
        take = lambda p: s[off(p):off(p) + N].copy()
        out = dict(s=partials.sum() / N, c=take(p_c), n=take(p_n), v=take(p_v), b=take(p_b) if p_b.value else None, partials=partials,
                   F=force.cpu().numpy().astype(np.float64), F_vir=f_vir.cpu().numpy().astype(np.float64), raw=virial.cpu().numpy(),
                   w=None, label=None, summary=None)
        if entry == "cluster" and cluster is not None:
            raw = c_scratch.cpu().numpy()
            at = lambda p: p.value - c_scratch.data_ptr()
            out.update(w=raw[at(p_w):at(p_w) + 8 * N].view(np.float64).copy(), label=raw[at(p_label):at(p_label) + 4 * N].view(np.uint32).copy(),
                       summary=raw[at(p_sum):at(p_sum) + 16].view(np.uint32).copy())
        else:
            assert p_w.value is None and p_label.value is None and p_sum.value is None
        return out
    return gate.done(read)


_systems = {}
_refs = {}


def system(dtype):
    """two_crystallites() rounded to the dtype, with its list at 1.55: built once per dtype"""
    key = np.dtype(dtype).name
    if key not in _systems:
        case = cr.two_crystallites()
        pos = case["pos"].astype(dtype).astype(np.float64)
        _systems[key] = dict(case, pos=pos, nl=util.build_nlist(pos, case["L"], 1.55))
    return _systems[key]


def reference(combo, dtype, bias=BIAS):
    """(options, (v_min, r_link), the restatement's answer): computed once per combination and dtype and left unchanged"""
    key = (combo, np.dtype(dtype).name, bias)
    if key not in _refs:
        s = system(dtype)
        opt, window = cr.COMBOS[combo]
        cluster, margin = cr.choose(s["pos"], s["types"], s["L"], s["nl"], opt, window)
        assert margin[0] > 1e-6 and margin[1] > 1e-6, margin
        _refs[key] = (opt, cluster, cr.compute(s["pos"], s["types"], s["L"], s["nl"], cluster=cluster, bias=bias, **cr.ARGS, **opt))
    return _refs[key]


def compare(g, r, s, dtype, bias=BIAS):
    top = lambda x: np.abs(x).max()
    N = len(s["pos"])
    types = s["types"]
    assert np.array_equal(g["w"], r["w"]) and np.array_equal(g["label"], r["label"]) and np.array_equal(g["summary"], r["summary"])
    F_ref = -bias * r["grad"]
    fs, err = top(F_ref), top(g["F"][:, :3] - F_ref)
    vg = g["raw"][:, :N].astype(np.float64).T
    v_top, v_err = top(r["virial"]), top(vg - r["virial"])
    w_top, w_err = top(r["W"]), top(vg.sum(axis=0) - r["W"])
    print("largest cluster %s; v_i: max |d| %.3e of %.3e; s %.15g vs %.15g (%.2e relative); forces %.3e of max |F| %.3e (%.3e relative); virial "
          "%.3e of %.3e (%.3e relative); sums %.3e of max |W| %.3e (%.3e relative)"
          % (g["summary"], top(g["v"] - r["v"]), top(r["v"]), g["s"], r["s"], abs(g["s"] / r["s"] - 1.0), err, fs, err / fs, v_err, v_top,
             v_err / v_top, w_err, w_top, w_err / w_top))
    for key in ("F", "F_vir", "raw", "c", "n", "v", "partials"):
        assert np.isfinite(g[key]).all(), key
    for key in ("c", "n", "v") + (("b",) if r["b"] is not None else ()):
        assert top(g[key] - r[key]) <= 1e-11 * top(r[key]), key           # v_i is the UNMASKED one on both sides
    assert g["s"] == pytest.approx(r["s"], rel=1e-10)
    tol = 1e-9 if dtype == np.float64 else 2e-7
    assert fs > 0 and v_top > 0
    assert err <= tol * fs
    assert v_err <= tol * v_top
    if dtype == np.float64:
        assert w_err <= 1e-9 * w_top
    assert np.array_equal(g["F"], g["F_vir"])
    assert np.all(g["F"][:, 3] == 0.0) and np.all(g["raw"][:, N:] == SENTINEL)
    other = types != 0
    assert other.sum() > 0 and np.all(g["F"][other] == 0.0) and np.all(vg[other] == 0.0)
    far = cr.far_from_members(s["pos"], s["L"], r["w"], 2 * cr.ARGS["r_cut"])
    assert far.sum() > 100
    assert np.all(g["F"][far] == 0.0) and np.all(vg[far] == 0.0)          # exactly: their rows, beta and a0 are zero


# ---- 1. parity through the C ABI -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("combo", sorted(cr.COMBOS))
def test_cluster_parity(abi, dtype, combo):
    s = system(dtype)
    opt, cluster, r = reference(combo, dtype)
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], dtype, opt=opt, cluster=cluster)
    assert r["summary"][1] >= 150 and r["summary"][2] >= 2               # the big crystallite, and at least the small one beside it
    compare(g, r, s, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("entry", ["null", "zero"])
def test_cluster_off_is_the_bonds_entry_point_bit_for_bit(abi, dtype, entry):
    s = system(dtype)
    for combo in ("plain", "switch+gate", "bonds+switch"):
        opt = cr.COMBOS[combo][0]
        old = run_gpu_bonds(abi, s["pos"], s["types"], s["L"], s["nl"], *ARGS, dtype, opt=opt, bias_on_device=False)
        new = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], dtype, opt=opt, cluster=(0.3, 1.2), entry=entry)
        for key in ("c", "n", "v", "partials", "F", "F_vir", "raw"):
            assert np.array_equal(old[key], new[key]), key
        assert (old["b"] is None) == (new["b"] is None) and (old["b"] is None or np.array_equal(old["b"], new["b"]))
        assert old["s"] == new["s"]


def test_average_with_a_cluster_is_unsupported(abi):
    s = system(np.float64)
    run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], np.float64, opt=dict(average=True, switch=(0.12, 3)), cluster=(0.3, 1.2),
            expect=UNSUPPORTED)


@pytest.mark.parametrize("combo", ["switch+gate", "bonds+switch+gate"])
def test_reproducible_bits(abi, combo):
    """integer atomics in the cluster pass, none behind it: two identical calls give identical bits"""
    s = system(np.float64)
    opt, cluster, r = reference(combo, np.float64)
    a = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], np.float64, opt=opt, cluster=cluster)
    b = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], np.float64, opt=opt, cluster=cluster)
    for key in ("c", "n", "v", "partials", "F", "raw", "w", "label", "summary"):
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("combo", ["switch", "bonds+switch"])
def test_nothing_solid(abi, combo):
    """v_min above every v_i: s == 0, every force and virial entry 0, no NaN"""
    s = system(np.float64)
    opt = cr.COMBOS[combo][0]
    g = run_gpu(abi, s["pos"], s["types"], s["L"], s["nl"], np.float64, opt=opt, cluster=(1.5, 1.2))
    N = len(s["pos"])
    assert g["summary"].tolist() == [NONE, 0, 0, 0] and not g["w"].any() and (g["label"] == NONE).all()
    assert g["s"] == 0.0 and np.all(g["partials"] == 0.0)
    assert np.all(g["F"] == 0.0) and np.all(g["F_vir"] == 0.0) and np.all(g["raw"][:, :N] == 0.0)
    assert np.isfinite(g["v"]).all() and g["v"].max() > 0.5              # v_i itself stays what it is


# ---- 2. through the Python API -------------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


API_OPT = dict(bonds=dict(d_lo=0.5, d_hi=0.7), switch=dict(c0=6.5, p=12))
COMBO = "bonds+switch"


def _begin(api, device=False):
    context, cv, integrate = api
    s = system(np.float64)
    context.initialize(s["pos"], s["types"], ["A", "B"], s["L"], dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5, r_buff=0.4, device=True) if device else cv.nlist_cell(r_cut=1.5)
    if not device:
        nl.update()                                                      # the host's list: built from the positions and handed over
    return s, meta, nl


def _kw(nl):
    return dict(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=cr.E6, nlist=nl, type="A")


@pytest.mark.parametrize("device", [False, True])
def test_cluster_alone_on_a_grid(api, ref, device):
    """cv.steinhardt_local(bonds, switch, cluster) on a 512-point well-tempered grid, 4 steps, with the host's list and with a list built
    on the device (mtd_nlist_build): value, log value and the engine's value, the getters, the bias factor and the forces"""
    context, cv, integrate = api
    s, meta, nl = _begin(api, device)
    opt, cluster, r = reference(COMBO, np.float64)
    val = r["s"]
    st = cv.steinhardt_local(**_kw(nl), sigma=0.02 * val, cluster=dict(v_min=cluster[0], r_link=cluster[1]), **API_OPT)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    context.run(4)
    t = context.current.system.getCurrentTimeStep()
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-10)
    assert st.cpp_force.getLogValue("cv_steinhardt_local", t) == pytest.approx(val, rel=1e-10)
    assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(val, rel=1e-10)
    assert np.array_equal(st.get_cluster_mask(), r["w"])
    labels = st.get_cluster_labels()
    assert labels.dtype == np.uint32 and np.array_equal(labels, r["label"])
    assert tuple(int(x) for x in st.get_largest_cluster()) == tuple(int(x) for x in r["summary"])
    v = st.get_switched()
    assert np.abs(v - r["v"]).max() <= 1e-11 * np.abs(r["v"]).max()      # unmasked
    assert v[r["w"] == 0.0].max() > 0.5                                  # ... the small crystallite is still there
    b = _oracle_bias(ref, dict(sigma=[0.02 * val], cv_min=[0.55 * val], cv_max=[1.3 * val], num_points=[512]), [val], 4)[-1]
    assert abs(b[0]) > 0
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    F = st.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert np.abs(F[:, :3] - F_ref).max() <= API_TOL * np.abs(F_ref).max()
    assert np.all(F[:, 3] == 0.0)
    far = cr.far_from_members(s["pos"], s["L"], r["w"], 2 * 1.4)
    assert np.all(F[far] == 0.0)


def test_set_options_without_a_cluster_restores_the_unmasked_variable(api):
    context, cv, integrate = api
    s, meta, nl = _begin(api)
    opt, cluster, r = reference(COMBO, np.float64)
    st = cv.steinhardt_local(**_kw(nl), sigma=1.0, cluster=dict(v_min=cluster[0], r_link=cluster[1]), **API_OPT)
    st.set_grid(0.0, 1.0, 64)
    context.run(1)
    t = context.current.system.getCurrentTimeStep()
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)
    st.set_options(cluster=None, **API_OPT)
    unmasked = r["v"].sum() / len(s["pos"])
    assert unmasked > 1.05 * r["s"]
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(unmasked, rel=1e-10)          # the same time step: the cache must have gone
    with pytest.raises(RuntimeError):
        st.get_cluster_mask()
    st.set_options(cluster=dict(v_min=cluster[0], r_link=cluster[1]), **API_OPT)
    assert st.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-10)
    assert np.array_equal(st.get_cluster_mask(), r["w"])


def test_invalid_clusters_raise(api):
    context, cv, integrate = api
    s, meta, nl = _begin(api)
    kw = _kw(nl)
    before = list(context.current.forces)
    for bad in (dict(v_min=0.3), dict(r_link=1.2), dict(v_min=0.3, r_link=1.2, r_max=2.0), (0.3, 1.2), dict(v_min=0.3, r_link=0.0),
                dict(v_min=0.3, r_link=-1.0), dict(v_min=float("nan"), r_link=1.2), dict(v_min=float("inf"), r_link=1.2),
                dict(v_min=0.3, r_link=float("nan")), dict(v_min=0.3, r_link=float("inf")), dict(v_min="x", r_link=1.2)):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.steinhardt_local(**kw, cluster=bad)
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.steinhardt_local(**kw, cluster=dict(v_min=0.3, r_link=1.2), average=True)
    dev = cv.nlist_cell(r_cut=1.5, r_buff=0.4, device=True)
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.steinhardt_local(**_kw(dev), cluster=dict(v_min=0.3, r_link=2.5))      # beyond the reach of the device-built list
    assert list(context.current.forces) == before                        # a refused construction leaves nothing behind
    st = cv.steinhardt_local(**kw)
    for getter in (st.get_cluster_mask, st.get_cluster_labels, st.get_largest_cluster):
        with pytest.raises(RuntimeError):
            getter()
    with pytest.raises(RuntimeError):
        st.cpp_force.setCluster(0.3, 0.0)
    st.cpp_force.setCluster(0.3, 1.2)
    with pytest.raises(RuntimeError):
        st.cpp_force.setAverage(True)
    st.cpp_force.clearCluster()
    st.cpp_force.setAverage(True)
    with pytest.raises(RuntimeError):
        st.cpp_force.setCluster(0.3, 1.2)
