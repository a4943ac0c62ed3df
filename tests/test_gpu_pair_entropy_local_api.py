"""GPU: cv.pair_entropy_local through the host classes, the Python API and the integrator, against the numpy restatement
(tests/pair_entropy_local_ref.py): the value the engine used to rel 1e-9, s_i / sbar_i / v_i to 1e-10 of their maximum, the applied force
to 1e-9 of max|F| at the bias factor the integrator reports, virials likewise (fp64 arrays throughout)."""
import ctypes as C

import numpy as np
import pytest

import pair_entropy_local_ref as pel
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

PAR = dict(r_max=2.0, sigma_r=0.1, n_bins=40)
R_LIST = 2.45
KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
AVERAGE, SWITCH = dict(r_on=1.2, r_cut=1.5), dict(c0=3.0, p=6)
SETS = {"plain": dict(), "switch": dict(switch=SWITCH), "average": dict(average=AVERAGE), "both": dict(average=AVERAGE, switch=SWITCH)}


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _system(seed=12, noise=0.05):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(seed).normal(0, noise, pos.shape)
    types = (np.arange(len(pos)) % 9 == 4).astype(np.int32)
    return pos, L, types


def _ref(pos, types, L, lists, bias=1.0, average=None, switch=None):
    kw = dict(average=None if average is None else (average["r_on"], average["r_cut"]),
              switch=None if switch is None else (switch["c0"], switch["p"]))
    return pel.compute(pos, types, L, lists, PAR["r_max"], PAR["sigma_r"], PAR["n_bins"], 0, bias=bias, **kw)


def _grid(var, val):
    lo, hi = (1.3 * val, 0.55 * val) if val < 0 else (0.0, 1.0)
    var.set_grid(lo, hi, 512)


def _check_step(var, meta, r, t):
    """value, per-particle arrays and the applied force of the step the integrator just made"""
    b = meta.cpp_integrator.getBiasFactors()[0]
    assert abs(b) > 0
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(r["cv"], rel=1e-9)
    assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["cv"], rel=1e-9)
    for got, key in ((var.get_local(), "s"), (var.get_averaged(), "sbar"), (var.get_switched(), "v")):
        err = np.abs(got - r[key]).max()
        print("%s: %.3e of %.3e" % (key, err, np.abs(r[key]).max()))
        assert got.shape == r[key].shape and err <= 1e-10 * np.abs(r[key]).max()
    F = var.cpp_force.getForceArray()
    F_ref = -b * r["gather"]
    print("force: %.3e of %.3e at bias factor %.6g" % (np.abs(F[:, :3] - F_ref).max(), np.abs(F_ref).max(), b))
    assert np.abs(F_ref).max() > 0 and np.abs(F[:, :3] - F_ref).max() <= 1e-9 * np.abs(F_ref).max()
    assert np.all(F[:, 3] == 0.0)
    return b


@pytest.mark.parametrize("name", sorted(SETS))
def test_value_locals_and_applied_force(api, name):
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists, **SETS[name])
    var = cv.pair_entropy_local(nlist=nl, type="A", sigma=0.02 * abs(r["cv"]), **PAR, **SETS[name])
    _grid(var, r["cv"])
    assert var.get_rcut() == {("A", "A"): pytest.approx(2.4), ("A", "B"): -1.0, ("B", "B"): -1.0}
    context.run(4)
    t = context.current.system.getCurrentTimeStep()
    assert t == 4
    _check_step(var, meta, r, t)
    assert np.all(var.cpp_force.getForceArray()[types == 1] == 0.0)
    assert var.cpp_force.getLogValue("cv_pair_entropy_local", t) == pytest.approx(r["cv"], rel=1e-9)
    assert "cv_pair_entropy_local" in var.cpp_force.getProvidedLogQuantities()
    if name == "both":
        assert 0.0 < r["cv"] < 1.0


def test_set_options_mid_run_invalidates_the_cached_step(api):
    """the options change between runs and, at one time step, between two reads: each read is that of the options in force"""
    context, cv, integrate = api
    pos, L, types = _system(seed=13)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    refs = {name: _ref(pos, types, L, lists, **kw) for name, kw in SETS.items()}
    var = cv.pair_entropy_local(nlist=nl, type="A", sigma=0.05, name="opt", **PAR)
    var.set_grid(-6.0, 1.5, 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    _check_step(var, meta, refs["plain"], t)
    for name in ("both", "average", "switch", "plain", "both"):
        var.set_options(**SETS[name])
        assert var.cpp_force.getCurrentValue(t) == pytest.approx(refs[name]["cv"], rel=1e-9), name     # same time step: not the cached value
        assert np.abs(var.get_switched() - refs[name]["v"]).max() <= 1e-10 * np.abs(refs[name]["v"]).max()
    context.run(1)
    _check_step(var, meta, refs["both"], context.current.system.getCurrentTimeStep())
    for bad in (dict(average=dict(r_on=1.5, r_cut=1.2)), dict(average=dict(r_on=1.0, r_cut=2.5)), dict(average=dict(r_on=1.0)),
                dict(switch=dict(c0=0.0, p=6)), dict(switch=dict(c0=1.0, p=0)), dict(switch=dict(c0=1.0, p=2.5)), dict(switch=(1.0, 6))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            var.set_options(**bad)
    assert var.cpp_force.getCurrentValue(context.current.system.getCurrentTimeStep()) == pytest.approx(refs["both"]["cv"], rel=1e-9)


def test_virial_with_the_pressure_flag_and_without(api):
    context, cv, integrate = api
    pos, L, types = _system(seed=15)
    N = len(pos)

    def run(pressure):
        context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
        context.current.system_definition.getParticleData().setPressureFlag(pressure)
        meta = integrate.mode_metadynamics(**KW)
        nl = cv.nlist_cell(r_cut=R_LIST)
        lists = nl.update()
        var = cv.pair_entropy_local(nlist=nl, type="A", sigma=0.02, **PAR, **SETS["both"])
        var.set_grid(0.0, 1.0, 512)
        context.run(3)
        return var, meta, lists

    var, meta, lists = run(True)
    b = meta.cpp_integrator.getBiasFactors()[0]
    r = _ref(pos, types, L, lists, bias=b, **SETS["both"])
    per, raw, W = var.get_virial(per_particle=True), var.cpp_force.getVirial(), var.get_virial()
    assert per.shape == (6, N) and per.dtype == np.float64 and W.shape == (6,)
    assert np.array_equal(raw[:, :N], per)
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["virial_sum"]).max(), w_top))
    assert top > 0 and w_top > 0
    assert np.abs(per.T - r["virial"]).max() <= 1e-9 * top
    assert np.abs(W - r["virial_sum"]).max() <= 1e-9 * w_top
    assert np.all(per[:, types == 1] == 0.0)
    F_on = var.cpp_force.getForceArray().copy()
    context.current = None
    var = run(False)[0]
    with pytest.raises(RuntimeError, match="pressure flag"):
        var.get_virial()
    with pytest.raises(RuntimeError, match="pressure flag"):
        var.get_virial(per_particle=True)
    assert np.array_equal(var.cpp_force.getForceArray(), F_on)           # the force bits do not depend on the virial


def test_device_list_follows_the_particles_and_a_short_one_is_refused(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST, r_buff=0.4, device=True)
    var = cv.pair_entropy_local(nlist=nl, type="A", sigma=0.02, **PAR, **SETS["both"])
    var.set_grid(0.0, 1.0, 512)
    p = pos
    for k in range(2):
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        r = _ref(p, types, L, util.build_nlist(p, L, R_LIST), **SETS["both"])
        _check_step(var, meta, r, t)
        assert nl.cpp_nlist.getNumRebuilds() == 1 + k
        p = p + np.random.default_rng(5 + k).normal(0, 0.12, p.shape)
        context.set_positions(p, types)
    # a device-built list that stops short of r_max + 4 sigma_r: refused by the Python class, and by the host class on its own
    n_forces = len(context.current.forces)
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.pair_entropy_local(nlist=cv.nlist_cell(r_cut=2.3, device=True), type="A", **PAR)
    assert len(context.current.forces) == n_forces
    sysdef = context.current.system_definition
    short = _metadynamics.NeighborList(sysdef)
    short.setDeviceBuild(2.3, 0.2, 1, 0)
    host = _metadynamics.PairEntropyLocal(sysdef, 2.0, 0.1, 40, short, 0, "_short")
    with pytest.raises(RuntimeError, match="must reach"):
        host.getCurrentValue(0)
    with pytest.raises(RuntimeError, match="n_bins"):
        _metadynamics.PairEntropyLocal(sysdef, 2.0, 0.1, 129, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="average"):
        host.setAverage(1.0, 2.5)
    with pytest.raises(RuntimeError, match="switch"):
        host.setSwitch(0.0, 6)


def test_half_list_and_distributed_context_are_refused(api, abi):
    context, cv, integrate = api
    from metadynamics import _metadynamics, xgmi
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    var = cv.pair_entropy_local(nlist=nl, type="A", **PAR)
    var.set_grid(-6.0, 0.0, 64)
    nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    nl.set_lists(*util.build_nlist(pos, L, R_LIST, half=True))
    with pytest.raises(RuntimeError, match="full neighbour list"):
        context.run(1)
    context.current = None
    # a (one-rank) mailbox in the execution configuration makes the run a domain-decomposed one
    lib = abi.load()
    h = C.c_void_p()
    abi.check(lib.mtd_comm_create(C.byref(h), 0, 1, 8))
    box = xgmi.Mailbox(h, 0, 1)
    try:
        context.initialize(pos, types, ["A", "B"], L, dtype=np.float64, n_global=len(pos))
        context.exec_conf.setMailbox(box.handle.value)
        integrate.mode_metadynamics(**KW)
        nl = cv.nlist_cell(r_cut=R_LIST)
        nl.update()
        var = cv.pair_entropy_local(nlist=nl, type="A", **PAR)
        var.set_grid(-6.0, 0.0, 64)
        with pytest.raises(RuntimeError, match="domain-decomposed runs are not supported"):
            var.cpp_force.getCurrentValue(0)
        with pytest.raises(RuntimeError, match="domain-decomposed runs are not supported"):
            context.run(1)
    finally:
        context.current = None
        box.close()


def test_bad_constructor_arguments_leave_the_force_list_alone(api):
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    good = cv.pair_entropy_local(nlist=nl, type="A", name="ok", **PAR, **SETS["both"])
    assert "cv_pair_entropy_local_ok" in good.cpp_force.getProvidedLogQuantities()
    n_forces = len(context.current.forces)
    for bad in (dict(type="Z"), dict(n_bins=0), dict(n_bins=129), dict(n_bins=12.5), dict(r_max=0.0), dict(sigma_r=-0.1), dict(r_max=float("nan")),
                dict(sigma_r=0.2),                                      # r_max + 4 sigma_r = 2.8 is beyond the list's 2.45
                dict(nlist=None), dict(average=dict(r_on=1.5, r_cut=1.2)), dict(average=dict(r_on=-0.1, r_cut=1.2)),
                dict(average=dict(r_on=1.2, r_cut=2.41)),               # the window must end inside r_max + 4 sigma_r = 2.4
                dict(average=dict(r_on=1.2)), dict(average=dict(r_on=1.2, r_cut=1.5, lam=1.0)), dict(average=(1.2, 1.5)), dict(average=True),
                dict(switch=dict(c0=0.0, p=6)), dict(switch=dict(c0=-1.0, p=6)), dict(switch=dict(c0=float("nan"), p=6)),
                dict(switch=dict(c0=1.0, p=0)), dict(switch=dict(c0=1.0, p=2.5)), dict(switch=dict(c0=1.0)), dict(switch=(1.0, 6))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.pair_entropy_local(**{**dict(nlist=nl, type="A"), **PAR, **bad})
        assert len(context.current.forces) == n_forces, bad             # a refused variable leaves nothing behind
