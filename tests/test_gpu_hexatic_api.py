"""GPU: cv.hexatic through the host classes and the Python API, against the numpy restatement (tests/hexatic_ref.py) driven with the bias
factors the integrator reports: the value the engine used to rtol 1e-9, force arrays to 1e-7 of max|F| (the bias factor is the
integrator's own), virials to 1e-9.  Where forces are compared, the particles are moved between steps: with every hill on one value the
bias factor is the rounding residue at the top of the hills.

The system is the noisy triangular monolayer of tests/test_gpu_hexatic.py, 12 x 12 particles in the box (12, 6 sqrt 3, 4)."""
import numpy as np
import pytest

import coordination_ref as cn
import hexatic_ref as hr

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

R_ON, R_CUT = 0.9, 1.35
R_LIST = 1.4
SWITCH, GATE = (0.5, 4), (2.0, 5.0)
KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _system(seed=12, noise=0.05):
    pos, L = hr.triangular_layer(12, 12)
    pos = pos + np.random.default_rng(seed).normal(0, noise, pos.shape)
    return pos, L, (np.arange(len(pos)) % 4 == 3).astype(np.int32)


def _ref(pos, types, L, lists, bias=1.0, **opt):
    r = hr.compute(pos, types, L, lists, hr.params(0, R_CUT, R_ON, **opt), bias=bias)
    n = r["coordination"]
    assert np.all((n == 0.0) | (n >= 1e-3))                             # the condition of tests/test_gpu_hexatic.py
    return r


def _grid(val):
    return dict(sigma=[0.02 * abs(val)], cv_min=[0.4 * val], cv_max=[1.6 * val], num_points=[512])


def _dicts(switch, gate):
    return (None if switch is None else dict(c0=switch[0], p=switch[1]), None if gate is None else dict(n_lo=gate[0], n_hi=gate[1]))


def _moved_steps(context, meta, var, nl, pos, types, L, steps=6, **opt):
    """`steps` steps of one at a time, the particles moved a little before every step but the first: value and force array against the
    restatement at every step; returns the last positions and restatement"""
    rng = np.random.default_rng(8)
    seen = []
    lists = nl.update()
    r = _ref(pos, types, L, lists, **opt)
    for step in range(1, steps + 1):
        if step > 1:
            pos = pos + rng.normal(0, 0.01, pos.shape)
            context.set_positions(pos, types)
            lists = nl.update()
            r = _ref(pos, types, L, lists, **opt)
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        assert t == step
        assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["s"], rel=1e-9)
        b = meta.cpp_integrator.getBiasFactors()[0]
        F = var.cpp_force.getForceArray()
        F_ref = -b * r["grad"]
        print("step %d: s %.9f, bias factor %.6e, max |F - F_ref| %.3e of max |F_ref| %.3e"
              % (step, r["s"], b, np.abs(F[:, :3] - F_ref).max(), np.abs(F_ref).max()))
        seen.append(b)
        if step > 1:
            assert abs(b) > 1e-3                                        # a slope of the deposited hills
            assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
        assert np.all(F[:, 3] == 0.0) and np.all(F[types == 1] == 0.0)
    assert len(set(seen)) == steps                                      # hills landed: the bias factor moved at every step
    return pos, lists, r


def test_hexatic_alone_on_a_grid(api):
    """512-point well-tempered grid, stride 1.  The particles are moved a little before every step, so that the hills land at different
    values and the bias factor is a slope of the grid: over six such steps the value is the restatement's and the force array is
    -(bias factor) x the restatement's gradient.  Then the getters, their shapes and the log quantity"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    val = _ref(pos, types, L, nl.update())["s"]
    assert val > 0.3
    kw = _grid(val)
    var = cv.hexatic(R_CUT, R_ON, nl, "A", sigma=kw["sigma"][0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    pos, lists, r = _moved_steps(context, meta, var, nl, pos, types, L)
    val = r["s"]
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-9)
    assert var.cpp_force.getLogValue("cv_hexatic", t) == pytest.approx(val, rel=1e-9)
    assert "cv_hexatic" in var.cpp_force.getProvidedLogQuantities()
    loc, sw, cnum, psi, Psi = var.get_local(), var.get_switched(), var.get_coordination(), var.get_psi(), var.get_global_psi()
    assert loc.shape == sw.shape == cnum.shape == (len(pos),) and psi.shape == (len(pos), 2) and len(Psi) == 2
    assert np.abs(loc - r["local"]).max() <= 1e-9 * np.abs(r["local"]).max()
    assert np.abs(cnum - r["coordination"]).max() <= 1e-9 * np.abs(r["coordination"]).max()
    assert np.abs(psi[:, 0] + 1j * psi[:, 1] - r["psi"]).max() <= 1e-9 * np.abs(r["psi"]).max()
    assert abs(complex(*Psi) - r["Psi"]) <= 1e-9 * np.abs(r["psi"]).max()
    assert np.array_equal(loc, sw) and np.all(loc[types == 1] == 0.0) and np.all(cnum[types == 1] == 0.0) and np.all(psi[types == 1] == 0.0)
    assert np.abs(loc - (psi ** 2).sum(axis=1)).max() <= 1e-15          # c_i = |psi_i|^2 (values <= 1: a few ulps)
    assert loc[types == 0].mean() == pytest.approx(val, rel=1e-9)
    named = cv.hexatic(R_CUT, R_ON, nl, "A", name="layer", k=4, axis="x")
    assert "cv_hexatic_layer" in named.cpp_force.getProvidedLogQuantities()
    assert (named.k, named.axis, named.global_order, named.r_cut) == (4, "x", False, R_CUT) and named.cpp_force.getRCut() == R_CUT
    assert named.get_rcut() == {("A", "A"): R_CUT, ("A", "B"): -1.0, ("B", "B"): -1.0}
    rx = _ref(pos, types, L, lists, k=4, axis="x")
    assert named.cpp_force.getCurrentValue(t) == pytest.approx(rx["s"], rel=1e-9)


def test_hexatic_global_order_on_a_grid(api):
    """|Psi|^2 on the grid: value, force array (the adjoint rows k_hex_finalize writes) and Psi itself"""
    context, cv, integrate = api
    pos, L, types = _system(seed=14)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    val = _ref(pos, types, L, nl.update(), global_order=True)["s"]
    assert val > 0.3
    kw = _grid(val)
    var = cv.hexatic(R_CUT, R_ON, nl, "A", global_order=True, sigma=kw["sigma"][0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    pos, lists, r = _moved_steps(context, meta, var, nl, pos, types, L, global_order=True)
    Psi = complex(*var.get_global_psi())
    assert abs(Psi - r["Psi"]) <= 1e-9 and abs(Psi) ** 2 == pytest.approx(r["s"], rel=1e-9)
    assert np.abs(var.get_local() - r["local"]).max() <= 1e-9 and np.array_equal(var.get_local(), var.get_switched())
    for bad in (dict(switch=dict(c0=0.5, p=4)), dict(gate=dict(n_lo=2.0, n_hi=5.0))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            var.set_options(**bad)
    var.set_options()
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-9)


def test_hexatic_constructor_refusals_leave_nothing_behind(api):
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    ok = dict(r_cut=R_CUT, r_on=R_ON, nlist=nl, type="A")
    cv.hexatic(**ok)
    cv.hexatic(**{**ok, "switch": dict(c0=0.5, p=4), "gate": dict(n_lo=0, n_hi=3)})
    cv.hexatic(**{**ok, "global_order": True, "k": 12, "axis": "y"})
    n_forces = len(context.current.forces)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(type="Z"), dict(r_on=-0.1), dict(r_on=nan), dict(r_on=1.35), dict(r_on=2.0), dict(r_cut=nan), dict(r_cut=inf),
                dict(r_cut=0.0, r_on=0.0),
                dict(r_cut=1.45),                                       # beyond the list's 1.4
                dict(k=0), dict(k=13), dict(k=-1), dict(k=2.5), dict(k="six"), dict(k=None),
                dict(axis="w"), dict(axis=2), dict(axis=None), dict(axis="Z"), dict(nlist=None),
                dict(switch=dict(c0=0.6)), dict(switch=dict(p=6)), dict(switch=dict(c0=0.6, p=6, q=1)), dict(switch=dict(c0=0.0, p=6)),
                dict(switch=dict(c0=0.6, p=0)), dict(switch=dict(c0=0.6, p=2.5)), dict(switch=dict(c0=nan, p=6)), dict(switch=(0.6, 6)),
                dict(gate=dict(n_lo=-0.5, n_hi=3.0)), dict(gate=dict(n_lo=3.0, n_hi=3.0)), dict(gate=dict(n_lo=1.0)),
                dict(gate=dict(n_lo=1.0, n_hi=inf)), dict(gate=dict(n_lo=1.0, n_hi=3.0, x=1)), dict(gate=(1.0, 3.0)),
                dict(global_order=True, switch=dict(c0=0.6, p=6)), dict(global_order=True, gate=dict(n_lo=1.0, n_hi=3.0))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.hexatic(**{**ok, **bad})
        assert len(context.current.forces) == n_forces, bad            # a refused variable leaves nothing behind
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.hexatic(R_CUT, R_ON, cv.nlist_cell(r_cut=1.2), "A")
    assert len(context.current.forces) == n_forces


def test_hexatic_set_options_between_runs(api):
    context, cv, integrate = api
    pos, L, types = _system(seed=13)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists, switch=SWITCH, gate=GATE)
    val = r["s"]
    assert 0.05 < val < 0.999
    k1 = _grid(val)
    sw, gt = _dicts(SWITCH, GATE)
    var = cv.hexatic(R_CUT, R_ON, nl, "A", switch=sw, gate=gt, sigma=k1["sigma"][0])
    var.set_grid(k1["cv_min"][0], k1["cv_max"][0], 512)
    context.run(3)
    # moved once, so that the hills of the first three steps lie beside the value and the bias factor is a slope of the grid
    pos = pos + np.random.default_rng(9).normal(0, 0.01, pos.shape)
    context.set_positions(pos, types)
    lists = nl.update()
    r = _ref(pos, types, L, lists, switch=SWITCH, gate=GATE)
    context.run(3)
    assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["s"], rel=1e-9)
    b = meta.cpp_integrator.getBiasFactors()[0]
    assert abs(b) > 1e-3
    F = var.cpp_force.getForceArray()
    assert np.abs(F[:, :3] + b * r["grad"]).max() <= 1e-7 * np.abs(b * r["grad"]).max()
    assert np.abs(var.get_switched() - r["switched"]).max() <= 1e-9 and np.abs(var.get_local() - r["local"]).max() <= 1e-9 * np.abs(r["local"]).max()
    # other options and none: each invalidates the step's results, and the variable computes anew when it is next asked
    t = context.current.system.getCurrentTimeStep()
    for want in ((None, GATE), (SWITCH, None), (None, None), ((0.8, 3), (0.0, 2.5)), (SWITCH, GATE)):
        var.set_options(*_dicts(*want))
        rr = _ref(pos, types, L, lists, switch=want[0], gate=want[1])
        assert var.cpp_force.getCurrentValue(t) == pytest.approx(rr["s"], rel=1e-9)
        assert np.abs(var.get_switched() - rr["switched"]).max() <= 1e-9 * np.abs(rr["switched"]).max()
        assert np.abs(var.get_local() - rr["local"]).max() <= 1e-9 * np.abs(rr["local"]).max()
    # a refused call leaves both as they were: the value stays that of (SWITCH, GATE)
    for bad in (dict(switch=dict(c0=0.6)), dict(switch=dict(c0=-1.0, p=4)), dict(switch=dict(c0=0.6, p=0)), dict(switch=(0.6, 4)),
                dict(gate=dict(n_lo=-0.5, n_hi=3.0)), dict(gate=dict(n_lo=2.0, n_hi=2.0)), dict(switch=None, gate=dict(n_lo=3.0, n_hi=2.0)),
                dict(switch=dict(c0=0.9, p=2), gate=dict(n_lo=-0.5, n_hi=3.0))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            var.set_options(**bad)
        assert var.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-9), bad
    context.run(1)                                                      # the first options again: the next step's forces are theirs
    b0 = meta.cpp_integrator.getBiasFactors()[0]
    F = var.cpp_force.getForceArray()
    assert abs(b0) > 1e-3 and np.abs(F[:, :3] + b0 * r["grad"]).max() <= 1e-7 * np.abs(b0 * r["grad"]).max()


def test_hexatic_with_coordination_on_a_2d_grid(api):
    """two row variables on one list and one 2-d grid, for one step sequence: both values and both force arrays"""
    context, cv, integrate = api
    pos, L, types = _system(seed=16)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
    cpar = cn.params(0, 0, 1.15, R_LIST)
    rc = cn.compute(pos, types, L, lists, cpar)
    k1, k2 = _grid(r["s"]), _grid(rc["s"])
    var = cv.hexatic(R_CUT, R_ON, nl, "A", sigma=k1["sigma"][0])
    var.set_grid(k1["cv_min"][0], k1["cv_max"][0], 64)
    coord = cv.coordination(1.15, nl, "A", sigma=k2["sigma"][0])
    coord.set_grid(k2["cv_min"][0], k2["cv_max"][0], 64)
    context.run(3)
    pos = pos + np.random.default_rng(9).normal(0, 0.01, pos.shape)
    context.set_positions(pos, types)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
    rc = cn.compute(pos, types, L, lists, cpar)
    context.run(3)
    cvg = meta.cpp_integrator.getCurrentValues()
    b = meta.cpp_integrator.getBiasFactors()
    print("values %s, bias factors %s" % (list(cvg), list(b)))
    assert cvg[0] == pytest.approx(r["s"], rel=1e-9) and cvg[1] == pytest.approx(rc["s"], rel=1e-9)
    assert abs(b[0]) > 1e-3 and b[1] != 0.0
    F = var.cpp_force.getForceArray()
    assert np.abs(F[:, :3] + b[0] * r["grad"]).max() <= 1e-7 * np.abs(b[0] * r["grad"]).max()
    Fc = coord.cpp_force.getForceArray()
    assert np.abs(Fc[:, :3] + b[1] * rc["grad"]).max() <= 1e-7 * np.abs(b[1] * rc["grad"]).max()


def test_hexatic_device_list_gives_the_host_lists_value(api):
    """cv.nlist_cell(device=True), never update()d by the script: the list is built for the pairs of the variable's type, in the
    rectangular box of the layer; value and forces are those of the host-built list"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST, r_buff=0.3, device=True)
    r = _ref(pos, types, L, hr.box_nlist(pos, L, R_LIST))
    var = cv.hexatic(R_CUT, R_ON, nl, "A", sigma=0.02 * r["s"])
    assert nl._types == {0} and nl._type == 0
    var.set_grid(0.1 * r["s"], 1.6 * r["s"], 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-9)
    assert nl.cpp_nlist.getNumRebuilds() == 1
    p = pos + np.random.default_rng(5).normal(0, 0.01, pos.shape)
    context.set_positions(p, types)
    context.run(1)
    t = context.current.system.getCurrentTimeStep()
    r = _ref(p, types, L, hr.box_nlist(p, L, R_LIST))
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-9)
    b = meta.cpp_integrator.getBiasFactors()[0]
    F = var.cpp_force.getForceArray()
    assert abs(b) > 1e-3 and np.abs(F[:, :3] + b * r["grad"]).max() <= 1e-7 * np.abs(b * r["grad"]).max()


KAPPA = 35.0


@pytest.mark.parametrize("opt", [dict(), dict(switch=SWITCH, gate=GATE), dict(global_order=True), dict(k=4, axis="x")],
                         ids=["plain", "switch+gate", "global", "k=4 about x"])
def test_hexatic_virial_with_the_pressure_flag_and_without(api, opt):
    """flag set: get_virial() against the restatement at the bias factor the integrator reports plus the umbrella's; flag off: it raises,
    and the force array is the same bit for bit"""
    context, cv, integrate = api

    def run(pressure):
        pos, L, types = _system(seed=15)
        context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
        context.current.system_definition.getParticleData().setPressureFlag(pressure)
        meta = integrate.mode_metadynamics(**KW)
        nl = cv.nlist_cell(r_cut=R_LIST)
        lists = nl.update()
        val = _ref(pos, types, L, lists, **opt)["s"]
        kw = _grid(val)
        sw, gt = _dicts(opt.get("switch"), opt.get("gate"))
        var = cv.hexatic(R_CUT, R_ON, nl, "A", k=opt.get("k", 6), axis=opt.get("axis", "z"), global_order=opt.get("global_order", False),
                         switch=sw, gate=gt, sigma=kw["sigma"][0])
        var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
        cv0 = 0.8 * val
        var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
        context.run(3)
        return var, meta, pos, types, L, lists, cv0

    var, meta, pos, types, L, lists, cv0 = run(True)
    s = meta.cpp_integrator.getCurrentValues()[0]
    total = meta.cpp_integrator.getBiasFactors()[0] + KAPPA * (s - cv0)
    r = _ref(pos, types, L, lists, bias=total, **opt)
    N = len(pos)
    per, raw, W = var.get_virial(per_particle=True), var.cpp_force.getVirial(), var.get_virial()
    assert per.shape == (6, N) and per.dtype == np.float64 and W.shape == (6,)
    assert np.array_equal(raw[:, :N], per)
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["virial_sum"]).max(), w_top))
    assert w_top > 1e-6
    assert np.abs(per.T - r["virial"]).max() <= 1e-9 * top
    assert np.abs(W - r["virial_sum"]).max() <= 1e-9 * w_top
    F_on = var.cpp_force.getForceArray().copy()
    assert np.abs(F_on[:, :3] + total * r["grad"]).max() <= 1e-9 * np.abs(total * r["grad"]).max()
    context.current.system_definition.getParticleData().setPressureFlag(False)
    context.run(1)
    assert np.all(var.cpp_force.getVirial() == 0.0)
    with pytest.raises(RuntimeError):
        var.get_virial()
    context.current = None
    var = run(False)[0]
    with pytest.raises(RuntimeError):
        var.get_virial(per_particle=True)
    assert np.array_equal(var.cpp_force.getForceArray(), F_on)


def test_hexatic_refusal_texts(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    import util
    pos, L, types = _system()
    L = 12.0                                                            # (a cubic box: the half list below comes from util.build_nlist)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    var = cv.hexatic(R_CUT, R_ON, nl, "A")
    var.set_grid(0.0, 1.5, 64)
    nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    nl.set_lists(*util.build_nlist(pos, L, R_LIST, half=True))
    with pytest.raises(RuntimeError, match="full neighbour list"):
        context.run(1)
    # the host class on its own (as a C++ caller would): the window, k, the axis, the options, and a device-built list short of r_cut
    sysdef = context.current.system_definition
    with pytest.raises(RuntimeError, match="0 <= r_on < r_cut"):
        _metadynamics.HexaticOrder(sysdef, 6, 2, 1.3, 1.3, False, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="1 <= k <= 12"):
        _metadynamics.HexaticOrder(sysdef, 0, 2, 1.3, 0.9, False, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="1 <= k <= 12"):
        _metadynamics.HexaticOrder(sysdef, 13, 2, 1.3, 0.9, False, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="the axis is 0, 1 or 2"):
        _metadynamics.HexaticOrder(sysdef, 6, 3, 1.3, 0.9, False, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="neighbour list is required"):
        _metadynamics.HexaticOrder(sysdef, 6, 2, 1.3, 0.9, False, None, 0, "")
    short = _metadynamics.NeighborList(sysdef)
    short.setDeviceBuild(1.2, 0.2, 1, 0)
    v = _metadynamics.HexaticOrder(sysdef, 6, 2, 1.3, 0.9, False, short, 0, "_short")
    with pytest.raises(RuntimeError, match="switch needs c0 > 0"):
        v.setSwitch(0.0, 6)
    with pytest.raises(RuntimeError, match="gate needs 0 <= n_lo < n_hi"):
        v.setGate(-0.5, 3.0)
    with pytest.raises(RuntimeError, match="must reach"):
        v.getCurrentValue(0)
    glob = _metadynamics.HexaticOrder(sysdef, 6, 2, 1.3, 0.9, True, nl.cpp_nlist, 0, "_glob")
    with pytest.raises(RuntimeError, match="global_order does not sum"):
        glob.setSwitch(0.6, 6)
    with pytest.raises(RuntimeError, match="global_order does not sum"):
        glob.setGate(1.0, 3.0)
    glob.clearSwitch()
    glob.clearGate()
