"""GPU: cv.tetrahedral through the host classes and the Python API, against the numpy restatement (tests/tetrahedral_ref.py) driven with
the bias factors the integrator reports: the value the engine used to rtol 1e-9, force arrays to 1e-7 of max|F| (the bias factor is the
integrator's own), virials to 1e-9.  Where forces are compared, the particles are moved between steps: with every hill on one value the
bias factor is the rounding residue at the top of the hills."""
import numpy as np
import pytest

import tetrahedral_ref as tr
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

R_ON, R_CUT = 0.9, 1.3
R_LIST = 1.35
SWITCH, GATE = (0.6, 6), (1.5, 3.5)
KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _system(seed=12, noise=0.05):
    pos, L = tr.diamond_lattice(3)
    pos = pos + np.random.default_rng(seed).normal(0, noise, pos.shape)
    return pos, L, (np.arange(len(pos)) % 4 == 3).astype(np.int32)


def _ref(pos, types, L, lists, bias=1.0, **opt):
    r = tr.compute(pos, types, L, lists, tr.params(0, R_CUT, R_ON, **opt), bias=bias)
    W = r["W"]
    assert np.all((W == 0.0) | (W >= 1e-3))                             # the condition of tests/test_gpu_tetrahedral.py
    return r


def _grid(val):
    return dict(sigma=[0.02 * abs(val)], cv_min=[0.4 * val], cv_max=[1.6 * val], num_points=[512])


def _dicts(switch, gate):
    return (None if switch is None else dict(c0=switch[0], p=switch[1]), None if gate is None else dict(n_lo=gate[0], n_hi=gate[1]))


def test_tetrahedral_alone_on_a_grid(api):
    """512-point well-tempered grid, stride 1.  The particles are moved a little before every step, so that the hills land at different
    values and the bias factor is a slope of the grid: over six such steps the value is the restatement's and the force array is
    -(bias factor) x the restatement's gradient.  Then the getters and the log quantity"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
    val = r["s"]
    assert val > 0.8
    kw = _grid(val)
    var = cv.tetrahedral(R_CUT, R_ON, nl, "A", sigma=kw["sigma"][0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    rng = np.random.default_rng(8)
    seen = []
    for step in range(1, 7):
        if step > 1:
            pos = pos + rng.normal(0, 0.01, pos.shape)
            context.set_positions(pos, types)
            lists = nl.update()
            r = _ref(pos, types, L, lists)
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
    assert len(set(seen)) == 6                                          # hills landed: the bias factor moved at every step
    val = r["s"]
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-9)
    assert var.cpp_force.getLogValue("cv_tetrahedral", t) == pytest.approx(val, rel=1e-9)
    assert "cv_tetrahedral" in var.cpp_force.getProvidedLogQuantities()
    loc, sw, cn = var.get_local(), var.get_switched(), var.get_coordination()
    assert loc.shape == sw.shape == cn.shape == (len(pos),)
    assert np.abs(loc - r["local"]).max() <= 1e-9 * np.abs(r["local"]).max()
    assert np.abs(cn - r["coordination"]).max() <= 1e-9 * np.abs(r["coordination"]).max()
    assert np.array_equal(loc, sw) and np.all(loc[types == 1] == 0.0) and np.all(cn[types == 1] == 0.0)
    assert loc[types == 0].mean() == pytest.approx(val, rel=1e-9)
    named = cv.tetrahedral(R_CUT, R_ON, nl, "A", name="ice")
    assert "cv_tetrahedral_ice" in named.cpp_force.getProvidedLogQuantities()
    assert named.cos0 == -1.0 / 3.0 and named.normalise is True and named.r_cut == R_CUT and named.cpp_force.getRCut() == R_CUT
    assert named.get_rcut() == {("A", "A"): R_CUT, ("A", "B"): -1.0, ("B", "B"): -1.0}


def test_tetrahedral_constructor_refusals_leave_nothing_behind(api):
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    ok = dict(r_cut=R_CUT, r_on=R_ON, nlist=nl, type="A")
    cv.tetrahedral(**ok)
    cv.tetrahedral(**{**ok, "switch": dict(c0=0.6, p=6), "gate": dict(n_lo=1, n_hi=3)})
    cv.tetrahedral(**{**ok, "normalise": False, "cos0": 0.0})
    n_forces = len(context.current.forces)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(type="Z"), dict(r_on=-0.1), dict(r_on=nan), dict(r_on=1.3), dict(r_on=2.0), dict(r_cut=nan), dict(r_cut=inf),
                dict(r_cut=0.0, r_on=0.0),
                dict(r_cut=1.4),                                        # beyond the list's 1.35
                dict(cos0=-1.01), dict(cos0=1.5), dict(cos0=nan), dict(nlist=None),
                dict(switch=dict(c0=0.6)), dict(switch=dict(p=6)), dict(switch=dict(c0=0.6, p=6, q=1)), dict(switch=dict(c0=0.0, p=6)),
                dict(switch=dict(c0=0.6, p=0)), dict(switch=dict(c0=0.6, p=2.5)), dict(switch=dict(c0=nan, p=6)), dict(switch=(0.6, 6)),
                dict(gate=dict(n_lo=0.5, n_hi=3.0)),                    # n_lo < 1
                dict(gate=dict(n_lo=0.0, n_hi=3.0)), dict(gate=dict(n_lo=3.0, n_hi=3.0)), dict(gate=dict(n_lo=1.0)), dict(gate=dict(n_lo=1.0, n_hi=inf)),
                dict(gate=dict(n_lo=1.0, n_hi=3.0, x=1)), dict(gate=(1.0, 3.0)),
                dict(normalise=False, switch=dict(c0=0.6, p=6)), dict(normalise=False, gate=dict(n_lo=1.0, n_hi=3.0))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.tetrahedral(**{**ok, **bad})
        assert len(context.current.forces) == n_forces, bad            # a refused variable leaves nothing behind
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.tetrahedral(R_CUT, R_ON, cv.nlist_cell(r_cut=1.2), "A")
    assert len(context.current.forces) == n_forces


def test_tetrahedral_set_options_between_runs(api):
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
    var = cv.tetrahedral(R_CUT, R_ON, nl, "A", switch=sw, gate=gt, sigma=k1["sigma"][0])
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
    for want in ((None, GATE), (SWITCH, None), (None, None), ((0.8, 3), (1.0, 2.5)), (SWITCH, GATE)):
        var.set_options(*_dicts(*want))
        rr = _ref(pos, types, L, lists, switch=want[0], gate=want[1])
        assert var.cpp_force.getCurrentValue(t) == pytest.approx(rr["s"], rel=1e-9)
        assert np.abs(var.get_switched() - rr["switched"]).max() <= 1e-9 * np.abs(rr["switched"]).max()
        assert np.abs(var.get_local() - rr["local"]).max() <= 1e-9 * np.abs(rr["local"]).max()
    # a refused call leaves both as they were: the value stays that of (SWITCH, GATE)
    for bad in (dict(switch=dict(c0=0.6)), dict(switch=dict(c0=-1.0, p=4)), dict(switch=dict(c0=0.6, p=0)), dict(switch=(0.6, 4)),
                dict(gate=dict(n_lo=0.5, n_hi=3.0)), dict(gate=dict(n_lo=2.0, n_hi=2.0)), dict(switch=None, gate=dict(n_lo=0.0, n_hi=2.0)),
                dict(switch=dict(c0=0.9, p=2), gate=dict(n_lo=0.5, n_hi=3.0))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            var.set_options(**bad)
        assert var.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-9), bad
    context.run(1)                                                      # the first options again: the next step's forces are theirs
    b0 = meta.cpp_integrator.getBiasFactors()[0]
    F = var.cpp_force.getForceArray()
    assert abs(b0) > 1e-3 and np.abs(F[:, :3] + b0 * r["grad"]).max() <= 1e-7 * np.abs(b0 * r["grad"]).max()
    # the penalty takes neither
    pen = cv.tetrahedral(R_CUT, R_ON, nl, "A", normalise=False, name="sw")
    rp = _ref(pos, types, L, lists, normalise=False)
    assert pen.cpp_force.getCurrentValue(t) == pytest.approx(rp["s"], rel=1e-9)
    assert np.abs(pen.get_local() - rp["local"]).max() <= 1e-9 * np.abs(rp["local"]).max() and np.array_equal(pen.get_local(), pen.get_switched())
    for bad in (dict(switch=sw), dict(gate=gt)):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            pen.set_options(**bad)
    pen.set_options()


def test_tetrahedral_device_list_and_no_update(api):
    """cv.nlist_cell(device=True), never update()d by the script: the list is built for the pairs of the variable's type; particles
    displaced between runs by more than r_buff / 2: the list rebuilds and the value follows"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST, r_buff=0.3, device=True)
    val0 = _ref(pos, types, L, util.build_nlist(pos, L, R_LIST))["s"]
    var = cv.tetrahedral(R_CUT, R_ON, nl, "A", sigma=0.02 * val0)
    assert nl._types == {0} and nl._type == 0
    var.set_grid(0.1 * val0, 1.6 * val0, 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(val0, rel=1e-9)
    assert nl.cpp_nlist.getNumRebuilds() == 1
    rng = np.random.default_rng(5)
    p = pos.copy()
    values = [val0]
    for k in range(2):
        p = p + rng.normal(0, 0.06, p.shape)
        assert np.sqrt(((p - pos) ** 2).sum(-1)).max() > 0.15
        context.set_positions(p, types)
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        r = _ref(p, types, L, util.build_nlist(p, L, R_LIST))
        values.append(r["s"])
        assert var.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-9)
        assert nl.cpp_nlist.getNumRebuilds() == 2 + k
        b = meta.cpp_integrator.getBiasFactors()[0]
        F = var.cpp_force.getForceArray()
        F_ref = -b * r["grad"]
        assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert abs(values[-1] - values[0]) > 1e-3 * abs(values[0])


KAPPA = 35.0


def _umbrella_run(api, pressure, steps=3, **opt):
    context, cv, integrate = api
    pos, L, types = _system(seed=15)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    val = _ref(pos, types, L, lists, **opt)["s"]
    kw = _grid(val)
    sw, gt = _dicts(opt.get("switch"), opt.get("gate"))
    var = cv.tetrahedral(R_CUT, R_ON, nl, "A", normalise=opt.get("normalise", True), switch=sw, gate=gt, sigma=kw["sigma"][0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    cv0 = 0.8 * val
    var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(steps)
    return var, meta, pos, types, L, lists, val, cv0, kw


@pytest.mark.parametrize("opt", [dict(), dict(switch=SWITCH, gate=GATE), dict(normalise=False)], ids=["plain", "switch+gate", "penalty"])
def test_tetrahedral_virial_with_the_pressure_flag_and_without(api, opt):
    """flag set: get_virial() against the restatement at the bias factor the integrator reports plus the umbrella's; flag off: it raises,
    and the force array is the same bit for bit; a stale array reads back as zeros"""
    context, cv, integrate = api
    var, meta, pos, types, L, lists, val, cv0, _ = _umbrella_run(api, True, **opt)
    s = meta.cpp_integrator.getCurrentValues()[0]
    total = meta.cpp_integrator.getBiasFactors()[0] + KAPPA * (s - cv0)
    r = _ref(pos, types, L, lists, bias=total, **opt)
    N = len(pos)
    per, raw, W = var.get_virial(per_particle=True), var.cpp_force.getVirial(), var.get_virial()
    assert per.shape == (6, N) and per.dtype == np.float64 and W.shape == (6,)
    assert np.array_equal(raw[:, :N], per)
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["virial_sum"]).max(), w_top))
    assert w_top > 1e-3
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
    var = _umbrella_run(api, False, **opt)[0]
    with pytest.raises(RuntimeError):
        var.get_virial(per_particle=True)
    assert np.array_equal(var.cpp_force.getForceArray(), F_on)


def test_tetrahedral_refusal_texts(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    var = cv.tetrahedral(R_CUT, R_ON, nl, "A")
    var.set_grid(0.0, 1.5, 64)
    nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    nl.set_lists(*util.build_nlist(pos, L, R_LIST, half=True))
    with pytest.raises(RuntimeError, match="full neighbour list"):
        context.run(1)
    # the host class on its own (as a C++ caller would): the window, cos0, the options, and a device-built list that stops short of r_cut
    sysdef = context.current.system_definition
    with pytest.raises(RuntimeError, match="0 <= r_on < r_cut"):
        _metadynamics.TetrahedralOrder(sysdef, 1.3, 1.3, -1.0 / 3.0, True, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="-1 <= cos0 <= 1"):
        _metadynamics.TetrahedralOrder(sysdef, 1.3, 0.9, 1.2, True, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="neighbour list is required"):
        _metadynamics.TetrahedralOrder(sysdef, 1.3, 0.9, 0.0, True, None, 0, "")
    short = _metadynamics.NeighborList(sysdef)
    short.setDeviceBuild(1.2, 0.2, 1, 0)
    v = _metadynamics.TetrahedralOrder(sysdef, 1.3, 0.9, -1.0 / 3.0, True, short, 0, "_short")
    with pytest.raises(RuntimeError, match="switch needs c0 > 0"):
        v.setSwitch(0.0, 6)
    with pytest.raises(RuntimeError, match="gate needs 1 <= n_lo < n_hi"):
        v.setGate(0.5, 3.0)
    with pytest.raises(RuntimeError, match="must reach"):
        v.getCurrentValue(0)
    pen = _metadynamics.TetrahedralOrder(sysdef, 1.3, 0.9, -1.0 / 3.0, False, nl.cpp_nlist, 0, "_pen")
    with pytest.raises(RuntimeError, match="switch needs the normalised variable"):
        pen.setSwitch(0.6, 6)
    with pytest.raises(RuntimeError, match="gate needs the normalised variable"):
        pen.setGate(1.0, 3.0)
    pen.clearSwitch()
    pen.clearGate()
