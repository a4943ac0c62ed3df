"""GPU: cv.coordination through the host classes and the Python API, against the numpy restatement (tests/coordination_ref.py) and the
oracle's bias grid driven with the restatement's values: the value the engine used and the bias factor to rtol 1e-7, force arrays to 1e-7
of max|F| (the bias factor is the integrator's own), virials to 1e-9 at the bias factor the integrator reports.  Where a bias factor is
compared, the particles are moved between steps: with every hill on one value the factor is the rounding residue at the top of the hills.

The 2-d grid pairs the variable with cv.lamellar, as tests/test_gpu_debye_api.py does."""
import numpy as np
import pytest

import coordination_ref as cn
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

R0, R_CUT = 1.15, 2.0
R_LIST = 2.05
KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _system(seed=12, noise=0.05):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(seed).normal(0, noise, pos.shape)
    return pos, L, (np.arange(len(pos)) % 2).astype(np.int32)


def _ref(pos, types, L, lists, bias=1.0, pair=(0, 1), switch=None):
    return cn.compute(pos, types, L, lists, cn.params(pair[0], pair[1], R0, R_CUT, switch=switch), bias=bias)


def _grid(val):
    return dict(sigma=[0.02 * abs(val)], cv_min=[0.4 * val], cv_max=[1.6 * val], num_points=[512])


def test_coordination_alone_on_a_grid(api, ref):
    """512-point well-tempered grid, stride 1: value in the log and on the grid.  The particles are moved a little before every step, so
    that the hills land at different values and the bias factor is a slope of the grid and not the rounding residue at the top of one
    hill: over six such steps the bias factor is the oracle's, driven with the restatement's values, and the force array is
    -(bias factor) x the restatement's gradient.  Then local and switched values and the log quantity"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
    val = r["s"]
    assert val > 5.0
    kw = _grid(val)
    var = cv.coordination(R0, nl, "A", partner="B", r_cut=R_CUT, sigma=kw["sigma"][0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    oracle = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    rng = np.random.default_rng(8)
    seen, previous = [], val
    for step in range(1, 7):
        if step > 1:
            pos = pos + rng.normal(0, 0.015, pos.shape)
            context.set_positions(pos, types)
            lists = nl.update()
            r = _ref(pos, types, L, lists)
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        assert t == step
        assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["s"], rel=1e-9)
        b = meta.cpp_integrator.getBiasFactors()[0]
        # every run() begins with the integrator's prepRun, which updates the potential at the step it starts from with the value from
        # before the particles were moved (tests/test_gpu_debye_api.py); then the step itself, with this value
        oracle.update_bias(step - 1, [previous])
        b_ref = oracle.update_bias(step, [r["s"]])[0]
        previous = r["s"]
        F = var.cpp_force.getForceArray()
        F_ref = -b * r["grad"]
        print("step %d: s %.6f, bias factor %.6e (oracle %.6e), max |F - F_ref| %.3e of max |F_ref| %.3e"
              % (step, r["s"], b, b_ref, np.abs(F[:, :3] - F_ref).max(), np.abs(F_ref).max()))
        seen.append(b)
        if step > 1:
            assert abs(b) > 1e-3                                        # a slope of the deposited hills
            assert b == pytest.approx(b_ref, rel=1e-7)
            assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
        assert np.all(F[:, 3] == 0.0)
    assert len(set(seen)) == 6                                          # hills landed: the bias factor moved at every step
    val = r["s"]
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-9)
    assert var.cpp_force.getLogValue("cv_coordination", t) == pytest.approx(val, rel=1e-9)
    assert "cv_coordination" in var.cpp_force.getProvidedLogQuantities()
    loc, sw = var.get_local(), var.get_switched()
    assert loc.shape == (len(pos),) and np.abs(loc - r["local"]).max() <= 1e-9 * np.abs(r["local"]).max()
    assert np.array_equal(loc, sw) and np.all(loc[types == 1] == 0.0)
    assert loc[types == 0].mean() == pytest.approx(val, rel=1e-9)
    named = cv.coordination(R0, nl, "A", name="self")
    assert "cv_coordination_self" in named.cpp_force.getProvidedLogQuantities()
    assert named.partner == "A" and named.r_cut == pytest.approx(R_LIST) and (named.n, named.m, named.d_0) == (6, 12, 0.0)


def test_coordination_get_rcut_for_three_type_names(api):
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types % 3, ["A", "B", "C"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    off = -1.0
    ab = cv.coordination(R0, nl, "A", partner="B", r_cut=R_CUT)
    assert ab.get_rcut() == {("A", "A"): off, ("A", "B"): pytest.approx(2.0), ("A", "C"): off, ("B", "B"): off, ("B", "C"): off, ("C", "C"): off}
    cb = cv.coordination(R0, nl, "C", partner="B", r_cut=1.5)
    assert cb.get_rcut() == {("A", "A"): off, ("A", "B"): off, ("A", "C"): off, ("B", "B"): off, ("B", "C"): pytest.approx(1.5), ("C", "C"): off}
    cc = cv.coordination(R0, nl, "C")
    assert cc.get_rcut() == {("A", "A"): off, ("A", "B"): off, ("A", "C"): off, ("B", "B"): off, ("B", "C"): off,
                             ("C", "C"): pytest.approx(R_LIST)}


def test_coordination_constructor_refusals_leave_nothing_behind(api):
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    ok = dict(r_0=R0, nlist=nl, type="A", partner="B", r_cut=R_CUT)
    cv.coordination(**ok)
    cv.coordination(**{**ok, "switch": dict(c0=5.0, p=8, less=True)})
    n_forces = len(context.current.forces)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(type="Z"), dict(partner="Z"), dict(n=12), dict(n=13), dict(n=0), dict(n=6, m=6), dict(m=33), dict(n=32, m=40),
                dict(n=5.5), dict(r_0=0.0), dict(r_0=-1.0), dict(r_0=nan), dict(r_0=inf), dict(d_0=-0.1), dict(d_0=nan),
                dict(d_0=2.0), dict(d_0=2.5),                           # r_cut <= d_0
                dict(r_cut=0.0), dict(r_cut=nan), dict(r_cut=inf),
                dict(r_cut=2.1),                                        # beyond the list's 2.05
                dict(nlist=None), dict(switch=dict(c0=5.0)), dict(switch=dict(p=8)), dict(switch=dict(c0=5.0, p=8, q=1)),
                dict(switch=dict(c0=0.0, p=8)), dict(switch=dict(c0=5.0, p=0)), dict(switch=dict(c0=5.0, p=2.5)), dict(switch=dict(c0=nan, p=8)),
                dict(switch=(5.0, 8))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.coordination(**{**ok, **bad})
        assert len(context.current.forces) == n_forces, bad            # a refused variable leaves nothing behind
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.coordination(R0, cv.nlist_cell(r_cut=1.9), "A", r_cut=2.0)
    assert len(context.current.forces) == n_forces


def test_coordination_with_lamellar_on_a_2d_grid_and_set_switch_between_runs(api, ref):
    context, cv, integrate = api
    pos, L, _ = _system(seed=13)
    types = (np.random.default_rng(4).random(len(pos)) < 0.5).astype(np.int32)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    switch = (6.0, 8)
    r = _ref(pos, types, L, lists, switch=switch)
    val = r["s"]
    assert 0.05 < val < 0.95
    rbox = ref.Box.make(L)
    vec = [(0, 0, 2)]
    k1 = _grid(val)
    var = cv.coordination(R0, nl, "A", partner="B", r_cut=R_CUT, switch=dict(c0=switch[0], p=switch[1]), sigma=k1["sigma"][0])
    var.set_grid(k1["cv_min"][0], k1["cv_max"][0], 64)
    lam = cv.lamellar(sigma=0.05, mode=dict(A=1.0, B=-1.0), lattice_vectors=vec)
    lam.set_grid(cv_min=-1.0, cv_max=1.0, num_points=64)
    context.run(3)
    # moved once, so that the hills of the first three steps lie beside the value and the bias factors are slopes of the grid
    pos = pos + np.random.default_rng(9).normal(0, 0.015, pos.shape)
    context.set_positions(pos, types)
    lists = nl.update()
    r = _ref(pos, types, L, lists, switch=switch)
    opt = util.oracle_postype(pos, types)
    context.run(3)
    cvg = meta.cpp_integrator.getCurrentValues()
    assert cvg[0] == pytest.approx(r["s"], rel=1e-9)
    assert cvg[1] == pytest.approx(ref.lamellar_cv(vec, opt, util.MODE_AB, rbox), rel=1e-6, abs=1e-9)
    b = meta.cpp_integrator.getBiasFactors()
    print("values %s, bias factors %s" % (list(cvg), list(b)))
    assert abs(b[0]) > 1e-3
    F = var.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    sw = var.get_switched()
    assert np.abs(sw - r["switched"]).max() <= 1e-9 and np.abs(var.get_local() - r["local"]).max() <= 1e-9 * r["local"].max()
    Fl = lam.cpp_force.getForceArray()
    Fl_ref = ref.lamellar_forces(vec, opt, util.MODE_AB, rbox, b[1])
    assert np.abs(Fl[:, :3] - Fl_ref[:, :3]).max() <= 1e-5 * np.abs(Fl_ref[:, :3]).max()
    # another switch, `less`, and none: each invalidates the step's results, and the variable computes anew when it is next asked
    t = context.current.system.getCurrentTimeStep()
    for new, want in ((dict(c0=5.0, p=4, less=True), (5.0, 4, True)), (None, None), (dict(c0=7.0, p=6), (7.0, 6)),
                      (dict(c0=switch[0], p=switch[1]), switch)):
        var.set_switch(new)
        rr = _ref(pos, types, L, lists, switch=want)
        assert var.cpp_force.getCurrentValue(t) == pytest.approx(rr["s"], rel=1e-9)
        assert np.abs(var.get_switched() - rr["switched"]).max() <= 1e-9 * np.abs(rr["switched"]).max()
        assert np.abs(var.get_local() - rr["local"]).max() <= 1e-9 * np.abs(rr["local"]).max()
    context.run(1)                                                      # the first switch again: the next step's forces are its forces
    b0 = meta.cpp_integrator.getBiasFactors()[0]
    F = var.cpp_force.getForceArray()
    assert abs(b0) > 1e-3 and np.abs(F[:, :3] + b0 * r["grad"]).max() <= 1e-7 * np.abs(b0 * r["grad"]).max()
    for bad in (dict(c0=5.0), dict(c0=-1.0, p=4), dict(c0=5.0, p=0), (5.0, 4)):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            var.set_switch(bad)


def test_coordination_device_list_with_two_types_and_no_update(api):
    """cv.nlist_cell(device=True), never update()d by the script, with A != B: the variable attaches BOTH type ids, so the list is built
    for all pairs and holds the A-B pairs — the value is > 0 and the restatement's; particles displaced between runs by more than
    r_buff / 2: the list rebuilds and the value follows"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST, r_buff=0.4, device=True)
    val0 = _ref(pos, types, L, util.build_nlist(pos, L, R_LIST))["s"]
    var = cv.coordination(R0, nl, "A", partner="B", r_cut=R_CUT, sigma=0.02 * val0)
    assert nl._types == {0, 1} and nl._type == -1
    var.set_grid(0.1 * val0, 1.6 * val0, 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    got = var.cpp_force.getCurrentValue(t)
    assert got > 5.0 and got == pytest.approx(val0, rel=1e-9)
    assert nl.cpp_nlist.getNumRebuilds() == 1
    rng = np.random.default_rng(5)
    p = pos.copy()
    values = [val0]
    for k in range(2):
        p = p + rng.normal(0, 0.12, p.shape)
        assert np.sqrt(((p - pos) ** 2).sum(-1)).max() > 0.2
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
    # one type on both sides: the list of that type pair is enough
    context.current = None
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST, device=True)
    cv.coordination(R0, nl, "B")
    assert nl._types == {1} and nl._type == 1


KAPPA = 35.0


def _umbrella_run(api, pressure, steps=3, switch=None):
    context, cv, integrate = api
    pos, L, types = _system(seed=15)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    val = _ref(pos, types, L, lists, switch=switch)["s"]
    kw = _grid(val)
    var = cv.coordination(R0, nl, "A", partner="B", r_cut=R_CUT, sigma=kw["sigma"][0],
                          switch=None if switch is None else dict(c0=switch[0], p=switch[1]))
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    cv0 = 0.8 * val
    var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(steps)
    return var, meta, pos, types, L, lists, val, cv0, kw


@pytest.mark.parametrize("switch", [None, (6.0, 8)], ids=["plain", "switch"])
def test_coordination_virial_with_the_pressure_flag_and_without(api, switch):
    """flag set: get_virial() against the restatement at the bias factor the integrator reports plus the umbrella's; flag off: it raises,
    and the force array is the same bit for bit; a stale array reads back as zeros"""
    context, cv, integrate = api
    var, meta, pos, types, L, lists, val, cv0, _ = _umbrella_run(api, True, switch=switch)
    s = meta.cpp_integrator.getCurrentValues()[0]
    total = meta.cpp_integrator.getBiasFactors()[0] + KAPPA * (s - cv0)
    r = _ref(pos, types, L, lists, bias=total, switch=switch)
    N = len(pos)
    per, raw, W = var.get_virial(per_particle=True), var.cpp_force.getVirial(), var.get_virial()
    assert per.shape == (6, N) and per.dtype == np.float64 and W.shape == (6,)
    assert np.array_equal(raw[:, :N], per)
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["virial_sum"]).max(), w_top))
    assert w_top > 0.05
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
    var = _umbrella_run(api, False, switch=switch)[0]
    with pytest.raises(RuntimeError):
        var.get_virial(per_particle=True)
    assert np.array_equal(var.cpp_force.getForceArray(), F_on)


def test_coordination_refuses_a_half_list_and_a_short_list(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types = _system()
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    var = cv.coordination(R0, nl, "A", partner="B", r_cut=R_CUT)
    var.set_grid(0.0, 8.0, 64)
    nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    nl.set_lists(*util.build_nlist(pos, L, R_LIST, half=True))
    with pytest.raises(RuntimeError, match="full neighbour list"):
        context.run(1)
    # the host classes on their own (as a C++ caller would): exponents, m above the capacity, r_cut inside d_0, a bad switch, and a
    # device-built list that stops short of r_cut
    sysdef = context.current.system_definition
    with pytest.raises(RuntimeError, match="1 <= n < m"):
        _metadynamics.CoordinationNumber(sysdef, R0, 0.0, 12, 12, 2.0, nl.cpp_nlist, 0, 1, "")
    with pytest.raises(RuntimeError, match="m <= 32"):
        _metadynamics.CoordinationNumber(sysdef, R0, 0.0, 6, 33, 2.0, nl.cpp_nlist, 0, 1, "")
    with pytest.raises(RuntimeError, match="r_cut > d_0"):
        _metadynamics.CoordinationNumber(sysdef, R0, 2.0, 6, 12, 2.0, nl.cpp_nlist, 0, 1, "")
    short = _metadynamics.NeighborList(sysdef)
    short.setDeviceBuild(1.9, 0.2, 1, -1)
    v = _metadynamics.CoordinationNumber(sysdef, R0, 0.0, 6, 12, 2.0, short, 0, 1, "_short")
    with pytest.raises(RuntimeError, match="switch needs"):
        v.setSwitch(0.0, 8, False)
    with pytest.raises(RuntimeError, match="must reach"):
        v.getCurrentValue(0)
