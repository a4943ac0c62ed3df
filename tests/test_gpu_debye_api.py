"""GPU: cv.debye_structure_factor through the host classes and the Python API, against the numpy restatement (tests/debye_ref.py) and the
oracle's bias grid driven with the restatement's values: the value the engine used and the bias factor to rtol 1e-7, force arrays to 1e-7
of max|F| (the bias factor is the integrator's own), virials to 1e-9 at the bias factor the integrator reports.  Where a bias factor is
compared, the particles are moved between steps: with every hill on one value the factor is the rounding residue at the top of the hills.

The 2-d grid pairs the variable with cv.lamellar: cv.potential_energy can only be the single variable of a run (the integrator's rule,
IntegratorMetaDynamics::update, as in tests/test_gpu_env_similarity_api.py); that the pairing with it is refused is asserted."""
import numpy as np
import pytest

import debye_ref as dsf
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

Q, WEIGHTS, R_CUT = (7.695, 8.886), (1.0, -0.5), 2.4
R_LIST = 2.45
KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _system(seed=12, noise=0.05):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(seed).normal(0, noise, pos.shape)
    return pos, L, np.zeros(len(pos), dtype=np.int32)


def _ref(pos, types, L, lists, bias=1.0, type_id=0):
    return dsf.compute(pos, types, L, lists, Q, R_CUT, type_id, c=WEIGHTS, bias=bias)


def _grid(val):
    """s = I(Q111) - I(Q200) / 2 is positive: the grid runs from 0.4 s up to 1.6 s"""
    return dict(sigma=[0.02 * abs(val)], cv_min=[0.4 * val], cv_max=[1.6 * val], num_points=[512])


def _oracle_bias(ref, kw, values, steps):
    g = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    return [g.update_bias(t, values) for t in range(steps + 1)]


def test_debye_alone_on_a_grid(api, ref):
    """512-point well-tempered grid, stride 1: value in the log and on the grid.  The particles are moved a little before every step, so
    that the hills land at different values and the bias factor is a slope of the grid and not the rounding residue at the top of one
    hill: over six such steps the bias factor is the oracle's, driven with the restatement's values, and the force array is
    -(bias factor) x the restatement's gradient.  Then intensities, local values and the spectrum"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
    val = r["s"]
    assert val > 1.0
    kw = _grid(val)
    var = cv.debye_structure_factor(Q, R_CUT, nl, "A", weights=WEIGHTS, sigma=kw["sigma"][0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    assert var.get_rcut() == {("A", "A"): pytest.approx(2.4)}
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
        # every run() begins with the integrator's prepRun, which updates the potential at the step it starts from (and deposits there
        # too): the variable has computed that time step already, so it hands over the value from before the particles were moved
        # (set_positions between runs belongs to the stand-alone system, not to a simulation); then the step itself, with this value
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
    assert var.cpp_force.getLogValue("cv_debye_structure_factor", t) == pytest.approx(val, rel=1e-9)
    assert "cv_debye_structure_factor" in var.cpp_force.getProvidedLogQuantities()
    I = var.get_intensities()
    assert I.shape == (2,) and np.abs(I - r["I"]).max() <= 1e-9 * np.abs(r["I"]).max()
    loc = var.get_local()
    assert loc.shape == (len(pos),) and np.abs(loc - r["local"]).max() <= 1e-9 * np.abs(r["local"]).max()
    assert loc.mean() == pytest.approx(val, rel=1e-9)
    for n_q, lo, hi in ((1, Q[0], Q[0]), (64, 2.0, 14.0), (256, 2.0, 14.0)):
        Qm, spec = var.get_spectrum(lo, hi, n_q)
        Q_ref, I_ref = dsf.spectrum(pos, types, L, lists, R_CUT, 0, lo, hi, n_q)
        assert np.array_equal(Qm, Q_ref) and spec.shape == (n_q,)
        assert np.abs(spec - I_ref).max() <= 1e-10 * np.abs(I_ref).max()
    assert var.get_spectrum(Q[0], Q[0], 1)[1][0] == pytest.approx(I[0], rel=1e-12)
    # the spectrum left the step's results alone
    assert np.array_equal(var.get_intensities(), I) and np.array_equal(var.cpp_force.getForceArray(), F)
    for bad in ((0.0, 2.0, 4), (3.0, 2.0, 4), (1.0, 2.0, 0), (1.0, 2.0, 257), (1.0, float("inf"), 4), (float("nan"), 2.0, 4), (1.0, 2.0, 2.5)):
        with pytest.raises(RuntimeError):
            var.get_spectrum(*bad)
    named = cv.debye_structure_factor(Q[0], R_CUT, nl, "A", name="fcc")
    assert "cv_debye_structure_factor_fcc" in named.cpp_force.getProvidedLogQuantities()
    assert named.q == [Q[0]] and named.weights == [1.0]                 # a single number, weights 1.0 each


def test_debye_constructor_refusals_leave_nothing_behind(api):
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    ok = dict(q=Q, r_cut=R_CUT, nlist=nl, type="A", weights=WEIGHTS)
    cv.debye_structure_factor(**ok)
    n_forces = len(context.current.forces)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(type="Z"), dict(q=()), dict(q=(1.0,) * 9, weights=None), dict(q=0.0, weights=None), dict(q=-1.0, weights=None),
                dict(q=(7.7, nan)), dict(q=(7.7, inf)), dict(q="peak"), dict(weights=(1.0,)), dict(weights=(1.0, nan)), dict(weights=(1.0, inf)),
                dict(weights=(1.0, 2.0, 3.0)), dict(r_cut=0.0), dict(r_cut=-2.4), dict(r_cut=nan), dict(r_cut=inf),
                dict(r_cut=2.5),                                        # beyond the list's 2.45
                dict(nlist=None)):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.debye_structure_factor(**{**ok, **bad})
        assert len(context.current.forces) == n_forces, bad            # a refused variable leaves nothing behind
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.debye_structure_factor(Q, 2.4, cv.nlist_cell(r_cut=2.3), "A")
    assert len(context.current.forces) == n_forces


def test_debye_with_lamellar_on_a_2d_grid(api, ref):
    context, cv, integrate = api
    pos, L, _ = _system(seed=13)
    types = (np.random.default_rng(4).random(len(pos)) < 0.5).astype(np.int32)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
    val = r["s"]
    rbox = ref.Box.make(L)
    opt = util.oracle_postype(pos, types)
    vec = [(0, 0, 2)]
    k1 = _grid(val)
    var = cv.debye_structure_factor(Q, R_CUT, nl, "A", weights=WEIGHTS, sigma=k1["sigma"][0])
    var.set_grid(k1["cv_min"][0], k1["cv_max"][0], 64)
    lam = cv.lamellar(sigma=0.05, mode=dict(A=1.0, B=-1.0), lattice_vectors=vec)
    lam.set_grid(cv_min=-1.0, cv_max=1.0, num_points=64)
    context.run(3)
    # moved once, so that the hills of the first three steps lie beside the value and the bias factors are slopes of the grid, not the
    # rounding residue at the top of a hill; they are the integrator's own here (tests above hold them against the oracle)
    pos = pos + np.random.default_rng(9).normal(0, 0.015, pos.shape)
    context.set_positions(pos, types)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
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
    assert np.all(F[types == 1] == 0.0)
    Fl = lam.cpp_force.getForceArray()
    Fl_ref = ref.lamellar_forces(vec, opt, util.MODE_AB, rbox, b[1])
    assert np.abs(Fl[:, :3] - Fl_ref[:, :3]).max() <= 1e-5 * np.abs(Fl_ref[:, :3]).max()


def test_debye_beside_potential_energy_is_the_integrators_refusal(api):
    """cv.potential_energy beside it: the integrator's own rule (a variable that needs the net force is the only one of its run) refuses
    the pairing, whatever the second variable is"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    nl.update()
    var = cv.debye_structure_factor(Q, R_CUT, nl, "A", weights=WEIGHTS, sigma=0.05)
    var.set_grid(0.5, 2.5, 64)
    pe = cv.potential_energy(sigma=40.0)
    pe.set_grid(-100.0, 100.0, 16)
    with pytest.raises(RuntimeError, match="Only one collective variable requiring the potential energy"):
        context.run(1)


def test_debye_device_list_with_no_update(api, ref):
    """cv.nlist_cell(device=True), never update()d by the script: the list is built on the device for this variable's type pair;
    particles displaced between runs by more than r_buff / 2 — the list rebuilds and the value follows"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST, r_buff=0.4, device=True)
    val0 = _ref(pos, types, L, util.build_nlist(pos, L, R_LIST))["s"]
    var = cv.debye_structure_factor(Q, R_CUT, nl, "A", weights=WEIGHTS, sigma=0.02 * val0)
    var.set_grid(0.1 * val0, 1.6 * val0, 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(val0, rel=1e-9)
    assert nl.cpp_nlist.getNumRebuilds() == 1
    rng = np.random.default_rng(5)
    p = pos.copy()
    values = [val0]
    for k in range(3):
        p = p + rng.normal(0, 0.12, p.shape)
        assert np.sqrt(((p - pos) ** 2).sum(-1)).max() > 0.2
        context.set_positions(p, types)
        context.run(1)
        t = context.current.system.getCurrentTimeStep()
        r = _ref(p, types, L, util.build_nlist(p, L, R_LIST))
        values.append(r["s"])
        assert var.cpp_force.getCurrentValue(t) == pytest.approx(r["s"], rel=1e-9)
        assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["s"], rel=1e-9)
        assert nl.cpp_nlist.getNumRebuilds() == 2 + k
        b = meta.cpp_integrator.getBiasFactors()[0]
        F = var.cpp_force.getForceArray()
        F_ref = -b * r["grad"]
        assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert abs(values[-1] - values[0]) > 1e-3 * abs(values[0])


KAPPA = 35.0


def _umbrella_run(api, pressure, steps=3):
    context, cv, integrate = api
    pos, L, types = _system(seed=15)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    val = _ref(pos, types, L, lists)["s"]
    kw = _grid(val)
    var = cv.debye_structure_factor(Q, R_CUT, nl, "A", weights=WEIGHTS, sigma=kw["sigma"][0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    cv0 = 0.8 * val
    var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(steps)
    return var, meta, pos, types, L, lists, val, cv0, kw


def test_debye_virial_with_the_pressure_flag_and_without(api):
    """flag set: get_virial() against the restatement at the bias factor the integrator reports plus the umbrella's; flag off: it raises,
    and the force array is the same bit for bit; a stale array reads back as zeros"""
    context, cv, integrate = api
    var, meta, pos, types, L, lists, val, cv0, _ = _umbrella_run(api, True)
    s = meta.cpp_integrator.getCurrentValues()[0]
    total = meta.cpp_integrator.getBiasFactors()[0] + KAPPA * (s - cv0)
    r = _ref(pos, types, L, lists, bias=total)
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
    var = _umbrella_run(api, False)[0]
    with pytest.raises(RuntimeError):
        var.get_virial(per_particle=True)
    assert np.array_equal(var.cpp_force.getForceArray(), F_on)


def test_debye_refuses_a_half_list_and_a_short_list(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    var = cv.debye_structure_factor(Q, R_CUT, nl, "A")
    var.set_grid(0.0, 8.0, 64)
    nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    nl.set_lists(*util.build_nlist(pos, L, R_LIST, half=True))
    with pytest.raises(RuntimeError, match="full neighbour list"):
        context.run(1)
    # the host classes on their own (as a C++ caller would): nine peaks, a weight too few, and a device-built list that stops short of r_cut
    sysdef = context.current.system_definition
    with pytest.raises(RuntimeError, match="wave numbers"):
        _metadynamics.DebyeStructureFactor(sysdef, [1.0] * 9, [1.0] * 9, 2.4, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="one weight per wave number"):
        _metadynamics.DebyeStructureFactor(sysdef, [1.0, 2.0], [1.0], 2.4, nl.cpp_nlist, 0, "")
    short = _metadynamics.NeighborList(sysdef)
    short.setDeviceBuild(2.3, 0.2, 1, 0)
    v = _metadynamics.DebyeStructureFactor(sysdef, [7.7], [1.0], 2.4, short, 0, "_short")
    with pytest.raises(RuntimeError, match="must reach"):
        v.getCurrentValue(0)
