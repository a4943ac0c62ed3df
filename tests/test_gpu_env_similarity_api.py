"""GPU: cv.environment_similarity through the host classes and the Python API against the numpy restatement
(tests/env_similarity_ref.py), with the bias factor the engine applied: the value to 1e-9 relative, k_i, k^e_i and v_i to 1e-10 of their
maximum, force arrays and virials to 1e-9 (fp64 arrays)."""
import numpy as np
import pytest

import env_similarity_ref as es
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIGMA_ENV, R_ON, R_CUT = 0.12, 1.3, 1.5
R_LIST = 1.55
SWITCH = dict(c0=0.5, p=6)
KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
KAPPA = 35.0


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _system(seed=12, noise=0.05):
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(seed).normal(0, noise, pos.shape)
    return pos, L, np.zeros(len(pos), dtype=np.int32)


def _rot_z(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _ref(pos, types, L, lists, templates, bias=1.0, lam=100.0, sw=None):
    return es.compute(pos, types, L, lists, templates, SIGMA_ENV, R_ON, R_CUT, 0, lam=lam, sw=None if sw is None else (sw["c0"], sw["p"]), bias=bias)


def _check(var, meta, r_of_bias, t, E):
    """value, per-particle arrays and the force array against the restatement at the bias factor the engine applied"""
    b = meta.cpp_integrator.getBiasFactors()[0]
    r = r_of_bias(b)
    assert abs(b) > 0
    val = var.cpp_force.getCurrentValue(t)
    print("value %.15g vs %.15g, bias factor %.6g" % (val, r["s"], b))
    assert val == pytest.approx(r["s"], rel=1e-9)
    assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["s"], rel=1e-9)
    k, ke, v = var.get_local(), var.get_environments(), var.get_switched()
    assert k.shape == (len(r["k"]),) and ke.shape == (len(r["k"]), E) and v.shape == k.shape
    for got, want in ((k, r["k"]), (ke, r["ke"]), (v, r["v"])):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    F = var.cpp_force.getForceArray()
    F_ref = -b * r["grad"]
    print("forces: %.3e of max |F| %.3e" % (np.abs(F[:, :3] - F_ref).max(), np.abs(F_ref).max()))
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-9 * np.abs(F_ref).max()
    assert np.all(F[:, 3] == 0.0)
    return r


@pytest.mark.parametrize("device_list", [False, True])
def test_environment_similarity_alone_on_a_grid(api, device_list):
    """512-point well-tempered grid, stride 1; a switch set mid-run takes effect with the next step"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST, r_buff=0.2, device=device_list)
    lists = util.build_nlist(pos, L, R_LIST)
    if not device_list:
        nl.update()
    T = cv.environment_templates("fcc", np.sqrt(2.0))
    var = cv.environment_similarity(T, SIGMA_ENV, R_CUT, R_ON, nl, "A", sigma=0.02)
    var.set_grid(0.0, 1.0, 512)
    assert var.get_rcut() == {("A", "A"): pytest.approx(R_CUT)}
    context.run(4)
    t = context.current.system.getCurrentTimeStep()
    r = _check(var, meta, lambda b: _ref(pos, types, L, lists, T, bias=b), t, 1)
    assert r["s"] == pytest.approx(0.78, abs=0.02)
    assert var.cpp_force.getLogValue("cv_environment_similarity", t) == pytest.approx(r["s"], rel=1e-9)
    assert "cv_environment_similarity" in var.cpp_force.getProvidedLogQuantities()
    with pytest.raises(RuntimeError):
        var.get_virial()                                                # no pressure flag
    var.set_switch(SWITCH)
    context.run(1)
    t = context.current.system.getCurrentTimeStep()
    rs = _check(var, meta, lambda b: _ref(pos, types, L, lists, T, bias=b, sw=SWITCH), t, 1)
    assert abs(rs["s"] - r["s"]) > 0.05
    var.set_switch(None)
    context.run(1)
    _check(var, meta, lambda b: _ref(pos, types, L, lists, T, bias=b), context.current.system.getCurrentTimeStep(), 1)
    named = cv.environment_similarity(T, SIGMA_ENV, R_CUT, R_ON, nl, "A", name="fcc")
    assert "cv_environment_similarity_fcc" in named.cpp_force.getProvidedLogQuantities()
    n_forces = len(context.current.forces)
    for bad in (dict(type="Z"), dict(templates=[]), dict(templates=T[:11] + [[2.0, 0.0, 0.0]]), dict(r_cut=1.6, r_on=1.4),
                dict(switch=dict(c0=0.0, p=6))):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.environment_similarity(**{**dict(templates=T, sigma_env=SIGMA_ENV, r_cut=R_CUT, r_on=R_ON, nlist=nl, type="A"), **bad})
    assert len(context.current.forces) == n_forces                      # a refused variable leaves nothing behind


def test_environment_similarity_two_environments_with_a_switch(api):
    """fcc and the same template turned by 5 degrees, lambda 20 (unsaturated weights), switch: the general beta table through the API"""
    context, cv, integrate = api
    pos, L, types = _system(seed=13)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    fcc = np.array(cv.environment_templates("fcc", np.sqrt(2.0)))
    T = [fcc.tolist(), (fcc @ _rot_z(5.0).T).tolist()]
    var = cv.environment_similarity(T, SIGMA_ENV, R_CUT, R_ON, nl, "A", lam=20.0, switch=SWITCH, sigma=0.02)
    var.set_grid(0.0, 1.2, 512)
    context.run(3)
    _check(var, meta, lambda b: _ref(pos, types, L, lists, T, bias=b, lam=20.0, sw=SWITCH), context.current.system.getCurrentTimeStep(), 2)


def _umbrella_run(api, pressure, steps=3):
    context, cv, integrate = api
    pos, L, types = _system(seed=15)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    T = cv.environment_templates("fcc", np.sqrt(2.0))
    var = cv.environment_similarity(T, SIGMA_ENV, R_CUT, R_ON, nl, "A", switch=SWITCH, sigma=0.02)
    var.set_grid(0.0, 1.2, 512)
    cv0 = 0.6
    var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(steps)
    return var, meta, pos, types, L, lists, T, cv0


def test_environment_similarity_virial_with_the_pressure_flag_and_without(api):
    """flag set: get_virial() against the restatement at the bias factor the integrator reports plus the umbrella's; flag off: it raises, the
    force array is the same bit for bit, and a stale array reads back as zeros"""
    context, cv, integrate = api
    var, meta, pos, types, L, lists, T, cv0 = _umbrella_run(api, True)
    s = meta.cpp_integrator.getCurrentValues()[0]
    total = meta.cpp_integrator.getBiasFactors()[0] + KAPPA * (s - cv0)
    r = _ref(pos, types, L, lists, T, bias=total, sw=SWITCH)
    N = len(pos)
    per, raw, W = var.get_virial(per_particle=True), var.cpp_force.getVirial(), var.get_virial()
    assert per.shape == (6, N) and per.dtype == np.float64 and W.shape == (6,)
    assert np.array_equal(raw[:, :N], per)
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["virial_sum"]).max(), w_top))
    assert w_top > 0.01
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


def test_environment_similarity_with_lamellar_on_a_2d_grid(api, ref):
    """two variables on a 2-d grid: the value reaches the engine as a device-resident source (enqueueCurrentValue: block sums of v_i, no
    read-back in the step); values, bias factor and force array against the restatement.  The second variable is cv.lamellar:
    cv.potential_energy can only be the single variable of a run (the integrator's rule, IntegratorMetaDynamics::update), so the pairing
    of tests/test_gpu_pair_entropy_api.py is used"""
    context, cv, integrate = api
    pos, L, _ = _system(seed=14)
    types = (np.random.default_rng(4).random(len(pos)) < 0.5).astype(np.int32)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    T = cv.environment_templates("fcc", np.sqrt(2.0))
    var = cv.environment_similarity(T, SIGMA_ENV, R_CUT, R_ON, nl, "A", sigma=0.02)
    var.set_grid(0.0, 1.0, 64)
    vec = [(0, 0, 2)]
    lam = cv.lamellar(sigma=0.05, mode=dict(A=1.0, B=-1.0), lattice_vectors=vec)
    lam.set_grid(cv_min=-1.0, cv_max=1.0, num_points=64)
    context.run(4)
    cvg = meta.cpp_integrator.getCurrentValues()
    r = _ref(pos, types, L, lists, T)
    assert 0.0 < r["s"] < 1.0 and cvg[0] == pytest.approx(r["s"], rel=1e-9)
    assert cvg[1] == pytest.approx(ref.lamellar_cv(vec, util.oracle_postype(pos, types), util.MODE_AB, ref.Box.make(L)), rel=1e-6, abs=1e-9)
    b = meta.cpp_integrator.getBiasFactors()
    F = var.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert abs(b[0]) > 0 and np.abs(F[:, :3] - F_ref).max() <= 1e-9 * np.abs(F_ref).max()
    assert np.all(F[types == 1] == 0.0)


def test_environment_similarity_refuses_a_half_list_and_a_short_list(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    T = cv.environment_templates("fcc", np.sqrt(2.0))
    var = cv.environment_similarity(T, SIGMA_ENV, R_CUT, R_ON, nl, "A")
    var.set_grid(0.0, 1.0, 64)
    nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    nl.set_lists(*util.build_nlist(pos, L, R_LIST, half=True))
    with pytest.raises(RuntimeError, match="full neighbour list"):
        context.run(1)
    # the host classes on their own (as a C++ caller would): too many environments, and a device-built list that stops short of r_cut
    sysdef = context.current.system_definition
    with pytest.raises(RuntimeError, match="environments"):
        _metadynamics.EnvironmentSimilarity(sysdef, [T] * 5, SIGMA_ENV, R_CUT, R_ON, 100.0, nl.cpp_nlist, 0, "")
    with pytest.raises(RuntimeError, match="r_cut"):
        _metadynamics.EnvironmentSimilarity(sysdef, [T[:11] + [[1.5, 0.0, 0.0]]], SIGMA_ENV, R_CUT, R_ON, 100.0, nl.cpp_nlist, 0, "")
    short = _metadynamics.NeighborList(sysdef)
    short.setDeviceBuild(1.4, 0.0, 1, 0)
    v2 = _metadynamics.EnvironmentSimilarity(sysdef, [T], SIGMA_ENV, R_CUT, R_ON, 100.0, short, 0, "_short")
    with pytest.raises(RuntimeError, match="must reach"):
        v2.getCurrentValue(0)
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.environment_similarity(T, SIGMA_ENV, R_CUT, R_ON, cv.nlist_cell(r_cut=1.4), "A")
