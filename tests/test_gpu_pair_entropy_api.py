"""GPU: cv.pair_entropy through the host classes and the Python API, against the numpy restatement (tests/pair_entropy_ref.py) and the
oracle's bias grid driven with the restatement's value: the value the engine used and the bias factor to rtol 1e-7, force arrays to 1e-7
of max|F| (the bias factor is the integrator's own), virials to 1e-9 at the bias factor the integrator reports."""
import numpy as np
import pytest

import pair_entropy_ref as pe
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

PAR = dict(r_max=2.0, sigma_r=0.1, n_bins=40)
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
    return pe.compute(pos, types, L, lists, PAR["r_max"], PAR["sigma_r"], PAR["n_bins"], type_id, bias=bias)


def _grid(val):
    """S is negative: the grid runs from 1.3 S up to 0.55 S"""
    return dict(sigma=[0.02 * abs(val)], cv_min=[1.3 * val], cv_max=[0.55 * val], num_points=[512])


def _oracle_bias(ref, kw, values, steps):
    g = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    return [g.update_bias(t, values) for t in range(steps + 1)]


def test_pair_entropy_alone_on_a_grid(api, ref):
    """512-point well-tempered grid, 6 steps, stride 1: value, bias factor, force array and g(r)"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
    val = r["S"]
    kw = _grid(val)
    s2 = cv.pair_entropy(nlist=nl, type="A", sigma=kw["sigma"][0], **PAR)
    s2.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    assert s2.get_rcut() == {("A", "A"): pytest.approx(2.4)}
    context.run(6)
    t = context.current.system.getCurrentTimeStep()
    assert t == 6
    assert s2.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-9)
    assert s2.cpp_force.getLogValue("cv_pair_entropy", t) == pytest.approx(val, rel=1e-9)
    assert "cv_pair_entropy" in s2.cpp_force.getProvidedLogQuantities()
    assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(val, rel=1e-9)
    b = _oracle_bias(ref, kw, [val], 6)[-1]
    assert abs(b[0]) > 0
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    F = s2.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert np.all(F[:, 3] == 0.0)
    r_b, g = s2.get_gr()
    assert np.array_equal(r_b, r["r_b"]) and g.shape == (40,)
    assert np.abs(g - r["g"]).max() <= 1e-10 * r["g"].max()
    named = cv.pair_entropy(nlist=nl, type="A", name="liq", **PAR)
    assert "cv_pair_entropy_liq" in named.cpp_force.getProvidedLogQuantities()
    n_forces = len(context.current.forces)
    for bad in (dict(type="Z"), dict(n_bins=0), dict(n_bins=257), dict(n_bins=12.5), dict(r_max=0.0), dict(sigma_r=-0.1), dict(r_max=float("nan")),
                dict(sigma_r=0.2)):                                     # r_max + 4 sigma_r = 2.8 is beyond the list's 2.45
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.pair_entropy(**{**dict(nlist=nl, type="A"), **PAR, **bad})
    assert len(context.current.forces) == n_forces                      # a refused variable leaves nothing behind


def test_pair_entropy_with_lamellar_on_a_2d_grid(api, ref):
    context, cv, integrate = api
    pos, L, _ = _system(seed=13)
    types = (np.random.default_rng(4).random(len(pos)) < 0.5).astype(np.int32)
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    lists = nl.update()
    r = _ref(pos, types, L, lists)
    val = r["S"]
    rbox = ref.Box.make(L)
    opt = util.oracle_postype(pos, types)
    vec = [(0, 0, 2)]
    k1 = _grid(val)
    s2 = cv.pair_entropy(nlist=nl, type="A", sigma=k1["sigma"][0], **PAR)
    s2.set_grid(k1["cv_min"][0], k1["cv_max"][0], 64)
    lam = cv.lamellar(sigma=0.05, mode=dict(A=1.0, B=-1.0), lattice_vectors=vec)
    lam.set_grid(cv_min=-1.0, cv_max=1.0, num_points=64)
    context.run(6)
    cvg = meta.cpp_integrator.getCurrentValues()
    assert cvg[0] == pytest.approx(val, rel=1e-9)
    assert cvg[1] == pytest.approx(ref.lamellar_cv(vec, opt, util.MODE_AB, rbox), rel=1e-6, abs=1e-9)
    kw = dict(sigma=[k1["sigma"][0], 0.05], cv_min=[k1["cv_min"][0], -1.0], cv_max=[k1["cv_max"][0], 1.0], num_points=[64, 64])
    b = _oracle_bias(ref, kw, [val, cvg[1]], 6)[-1]
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    F = s2.cpp_force.getForceArray()
    F_ref = -b[0] * r["grad"]
    assert np.abs(F_ref).max() > 0
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert np.all(F[types == 1] == 0.0)
    Fl = lam.cpp_force.getForceArray()
    Fl_ref = ref.lamellar_forces(vec, opt, util.MODE_AB, rbox, b[1])
    assert np.abs(Fl[:, :3] - Fl_ref[:, :3]).max() <= 1e-5 * np.abs(Fl_ref[:, :3]).max()


def test_pair_entropy_device_list_follows_the_particles(api, ref):
    """cv.nlist_cell(device=True): particles displaced between runs by more than r_buff / 2 — the list rebuilds and the value follows"""
    context, cv, integrate = api
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST, r_buff=0.4, device=True)
    val0 = _ref(pos, types, L, util.build_nlist(pos, L, R_LIST))["S"]
    s2 = cv.pair_entropy(nlist=nl, type="A", sigma=0.02 * abs(val0), **PAR)
    s2.set_grid(1.3 * val0, 0.02 * val0, 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    assert s2.cpp_force.getCurrentValue(t) == pytest.approx(val0, rel=1e-9)
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
        values.append(r["S"])
        assert s2.cpp_force.getCurrentValue(t) == pytest.approx(r["S"], rel=1e-9)
        assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(r["S"], rel=1e-9)
        assert nl.cpp_nlist.getNumRebuilds() == 2 + k
        b = meta.cpp_integrator.getBiasFactors()[0]
        F = s2.cpp_force.getForceArray()
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
    val = _ref(pos, types, L, lists)["S"]
    kw = _grid(val)
    s2 = cv.pair_entropy(nlist=nl, type="A", sigma=kw["sigma"][0], **PAR)
    s2.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    cv0 = 0.8 * val
    s2.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(steps)
    return s2, meta, pos, types, L, lists, val, cv0, kw


def test_pair_entropy_harmonic_umbrella_adds_to_the_bias_factor(api, ref):
    context, cv, integrate = api
    s2, meta, pos, types, L, lists, val, cv0, kw = _umbrella_run(api, False)
    t = context.current.system.getCurrentTimeStep()
    b = _oracle_bias(ref, kw, [val], 3)[-1]
    assert np.allclose(meta.cpp_integrator.getBiasFactors(), b, rtol=1e-7)
    total = b[0] + KAPPA * (val - cv0)
    assert abs(KAPPA * (val - cv0)) > 0.1 * abs(total)
    F = s2.cpp_force.getForceArray()
    F_ref = -total * _ref(pos, types, L, lists)["grad"]
    assert np.abs(F[:, :3] - F_ref).max() <= 1e-7 * np.abs(F_ref).max()
    assert s2.cpp_force.getUmbrellaPotential(t) == pytest.approx(0.5 * KAPPA * (val - cv0) ** 2, rel=1e-8)


def test_pair_entropy_virial_with_the_pressure_flag_and_without(api):
    """flag set: get_virial() against the restatement at the bias factor the integrator reports plus the umbrella's; flag off: it raises, and
    the force array is the same bit for bit; a stale array reads back as zeros"""
    context, cv, integrate = api
    s2, meta, pos, types, L, lists, val, cv0, _ = _umbrella_run(api, True)
    s = meta.cpp_integrator.getCurrentValues()[0]
    total = meta.cpp_integrator.getBiasFactors()[0] + KAPPA * (s - cv0)
    r = _ref(pos, types, L, lists, bias=total)
    N = len(pos)
    per, raw, W = s2.get_virial(per_particle=True), s2.cpp_force.getVirial(), s2.get_virial()
    assert per.shape == (6, N) and per.dtype == np.float64 and W.shape == (6,)
    assert np.array_equal(raw[:, :N], per)
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["virial_sum"]).max(), w_top))
    assert w_top > 0.05
    assert np.abs(per.T - r["virial"]).max() <= 1e-9 * top
    assert np.abs(W - r["virial_sum"]).max() <= 1e-9 * w_top
    F_on = s2.cpp_force.getForceArray().copy()
    assert np.abs(F_on[:, :3] + total * r["grad"]).max() <= 1e-9 * np.abs(total * r["grad"]).max()
    context.current.system_definition.getParticleData().setPressureFlag(False)
    context.run(1)
    assert np.all(s2.cpp_force.getVirial() == 0.0)
    with pytest.raises(RuntimeError):
        s2.get_virial()
    context.current = None
    s2 = _umbrella_run(api, False)[0]
    with pytest.raises(RuntimeError):
        s2.get_virial(per_particle=True)
    assert np.array_equal(s2.cpp_force.getForceArray(), F_on)


def test_pair_entropy_refuses_a_half_list_and_a_short_list(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L, types = _system()
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=R_LIST)
    s2 = cv.pair_entropy(nlist=nl, type="A", **PAR)
    s2.set_grid(-4.0, 0.0, 64)
    nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
    nl.set_lists(*util.build_nlist(pos, L, R_LIST, half=True))
    with pytest.raises(RuntimeError, match="full neighbour list"):
        context.run(1)
    # the host classes on their own (as a C++ caller would): n_bins = 257, and a device-built list that stops short of r_max + 4 sigma_r
    sysdef = context.current.system_definition
    with pytest.raises(RuntimeError, match="n_bins"):
        _metadynamics.PairEntropy(sysdef, 2.0, 0.1, 257, nl.cpp_nlist, 0, "")
    short = _metadynamics.NeighborList(sysdef)
    short.setDeviceBuild(2.3, 0.2, 1, 0)
    var = _metadynamics.PairEntropy(sysdef, 2.0, 0.1, 40, short, 0, "_short")
    with pytest.raises(RuntimeError, match="must reach"):
        var.getCurrentValue(0)
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        cv.pair_entropy(nlist=cv.nlist_cell(r_cut=2.3), type="A", **PAR)
