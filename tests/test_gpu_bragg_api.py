"""GPU: cv.bragg through the host classes and the Python API, against the numpy restatement (tests/bragg_ref.py) and the oracle's bias grid
driven with the restatement's values, ten steps each: alone on a 1-d grid, and beside cv.lamellar on a 2-d well-tempered grid.

Bounds.  The value and the forces carry the bounds of tests/test_gpu_bragg.py (value_bound; 1e-5 of max |F|, at the bias factor the
integrator reports).  The bias factor is held against the oracle's engine fed with the RESTATEMENT's values, while the engine under test
saw the kernels' values, which differ by up to d_c = the value bound of variable c (cv.lamellar: 1e-6 |s| + 1e-9, its own).  A bias factor
is -sum_hills W_i (s_c - s_c,i) / sigma_c^2 times Gaussians <= 1: moving the point of evaluation and every hill by d changes it by at most
2 n W / sigma_c * sum_d (d_d / sigma_d) for n hills of height <= W (the slope of x exp(-x^2 / 2) is at most 1); doubled once more for the
well-tempered heights, which depend on the potential at the same shifted points: tol_c = 4 n W / sigma_c * sum_d d_d / sigma_d.

The particles are moved between steps (noise 0.08: the ordered peak loses about 1.5 % per step through its Debye-Waller factor), so that
the hills land at different values and a bias factor is a slope of the grid, not the rounding residue at the top of one hill.  Every run()
begins with the integrator's prepRun, which updates the potential at the step it starts from: cv.bragg has computed that time step already
and hands over its value from before the move, cv.lamellar always recomputes (tests/test_gpu_debye_api.py)."""
import numpy as np
import pytest

import bragg_ref as br
import util
from test_gpu_bragg import condition, value_bound

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
BOX = (11.0, 13.5, 9.25)
HKL = [(0, 0, 3), (1, -1, 0), (2, 1, -1)]
MODE = dict(A=1.0, B=-1.0)
COEFF = [1.0, -1.0]
N = 2049
STEPS = 10


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _system(seed=3):
    """A / B layers along (0, 0, 3), fractional z moved by 0.05 sign(a) sin(2 pi 3 z)"""
    rng = np.random.default_rng(seed)
    f = rng.random((N, 3)) - 0.5
    types = (np.arange(N) % 2).astype(np.int32)
    f[:, 2] += 0.05 * np.where(types == 0, 1.0, -1.0) * np.sin(2 * np.pi * 3 * f[:, 2])
    return f * np.array(BOX), types


def _ref(pos, types, weights=None, modulus=False, bias=1.0, hkl=HKL):
    return br.compute(pos, types, COEFF, hkl, BOX, weights, modulus, bias=bias)


def _moved(pos, rng):
    pos = pos + rng.normal(0, 0.08, pos.shape)
    return pos - np.rint(pos / np.array(BOX)) * np.array(BOX)


def _check_forces(var, r, bias):
    F = var.cpp_force.getForceArray().astype(np.float64)
    F_ref = -bias * r["dsdr"]
    top = np.abs(F_ref).max()
    err = np.abs(F[:, :3] - F_ref).max()
    print("    forces: max |d| %.3e of max |F| %.3e (%.3e rel)" % (err, top, err / top if top else 0.0))
    assert err <= 1e-5 * top and np.all(F[:, 3] == 0.0)
    return F


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bragg_alone_on_a_grid(api, ref, dtype):
    context, cv, integrate = api
    pos, types = _system()
    pos = pos.astype(dtype).astype(np.float64)
    context.initialize(pos, types, ["A", "B"], BOX, dtype=dtype)
    meta = integrate.mode_metadynamics(**KW)
    r = _ref(pos, types)
    val = r["s"]
    assert val > 0.01
    kw = dict(sigma=[0.02 * val], cv_min=[0.4 * val], cv_max=[1.6 * val], num_points=[512])
    var = cv.bragg(MODE, HKL, sigma=kw["sigma"][0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    assert meta is not None and var.weights == [1.0 / 3.0] * 3 and var.modulus is False
    oracle = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    rng = np.random.default_rng(8)
    seen, previous = [], val
    for step in range(1, STEPS + 1):
        if step > 1:
            pos = _moved(pos, rng).astype(dtype).astype(np.float64)
            context.set_positions(pos, types)
            r = _ref(pos, types)
        context.run(1)
        assert context.current.system.getCurrentTimeStep() == step
        s = meta.cpp_integrator.getCurrentValues()[0]
        b = meta.cpp_integrator.getBiasFactors()[0]
        oracle.update_bias(step - 1, [previous])
        b_ref = oracle.update_bias(step, [r["s"]])[0]
        previous = r["s"]
        d = value_bound(r, N, False)
        tol_b = 4 * 2 * step * KW["W"] / kw["sigma"][0] * d / kw["sigma"][0]
        print("step %d: s %.9g vs %.9g (|d| %.3e of bound %.3e); bias factor %.6e vs oracle %.6e (|d| %.3e of bound %.3e)"
              % (step, s, r["s"], abs(s - r["s"]), d, b, b_ref, abs(b - b_ref), tol_b))
        assert abs(s - r["s"]) <= d
        assert abs(b - b_ref) <= tol_b
        if step > 1:
            assert abs(b) > 10 * tol_b                                   # a slope of the deposited hills, well above what the bound lets pass
        _check_forces(var, r, b)
        seen.append(b)
    assert len(set(seen)) == STEPS
    assert meta.cpp_integrator.lastStepRoute().startswith("generic")     # the general route: no launch shared with the lamellar kernels
    # the getters and the log
    t = context.current.system.getCurrentTimeStep()
    assert abs(var.cpp_force.getCurrentValue(t) - r["s"]) <= d
    assert var.cpp_force.getLogValue("cv_bragg", t) == var.cpp_force.getCurrentValue(t)
    assert "cv_bragg" in var.cpp_force.getProvidedLogQuantities() and "umbrella_energy_cv_bragg" in var.cpp_force.getProvidedLogQuantities()
    S, rho = var.get_structure_factors(), var.get_amplitudes()
    m = np.sqrt((r["rho"] ** 2).sum(axis=1))
    assert S.shape == (3,) and rho.shape == (3, 2)
    assert np.sqrt(((rho - r["rho"]) ** 2).sum(axis=1)).max() <= 1e-6 * max(m.max(), np.sqrt(N))
    assert np.abs(S - r["S"]).max() <= 2e-6 * m.max() * max(m.max(), np.sqrt(N)) / r["A2"]
    assert S[0] > 20 * S[1:].max()
    named = cv.bragg(MODE, [(0, 0, 3)], name="z", modulus=True)
    assert "cv_bragg_z" in named.cpp_force.getProvidedLogQuantities() and named.cpp_force.getModulus() and named.weights == [1.0]


def test_bragg_with_lamellar_on_a_2d_grid(api, ref):
    """the modulus form beside cv.lamellar with the same vectors: the lamellar variable keeps its shared launches (its sums in launch A,
    its forces in the engine's launch), the new one takes the general route, and both bias factors are the oracle's"""
    context, cv, integrate = api
    pos, types = _system(seed=4)
    context.initialize(pos, types, ["A", "B"], BOX, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    rbox = ref.Box.make(BOX)
    r = _ref(pos, types, modulus=True)
    lam_ref = ref.lamellar_cv(HKL, util.oracle_postype(pos, types), COEFF, rbox)
    val = r["s"]
    sig = [0.02 * val, 0.01]
    kw = dict(sigma=sig, cv_min=[0.4 * val, -1.0], cv_max=[1.6 * val, 1.0], num_points=[128, 256])
    var = cv.bragg(MODE, HKL, modulus=True, sigma=sig[0])
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 128)
    lam = cv.lamellar(sigma=sig[1], mode=MODE, lattice_vectors=HKL)
    lam.set_grid(cv_min=-1.0, cv_max=1.0, num_points=256)
    oracle = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    rng = np.random.default_rng(9)
    previous = val
    for step in range(1, STEPS + 1):
        if step > 1:
            pos = _moved(pos, rng)
            context.set_positions(pos, types)
            r = _ref(pos, types, modulus=True)
        condition(r, True)                                               # (force parity in the modulus form: tests/test_gpu_bragg.py)
        opt = util.oracle_postype(pos, types)
        lam_ref = ref.lamellar_cv(HKL, opt, COEFF, rbox)
        context.run(1)
        s = meta.cpp_integrator.getCurrentValues()
        b = meta.cpp_integrator.getBiasFactors()
        oracle.update_bias(step - 1, [previous, lam_ref])
        b_ref = oracle.update_bias(step, [r["s"], lam_ref])
        previous = r["s"]
        d = [value_bound(r, N, True), 1e-6 * abs(lam_ref) + 1e-9]
        tol_b = [4 * 2 * step * KW["W"] / sig[c] * (d[0] / sig[0] + d[1] / sig[1]) for c in range(2)]
        print("step %d: s %s vs (%.9g, %.9g), bounds %s; bias factors %s vs oracle %s, bounds %s" % (step, list(s), r["s"], lam_ref, d, list(b),
                                                                                                 list(b_ref), tol_b))
        assert abs(s[0] - r["s"]) <= d[0] and abs(s[1] - lam_ref) <= d[1]
        assert abs(b[0] - b_ref[0]) <= tol_b[0] and abs(b[1] - b_ref[1]) <= tol_b[1]
        _check_forces(var, r, b[0])
        Fl = lam.cpp_force.getForceArray()
        Fl_ref = ref.lamellar_forces(HKL, opt, COEFF, rbox, b[1])
        assert np.abs(Fl[:, :3] - Fl_ref[:, :3]).max() <= 1e-5 * np.abs(Fl_ref[:, :3]).max()
    assert abs(b[0]) > 10 * tol_b[0] and abs(b[1]) > 10 * tol_b[1]
    route = meta.cpp_integrator.lastStepRoute()
    print("route:", route)
    assert route.startswith("generic") and "launch_a" in route and "lamellar_slots" in route


def test_lamellar_is_the_same_with_and_without_bragg_beside_it(api, ref):
    """cv.lamellar alone (the fused step) and beside cv.bragg (launch A and the engine's launch of a mixed set) on the same snapshot:
    the same value within the engine's bound for it (1e-6 relative), the same force per unit of bias factor to 1e-5 of its maximum"""
    context, cv, integrate = api
    pos, types = _system(seed=5)
    out = []
    for with_bragg in (False, True):
        context.initialize(pos, types, ["A", "B"], BOX, dtype=np.float32)
        meta = integrate.mode_metadynamics(**KW)
        if with_bragg:
            var = cv.bragg(MODE, HKL, sigma=0.002)
            var.set_grid(0.0, 0.2, 64)
        lam = cv.lamellar(sigma=0.01, mode=MODE, lattice_vectors=HKL)
        lam.set_grid(cv_min=-1.0, cv_max=1.0, num_points=256)
        context.run(1)
        context.set_positions(_moved(pos, np.random.default_rng(6)), types)
        context.run(2)
        c = 1 if with_bragg else 0
        out.append((meta.cpp_integrator.getCurrentValues()[c], meta.cpp_integrator.getBiasFactors()[c],
                    lam.cpp_force.getForceArray().astype(np.float64), meta.cpp_integrator.lastStepRoute()))
        context.current = None
    (s0, b0, F0, route0), (s1, b1, F1, route1) = out
    print("alone: s %.9g, bias %.6e, %s; beside cv.bragg: s %.9g, bias %.6e, %s" % (s0, b0, route0, s1, b1, route1))
    assert route0.startswith("fused") and route1.startswith("generic")
    assert abs(s1 - s0) <= 1e-6 * abs(s0) and abs(b0) > 1e-3 and abs(b1) > 1e-3
    assert np.abs(F1[:, :3] / b1 - F0[:, :3] / b0).max() <= 1e-5 * np.abs(F0[:, :3] / b0).max()


KAPPA = 35.0


@pytest.mark.parametrize("modulus", [False, True])
def test_harmonic_umbrella(api, modulus):
    """forces = -(metadynamics bias factor + kappa (s - cv0)) x the gradient, through the base class; computeDerivatives gives the bare
    gradient"""
    context, cv, integrate = api
    pos, types = _system(seed=7)
    context.initialize(pos, types, ["A", "B"], BOX, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    r = _ref(pos, types, modulus=modulus)
    condition(r, modulus)
    val = r["s"]
    var = cv.bragg(MODE, HKL, modulus=modulus, sigma=0.02 * val)
    var.set_grid(0.4 * val, 1.6 * val, 256)
    cv0 = 0.8 * val
    var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(3)
    s = meta.cpp_integrator.getCurrentValues()[0]
    b = meta.cpp_integrator.getBiasFactors()[0]
    total = b + KAPPA * (s - cv0)
    print("s %.9g, bias factor %.6e, umbrella part %.6e" % (s, b, KAPPA * (s - cv0)))
    assert abs(KAPPA * (s - cv0)) > 1e-3
    _check_forces(var, r, total)
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getLogValue("umbrella_energy_cv_bragg", t) == pytest.approx(0.5 * KAPPA * (s - cv0) ** 2, rel=1e-9)
    var.cpp_force.computeDerivatives(t)
    _check_forces(var, r, 1.0)


def test_set_weights_and_trig_mode_take_effect_between_runs(api):
    context, cv, integrate = api
    pos, types = _system(seed=8)
    context.initialize(pos, types, ["A", "B"], BOX, dtype=np.float32)
    pos = pos.astype(np.float32).astype(np.float64)
    meta = integrate.mode_metadynamics(**KW)
    var = cv.bragg(MODE, HKL, sigma=0.05)
    var.set_grid(0.0, 0.5, 128)
    context.run(1)
    r = _ref(pos, types)
    s0 = meta.cpp_integrator.getCurrentValues()[0]
    assert abs(s0 - r["s"]) <= value_bound(r, N, False)
    w = [0.1, 2.0, 0.5]
    var.set_weights(w)
    assert var.weights == w and list(var.cpp_force.getWeights()) == w
    context.run(1)
    r = _ref(pos, types, weights=w)
    s1 = meta.cpp_integrator.getCurrentValues()[0]
    print("weights 1/3 each: s %.9g; %s: s %.9g vs %.9g" % (s0, w, s1, r["s"]))
    assert abs(s1 - r["s"]) <= value_bound(r, N, False) and abs(s1 - s0) > 100 * value_bound(r, N, False)
    _check_forces(var, r, meta.cpp_integrator.getBiasFactors()[0])
    var.set_weights(None)
    t = context.current.system.getCurrentTimeStep()
    assert var.cpp_force.getCurrentValue(t) == s0                        # the cached step was formed anew, with the same bits as before
    for mode, code in (("hardware", 1), ("accurate", 2), ("default", 0)):
        var.set_trig_mode(mode)
        assert var.cpp_force.getTrigMode() == code
        assert abs(var.cpp_force.getCurrentValue(t) - s0) <= 2 * value_bound(r, N, False)
    for bad in ([1.0], [1.0, 2.0, float("nan")], [1.0, 2.0, float("inf")], "abc", [1.0] * 4):
        with pytest.raises(RuntimeError, match="Error setting parameters of collective variable."):
            var.set_weights(bad)
    with pytest.raises(RuntimeError, match="Error setting parameters of collective variable."):
        var.set_trig_mode("fast")
    assert var.weights == [1.0 / 3.0] * 3


def test_constructor_refusals_follow_lamellar_and_leave_nothing_behind(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, types = _system()
    context.initialize(pos, types, ["A", "B"], BOX, dtype=np.float32)
    integrate.mode_metadynamics(**KW)
    ok = dict(mode=MODE, lattice_vectors=HKL)
    cv.bragg(**ok)
    n_forces = len(context.current.forces)
    nan = float("nan")
    for bad in (dict(lattice_vectors=[]), dict(lattice_vectors=[(0, 0, 1)] * 17), dict(lattice_vectors=[(0, 0)]), dict(mode=[1.0, -1.0]),
                dict(mode=dict(A=1.0)), dict(mode=dict(A=1.0, B=nan)), dict(weights=[1.0]), dict(weights=[1.0, 2.0, nan]), dict(weights=[1.0] * 4),
                dict(weights="abc")):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.bragg(**{**ok, **bad})
        assert len(context.current.forces) == n_forces, bad
    # the host class on its own, as a C++ caller would use it
    sysdef = context.current.system_definition
    vec = _metadynamics.std_vector_int3()
    vec.append(_metadynamics.make_int3(0, 0, 3))
    with pytest.raises(RuntimeError, match="Number of mode parameters"):
        _metadynamics.BraggIntensity(sysdef, [1.0], vec, [1.0], False, "")
    with pytest.raises(RuntimeError, match="one weight per lattice vector"):
        _metadynamics.BraggIntensity(sysdef, [1.0, -1.0], vec, [1.0, 2.0], False, "")
    with pytest.raises(RuntimeError, match="lattice vectors are supported"):
        _metadynamics.BraggIntensity(sysdef, [1.0, -1.0], _metadynamics.std_vector_int3(), [], False, "")
    v = _metadynamics.BraggIntensity(sysdef, [1.0, -1.0], vec, [1.0], True, "_x")
    with pytest.raises(RuntimeError, match="trig mode"):
        v.setTrigMode(3)
    assert v.getCurrentValue(0) > 0.1                                    # the modulus form on the ordered snapshot
