"""GPU: cv.probe_volume through the host class and the Python API, against the restatement (tests/probe_volume_ref.py) and the oracle's
bias grid driven with the restatement's values, ten steps: value, bias factor (the hills) and bias force at every step; then the setters
between runs, the getters, the virial with and without the pressure flag, a box change, and the constructor's refusals.

Bounds.  Value and forces carry the bounds of tests/test_gpu_probe_volume.py (1e-12 sum_{h > 0} |a_i|; 1e-12 |bias| max|a| Phi(0) plus the
storage rounding of fp32 arrays).  The bias factor is held against the oracle's engine fed with the RESTATEMENT's values, while the engine
under test saw the kernels' values, which differ by up to d = the value bound: as in tests/test_gpu_bragg_api.py, moving the point of
evaluation and every hill by d changes a bias factor by at most tol = 4 n W / sigma * d / sigma for n hills of height <= W, plus the
engine's own fp64 rounding of a sum of n terms of size <= W / sigma, 1e-13 n W / sigma.

The particles are moved between steps, so that the hills land at different values and a bias factor is a slope of the grid."""
import numpy as np
import pytest

import probe_volume_ref as pv
from test_gpu_probe_volume import storage

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

INF = float("inf")
KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
BOX = (16.0, 18.5, 15.0)
WEIGHTS = dict(A=1.0, B=-0.5, C=0.0)
COEFF = [1.0, -0.5, 0.0]
CENTRE = [0.4, -0.3, 6.9]                                                    # the slab reaches through the periodic boundary in z
N = 2049
STEPS = 10
REGIONS = {
    "slab": (dict(shape="box", half_widths=[INF, INF, 1.5]), pv.region("box", CENTRE, 0.3, w=[INF, INF, 1.5])),
    "sphere": (dict(shape="sphere", radius=4.0), pv.region("sphere", CENTRE, 0.3, R=4.0)),
    "cylinder": (dict(shape="cylinder", radius=3.0, axis="y", half_length=4.0), pv.region("cylinder", CENTRE, 0.3, R=3.0, w=4.0, axis=1)),
    "box": (dict(shape="box", half_widths=[3.0, 4.0, 2.0]), pv.region("box", CENTRE, 0.3, w=[3.0, 4.0, 2.0])),
}


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _system(seed=3):
    rng = np.random.default_rng(seed)
    pos = (rng.random((N, 3)) - 0.5) * np.array(BOX)
    return pos, rng.integers(0, 3, N).astype(np.int32)


def _moved(pos, rng, box=BOX):
    pos = pos + rng.normal(0, 0.08, pos.shape)
    return pos - np.rint(pos / np.array(box)) * np.array(box)


def _ref(pos, types, reg, bias=1.0, box=BOX, coeff=COEFF):
    return pv.compute(pos, types, coeff, reg, box, None, bias=bias)


def _value_bound(r):
    return 1e-12 * np.abs(r["a"][r["h"] > 0]).sum()


def _check_forces(var, r, reg, bias, dtype):
    """r: the restatement at bias 1 (F = -a grad h)"""
    F = var.cpp_force.getForceArray().astype(np.float64)
    F_ref = bias * r["F"]
    tol = 1e-12 * abs(bias) * max(np.abs(COEFF)) * pv.phi(0.0, reg["sigma_s"], reg["r_c"]) + storage(F_ref, dtype)
    frac = (np.abs(F[:, :3] - F_ref) / tol).max()
    print("    forces: worst fraction of the bound %.3g, max |F| %.3e" % (frac, np.abs(F_ref).max()))
    assert frac <= 1.0 and np.all(F[:, 3] == 0.0) and np.abs(F_ref).max() > 0
    return F


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["slab", "sphere"])
def test_probe_volume_alone_on_a_grid(api, ref, name, dtype):
    context, cv, integrate = api
    kwargs, reg = REGIONS[name]
    pos, types = _system()
    pos = pos.astype(dtype).astype(np.float64)
    context.initialize(pos, types, ["A", "B", "C"], BOX, dtype=dtype)
    meta = integrate.mode_metadynamics(**KW)
    r = _ref(pos, types, reg)
    val = r["s"]
    assert val > 10.0
    kw = dict(sigma=[0.02 * val], cv_min=[0.4 * val], cv_max=[1.6 * val], num_points=[512])
    var = cv.probe_volume(centre=CENTRE, sigma_s=0.3, weights=WEIGHTS, sigma=kw["sigma"][0], **kwargs)
    var.set_grid(kw["cv_min"][0], kw["cv_max"][0], 512)
    assert var.weights == COEFF
    oracle = ref.Metad(W=1.0, T_shift=7.0, T=1.0, stride=1, mode="well_tempered", **kw)
    rng = np.random.default_rng(8)
    seen, previous = [], val
    for step in range(1, STEPS + 1):
        if step > 1:
            pos = _moved(pos, rng).astype(dtype).astype(np.float64)
            context.set_positions(pos, types)
            r = _ref(pos, types, reg)
        context.run(1)
        assert context.current.system.getCurrentTimeStep() == step
        s = meta.cpp_integrator.getCurrentValues()[0]
        b = meta.cpp_integrator.getBiasFactors()[0]
        oracle.update_bias(step - 1, [previous])
        b_ref = oracle.update_bias(step, [r["s"]])[0]
        previous = r["s"]
        d = _value_bound(r)
        tol_b = 4 * 2 * step * KW["W"] / kw["sigma"][0] * d / kw["sigma"][0] + 1e-13 * 2 * step * KW["W"] / kw["sigma"][0]
        print("step %d: s %.15g vs %.15g (|d| %.3e of bound %.3e); bias factor %.6e vs oracle %.6e (|d| %.3e of bound %.3e)"
              % (step, s, r["s"], abs(s - r["s"]), d, b, b_ref, abs(b - b_ref), tol_b))
        assert abs(s - r["s"]) <= d
        assert abs(b - b_ref) <= tol_b
        if step > 1:
            # (step 1 sits on top of its own hill: the bias factor is the rounding residue of a slope that vanishes, 1e-15, and the
            # force pass may see another residue than the one reported)
            assert abs(b) > 1e3 * tol_b                                  # a slope of the deposited hills, far above what the bound lets pass
            _check_forces(var, r, reg, b, dtype)
        seen.append(b)
    assert len(set(seen)) == STEPS
    assert meta.cpp_integrator.lastStepRoute().startswith("generic")     # the general route: the fused step is untouched
    # the getters and the log
    t = context.current.system.getCurrentTimeStep()
    assert abs(var.cpp_force.getCurrentValue(t) - r["s"]) <= d
    assert var.cpp_force.getLogValue("cv_probe_volume", t) == var.cpp_force.getCurrentValue(t)
    assert "cv_probe_volume" in var.cpp_force.getProvidedLogQuantities() and "umbrella_energy_cv_probe_volume" in var.cpp_force.getProvidedLogQuantities()
    near = np.abs(np.abs(r["d"][:, 2]) - 1.5).min() if name == "slab" else np.abs(np.sqrt((r["d"] ** 2).sum(axis=1)) - 4.0).min()
    assert near > 1e-9 and var.get_count() == r["count"] and r["count"] != 0
    h = var.get_local()
    assert h.shape == (N,) and np.abs(h - r["h"]).max() <= 1e-12
    named = cv.probe_volume("sphere", CENTRE, 0.3, radius=2.0, name="cavity")
    assert "cv_probe_volume_cavity" in named.cpp_force.getProvidedLogQuantities() and named.weights == [1.0] * 3


def test_set_region_and_set_weights_take_effect_between_runs(api):
    """a probe volume is moved and grown in stages: every shape in turn on one variable, then other weights"""
    context, cv, integrate = api
    pos, types = _system(seed=8)
    context.initialize(pos, types, ["A", "B", "C"], BOX, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    kwargs, reg = REGIONS["slab"]
    var = cv.probe_volume(centre=CENTRE, sigma_s=0.3, weights=WEIGHTS, sigma=2.0, **kwargs)
    var.set_grid(0.0, 400.0, 128)
    context.run(1)
    values = [meta.cpp_integrator.getCurrentValues()[0]]
    r = _ref(pos, types, reg)
    assert abs(values[0] - r["s"]) <= _value_bound(r)
    for name in ("sphere", "cylinder", "box"):
        kwargs, reg = REGIONS[name]
        centre = [1.5, 2.0, -3.0]
        reg = dict(reg, centre=np.array(centre), sigma_s=0.2, r_c=0.5)
        var.set_region(centre=centre, sigma_s=0.2, r_c=0.5, **kwargs)
        context.run(1)
        r = _ref(pos, types, reg)
        s = meta.cpp_integrator.getCurrentValues()[0]
        print("%s: s %.15g vs %.15g, count %.6g" % (name, s, r["s"], var.get_count()))
        assert abs(s - r["s"]) <= _value_bound(r) and min(abs(s - v) for v in values) > 1e-3
        assert var.get_count() == r["count"] and np.abs(var.get_local() - r["h"]).max() <= 1e-12
        values.append(s)
    w = dict(A=0.0, B=2.0, C=-1.0)
    var.set_weights(w)
    assert var.weights == [0.0, 2.0, -1.0] and list(var.cpp_force.getWeights()) == [0.0, 2.0, -1.0]
    t = context.current.system.getCurrentTimeStep()
    r = _ref(pos, types, reg, coeff=[0.0, 2.0, -1.0])
    assert abs(var.cpp_force.getCurrentValue(t) - r["s"]) <= _value_bound(r)      # the cached step was formed anew
    assert abs(r["s"] - values[-1]) > 1e-3
    var.set_weights(None)
    assert var.weights == [1.0] * 3
    # refused: the variable stays as it was
    before = var.cpp_force.getCurrentValue(t)
    for bad in (dict(shape="sphere", centre=centre, sigma_s=0.2, radius=0.3), dict(shape="sphere", centre=centre, sigma_s=0.2, radius=7.4),
                dict(shape="box", centre=centre, sigma_s=0.2, half_widths=[INF] * 3), dict(shape="box", centre=centre, sigma_s=-0.2, half_widths=[1, 1, 1]),
                dict(shape="box", centre=centre, sigma_s=0.2, radius=1.0), dict(shape="ball", centre=centre, sigma_s=0.2, radius=1.0),
                dict(shape="cylinder", centre=centre, sigma_s=0.2, radius=1.0), dict(shape="sphere", centre=[0.0, float("nan"), 0.0], sigma_s=0.2, radius=1.0)):
        with pytest.raises(RuntimeError, match="Error setting parameters of collective variable."):
            var.set_region(**bad)
    for bad in (dict(A=1.0), dict(A=1.0, B=1.0, C=float("nan")), [1.0, 1.0, 1.0], dict(A=1.0, B=1.0, C=1.0, D=1.0)):
        with pytest.raises(RuntimeError, match="Error setting parameters of collective variable."):
            var.set_weights(bad)
    assert var.cpp_force.getCurrentValue(t) == before


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_virial_with_the_pressure_flag_and_a_box_change(api, dtype):
    """without the flag no virial is formed and get_virial raises; with it every row is the restatement's.  Then box and positions are
    scaled together: the centre follows, the widths do not"""
    context, cv, integrate = api
    pos, types = _system(seed=9)
    pos = pos.astype(dtype).astype(np.float64)
    context.initialize(pos, types, ["A", "B", "C"], BOX, dtype=dtype)
    meta = integrate.mode_metadynamics(**KW)
    kwargs, reg = REGIONS["box"]
    var = cv.probe_volume(centre=CENTRE, sigma_s=0.3, weights=WEIGHTS, sigma=1.0, **kwargs)
    var.set_grid(0.0, 200.0, 256)
    rng = np.random.default_rng(10)
    context.run(1)
    with pytest.raises(RuntimeError, match="pressure flag"):
        var.get_virial()
    pdata = context.current.system_definition.getParticleData()
    for flag in (False, True):
        pdata.setPressureFlag(flag)
        pos = _moved(pos, rng).astype(dtype).astype(np.float64)
        context.set_positions(pos, types)
        context.run(1)
        b = meta.cpp_integrator.getBiasFactors()[0]
        r = _ref(pos, types, reg)
        assert abs(b) > 1e-3
        _check_forces(var, r, reg, b, dtype)
    v = var.get_virial(per_particle=True)
    v_ref = b * r["virial"]
    phi0 = pv.phi(0.0, 0.3, 0.6)
    tol = 1e-12 * abs(b) * phi0 * np.abs(r["d"]).max() + storage(v_ref, dtype)
    frac = (np.abs(v - v_ref) / tol).max()
    print("virial: worst fraction of the bound %.3g, sums %s vs %s" % (frac, var.get_virial(), v_ref.sum(axis=1)))
    assert v.shape == (6, N) and frac <= 1.0 and np.abs(v_ref).max() > 0
    assert np.abs(var.get_virial() - v.sum(axis=1)).max() == 0.0
    # a box change: everything scaled by 0.97 about the origin (lo = -L / 2 scales with it)
    from metadynamics import _metadynamics
    k = 0.97
    box2 = tuple(k * x for x in BOX)
    pdata.setGlobalBox(_metadynamics.BoxDim(*box2))
    pos2 = (k * pos).astype(dtype).astype(np.float64)
    context.set_positions(pos2, types)
    context.run(1)
    reg2 = dict(reg, centre=k * np.array(CENTRE))
    r2 = _ref(pos2, types, reg2, box=box2)
    s = meta.cpp_integrator.getCurrentValues()[0]
    r_fixed = _ref(pos2, types, reg, box=box2)
    print("after the box change: s %.15g vs %.15g (centre following); with the centre left behind it would be %.15g" % (s, r2["s"], r_fixed["s"]))
    assert abs(s - r2["s"]) <= _value_bound(r2) and abs(r2["s"] - r_fixed["s"]) > 1e-3
    # a box that has shrunk below the region is refused at the step
    pdata.setGlobalBox(_metadynamics.BoxDim(16.0, 18.5, 5.0))
    with pytest.raises(RuntimeError):
        context.run(1)


def test_harmonic_umbrella(api):
    """forces = -(metadynamics bias factor + kappa (s - cv0)) a grad h through the base class, the bias as a host scalar;
    computeDerivatives gives the bare gradient"""
    context, cv, integrate = api
    pos, types = _system(seed=7)
    context.initialize(pos, types, ["A", "B", "C"], BOX, dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    kwargs, reg = REGIONS["cylinder"]
    r = _ref(pos, types, reg)
    val = r["s"]
    var = cv.probe_volume(centre=CENTRE, sigma_s=0.3, weights=WEIGHTS, sigma=0.05 * abs(val), **kwargs)
    var.set_grid(val - 10.0, val + 10.0, 256)
    cv0, kappa = val - 2.0, 0.35
    var.set_params(umbrella="harmonic", kappa=kappa, cv0=cv0)
    context.run(3)
    s = meta.cpp_integrator.getCurrentValues()[0]
    b = meta.cpp_integrator.getBiasFactors()[0]
    total = b + kappa * (s - cv0)
    print("s %.12g, bias factor %.6e, umbrella part %.6e" % (s, b, kappa * (s - cv0)))
    assert abs(kappa * (s - cv0)) > 0.5
    _check_forces(var, r, reg, total, np.float64)
    t = context.current.system.getCurrentTimeStep()
    var.cpp_force.computeDerivatives(t)
    _check_forces(var, r, reg, 1.0, np.float64)


def test_constructor_refusals_leave_nothing_behind(api):
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, types = _system()
    context.initialize(pos, types, ["A", "B", "C"], BOX, dtype=np.float32)
    integrate.mode_metadynamics(**KW)
    ok = dict(shape="sphere", centre=CENTRE, sigma_s=0.3, radius=2.0)
    cv.probe_volume(**ok)
    n_forces = len(context.current.forces)
    nan = float("nan")
    for bad in (dict(shape="ball"), dict(radius=None), dict(radius=0.6), dict(radius=nan), dict(radius=7.0), dict(sigma_s=0.0), dict(sigma_s=nan),
                dict(r_c=0.0), dict(r_c=-1.0), dict(half_widths=[1.0, 1.0, 1.0]), dict(axis="x"), dict(half_length=1.0), dict(centre=[0.0, 0.0]),
                dict(centre=[0.0, nan, 0.0]), dict(weights=dict(A=1.0)), dict(weights=dict(A=1.0, B=nan, C=0.0)), dict(weights=[1.0, 1.0, 1.0]),
                dict(shape="box", radius=None, half_widths=[INF, INF, INF]), dict(shape="box", radius=None, half_widths=[1.0, 0.0, 1.0]),
                dict(shape="box", radius=None, half_widths=[7.5, 1.0, 1.0]), dict(shape="box", radius=None), dict(shape="box", half_widths=[1.0, 1.0, 1.0]),
                dict(shape="cylinder"), dict(shape="cylinder", axis="w"), dict(shape="cylinder", axis="z", half_length=0.0),
                dict(shape="cylinder", axis="z", half_length=7.0)):
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.probe_volume(**{**ok, **bad})
        assert len(context.current.forces) == n_forces, bad
    # the host class on its own, as a C++ caller would use it
    sysdef = context.current.system_definition
    with pytest.raises(RuntimeError, match="one weight per particle type"):
        _metadynamics.ProbeVolume(sysdef, 1, CENTRE, [INF] * 3, 2.0, 0, 0.3, 0.6, [1.0], "")
    with pytest.raises(RuntimeError, match="the region is refused"):
        _metadynamics.ProbeVolume(sysdef, 1, CENTRE, [INF] * 3, 0.5, 0, 0.3, 0.6, [1.0, 1.0, 1.0], "")
    with pytest.raises(RuntimeError, match="finite weights"):
        _metadynamics.ProbeVolume(sysdef, 1, CENTRE, [INF] * 3, 2.0, 0, 0.3, 0.6, [1.0, nan, 1.0], "")
    v = _metadynamics.ProbeVolume(sysdef, 1, CENTRE, [INF] * 3, 2.0, 0, 0.3, 0.6, [1.0, 1.0, 1.0], "_x")
    f = v.getFractionalCentre()
    assert np.abs(np.array(f) - (np.array(CENTRE) / np.array(BOX) + 0.5)).max() <= 1e-15
    with pytest.raises(RuntimeError, match="the region is refused"):
        v.setRegion(1, CENTRE, [INF] * 3, 7.0, 0, 0.3, 0.6)                  # 7.6 > 15 / 2
    assert list(v.getFractionalCentre()) == list(f) and v.getCurrentValue(0) > 5.0
