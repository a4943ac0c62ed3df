"""GPU: the largest-cluster option of cv.coordination and cv.tetrahedral through the host classes, the Python API and
integrate.mode_metadynamics on the fixtures of tests/row_cluster_ref.py, against that restatement driven with the bias factor the integrator
reports plus the umbrella's: the value to rtol 1e-9, force array and per-particle virial to 1e-9 of their maxima (the tolerances of
tests/test_gpu_coordination_api.py and tests/test_gpu_tetrahedral_api.py), mask, labels and summary exactly."""
import numpy as np
import pytest

import coordination_ref as cn
import row_cluster_ref as rc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
KAPPA = 35.0
NONE = rc.NONE


@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _case(kind):
    return rc.coordination_case("switch") if kind == "coordination" else rc.tetrahedral_case("switch+gate")


def _r_list(kind):
    return rc.COORD_LIST if kind == "coordination" else rc.TET_LIST


def _make(cv, kind, c, nl, **kw):
    par = c["par"]
    if kind == "coordination":
        sw = par["switch"]
        return cv.coordination(par["r_0"], nl, "A", r_cut=par["r_cut"], switch=None if sw is None else dict(c0=sw[0], p=sw[1]), **kw)
    sw, gt = par["switch"], par["gate"]
    return cv.tetrahedral(par["r_cut"], par["r_on"], nl, "A", normalise=par["normalise"], switch=None if sw is None else dict(c0=sw[0], p=sw[1]),
                          gate=None if gt is None else dict(n_lo=gt[0], n_hi=gt[1]), **kw)


def _ref(kind, c, lists, cluster, bias=1.0):
    f = rc.coordination if kind == "coordination" else rc.tetrahedral
    return f(c["pos"], c["types"], c["L"], lists, c["par"], cluster=cluster, bias=bias)


@pytest.mark.parametrize("kind", ["coordination", "tetrahedral"])
def test_cluster_on_a_grid_with_an_umbrella(api, kind):
    """set_cluster, three steps under a harmonic umbrella with the pressure flag set: the value the engine used, the force array,
    get_virial(), the three getters and get_switched() (unmasked); then set_cluster(None): the plain variable's value, bit for bit"""
    context, cv, integrate = api
    c = _case(kind)
    pos, types, L = c["pos"], c["types"], c["L"]
    cluster = dict(v_min=c["cluster"][0], r_link=c["cluster"][1])
    context.initialize(pos, types, ["A", "B"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(True)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=_r_list(kind))
    lists = nl.update()
    val = _ref(kind, c, lists, c["cluster"])["s"]
    assert val == pytest.approx(c["ref"]["s"], rel=1e-12)               # the host list holds the fixture's pairs
    var = _make(cv, kind, c, nl, sigma=0.02 * val)
    var.set_grid(0.4 * val, 1.6 * val, 512)
    for getter in (var.get_cluster_mask, var.get_cluster_labels, var.get_largest_cluster):
        with pytest.raises(RuntimeError, match="no clusters without the cluster option"):
            getter()
    var.set_cluster(cluster)
    cv0 = 0.8 * val
    var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(3)
    t = context.current.system.getCurrentTimeStep()
    s = meta.cpp_integrator.getCurrentValues()[0]
    assert s == pytest.approx(val, rel=1e-9) and var.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-9)
    total = meta.cpp_integrator.getBiasFactors()[0] + KAPPA * (s - cv0)
    r = _ref(kind, c, lists, c["cluster"], bias=total)
    F = var.cpp_force.getForceArray()
    per, W = var.get_virial(per_particle=True), var.get_virial()
    top_f, top_v, top_w = np.abs(r["force"]).max(), np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max()
    print("%s: s %.12g vs %.12g, bias %.6e; forces %.3e of %.3e; virial per particle %.3e of %.3e, sums %.3e of %.3e"
          % (kind, s, val, total, np.abs(F[:, :3] - r["force"]).max(), top_f, np.abs(per.T - r["virial"]).max(), top_v,
             np.abs(W - r["virial_sum"]).max(), top_w))
    assert abs(total) > 1e-3 and top_f > 0 and top_w > 0
    assert np.abs(F[:, :3] - r["force"]).max() <= 1e-9 * top_f
    assert np.abs(per.T - r["virial"]).max() <= 1e-9 * top_v and np.abs(W - r["virial_sum"]).max() <= 1e-9 * top_w
    w, labels, largest = var.get_cluster_mask(), var.get_cluster_labels(), var.get_largest_cluster()
    assert w.dtype == np.float64 and labels.dtype == np.uint32 and w.shape == labels.shape == (len(pos),)
    assert np.array_equal(w, r["w"]) and np.array_equal(labels, r["label"]) and tuple(largest) == tuple(int(x) for x in r["summary"])
    assert largest[1] == w.sum() and largest[0] != NONE
    far = rc.far_from_members(pos, L, r["w"], 2.0 * c["par"]["r_cut"])
    assert far.any() and np.all(F[far] == 0.0) and np.all(per[:, far] == 0.0)
    sw = var.get_switched()
    assert np.abs(sw - r["switched"]).max() <= 1e-9 * np.abs(r["switched"]).max() and np.abs(sw[w == 0.0]).max() > 0.1    # unmasked
    # off again: the plain variable, bit for bit — a second variable that never had the option says what that is
    var.set_cluster(None)
    plain = _make(cv, kind, c, nl, name="plain")
    v_off, v_plain = var.cpp_force.getCurrentValue(t), plain.cpp_force.getCurrentValue(t)
    assert v_off == v_plain and v_plain == pytest.approx(_ref(kind, c, lists, None)["s"], rel=1e-9) and v_plain > val
    with pytest.raises(RuntimeError, match="no clusters without the cluster option"):
        var.get_cluster_mask()
    # and on: the masked value is back
    var.set_cluster(cluster)
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-9)


def test_refusals(api):
    context, cv, integrate = api
    c = rc.coordination_case("switch")
    context.initialize(c["pos"], c["types"], ["A", "B"], c["L"], dtype=np.float64)
    integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=rc.COORD_LIST)
    nl.update()
    ok = dict(v_min=0.3, r_link=1.2)
    refused = "Error creating collective variable."
    # coordination: no cluster without a switch, no switch taken away under a cluster
    var = cv.coordination(1.2, nl, "A", r_cut=1.5)
    with pytest.raises(RuntimeError, match=refused):
        var.set_cluster(ok)
    with pytest.raises(RuntimeError, match="needs a switch"):
        var.cpp_force.setCluster(0.3, 1.2)
    var.set_switch(dict(c0=6, p=8))
    var.set_cluster(ok)
    with pytest.raises(RuntimeError, match=refused):
        var.set_switch(None)
    with pytest.raises(RuntimeError, match="needs the switch"):
        var.cpp_force.clearSwitch()
    var.set_switch(dict(c0=5, p=6, less=True))                          # another switch is fine
    for bad in (dict(v_min=0.3), dict(v_min=float("nan"), r_link=1.2), dict(v_min=0.3, r_link=0.0), dict(v_min=0.3, r_link=1.2, x=1), (0.3, 1.2)):
        with pytest.raises(RuntimeError, match=refused):
            var.set_cluster(bad)
    with pytest.raises(RuntimeError, match="finite v_min and r_link > 0"):
        var.cpp_force.setCluster(0.3, -1.0)
    t = context.current.system.getCurrentTimeStep()
    want = rc.coordination(c["pos"], c["types"], c["L"], c["nl"], cn.params(switch=(5, 6, True), **rc.COORD_PAR), cluster=(0.3, 1.2))
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(want["s"], rel=1e-9)    # the refused calls left the option as it was
    assert var.get_largest_cluster()[1] == want["summary"][1]
    var.set_cluster(None)
    var.set_switch(None)
    # tetrahedral: not on the penalty
    pen = cv.tetrahedral(1.4, 1.2, nl, "A", normalise=False)
    with pytest.raises(RuntimeError, match=refused):
        pen.set_cluster(ok)
    with pytest.raises(RuntimeError, match="needs the normalised variable"):
        pen.cpp_force.setCluster(0.3, 1.2)
    # r_link beyond the reach of a device-built list
    dev = cv.nlist_cell(r_cut=rc.COORD_LIST, device=True)
    for var in (cv.coordination(1.2, dev, "A", r_cut=1.5, switch=dict(c0=6, p=8), name="dev"), cv.tetrahedral(1.4, 1.2, dev, "A", name="dev")):
        with pytest.raises(RuntimeError, match=refused):
            var.set_cluster(dict(v_min=0.3, r_link=1.6))
        with pytest.raises(RuntimeError, match="must reach r_link"):
            var.cpp_force.setCluster(0.3, 1.6)
        var.set_cluster(dict(v_min=0.3, r_link=1.55))


@pytest.mark.parametrize("kind", ["coordination", "tetrahedral"])
def test_device_built_list(api, kind):
    """cv.nlist_cell(device=True), never update()d by the script"""
    context, cv, integrate = api
    c = _case(kind)
    context.initialize(c["pos"], c["types"], ["A", "B"], c["L"], dtype=np.float64)
    meta = integrate.mode_metadynamics(**KW)
    nl = cv.nlist_cell(r_cut=_r_list(kind), r_buff=0.3, device=True)
    val = c["ref"]["s"]
    var = _make(cv, kind, c, nl, sigma=0.02 * val)
    var.set_cluster(dict(v_min=c["cluster"][0], r_link=c["cluster"][1]))
    var.set_grid(0.4 * val, 1.6 * val, 512)
    context.run(2)
    t = context.current.system.getCurrentTimeStep()
    assert meta.cpp_integrator.getCurrentValues()[0] == pytest.approx(val, rel=1e-9)
    assert var.cpp_force.getCurrentValue(t) == pytest.approx(val, rel=1e-9)
    assert np.array_equal(var.get_cluster_mask(), c["ref"]["w"]) and np.array_equal(var.get_cluster_labels(), c["ref"]["label"])
    assert tuple(var.get_largest_cluster()) == tuple(int(x) for x in c["ref"]["summary"])
    assert nl.cpp_nlist.getNumRebuilds() == 1
