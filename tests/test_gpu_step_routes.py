"""GPU: which route a step of the host classes takes (IntegratorMetaDynamics::lastStepRoute, written by the step's functions as they
run) for every kind of variable set — the rows of tools/host_bits.py, which dumps the same runs' values for a comparison between two
trees.  The expected routes are read off the code of the step as it stood before planStep existed (one interleaved function):

  * a set of lamellar variables without umbrella, not adaptive, no walkers, setFusedPath on: the fused step, up to 6 variables;
  * otherwise, in a set of at most 3 variables, the lamellar variables without umbrella share launch A and the engine's launch
    (`lamellar_slots`); with exactly ONE mesh in the set their sums ride in its assignment instead (`rider`; the first assignment of a
    mesh carries them too) and the engine's launch goes into the mesh's force pass (`mesh_merged`) — unless the pressure flag is set.
    Tiles: a 16^3 mesh has 4 tiles = 8 force blocks, the grids here need at most 5 grid blocks, so deposit steps merge as well;
  * one mesh without lamellar company: `mesh_merged` unless setFusedPath(False);
  * cv.steinhardt alone updates the engine itself (`self`); walkers take the engine's walker launch; everything else `own`.

context.run(n) calls prepRun first, which is a step of its own at the current time step: the first record below is that step alone
(run(0): the very first step of the set, the mesh's first assignment), the other four are the steps of run(1) — each preceded by an
unobserved prepRun step at a time step whose values the variables have already."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("host_bits", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "host_bits.py"))
host_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host_bits)

FUSED = "fused sums=- engine=fused_step"
ROUTES = {
    "one_lamellar": FUSED,
    "four_lamellar": FUSED,
    "one_lamellar_unfused": "generic sums=- engine=own",
    "lamellar_and_umbrella": "generic sums=launch_a engine=lamellar_slots",
    "lamellar_and_mesh": "generic sums=rider engine=mesh_merged",
    "lamellar_and_mesh_pressure": "generic sums=rider engine=lamellar_slots",
    "lamellar_and_two_meshes": "generic sums=launch_a engine=lamellar_slots",
    "mesh_alone": "generic sums=- engine=mesh_merged",
    "mesh_alone_unfused": "generic sums=- engine=own",
    "steinhardt_alone": "generic sums=- engine=self",
    "steinhardt_and_lamellar": "generic sums=launch_a engine=lamellar_slots",
    "one_lamellar_walkers": "generic sums=- engine=walkers",
    "one_lamellar_adaptive": "generic sums=- engine=own",
    "box_variables": "generic sums=- engine=own",
}


@pytest.fixture()
def fresh_context():
    from metadynamics import context
    yield context
    context.current = None


def _steps(context, meta, want):
    """the prepRun step of run(0), then four steps one by one: route and usedFusedPath of each"""
    integ = meta.cpp_integrator
    assert integ.lastStepRoute() == "" and not integ.usedFusedPath()
    for n in (0, 1, 1, 1, 1):
        context.run(n)
        t = context.current.system.getCurrentTimeStep()
        assert integ.lastStepRoute() == want, (t, integ.lastStepRoute())
        assert integ.usedFusedPath() == want.startswith("fused "), t
    assert context.current.system.getCurrentTimeStep() == 4
    assert integ.getNumGaussians() >= 3                              # (stride 2: the deposits of time steps 0, 2, 4; prepRun deposits again)


def test_every_row_has_a_route():
    assert set(ROUTES) == set(host_bits.ROWS)


@pytest.mark.parametrize("row", sorted(ROUTES))
def test_route_of_every_step(fresh_context, row, capfd):
    context = fresh_context
    meta, cvs = host_bits.ROWS[row](np.float64 if "mesh" in row else np.float32)
    _steps(context, meta, ROUTES[row])
    err = capfd.readouterr().err
    # walkers without a communicator: said once, not once per step
    assert err.count("running as a single walker") == (1 if row == "one_lamellar_walkers" else 0)


def test_removed_stream_switches_change_nothing(fresh_context, monkeypatch):
    """MTD_SIDE_STREAM=1 and MTD_MESH_OVERLAP=1 once moved launches of the lamellar + mesh step to a second stream (both measured
    slower); the switches are gone: a process that sets them takes the default route and gets the same bits"""
    context = fresh_context

    def run():
        meta, cvs = host_bits.ROWS["lamellar_and_mesh"](np.float32)
        _steps(context, meta, ROUTES["lamellar_and_mesh"])
        integ = meta.cpp_integrator
        out = dict(cv=np.array(integ.getCurrentValues()), bias=np.array(integ.getBiasFactors()),
                   F=[np.array(c.cpp_force.getForceArray()) for c in cvs])
        context.current = None
        return out

    monkeypatch.setenv("MTD_SIDE_STREAM", "1")
    monkeypatch.setenv("MTD_MESH_OVERLAP", "1")
    switched = run()
    monkeypatch.delenv("MTD_SIDE_STREAM")
    monkeypatch.delenv("MTD_MESH_OVERLAP")
    plain = run()
    assert np.array_equal(switched["cv"], plain["cv"]) and np.array_equal(switched["bias"], plain["bias"])
    assert np.all(plain["bias"] != 0.0)
    for a, b in zip(switched["F"], plain["F"]):
        assert np.array_equal(a, b) and np.abs(a).max() > 0
