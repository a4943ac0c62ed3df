"""CPU self-check of tests/grid_paths.py (no GPU): the paths can catch what they are for.

A bias step that reads a stale patch evaluates dV/ds on the grid as it was one deposit earlier.  On the oracle alone: every
`hit` step of the paths (the steps the engine serves from the patch) sees a derivative that differs between the current grid
and the grid of one deposit earlier by at least 1000 x the 1e-9 that test_gpu_metad.compare allows the bias factors — relative
to the larger component.  If a grid or sigma in grid_paths.py is changed, this is what has to stay green.

Observed: with stride 1 the smallest difference on a `hit` step is 3.0e-4 (three variables, well-tempered); with stride 3,
12 of 13, 25 of 25 and 60 of 61 `hit` steps differ by 1e-6 or more (the others follow a deposit made far away).
"""
import numpy as np
import pytest

import grid_paths

STALE_MIN = 1000 * 1e-9


def stale_errors(ref, n_cv, stride, mode, particle):
    """per step: (label, relative difference of dV/ds between the grid of one deposit earlier and the current grid)"""
    kw = grid_paths.settings(n_cv, stride, mode, particle)
    g = grid_paths.grid(n_cv, particle)
    steps = grid_paths.path(n_cv, particle)
    r = ref.Metad(**kw)
    view = r.array("grid")
    earlier = view.copy()
    out = []
    for t, ((cell, frac, label), (vals, _)) in enumerate(zip(steps, grid_paths.values(steps, n_cv, particle))):
        if label != "off":
            assert grid_paths.cell_of(g, vals) == cell, (t, label, vals)
            assert all(lo <= v < hi for v, lo, hi in zip(vals, g["cv_min"], g["cv_max"])), (t, label, vals)
        else:
            assert any(not (lo <= v < hi) for v, lo, hi in zip(vals, g["cv_min"], g["cv_max"])), (t, vals)
        before = view.copy()
        b = r.update_bias(t, vals)
        assert not np.isnan(b).any(), (t, label, b)
        if not np.array_equal(before, view):
            earlier = before                                   # this step deposited
        now = np.array([r.derivative(c, vals) for c in range(n_cv)])
        current = view.copy()
        view[:] = earlier
        stale = np.array([r.derivative(c, vals) for c in range(n_cv)])
        view[:] = current
        assert np.array_equal(now, [r.derivative(c, vals) for c in range(n_cv)])
        scale = max(np.abs(now).max(), np.abs(stale).max())
        out.append((label, np.abs(now - stale).max() / scale if scale > 0 else 0.0))
    assert np.isfinite(r.array("weight")).all()
    return out


@pytest.mark.parametrize("particle", [False, True], ids=["grid", "particle_grid"])
@pytest.mark.parametrize("mode", ["well_tempered", "standard"])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("n_cv", [1, 2, 3])
def test_stale_patch_is_a_large_error(ref, n_cv, stride, mode, particle):
    errs = stale_errors(ref, n_cv, stride, mode, particle)
    assert len(errs) == {1: 26, 2: 46, 3: 90}[n_cv]
    hits = [e for label, e in errs if label == "hit"]
    assert len(hits) == 2 * 3 ** n_cv + 7
    good = sum(e >= STALE_MIN for e in hits)
    print("n_cv %d stride %d %s: %d of %d hit steps, min %.3g" % (n_cv, stride, mode, good, len(hits), min(hits)))
    if stride == 1:
        assert good == len(hits), (min(hits), hits)
    else:
        # (the steps near the corners follow a deposit made far away)
        assert good >= 0.8 * len(hits), (good, len(hits))


@pytest.mark.parametrize("n_cv", [1, 2, 3])
def test_path_shape(n_cv):
    """labels and moves agree: a `hit` step moves every variable by at most one cell, `mixed` one variable by two, and the walk
    used for the host-write tests stays within one cell of the centre"""
    steps = grid_paths.path(n_cv)
    n = grid_paths.grid(n_cv)["num_points"]
    for (prev, _, plabel), (cell, f, label) in zip(steps, steps[1:]):
        move = max(abs(a - b) for a, b in zip(prev, cell))
        if label == "hit" and plabel != "off":
            assert move <= 1, (prev, cell)
        if label == "mixed":
            assert move == 2 and sum(a != b for a, b in zip(prev, cell)) == 1
        if label != "off":
            assert all(0 <= c <= m - 2 for c, m in zip(cell, n)), cell
    walk = grid_paths.hit_walk(n_cv, 60, start=3)
    c0 = grid_paths.centre(n_cv)
    assert len(walk) == 60 and all(max(abs(a - b) for a, b in zip(cell, c0)) <= 1 for cell, _, _ in walk)
    assert all(f in grid_paths.FRACTIONS for _, f, _ in walk)
