"""Collective-variable paths written in grid cells (helper, no test).

The scalar chain of a bias step with at most three variables reads its stencil from a 6^n-cell patch of the bias grid kept
around the previous step's values (MetadState::patch_v) and falls back to the grid per lane.  Whether a step is served by the
patch, by the grid or by both depends only on how many cells every variable moved, so the paths here are lists of
(cell vector, fraction, label): s_i = cv_min_i + (cell_i + fraction) delta_i with delta_i = (cv_max_i - cv_min_i) / (n_i - 1).

Labels say what the chain has to do at the step when every step deposits (stride 1):
  hit    every stencil cell lies in the patch (a move of at most one cell per variable)
  mixed  some lanes are served by the patch, others load (a move of two cells in one variable)
  miss   the point itself has corners outside the patch, or there is no patch yet (the first step)
  edge   the first step in a corner of the grid (a long move: forward / backward differences, patch origin < 0 or > n - 6)
  off    a variable is off the grid (V = 0, nothing is interpolated)

tests/test_grid_paths.py proves on the oracle alone that a stale patch on a `hit` step is a large error;
tests/test_gpu_grid_patch.py drives the engine along the paths.
"""
import itertools

import numpy as np

# the smallest grids that still have an interior, both edges and, in 3-d, several ragged 256-cell grid blocks (1080 cells = 5)
GRIDS = {
    1: dict(num_points=[16], cv_min=[-1.0], cv_max=[1.0]),
    2: dict(num_points=[20, 14], cv_min=[-1.0, 0.0], cv_max=[1.0, 1.0]),
    3: dict(num_points=[12, 10, 9], cv_min=[-1.0, 0.0, 2.0], cv_max=[1.0, 1.0, 4.0]),
}
# the same grids with ranges a single lattice vector's s = cos(2 pi x / L) can reach, half a cell beyond cv_max of variable 0
# included: cv_max_0 + delta_0 / 2 = 0.96, 0.947, 0.982
PARTICLE_GRIDS = {
    1: dict(num_points=[16], cv_min=[-0.9], cv_max=[0.9]),
    2: dict(num_points=[20, 14], cv_min=[-0.9, 0.0], cv_max=[0.9, 0.9]),
    3: dict(num_points=[12, 10, 9], cv_min=[-0.9, 0.0, -0.9], cv_max=[0.9, 0.9, 0.9]),
}
# how far below cv_min the last variable goes, in cells.  Half a cell everywhere but on the 3-d particle grid, where
# -0.9 - 0.5 * 0.225 = -1.0125 is no cosine: 0.4 cells (-0.99) there
BELOW = {(3, True): 0.4}

FRACTIONS = (0.37, 0.61)


def grid(n_cv, particle=False):
    g = dict((PARTICLE_GRIDS if particle else GRIDS)[n_cv])
    g["delta"] = [(hi - lo) / (n - 1) for lo, hi, n in zip(g["cv_min"], g["cv_max"], g["num_points"])]
    return g


def settings(n_cv, stride=1, mode="well_tempered", particle=False):
    """keyword arguments of GpuMetad / mtd_ref.Metad for the grid of n_cv variables"""
    g = grid(n_cv, particle)
    return dict(sigma=[1.5 * d for d in g["delta"]], cv_min=g["cv_min"], cv_max=g["cv_max"], num_points=g["num_points"],
                W=1.0, T_shift=7.0, T=1.0, stride=stride, mode=mode)


def centre(n_cv, particle=False):
    return tuple(n // 2 for n in grid(n_cv, particle)["num_points"])


def out_and_back(n_cv, particle=False):
    """the closed loop at the head of every path: c0, then for every d in {-1, 0, 1}^n to c0 + d and back to c0; all but the
    very first step are `hit`.  (A cumulative walk over the 3^n moves leaves the grid; this one never drifts.)"""
    c0 = centre(n_cv, particle)
    cells = [(c0, "miss")]
    for d in itertools.product((-1, 0, 1), repeat=n_cv):
        cells.append((tuple(c + x for c, x in zip(c0, d)), "hit"))
        cells.append((c0, "hit"))
    return [(cell, FRACTIONS[k % 2], label) for k, (cell, label) in enumerate(cells)]


def path(n_cv, particle=False):
    """the whole path: 26 steps for one variable, 46 for two, 90 for three"""
    g = grid(n_cv, particle)
    n = g["num_points"]
    c0 = centre(n_cv, particle)
    cells = [(cell, label) for cell, _, label in out_and_back(n_cv, particle)]
    # +-2 (the point s +- delta has corners outside the patch) and +-3 cells (the point s has) in one variable, out and back
    for i in range(n_cv):
        for move, label in ((2, "mixed"), (-2, "mixed"), (3, "miss"), (-3, "miss")):
            cells.append((tuple(c + (move if j == i else 0) for j, c in enumerate(c0)), label))
            cells.append((c0, label))
    steps = [(cell, FRACTIONS[k % 2], label) for k, (cell, label) in enumerate(cells)]
    lo, lo1 = (0,) * n_cv, (1,) * n_cv
    hi, hi1 = tuple(x - 2 for x in n), tuple(x - 3 for x in n)
    # the low corner: s == cv_min exactly, patch origin -2, forward differences
    steps += [(lo, 0.0, "edge"), (lo1, 0.37, "hit"), (lo, 0.6, "hit"), (lo, 0.05, "hit")]
    # the high corner: the patch reaches past the grid's end, backward differences, the `upper >= len` clamp
    steps += [(hi, 0.999, "edge"), (hi1, 0.61, "hit"), (hi, 0.2, "hit")]
    # off the grid and back: variable 0 half a cell above cv_max, the last variable below cv_min
    below = BELOW.get((n_cv, particle), 0.5)
    steps += [((n[0] - 1,) + hi[1:], 0.5, "off"), (hi, 0.37, "hit"), (lo[:-1] + (-1,), 1.0 - below, "off"), (lo, 0.61, "hit")]
    return steps


def value(g, cell, fraction):
    return [lo + (c + fraction) * d for lo, c, d in zip(g["cv_min"], cell, g["delta"])]


def values(steps, n_cv, particle=False):
    """[(CV values, label)] of a list of steps"""
    g = grid(n_cv, particle)
    return [(value(g, cell, f), label) for cell, f, label in steps]


def cell_of(g, vals):
    """the cell a point lies in (floor, also below the grid)"""
    return tuple(int(np.floor((v - lo) / d)) for v, lo, d in zip(vals, g["cv_min"], g["delta"]))


def hit_walk(n_cv, count, particle=False, start=0):
    """`count` steps of the closed loop, repeated as often as needed, from its step `start` on: every step but the loop's very
    first stays within one cell of the previous one"""
    loop = out_and_back(n_cv, particle)
    seq = [loop[0]] + [loop[1 + k % (len(loop) - 1)] for k in range(start + count)]
    return seq[start:start + count]
