"""GPU: the bond-orientational order on HOOMD's row layout, and on rows of every length (tests/list_layouts.py).

1. Layouts: the variable runs on the compact list and on the same rows stored with slack (the slack holding stale but valid entries), in
   descending order and scattered.  Every output must be the compact run's BIT FOR BIT: every sum follows the place of an entry in its
   row and the particle index, never an address.
2. Row lengths: isolated clumps of 1 .. 26 particles (the sweep of the pair entropy, the same walk of eight lanes) give rows of
   0 .. 25 = 3 * 8 + 1 entries, every boundary of the two-deep look-ahead for each of the eight lanes of a group.  Run A: the clean list
   against the restatement with the unit's own compare() and tolerances; run B: every row padded with the entries the walk must skip
   (the particle itself, the other type inside the cut-off, a partner beyond it, an index >= N), against the restatement of the CLEAN
   list."""
import numpy as np
import pytest

import hexatic_ref as hr
import list_layouts as ll
from test_gpu_hexatic import OUTPUTS, compare, condition, params, reference, run_gpu, snapshot

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 11
R_CUT_SWEEP, R_ON_SWEEP = 2.8, 0.6                                       # the cut-off the clumps of the "pe" sweep were laid out for


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["plain", "switch+gate", "global"])
def test_every_layout_gives_the_compact_lists_bits(abi, dtype, name):
    s = snapshot("fcc", dtype)
    pos, types, L, nl = s["pos"], s["types"], s["L"], s["nl"]
    lists = {kind: ll.relayout(nl, kind, seed=SEED, n_positions=len(pos)) for kind in ll.KINDS}
    for kind in ll.OTHER_KINDS:
        head, nn, lst = (np.asarray(x).astype(np.int64) for x in lists[kind])
        assert len(lst) > nn.sum() + len(head) and head.min() > 0 and not np.array_equal(head[1:], np.cumsum(nn)[:-1])
    par = params("fcc", name)
    run = lambda lst: run_gpu(abi, pos, types, L, lst, par, dtype, virial=True)
    base = run(lists["compact"])
    compare(base, reference(s, par, name), 0.9, dtype, types=types, par=par)
    for kind in ll.OTHER_KINDS:
        got = run(lists[kind])
        for key in OUTPUTS:
            assert np.array_equal(got[key], base[key]), (kind, key)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("opt", [dict(), dict(k=4, axis="x", switch=(0.3, 4), gate=(1.0, 6.0)), dict(global_order=True), dict(k=1, axis="y")],
                         ids=["plain", "switch+gate", "global", "k=1"])
def test_rows_of_every_length(abi, dtype, opt):
    case = ll.sweep("pe", dtype)
    pos, types, L, nl = case["pos"], case["types"], case["L"], case["nl"]
    nn = np.asarray(nl[1])[:case["n_members"]]
    assert set(nn.tolist()) == set(range(3 * 8 + 2))                     # rows of 0 .. 25 entries
    inside, beyond, _ = ll.distances(case)
    assert inside <= R_CUT_SWEEP < beyond
    par = hr.params(0, R_CUT_SWEEP, R_ON_SWEEP, **opt)
    r = hr.compute(pos, types, L, nl, par, bias=ll.BIAS)
    condition(r, par)
    assert (r["r"] < R_ON_SWEEP).any() and (r["r"] > R_ON_SWEEP).any()   # the window crosses the clumps
    for lists in (nl, ll.padded(case, ghosts=True)):
        g = run_gpu(abi, pos, types, L, lists, par, dtype, virial=True, bias=ll.BIAS)
        compare(g, r, ll.BIAS, dtype, types=types, par=par)
