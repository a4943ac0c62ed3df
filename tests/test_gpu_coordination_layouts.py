"""GPU: the coordination number on HOOMD's row layout, and on rows of every length (tests/list_layouts.py).

1. Layouts: the variable runs on the compact list and on the same rows stored with slack (the slack holding stale but valid entries), in
   descending order and scattered, all particles central and (the plain variable: a switch refuses ghosts) with the trailing 200 as
   ghosts.  Every output must be the compact run's BIT FOR BIT: every sum follows the place of an entry in its row and the particle
   index, never an address.
2. Row lengths: isolated clumps of 1 .. 26 particles (the sweep of the pair entropy, the same walk of eight lanes) give rows of
   0 .. 25 = 3 * 8 + 1 entries, every boundary of the two-deep look-ahead for each of the eight lanes of a group, through both routes.
   Run A: the clean list against the restatement with the unit's own compare() and tolerances; run B: every row padded with the entries
   the walk must skip (the particle itself, the other type inside the cut-off, a partner beyond it; an entry j >= N counts here, so none
   is added), against the restatement of the CLEAN list; run C (plain): the last member of every clump a ghost."""
import numpy as np
import pytest

import coordination_ref as cn
import list_layouts as ll
from test_gpu_coordination import OUTPUTS, R0, R_CUT, SWITCHES, compare, noisy_fcc, run_gpu

import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 11
R_CUT_SWEEP = 2.8                                                        # the cut-off the clumps of the "pe" sweep were laid out for


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode,ghosts", [("plain", False), ("plain", True), ("switch", False), ("less", False)])
def test_every_layout_gives_the_compact_lists_bits(abi, dtype, mode, ghosts):
    pos, L = noisy_fcc(5)
    pos = pos.astype(dtype).astype(np.float64)
    types = (np.arange(len(pos)) % 3 == 1).astype(np.int32)
    nl = util.build_nlist(pos, L, R_CUT)
    n_rows = 300 if ghosts else None
    if ghosts:
        nl = ll.from_rows(ll.as_rows(nl)[:n_rows])
        assert (np.asarray(nl[2]) >= n_rows).any()
    lists = {kind: ll.relayout(nl, kind, seed=SEED, n_positions=len(pos)) for kind in ll.KINDS}
    for kind in ll.OTHER_KINDS:
        head, nn, lst = (np.asarray(x).astype(np.int64) for x in lists[kind])
        assert len(lst) > nn.sum() + len(head) and head.min() > 0 and not np.array_equal(head[1:], np.cumsum(nn)[:-1])
    for pair in ((0, 1), (0, 0)):
        par = cn.params(pair[0], pair[1], R0, R_CUT, switch=SWITCHES[mode])
        run = lambda lst: run_gpu(abi, pos, types, L, lst, par, dtype, virial=True, n_rows=n_rows)
        base = run(lists["compact"])
        compare(base, cn.compute(pos, types, L, nl, par, bias=0.9), 0.9, dtype, types=types, par=par)
        for kind in ll.OTHER_KINDS:
            got = run(lists[kind])
            for key in OUTPUTS:
                assert np.array_equal(got[key], base[key]), (kind, key)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", ["plain", "switch"])
def test_rows_of_every_length(abi, dtype, mode):
    case = ll.sweep("pe", dtype)
    pos, types, L, nl = case["pos"], case["types"], case["L"], case["nl"]
    nn = np.asarray(nl[1])[:case["n_members"]]
    assert set(nn.tolist()) == set(range(3 * 8 + 2))                     # rows of 0 .. 25 entries
    inside, beyond, _ = ll.distances(case)
    assert inside <= R_CUT_SWEEP < beyond
    par = cn.params(0, 0, 1.0, R_CUT_SWEEP, switch=(6.0, 4) if mode == "switch" else None)
    r = cn.compute(pos, types, L, nl, par, bias=ll.BIAS)
    for lists in (nl, ll.padded(case, ghosts=False)):
        g = run_gpu(abi, pos, types, L, lists, par, dtype, virial=True, bias=ll.BIAS)
        compare(g, r, ll.BIAS, dtype, types=types, par=par)
    if mode == "plain":
        s = ll.split_ghosts(case)
        g = run_gpu(abi, s["pos"], s["types"], L, s["nl"], par, dtype, virial=True, bias=ll.BIAS, n_rows=s["n_rows"])
        compare(g, cn.compute(s["pos"], s["types"], L, s["nl"], par, bias=ll.BIAS), ll.BIAS, dtype, types=s["types"], par=par)
