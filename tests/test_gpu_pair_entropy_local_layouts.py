"""GPU: the local pair entropy on HOOMD's row layout, and on rows of every length (tests/list_layouts.py).

1. Layouts: the variable runs on the compact list and on the same rows stored with slack (the slack holding stale but valid entries), in
   descending order and scattered.  Every output must be the compact run's BIT FOR BIT: H_ib is summed in integers, every other sum
   follows the place of an entry in its row and the particle index, never an address.
2. Row lengths: isolated clumps of 1 .. 26 particles give rows of 0 .. 25 = 3 * 8 + 1 entries, every boundary of the two-deep look-ahead
   for each of the eight lanes of a group, through all five launches.  Run A: the clean list against the restatement with the unit's own
   compare() and tolerances; run B: every row padded with the entries the walk must skip (the particle itself, the other type inside
   the cut-off, a partner beyond it, an index >= N), against the restatement of the CLEAN list."""
import numpy as np
import pytest

import list_layouts as ll
from test_gpu_pair_entropy_local import OUTPUTS, compare, noisy_fcc, reference, run_gpu

import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEED = 11
SETS = {"plain": dict(), "both": dict(average=(1.2, 1.5), switch=(3.0, 6))}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(SETS))
def test_every_layout_gives_the_compact_lists_bits(abi, dtype, name):
    pos, L = noisy_fcc(5)
    pos = pos.astype(dtype).astype(np.float64)
    types = (np.arange(len(pos)) % 9 == 4).astype(np.int32)
    nl = util.build_nlist(pos, L, 2.4)
    lists = {kind: ll.relayout(nl, kind, seed=SEED, n_positions=len(pos)) for kind in ll.KINDS}
    for kind in ll.OTHER_KINDS:
        head, nn, lst = (np.asarray(x).astype(np.int64) for x in lists[kind])
        assert len(lst) > nn.sum() + len(head) and head.min() > 0 and not np.array_equal(head[1:], np.cumsum(nn)[:-1])
    run = lambda lst: run_gpu(abi, pos, types, L, lst, 2.0, 0.1, 40, 0, dtype, virial=True, **SETS[name])
    base = run(lists["compact"])
    r = reference(pos, types, L, nl, 2.0, 0.1, 40, 0, bias=0.9, **SETS[name])
    compare(base, r, 0.9, dtype, types=types)
    for kind in ll.OTHER_KINDS:
        got = run(lists[kind])
        for key in OUTPUTS:
            assert np.array_equal(got[key], base[key]), (kind, key)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(SETS))
def test_rows_of_every_length(abi, dtype, name):
    case = ll.sweep("pe", dtype)
    pos, types, L, nl = case["pos"], case["types"], case["L"], case["nl"]
    par = ll.PE_SWEEP["par"]
    nn = np.asarray(nl[1])[:case["n_members"]]
    assert set(nn.tolist()) == set(range(3 * 8 + 2))                     # rows of 0 .. 25 entries
    kw = dict(SETS[name])
    if "average" in kw:
        kw = dict(average=(1.0, 1.6), switch=(28.0, 6))                   # (the median of -sbar_i in the clumps is 31)
    r = reference(pos, types, L, nl, *par, 0, bias=ll.BIAS, **kw)
    clean = run_gpu(abi, pos, types, L, nl, *par, 0, dtype, virial=True, bias=ll.BIAS, **kw)
    compare(clean, r, ll.BIAS, dtype, types=types)
    padded = run_gpu(abi, pos, types, L, ll.padded(case, ghosts=True), *par, 0, dtype, virial=True, bias=ll.BIAS, **kw)
    compare(padded, r, ll.BIAS, dtype, types=types)
