"""GPU: the stream contract of the largest-cluster entry points of the coordination number and the tetrahedral order
(mtd_coord_accumulate_cluster, mtd_tetrahedral_accumulate_cluster).  Their stream travels inside the call block, so the header-driven table of
tests/stream_coverage.py cannot see them; these are their cases, through the same gate (tests/stream_gate.py): the calls are queued on a
non-blocking stream behind a delay while every input buffer still holds another legal snapshot, and every output — the cluster pass's
among them — must be, bit for bit, what the NULL stream gives for the snapshot that arrives behind the delay, and differ from the other
snapshot's.

The file is named to be collected BEHIND tests/test_gpu_streams.py, not beside the units' other tests: the negative controls at the head
of tests/test_gpu_streams.py depend on which stream of torch's pool a gate gets."""
import numpy as np
import pytest

import row_cluster_gpu as rg
import row_cluster_ref as rc
import stream_gate
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CASES = {
    "coordination": (lambda: rc.coordination_case("switch+less"), rc.COORD_LIST, rg.OUTPUTS),
    "tetrahedral": (lambda: rc.tetrahedral_case("switch+gate"), rc.TET_LIST, rg.OUTPUTS + ("coordination",)),
}


@pytest.mark.parametrize("kind", list(CASES))
def test_accumulate_cluster_finalize_and_forces_on_a_callers_stream(abi, kind):
    """all launches of the step: the walk, the five of the cluster pass, the mask step, the sums, finalize, the second walk, with the virial"""
    case, r_list, keys = CASES[kind]
    c = case()
    order = np.arange(len(c["pos"]))[::-1]                               # the other legal snapshot: other indices, other positions, other bias
    pos_a = c["pos"][order] + np.random.default_rng(2).normal(0, 0.01, c["pos"].shape)
    a = dict(pos=pos_a, types=c["types"][order], L=c["L"], nl=util.build_nlist(pos_a, c["L"], r_list), bias=-1.7)
    b = dict(pos=c["pos"], types=c["types"], L=c["L"], nl=c["nl"], bias=0.9)

    def run(pos, types, L, nl, bias, gate=None):
        return rg.run(abi, kind, pos, types, L, nl, c["par"], np.float64, cluster=c["cluster"], bias=bias, gate=gate)

    got, want, gate = stream_gate.check("mtd_%s_accumulate_cluster + _finalize + _forces" % ("coord" if kind == "coordination" else "tetrahedral"), run,
                                        a, b, keys=keys)
    assert np.abs(got["F"]).max() > 0 and np.abs(got["virial"]).max() > 0 and got["summary"][1] > 1
