"""GPU: the stream contract of the bond-orientational order (mtd_hex_*).  Their stream travels inside mtd_hex_call, so the header-driven
table of tests/stream_coverage.py cannot see them; these are their cases, through the same gate (tests/stream_gate.py): the calls are
queued on a non-blocking stream behind a delay while every input buffer still holds another legal snapshot, and every output must be,
bit for bit, what the NULL stream gives for the snapshot that arrives behind the delay — and differ from the other snapshot's.

The file is named to be collected BEHIND tests/test_gpu_streams.py, not beside the unit's other tests: the negative controls at the head
of tests/test_gpu_streams.py depend on which stream of torch's pool a gate gets."""
import numpy as np
import pytest

import hexatic_ref as hr
import stream_gate
from test_gpu_hexatic import OUTPUTS, SNAPSHOTS, noisy, params, run_gpu

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _snapshots():
    kws = []
    for noise, bias in ((0.05, 0.9), (0.08, -1.7)):
        pos, L = noisy("layer", 12, sigma=noise)
        kws.append(dict(pos=pos, types=(np.arange(len(pos)) % 4 == 3).astype(np.int32), L=L,
                        nl=hr.box_nlist(pos, L, SNAPSHOTS["layer"]["r_cut"]), bias=bias))
    return kws


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["plain", "switch+gate", "global"])
def test_accumulate_finalize_and_forces_on_a_callers_stream(abi, dtype, name):
    """all launches of the three entry points of a step (walk, sums, finalize — in global mode the adjoint rows — second walk), with
    the virial"""
    kws = _snapshots()
    par = params("layer", name)

    def run(pos, types, L, nl, bias, gate=None):
        return run_gpu(abi, pos, types, L, nl, par, dtype, virial=True, bias=bias, gate=gate)

    got, want, gate = stream_gate.check("mtd_hex_accumulate + _finalize + _forces [%s, %s]" % (np.dtype(dtype).name, name), run, kws[0],
                                        kws[1], keys=OUTPUTS)
    assert np.abs(got["F"]).max() > 0 and np.abs(got["virial"]).max() > 0
