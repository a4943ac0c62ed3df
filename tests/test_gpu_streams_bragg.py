"""GPU: the stream contract of the Bragg intensity (mtd_bragg_*).  Their stream travels inside mtd_bragg_call, so the header-driven table
of tests/stream_coverage.py cannot see them; these are their cases, through the same gate (tests/stream_gate.py): the calls are queued on
a non-blocking stream behind a delay while every input buffer still holds another legal snapshot, and every output must be, bit for bit,
what the NULL stream gives for the snapshot that arrives behind the delay — and differ from the other snapshot's.

The file is named to be collected BEHIND tests/test_gpu_streams.py, not beside the unit's other tests: the negative controls at the head
of tests/test_gpu_streams.py depend on which stream of torch's pool a gate gets."""
import numpy as np
import pytest

import stream_gate
from test_gpu_bragg import COEFF16, HARDWARE, OUTPUTS, VECTORS, make_snapshot, run_gpu

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _snapshots(dtype):
    kws = []
    for seed, bias in ((1, 0.9), (2, -1.7)):
        s = make_snapshot(4097, "ordered", "triclinic", dtype, seed=seed)
        kws.append(dict(pos=s["pos"], types=s["types"], L=s["L"], tilt=s["tilt"], bias=bias))
    return kws


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("modulus", [False, True])
def test_accumulate_finalize_and_forces_on_a_callers_stream(abi, dtype, modulus):
    """all launches of the three entry points of a step: the sums kernel, the reduction of the block sums, finalize, the force pass"""
    kws = _snapshots(dtype)

    def run(pos, types, L, tilt, bias, gate=None):
        return run_gpu(abi, pos, types, L, VECTORS[:9], COEFF16, dtype, None, modulus, HARDWARE, bias=bias, tilt=tilt, gate=gate)

    got, want, gate = stream_gate.check("mtd_bragg_accumulate + _finalize + _forces [%s, %s]" % (np.dtype(dtype).name, "modulus" if modulus else "default"),
                                        run, kws[0], kws[1], keys=OUTPUTS)
    assert np.abs(got["F"]).max() > 0 and got["s"] > 0
