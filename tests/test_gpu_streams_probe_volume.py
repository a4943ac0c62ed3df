"""GPU: the stream contract of the probe volume (mtd_probe_*).  Their stream travels inside mtd_probe_call, so the header-driven table of
tests/stream_coverage.py cannot see them; these are their cases, through the same gate (tests/stream_gate.py): the calls are queued on a
non-blocking stream behind a delay while every input buffer still holds another legal snapshot, and every output must be, bit for bit,
what the NULL stream gives for the snapshot that arrives behind the delay — and differ from the other snapshot's.

The file is named to be collected BEHIND tests/test_gpu_streams.py, not beside the unit's other tests: the negative controls at the head
of tests/test_gpu_streams.py depend on which stream of torch's pool a gate gets."""
import numpy as np
import pytest

import stream_gate
from test_gpu_probe_volume import COEFF16, OUTPUTS, SHAPES, make_snapshot, run_gpu

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _snapshots(shape, dtype):
    kws = []
    for seed, bias in ((1, 0.9), (2, -1.7)):
        s = make_snapshot(shape, 0.3, "tilted", dtype, seed=seed)
        kws.append(dict(pos=s["pos"], types=s["types"], L=s["L"], tilt=s["tilt"], reg=s["reg"], bias=bias))
    return kws


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_accumulate_finalize_forces_and_local_on_a_callers_stream(abi, shape, dtype):
    """all launches of a step: the sums kernel, the reduction of the block sums, the force pass with its virial, and the h_i pass"""
    kws = _snapshots(shape, dtype)

    def run(pos, types, L, tilt, reg, bias, gate=None):
        return run_gpu(abi, pos, types, L, reg, COEFF16, dtype, bias=bias, tilt=tilt, gate=gate)

    got, want, gate = stream_gate.check("mtd_probe_accumulate + _finalize + _forces + _local [%s, %s]" % (shape, np.dtype(dtype).name),
                                        run, kws[0], kws[1], keys=OUTPUTS)
    assert np.abs(got["F"]).max() > 0 and got["s"] != 0 and got["count"] != 0
