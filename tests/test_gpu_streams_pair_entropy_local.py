"""GPU: the stream contract of mtd_pel_accumulate and mtd_pel_forces.  Their stream travels inside mtd_pel_call, so the header-driven
table of tests/stream_coverage.py cannot see them; this is their case, through the same gate (tests/stream_gate.py): the two calls are
queued on a non-blocking stream behind a delay while every input buffer still holds another legal snapshot, and every output must be,
bit for bit, what the NULL stream gives for the snapshot that arrives behind the delay — and differ from the other snapshot's.

The file is named to be collected directly BEHIND tests/test_gpu_streams.py, not beside the unit's other tests.  Every gate takes the next
stream of torch's pool, and the runtime spreads those streams over a few hardware queues, one of which the NULL stream uses too.  The
negative controls at the head of tests/test_gpu_streams.py need a stream that does NOT share the NULL stream's queue (their NULL-stream
call must run while the gated stream waits): with four more gates in front of them in the same process,
test_control_scale_on_the_null_stream_leaves_b_unscaled got such a stream and failed, twice in two runs of the whole suite, while it
passes on its own.  Behind that file nothing depends on which stream a gate gets."""
import numpy as np
import pytest

import stream_gate
import util
from test_gpu_pair_entropy_local import OUTPUTS, noisy_fcc, run_gpu

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SETS = {"plain": dict(), "both": dict(average=(1.2, 1.5), switch=(2.0, 6))}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(SETS))
def test_accumulate_and_forces_on_a_callers_stream(abi, dtype, name):
    """all launches of both entry points (count, accumulate, average; adjoint, forces) and the lazily built smoothing table"""
    kws = []
    for noise, bias in ((0.05, 0.9), (0.13, -1.7)):
        pos, L = noisy_fcc(5, sigma=noise)
        kws.append(dict(pos=pos, types=np.zeros(len(pos), dtype=np.int32), L=L, nl=util.build_nlist(pos, L, 2.4), bias=bias))

    def run(pos, types, L, nl, bias, gate=None):
        return run_gpu(abi, pos, types, L, nl, 2.0, 0.1, 40, 0, dtype, virial=True, bias=bias, gate=gate, **SETS[name])

    got, want, gate = stream_gate.check("mtd_pel_accumulate + mtd_pel_forces [%s, %s]" % (name, np.dtype(dtype).name), run, kws[0], kws[1],
                                        keys=OUTPUTS)
    assert np.abs(got["F"]).max() > 0 and np.abs(got["virial"]).max() > 0
