"""GPU: the stream contract of the Debye structure factor (mtd_dsf_*).  Their stream travels inside mtd_dsf_call, so the header-driven
table of tests/stream_coverage.py cannot see them; these are their cases, through the same gate (tests/stream_gate.py): the calls are
queued on a non-blocking stream behind a delay while every input buffer still holds another legal snapshot, and every output must be,
bit for bit, what the NULL stream gives for the snapshot that arrives behind the delay — and differ from the other snapshot's.

The file is named to be collected directly BEHIND tests/test_gpu_streams.py (and its neighbour for the local pair entropy), not beside the
unit's other tests: the negative controls at the head of tests/test_gpu_streams.py depend on which stream of torch's pool a gate gets."""
import numpy as np
import pytest

import stream_gate
import util
from test_gpu_debye import OUTPUTS, PEAKS, noisy_fcc, run_gpu

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _snapshots():
    kws = []
    for noise, bias in ((0.05, 0.9), (0.13, -1.7)):
        pos, L = noisy_fcc(5, sigma=noise)
        kws.append(dict(pos=pos, types=np.zeros(len(pos), dtype=np.int32), L=L, nl=util.build_nlist(pos, L, 2.4), bias=bias))
    return kws


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("store", [True, False], ids=["stored", "second_walk"])
def test_accumulate_finalize_and_forces_on_a_callers_stream(abi, dtype, store):
    """all launches of the three entry points of a step (walk, sums, finalize, scale — or the second walk), with the virial"""
    kws = _snapshots()
    q, c = PEAKS[3]

    def run(pos, types, L, nl, bias, gate=None):
        return run_gpu(abi, pos, types, L, nl, q, c, 2.4, 0, dtype, virial=True, bias=bias, gate=gate, store=store)

    got, want, gate = stream_gate.check("mtd_dsf_accumulate + _finalize + _forces [%s, %s]" % (np.dtype(dtype).name, store), run, kws[0], kws[1],
                                        keys=OUTPUTS)
    assert np.abs(got["F"]).max() > 0 and np.abs(got["virial"]).max() > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_spectrum_on_a_callers_stream(abi, dtype):
    """mtd_dsf_spectrum and mtd_dsf_spectrum_finalize behind a step on the same stream"""
    kws = _snapshots()
    q, c = PEAKS[1]

    def run(pos, types, L, nl, bias, gate=None):
        return run_gpu(abi, pos, types, L, nl, q, c, 2.4, 0, dtype, bias=bias, gate=gate, spectrum=(2.0, 14.0, 64))

    got, want, gate = stream_gate.check("mtd_dsf_spectrum + _spectrum_finalize [%s]" % np.dtype(dtype).name, run, kws[0], kws[1],
                                        keys=("spectrum", "spectrum_sums"))
    assert got["spectrum"].max() > 2.0
