"""GPU: the virial of cv.steinhardt's bias force in a DOMAIN-DECOMPOSED constant-pressure run (two ranks, separate processes sharing
cuda:0, z slabs with ghost particles, full lists: tests/_ql_virial_dd_worker.py).  Every rank writes the rows of its local particles —
they are the single-domain rows of the restatement to the parity bound of tests/test_gpu_ql_virial.py, 1e-9 of max|virial_i| — and the
ranks' sums add up to the single-domain sums to 1e-9 of max|W|."""
import pytest

from test_gpu_comm import _run_world

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def test_virial_domain_decomposed():
    r = _run_world(2, 0, worker="_ql_virial_dd_worker.py", timeout=300)
    assert r["connected"], "the mailbox could not be set up between processes on this box"
    v = r["virial"]
    print(v)
    assert v["timeouts"] == 0 and v["locals_total"] == v["rows_total"] == v["n_global"] and v["ghosts_total"] > 0, v
    assert v["cv_rel"] < 1e-10 and v["max_W"] > 0.05 and abs(v["umbrella_part"]) > 0.1 * abs(v["bias"]), v
    assert v["per_particle_rel"] <= 1e-9, v
    assert v["sum_rel"] <= 1e-9, v
    assert v["force_rel"] <= 1e-9, v
