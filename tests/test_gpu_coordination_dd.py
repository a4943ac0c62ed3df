"""GPU: cv.coordination in a DOMAIN-DECOMPOSED constant-pressure run (two ranks, separate processes sharing cuda:0, z slabs with ghost
particles, full lists: tests/_cn_dd_worker.py).  The plain A-B variable: its only exchange is the all-reduce of two sums (sum n_i and
N_A), so the value is the same bits on both ranks and the single-domain restatement's to 1e-10 relative; every rank writes the rows of its
local particles — forces, n_i and per-particle virial are the single-domain rows to 1e-9 — and the ranks' virial sums add up to the
single-domain sums to 1e-9 of max|W|.  With a switch the variable raises on both ranks."""
import pytest

from test_gpu_comm import _run_world

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def test_coordination_domain_decomposed():
    r = _run_world(2, 0, worker="_cn_dd_worker.py", timeout=300)
    assert r["connected"], "the mailbox could not be set up between processes on this box"
    v = r["cn"]
    print(v)
    assert v["timeouts"] == 0 and v["locals_total"] == v["rows_total"] == v["n_global"] and v["ghosts_total"] > 0, v
    assert len(set(v["value_bits"])) == 1, v
    assert v["cv_rel"] <= 1e-10 and v["max_W"] > 0.05 and abs(v["umbrella_part"]) > 0.1 * abs(v["bias"]), v
    assert v["per_particle_rel"] <= 1e-9, v
    assert v["sum_rel"] <= 1e-9, v
    assert v["force_rel"] <= 1e-9, v
    assert v["local_rel"] <= 1e-9, v
    assert v["switch_refused_on"] == 2, v
