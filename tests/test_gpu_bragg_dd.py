"""GPU: cv.bragg in a DOMAIN-DECOMPOSED run (two ranks, separate processes sharing cuda:0, the particles split 1 : 2 by index, no ghosts:
tests/_bragg_dd_worker.py), both forms on one grid under harmonic umbrellas.  The only exchange is the all-reduce of the 2K + 2 sums: the
value is the same bits on both ranks and the single-domain GPU result's to 1e-10 relative; every rank writes the rows of its local
particles, the single-domain rows to 1e-9 of max |F|."""
import pytest

from test_gpu_comm import _run_world

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def test_bragg_domain_decomposed():
    r = _run_world(2, 0, worker="_bragg_dd_worker.py", timeout=300)
    assert r["connected"], "the mailbox could not be set up between processes on this box"
    v = r["bragg"]
    print(v)
    assert v["timeouts"] == 0, v
    assert v["locals"] == [v["n_global"] // 3, v["n_global"] - v["n_global"] // 3] and v["route"].startswith("generic"), v
    for c in range(2):                                                   # the default form and the modulus form
        assert len(set(v["value_bits"][c])) == 1, v
        assert v["cv_rel"][c] <= 1e-10, v
        assert v["force_rel"][c] <= 1e-9 and v["force_w"][c] == 0.0, v
        assert abs(v["umbrella_part"][c]) > 0.1 * abs(v["bias"][c]) > 0.0, v
