"""GPU: the probe volume in a DOMAIN-DECOMPOSED run (two ranks, separate processes sharing cuda:0, no ghosts:
tests/_probe_volume_dd_worker.py), for a split that puts the region across the cut and a split that leaves one rank without particles,
through the entry points and through cv.probe_volume.  The only exchange is the all-reduce of the two sums.

What must hold.  Both ranks end with the same bits of value and count.  A particle's force and virial rows depend on its own position
alone: every rank's rows are the single-domain rows bit for bit.  The sharp count is a sum of small dyadic weights: exact, so equal.  The
value is the two-term fp64 sum of the rank totals, which commutes; but each rank total is summed over ANOTHER partition into threads and
blocks than the single-domain total, so the last bits may differ: the bound is 1e-12 sum_i |a_i|, and the test prints which happened.
Observed on an MI355X: see profiles/r30/README.md."""
import pytest

from test_gpu_comm import _run_world

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def test_probe_volume_domain_decomposed():
    r = _run_world(2, 0, worker="_probe_volume_dd_worker.py", timeout=300)
    assert r["connected"], "the mailbox could not be set up between processes on this box"
    a = r["abi"]
    print(a)
    assert a["straddling"] > 100 and a["straddling_right"] > 100, a      # the region lies across the cut
    for name in ("cut", "empty"):
        v = a[name]
        print("%s: value %.17g (single domain %.17g, same bits: %s), locals %s" % (name, v["value"], a["single_value"], v["value_same_bits_as_single"],
                                                                                  v["locals"]))
        assert len(set(v["value_bits"])) == 1 and len(set(v["count_bits"])) == 1, v
        assert all(v["rows_same_bits"]), v
        assert all(d == 0.0 for d in v["count_diff"]), v
        assert all(abs(d) <= 1e-12 * a["sum_abs"] for d in v["value_diff"]), v
    assert a["empty"]["locals"][1] == 0 and a["empty"]["locals"][0] == sum(a["cut"]["locals"]) and min(a["cut"]["locals"]) > 500
    assert a["empty"]["value_same_bits_as_single"]                        # one rank holds everything: the same partition, plus 0.0
    p = r["api"]
    print(p)
    assert p["timeouts"] == 0 and p["route"].startswith("generic"), p
    assert len(set(p["value_bits"])) == 1, p
    assert all(p["force_same_bits"]), p
    assert all(d == 0.0 for d in p["count_diff"]) and all(abs(d) <= 1e-12 * p["sum_abs"] for d in p["value_diff"]), p
    assert abs(p["bias"][0]) > 1e-3 and p["bias"][0] == p["bias"][1] and min(p["max_force"]) > 0.0, p
