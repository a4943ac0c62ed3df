"""CPU: the pure parts of tests/stream_gate.py — how a delay is sized, how two snapshots share one buffer, how results are compared."""
import os
import re

import numpy as np
import pytest

import stream_gate as sg


def test_delay_is_ten_times_the_host_time_inside_its_clamps():
    assert sg.delay_ms(0.0) == 20.0 and sg.delay_ms(1.999) == 20.0       # below the floor
    assert sg.delay_ms(2.0) == 20.0 and sg.delay_ms(2.5) == 25.0 and sg.delay_ms(37.25) == 372.5
    assert sg.delay_ms(50.0) == 500.0 and sg.delay_ms(1e6) == 500.0      # the cap
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sg.delay_ms(bad)


def test_delay_units_round_up_and_never_vanish():
    assert sg.delay_units(20.0, 1e5) == 2_000_000
    assert sg.delay_units(20.0, 0.26) == 6 and sg.delay_units(1e-9, 1e-3) == 1
    for bad in (0.0, -3.0, float("nan")):
        with pytest.raises(ValueError):
            sg.delay_units(20.0, bad)


def test_snapshots_of_one_input_share_one_shape():
    a, b = np.arange(5, dtype=np.int32), np.arange(8, dtype=np.int32) + 1
    pa, pb = sg.common_shape(a, b)
    assert pa.shape == pb.shape == (8,) and np.array_equal(pa[:5], a) and not pa[5:].any() and np.array_equal(pb, b)
    pb2, pa2 = sg.common_shape(b, a)
    assert np.array_equal(pa2, pa) and np.array_equal(pb2, pb)
    x = np.zeros((3, 4))
    assert sg.common_shape(x, x + 1)[1][0, 0] == 1.0
    with pytest.raises(ValueError):
        sg.common_shape(np.zeros((3, 4)), np.zeros((4, 4)))              # only 1-d arrays are padded
    with pytest.raises(ValueError):
        sg.common_shape(np.zeros(3, dtype=np.float32), np.zeros(3))
    with pytest.raises(ValueError):
        sg.pad_to(np.zeros(9), 8)


def test_comparisons_are_bitwise_and_per_key():
    a = dict(x=np.array([0.0, 1.0]), y=np.float64(2.0), z=None)
    b = dict(x=np.array([-0.0, 1.0]), y=np.float64(2.0), z=None)
    assert sg.differing_keys(a, b) == ["x"]                              # -0.0 == 0.0, but not the same bits
    assert sg.differing_keys(a, b, keys=["y"]) == []
    sg.assert_same_bits(a, dict(a), "same")
    with pytest.raises(AssertionError, match="differ from the NULL-stream result"):
        sg.assert_same_bits(b, a, "case")
    with pytest.raises(AssertionError, match="a stale input could pass"):
        sg.assert_all_differ(a, b, "case")                               # y is the same in both
    sg.assert_all_differ(a, b, "case", keys=["x"])
    nan = dict(x=np.array([np.nan]))
    assert sg.differing_keys(nan, dict(x=np.array([np.nan]))) == []      # the same NaN is the same bits
    t = (np.arange(3), np.float64(1.5))
    assert sg.differing_keys(t, (np.arange(3), np.float64(2.5))) == [1]


def test_every_entry_point_with_a_stream_is_accounted_for():
    """every function of include/mtd_abi.h with a mtd_stream_t argument has a line in tests/stream_coverage.py: the case of
    tests/test_gpu_streams.py that puts it on a stream of its own, or the reason it has none"""
    import stream_coverage as sc
    here = os.path.dirname(os.path.abspath(__file__))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(here), "include", "mtd_abi.h")).read(), flags=re.S)
    takes_stream = [m.group(1) for m in re.finditer(r"\b(mtd_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S) if "mtd_stream_t" in m.group(2)]
    assert len(takes_stream) > 60 and len(set(takes_stream)) == len(takes_stream)
    assert sorted(takes_stream) == sorted(sc.COVERAGE), set(takes_stream) ^ set(sc.COVERAGE)
    tests = set(re.findall(r"^def (test_\w+)\(", open(os.path.join(here, "test_gpu_streams.py")).read(), flags=re.M))
    for name, where in sc.COVERAGE.items():
        if where != sc.MULTI_PROCESS:
            assert re.match(r"test_\w+", where).group(0) in tests, (name, where)
