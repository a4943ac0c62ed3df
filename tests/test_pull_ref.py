"""CPU: the reference, the slice layout, the inputs and the lengths that tests/test_gpu_comm_pull.py runs the mailbox's all-reduces
against (tests/pull_ref.py) are themselves checked here — above all that the generated inputs let a bitwise comparison SEE a sum
taken in another order, and that the lengths reach every kind of slice layout (empty slices, a partial last slice, full slices)."""
import numpy as np
import pytest

import pull_ref as pr

WORLDS = range(1, 9)


def test_rank_order_sum_is_a_left_fold_from_plus_zero():
    a, b, c = np.array([2.0 ** -60, -0.0, 1.0]), np.array([1.0, -0.0, 2.0 ** 53]), np.array([-1.0, -0.0, -2.0 ** 53])
    s = pr.rank_order_sum([a, b, c])
    assert pr.bits(s).tolist() == [0, 0, 0]                          # (2^-60 + 1) - 1 = 0, +0 + -0 … = +0, (1 + 2^53) - 2^53 = 0
    r = pr.rank_order_sum([c, b, a])
    assert r.tolist() == [2.0 ** -60, 0.0, 1.0] and pr.bits(r)[1] == 0   # the other order keeps what the first one loses
    assert pr.bits(pr.rank_order_sum([np.array([-0.0])]))[0] == 0                      # one rank: still +0.0 + x


@pytest.mark.parametrize("world", WORLDS)
def test_slices_partition_the_buffer(world):
    for count in list(range(1, 301)) + pr.COUNTS(world):
        sl = pr.slices(count, world)
        c = pr.chunk(count, world)
        assert len(sl) == world and c % 32 == 0 and c * world >= count and (c - 32) * world < count, (count, world)
        pos = 0
        for r, (lo, hi) in enumerate(sl):
            assert lo == pos and lo <= hi <= count and hi - lo <= c, (count, world, r)
            assert (lo, hi) == (r * c, min((r + 1) * c, count)) or (r * c >= count and lo == hi == count), (count, world, r)
            pos = hi
        assert pos == count, (count, world)


@pytest.mark.parametrize("world", range(2, 9))
def test_counts_reach_every_slice_layout(world):
    counts = pr.COUNTS(world)
    assert counts[-1] == pr.CAP and pr.CAP - 1 in counts and pr.STRIDE + 77 in counts
    kinds = dict(empty=False, partial=False, full=False)
    for count in counts:
        lens = [hi - lo for lo, hi in pr.slices(count, world)]
        c = pr.chunk(count, world)
        if 0 in lens:
            kinds["empty"] = True
        last = [n for n in lens if n][-1]
        if last < c:
            kinds["partial"] = True
        if all(n == c for n in lens):
            kinds["full"] = True
    assert all(kinds.values()), (world, kinds)
    if world == 2:                                                   # the reduce launch wraps: one slice exceeds a sweep
        assert max(hi - lo for lo, hi in pr.slices(pr.CAP, 2)) > pr.STRIDE
    assert all(c > pr.STRIDE for c in counts[-3:])                   # stage and gather wrap


def test_planted_specials():
    world, count, seed = 3, 33, 5
    xs = [pr.inputs(count, r, seed, world) for r in range(world)]
    s = pr.rank_order_sum(xs)
    assert all(np.signbit(x[pr.I_NEG_ZERO]) and x[pr.I_NEG_ZERO] == 0 for x in xs) and pr.bits(s)[pr.I_NEG_ZERO] == 0
    assert s[pr.I_DENORMAL] == 6 * 5e-324 and 0 < s[pr.I_DENORMAL] < np.finfo(np.float64).tiny
    assert s[pr.I_INF] == np.inf and sum(np.isinf(x[pr.I_INF]) for x in xs) == 1
    assert np.isnan(s[pr.I_INF_PAIR]) and not any(np.isnan(x[pr.I_INF_PAIR]) for x in xs)
    assert np.isnan(s[pr.I_NAN]) and sum(np.isnan(x[pr.I_NAN]) for x in xs) == 1
    assert xs[0][pr.I_CANCEL] == -xs[-1][pr.I_CANCEL] and abs(xs[0][pr.I_CANCEL]) > 2.0 ** 35
    two = [pr.inputs(count, r, seed, 2) for r in range(2)]
    assert pr.bits(pr.rank_order_sum(two))[pr.I_CANCEL] == 0
    assert int(np.isnan(s).sum()) == 2
    # a count below an index plants nothing there, and never writes behind the end
    assert len(pr.inputs(1, 0, seed, world)) == 1 and len(pr.inputs(7, 2, seed, world)) == 7
    # the same arguments give the same array, another rank or seed another one
    assert np.array_equal(pr.bits(pr.inputs(40, 1, 9, 4)), pr.bits(pr.inputs(40, 1, 9, 4)))
    assert not np.array_equal(pr.bits(pr.inputs(40, 1, 9, 4)), pr.bits(pr.inputs(40, 2, 9, 4)))
    assert not np.array_equal(pr.bits(pr.inputs(40, 1, 9, 4)), pr.bits(pr.inputs(40, 1, 10, 4)))


@pytest.mark.parametrize("world", range(3, 9))
def test_a_wrong_order_shows_in_the_bits(world):
    """the condition that lets the GPU comparison see a reduce that adds the ranks in another order: at every listed length of 31
    or more — with the seeds the GPU test uses — the rank-order sum and the reverse-order sum differ in at least one FINITE element"""
    for i, count in enumerate(pr.COUNTS(world)):
        if count < 31:
            continue
        xs = [pr.inputs(count, r, pr.SEED_COUNTS + i, world) for r in range(world)]
        fwd, rev = pr.rank_order_sum(xs), pr.rank_order_sum(xs[::-1])
        finite = np.isfinite(fwd) & np.isfinite(rev)
        differ = finite & (pr.bits(fwd) != pr.bits(rev))
        assert differ.any(), (world, count)
        # and within EVERY non-empty slice of 31 or more elements, so that one rank's wrong order cannot hide
        for lo, hi in pr.slices(count, world):
            if hi - lo >= 31:
                assert differ[lo:hi].any(), (world, count, lo, hi)


def test_compare_counts_bits_and_nans():
    want = np.array([1.0, np.nan, 0.0, np.inf])
    assert pr.compare(want.copy(), want) == dict(bad_bits=0, bad_nan=0, first_bad=[])
    other_nan = want.copy()
    other_nan.view(np.uint64)[1] = 0x7ff8c0de00000000                # another NaN payload is still NaN
    assert pr.compare(other_nan, want)["bad_nan"] == 0 and pr.compare(other_nan, want)["bad_bits"] == 0
    assert pr.compare(np.array([1.0, np.nan, -0.0, np.inf]), want) == dict(bad_bits=1, bad_nan=0, first_bad=[2])
    assert pr.compare(np.array([np.nan, 1.0, 0.0, np.inf]), want) == dict(bad_bits=1, bad_nan=2, first_bad=[0, 1])
    assert pr.compare(np.array([np.nextafter(1.0, 2.0), np.nan, 0.0, np.inf]), want)["bad_bits"] == 1


def test_sentinels_and_small_max():
    s = pr.sentinels()
    assert len(s) == pr.SENTINELS == 64 and np.isfinite(s).all() and len(set(s.tolist())) == 64
    assert [pr.small_max(w) for w in (2, 3, 4)] == [3750, 2500, 1875]
    assert all(8 * pr.small_max(w) * w <= 60000 < 8 * (pr.small_max(w) + 1) * w for w in range(2, 9))
