"""GPU: mtd_comm_allreduce_pull, the shared buffers under it and mtd_comm_allreduce_small, directly through the C ABI between ranks
(separate processes on cuda:0 as in tests/test_gpu_comm.py; worker: tests/_pull_worker.py).

What the header promises is a sum "in rank order … same bits on every rank", so every comparison here is on BITS against
tests/pull_ref.py::rank_order_sum (checked on the CPU by tests/test_pull_ref.py: its inputs make another order of the additions
visible), on NaN-ness where the expectation is NaN, on 64 sentinel doubles behind every buffer, on return codes and on the timeout
counter.  There is no tolerance in this file.  Every rank computes all ranks' inputs and the expectation itself, so "equal to the
expectation on every rank" is also "the same bits on every rank"."""
import ctypes as C
import time

import numpy as np
import pytest

import pull_ref as pr
from test_gpu_comm import _run_world

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, TIMEOUT = -1, -2, -4


def clean(v, what):
    assert v["bad_bits"] == 0 and v["bad_nan"] == 0 and v["sentinels_ok"], (what, v)


@pytest.fixture(scope="module", params=[2, 3, 4])
def launch(request):
    """ONE launch per world: every scenario runs in it, the tests below read its report"""
    world = request.param
    t0 = time.time()
    r = _run_world(world, 0, worker="_pull_worker.py", timeout=240)
    print("pull worker, world %d: %.2f s wall; rank 0 after start-up: %s, late-rank delay %s" % (
        world, time.time() - t0, r["ranks"][0].get("phase_seconds"), r["ranks"][0].get("delay")) if r.get("connected") else "not connected: %s" % r)
    assert r["connected"], "the mailbox could not be set up between processes on this box"
    assert r["world"] == world and [x["rank"] for x in r["ranks"]] == list(range(world))
    return r


def test_refusals_and_setup(launch):
    """argument refusals of mtd_comm_allreduce_pull / _pull_attach / _share / _open on every rank; none of them touches a buffer or
    leaves the communicator unusable (the pull that follows is right); a second mtd_comm_open of a slot returns the first one's addresses"""
    for x in launch["ranks"]:
        assert x["refusals"] == {k: INVALID for k in (
            "pull_before_attach", "pull_null_comm", "pull_null_buffer", "pull_count_zero", "share_zero_bytes", "attach_null_in_peer",
            "attach_null_out_peer", "attach_zero_doubles", "attach_null_comm", "attach_null_arrays", "pull_after_refused_attach",
            "pull_above_capacity", "open_unknown_slot")}, x["refusals"]
        assert x["attach"] == 0 and x["refused_calls_left_the_buffer"]
        assert x["pull_bytes"] == [(8 * pr.CAP + 255) // 256 * 256, 256, 256, 512]
        assert x["local_is_own_peer"] and x["peers_distinct"]
        assert x["reopen_rc"] == 0 and x["reopen_same"]
        v = x["after_refusal"]
        assert v["rc"] == 0 and v["timeouts"] == 0
        clean(v, "the exchange after the refused ones")


def test_every_count(launch):
    """one synchronised call per length of pull_ref.COUNTS: empty slices, a partial last slice, full slices, the grid-stride wrap of
    the stage / gather launches (and of the reduce launch at two ranks), capacity - 1 and the capacity itself"""
    world = launch["world"]
    for x in launch["ranks"]:
        assert [v["count"] for v in x["counts"]] == pr.COUNTS(world)
        for v in x["counts"]:
            assert v["rc"] == 0 and v["timeouts"] == 0, (x["rank"], v)
            clean(v, (x["rank"], v["count"]))


def test_back_to_back_with_a_late_rank(launch):
    """two rounds of cap, 1, 33, cap - 1, 32·world, 7 with small all-reduces (3 doubles, the largest that fits) and a barrier in
    between, no host synchronisation until the end, rank k mod world about a millisecond late in front of call k: the re-use of the
    staging and slice buffers without further barriers (comm.hip), and both all-reduces bitwise"""
    world = launch["world"]
    for x in launch["ranks"]:
        r = x["rounds"]
        assert [c["count"] for c in r["calls"]] == pr.back_to_back(world) * 2 and r["n_max"] == pr.small_max(world)
        assert r["timeouts"] == 0 and r["barrier_token"] == 0.0
        for k, c in enumerate(r["calls"]):
            assert c["rc"] == [0, 0, 0], (x["rank"], k, c)
            for key in ("pull", "small3", "small_max"):
                clean(c[key], (x["rank"], k, c["count"], key))
        assert 50000 <= x["delay"]["cycles"] <= 3000000


def test_refused_small_allreduce_leaves_the_communicator_usable(launch):
    """mtd_comm_allreduce_small refuses n = 3751 at two ranks (MTD_ERR_UNSUPPORTED: the kernel's image of the message exceeds its
    local memory) on both ranks, and the 20 exchanges of n = 3750 that follow, with a late rank each, are bitwise right without a timeout.
    A refused call takes no exchange number (comm.hip): had it taken one, the next exchange would re-use the slot parity of the last
    one, and a peer one exchange ahead could store into the buffer a slower rank still polls.  This test CANNOT detect that skipped
    parity deterministically — both ranks refuse alike and stay in step, and the overwrite needs a peer a whole exchange ahead; the fix
    rests on the protocol's own argument (comm_device.hpp).  What is pinned here is that a refusal leaves the communicator usable."""
    if launch["world"] != 2:
        assert all("refused_small" not in x for x in launch["ranks"])
        return
    for x in launch["ranks"]:
        r = x["refused_small"]
        assert r["n"] == 3750 and r["rc_refused"] == UNSUPPORTED and r["refused_buffer_untouched"]
        assert r["rcs"] == [0] * 20 and r["timeouts"] == 0
        for k, v in enumerate(r["results"]):
            clean(v, (x["rank"], k))


def test_slot_cap(launch):
    """MTD_COMM_MAX_SHARED = 8 buffers per communicator: the ninth mtd_comm_share is refused on every rank (MTD_ERR_UNSUPPORTED),
    allocates nothing, and the pull all-reduce still works"""
    for x in launch["ranks"]:
        s = x["slot_cap"]
        assert s["rcs"] == [0] * 6 and s["slots"] == [2, 3, 4, 5, 6, 7] and s["addresses_distinct"]
        assert s["rc_ninth"] == UNSUPPORTED and not s["ninth_local"]
        assert s["reopen_rc"] == 0 and s["reopen_same"]
        assert s["pull"]["rc"] == 0 and s["pull"]["timeouts"] == 0
        clean(s["pull"], "pull with every slot taken")
        assert x["timeouts"] == 0


def test_single_rank_is_the_identity(abi):
    """world == 1: the sum over one rank — MTD_SUCCESS on a communicator that was never attached, whatever the count, and the buffer keeps
    its bits (-0.0, NaN payloads and denormals included)"""
    lib = abi.load()
    h = C.c_void_p()
    abi.check(lib.mtd_comm_create(C.byref(h), 0, 1, 8))
    try:
        x = pr.inputs(1000, 0, 77, 1)
        x.view(np.uint64)[17] = 0x7ff8c0de00000123                       # (not arithmetic: nothing may look at the values)
        host = np.concatenate([x, pr.sentinels()])
        t = torch.from_numpy(host.copy()).cuda()
        for count in (1, 33, 1000):
            assert lib.mtd_comm_allreduce_pull(h, t.data_ptr(), count, None) == 0
        assert lib.mtd_comm_allreduce_pull(h, t.data_ptr(), 0, None) == INVALID
        assert lib.mtd_comm_allreduce_pull(h, None, 1, None) == INVALID
        torch.cuda.synchronize()
        assert np.array_equal(pr.bits(t.cpu().numpy()), pr.bits(host))
        n = C.c_uint(7)
        abi.check(lib.mtd_comm_status(h, C.byref(n), None))
        assert n.value == 0
    finally:
        abi.check(lib.mtd_comm_destroy(h))


def test_silent_peer_poisons_the_pull():
    """A peer that never arrives (run ONCE, bounded in-kernel waits of 200 ms as in test_mailbox_timeout_is_fatal; rank 1's buffers stay
    mapped throughout): the call itself returns 0 at launch, all 1000 results carry the communication poison (upper word 0x7ff8c0de
    after masking the sign), the sentinels are untouched, the timeout counter is up, and the next pull returns MTD_ERR_COMM_TIMEOUT
    without touching its buffer"""
    t0 = time.time()
    r = _run_world(2, 1, extra_env={"MTD_COMM_TIMEOUT_MS": "200"}, worker="_pull_worker.py", timeout=240)
    print("pull worker, silent peer: %.2f s wall" % (time.time() - t0))
    assert r["connected"]
    for x in r["ranks"]:
        assert x["attach"] == 0 and x["good"]["rc"] == 0 and x["good"]["timeouts"] == 0
        clean(x["good"], "the good pull before")
    assert "expired" not in r["ranks"][1]
    e = r["ranks"][0]["expired"]
    assert e["rc_launch"] == 0
    assert e["n"] == 1000 and e["poisoned"] == 1000
    assert e["sentinels_ok"]
    assert e["timeouts"] > 0
    assert e["rc_next"] == TIMEOUT and e["next_untouched"] and e["rc_small"] == TIMEOUT
