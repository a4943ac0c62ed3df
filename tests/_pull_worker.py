"""Worker of tests/test_gpu_comm_pull.py: one rank of a world of processes that all use cuda:0, control plane gloo, everything else
through the C ABI (mtd_comm_share / _open / _pull_attach / _allreduce_pull / _allreduce_small).  Every rank computes all ranks'
inputs and the expected sums itself (tests/pull_ref.py) and reports what it found; rank 0 prints one JSON line with every rank's
report.  The assertions are in the test file.

    RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT from the environment; argv[1] = scenario (0: everything that must work,
    1: a peer that goes silent), argv[2] = spare
"""
import concurrent.futures
import ctypes as C
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "metadynamics-plugin_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch
import torch.distributed as dist

import pull_ref as pr
from metadynamics import _abi, xgmi

SENT = pr.sentinels()


def device(x):
    """x followed by the sentinels, on the device"""
    return torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float64), SENT])).cuda()


def verdict(t, want):
    """a device buffer after the call against the expectation: bits, NaN-ness, sentinels"""
    got = t.cpu().numpy()
    n = len(want)
    v = pr.compare(got[:n], want)
    v["sentinels_ok"] = bool(np.array_equal(pr.bits(got[n:]), pr.bits(SENT))) and len(got) == n + pr.SENTINELS
    return v


POOL = concurrent.futures.ThreadPoolExecutor(max_workers=4)


def expected(count, seed, world):
    """all ranks' inputs and their rank-order sum (the ranks' arrays on threads: generating them is most of this worker's time
    after start-up, and numpy's generators release the interpreter lock)"""
    xs = list(POOL.map(lambda r: pr.inputs(count, r, seed, world), range(world)))
    return xs, pr.rank_order_sum(xs)


def share_keeping_handles(lib, box, nbytes):
    """Mailbox.share, but the slot number and the gathered handles are kept for a second mtd_comm_open"""
    local, slot, h = C.c_void_p(), C.c_uint(), (C.c_ubyte * 64)()
    rc = lib.mtd_comm_share(box.handle, int(nbytes), C.byref(local), C.byref(slot), h)
    handles = torch.empty(box.world * 64, dtype=torch.uint8)
    dist.all_gather_into_tensor(handles, torch.frombuffer(bytearray(bytes(h)), dtype=torch.uint8))
    blob = handles.numpy().tobytes()
    peers = (C.c_void_p * box.world)()
    if rc == 0:
        rc = lib.mtd_comm_open(box.handle, slot.value, blob, peers)
    return rc, slot.value, blob, [peers[r] for r in range(box.world)]


def delay_cycles():
    """argument of torch.cuda._sleep for about a millisecond (the counter it spins on differs between devices: measured once)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    e0.record()
    torch.cuda._sleep(100000)
    e1.record()
    torch.cuda.synchronize()
    ms = max(e0.elapsed_time(e1), 1e-3)
    return int(min(max(100000 / ms, 50000), 3000000)), ms


def setup(lib, box, cap, out):
    """two exported buffers of the pull all-reduce, every refusal on the way"""
    world, rank = box.world, box.rank
    ref = out["refusals"] = {}
    probe = device(np.ones(4))
    before = probe.cpu().numpy().copy()
    ref["pull_before_attach"] = lib.mtd_comm_allreduce_pull(box.handle, probe.data_ptr(), 1, None)
    ref["pull_null_comm"] = lib.mtd_comm_allreduce_pull(None, probe.data_ptr(), 1, None)
    ref["pull_null_buffer"] = lib.mtd_comm_allreduce_pull(box.handle, None, 1, None)
    ref["pull_count_zero"] = lib.mtd_comm_allreduce_pull(box.handle, probe.data_ptr(), 0, None)
    local, slot, h = C.c_void_p(), C.c_uint(), (C.c_ubyte * 64)()
    ref["share_zero_bytes"] = lib.mtd_comm_share(box.handle, 0, C.byref(local), C.byref(slot), h)
    nbytes = lib.mtd_comm_pull_bytes(cap)
    out["pull_bytes"] = [int(nbytes), int(lib.mtd_comm_pull_bytes(1)), int(lib.mtd_comm_pull_bytes(32)), int(lib.mtd_comm_pull_bytes(33))]
    in_local, in_peers = box.share(dist, nbytes)
    out_local, out_peers = box.share(dist, nbytes)
    out["local_is_own_peer"] = in_peers[rank] == in_local and out_peers[rank] == out_local
    out["peers_distinct"] = len(set(in_peers + out_peers)) == 2 * world and all(in_peers + out_peers)
    a, b = (C.c_void_p * world)(*in_peers), (C.c_void_p * world)(*out_peers)
    holed = (C.c_void_p * world)(*in_peers)
    holed[(rank + 1) % world] = None
    ref["attach_null_in_peer"] = lib.mtd_comm_pull_attach(box.handle, cap, holed, b)
    ref["attach_null_out_peer"] = lib.mtd_comm_pull_attach(box.handle, cap, a, holed)
    ref["attach_zero_doubles"] = lib.mtd_comm_pull_attach(box.handle, 0, a, b)
    ref["attach_null_comm"] = lib.mtd_comm_pull_attach(None, cap, a, b)
    ref["attach_null_arrays"] = lib.mtd_comm_pull_attach(box.handle, cap, None, None)
    ref["pull_after_refused_attach"] = lib.mtd_comm_allreduce_pull(box.handle, probe.data_ptr(), 1, None)
    out["attach"] = lib.mtd_comm_pull_attach(box.handle, cap, a, b)
    ref["pull_above_capacity"] = lib.mtd_comm_allreduce_pull(box.handle, probe.data_ptr(), cap + 1, None)
    torch.cuda.synchronize()
    out["refused_calls_left_the_buffer"] = bool(np.array_equal(pr.bits(probe.cpu().numpy()), pr.bits(before)))
    # a second mtd_comm_open of an opened slot hands back the addresses of the first one and maps nothing anew (the handles it is
    # given are not looked at: a blob of zeros here, the real ones in slot_cap())
    again = (C.c_void_p * world)()
    out["reopen_rc"] = lib.mtd_comm_open(box.handle, 0, bytes(64 * world), again)
    out["reopen_same"] = [again[r] for r in range(world)] == in_peers
    ref["open_unknown_slot"] = lib.mtd_comm_open(box.handle, 2, bytes(64 * world), again)


def one_pull(lib, box, count, seed):
    xs, want = expected(count, seed, box.world)
    t = device(xs[box.rank])
    rc = lib.mtd_comm_allreduce_pull(box.handle, t.data_ptr(), count, None)
    torch.cuda.synchronize()
    v = verdict(t, want)
    v.update(count=count, rc=rc, timeouts=box.timeouts())
    return v


def rounds(lib, box, cap, out, cycles):
    """two rounds of pulls of different lengths with small all-reduces and a barrier in between, nothing waited for on the host until the
    end; in front of call k rank k mod world runs late"""
    world, rank = box.world, box.rank
    lengths = pr.back_to_back(world, cap) * 2
    n_max = pr.small_max(world)
    calls = []
    for k, count in enumerate(lengths):
        xs, want = expected(count, pr.SEED_ROUNDS + k, world)
        s3, want3 = expected(3, pr.SEED_SMALL + 2 * k, world)
        sn, wantn = expected(n_max, pr.SEED_SMALL + 2 * k + 1, world)
        calls.append(dict(count=count, t=device(xs[rank]), want=want, t3=device(s3[rank]), want3=want3, tn=device(sn[rank]), wantn=wantn))
    box.barrier()                                       # (creates the barrier's token before the timed part)
    torch.cuda.synchronize()
    dist.barrier()
    rcs = []
    for k, c in enumerate(calls):
        if k % world == rank:
            torch.cuda._sleep(cycles)
        rcs.append([lib.mtd_comm_allreduce_pull(box.handle, c["t"].data_ptr(), c["count"], None),
                    lib.mtd_comm_allreduce_small(box.handle, c["t3"].data_ptr(), 3, None),
                    lib.mtd_comm_allreduce_small(box.handle, c["tn"].data_ptr(), n_max, None)])
        box.barrier()
    torch.cuda.synchronize()
    res = []
    for c, rc in zip(calls, rcs):
        res.append(dict(count=c["count"], rc=rc, pull=verdict(c["t"], c["want"]), small3=verdict(c["t3"], c["want3"]),
                        small_max=verdict(c["tn"], c["wantn"])))
    out["rounds"] = dict(calls=res, timeouts=box.timeouts(), n_max=n_max, barrier_token=float(box._token.cpu()[0]))


def refused_small(lib, box, out, cycles):
    """world = 2: a small all-reduce refused for its size (n = 3751 does not fit the kernel's local memory), then 20 exchanges of the
    largest size that fits, with the late-rank pattern of rounds()"""
    world, rank = box.world, box.rank
    n = pr.small_max(world)
    big = device(np.ones(n + 1))
    rc_refused = lib.mtd_comm_allreduce_small(box.handle, big.data_ptr(), n + 1, None)
    calls = []
    for k in range(20):
        xs, want = expected(n, pr.SEED_REFUSED + k, world)
        calls.append((device(xs[rank]), want))
    torch.cuda.synchronize()
    dist.barrier()
    rcs = []
    for k, (t, _) in enumerate(calls):
        if k % world == rank:
            torch.cuda._sleep(cycles)
        rcs.append(lib.mtd_comm_allreduce_small(box.handle, t.data_ptr(), n, None))
    torch.cuda.synchronize()
    out["refused_small"] = dict(rc_refused=rc_refused, n=n, rcs=rcs, results=[verdict(t, want) for t, want in calls],
                                refused_buffer_untouched=bool((big.cpu().numpy()[:n + 1] == 1.0).all()), timeouts=box.timeouts())


def slot_cap(lib, box, out):
    """fill the shared-buffer slots (two are taken by the pull buffers), ask for one more, pull once more"""
    shared = []
    while len(shared) < 6:
        shared.append(share_keeping_handles(lib, box, 256))
    local, slot, h = C.c_void_p(), C.c_uint(), (C.c_ubyte * 64)()
    rc_ninth = lib.mtd_comm_share(box.handle, 256, C.byref(local), C.byref(slot), h)
    rc, s, blob, peers = shared[0]
    again = (C.c_void_p * box.world)()
    rc_again = lib.mtd_comm_open(box.handle, s, blob, again)                   # the real handles this time
    out["slot_cap"] = dict(rcs=[x[0] for x in shared], slots=[x[1] for x in shared], rc_ninth=rc_ninth, ninth_local=local.value,
                           reopen_rc=rc_again, reopen_same=[again[r] for r in range(box.world)] == peers,
                           addresses_distinct=len({p for x in shared for p in x[3]}) == 6 * box.world,
                           pull=one_pull(lib, box, 33, pr.SEED_CAP))


def everything(lib, box, out):
    world = box.world
    cap = pr.CAP
    phases, t = out.setdefault("phase_seconds", {}), time.time()

    def lap(name):
        nonlocal t
        phases[name], t = round(time.time() - t, 3), time.time()

    cycles, calib_ms = delay_cycles()
    out["delay"] = dict(cycles=cycles, ms_per_100000=calib_ms)
    setup(lib, box, cap, out)
    out["after_refusal"] = one_pull(lib, box, 33, pr.SEED_COUNTS - 1)
    lap("setup")
    out["counts"] = [one_pull(lib, box, count, pr.SEED_COUNTS + i) for i, count in enumerate(pr.COUNTS(world, cap))]
    lap("counts")
    rounds(lib, box, cap, out, cycles)
    lap("rounds")
    if world == 2:
        refused_small(lib, box, out, cycles)
        lap("refused_small")
    slot_cap(lib, box, out)
    out["timeouts"] = box.timeouts()
    lap("slot_cap")


def silent_peer(lib, box, out):
    """two ranks: one good pull, then rank 1 says nothing more while rank 0 pulls once — its bounded waits expire"""
    rank, world, n = box.rank, box.world, 1000
    nbytes = lib.mtd_comm_pull_bytes(n)
    _, in_peers = box.share(dist, nbytes)
    _, out_peers = box.share(dist, nbytes)
    out["attach"] = lib.mtd_comm_pull_attach(box.handle, n, (C.c_void_p * world)(*in_peers), (C.c_void_p * world)(*out_peers))
    out["good"] = one_pull(lib, box, n, pr.SEED_TIMEOUT)
    dist.barrier()
    if rank == 0:
        xs, _ = expected(n, pr.SEED_TIMEOUT + 1, world)
        t = device(xs[0])
        rc = lib.mtd_comm_allreduce_pull(box.handle, t.data_ptr(), n, None)
        torch.cuda.synchronize()                        # the waits expire (MTD_COMM_TIMEOUT_MS): it never hangs
        got = t.cpu().numpy()
        upper = (pr.bits(got[:n]) >> np.uint64(32)) & np.uint64(0x7fffffff)
        nxt = device(xs[0])
        rc_next = lib.mtd_comm_allreduce_pull(box.handle, nxt.data_ptr(), n, None)
        torch.cuda.synchronize()
        small = device(np.ones(1))
        out["expired"] = dict(rc_launch=rc, poisoned=int((upper == np.uint64(0x7ff8c0de)).sum()), n=n,
                              sentinels_ok=bool(np.array_equal(pr.bits(got[n:]), pr.bits(SENT))), timeouts=box.timeouts(),
                              rc_next=rc_next, next_untouched=bool(np.array_equal(pr.bits(nxt.cpu().numpy()), pr.bits(np.concatenate([xs[0], SENT])))),
                              rc_small=lib.mtd_comm_allreduce_small(box.handle, small.data_ptr(), 1, None))
    # rank 1 has been waiting here all along: its mailbox and its exported buffers stay mapped until rank 0 is done
    dist.barrier()


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    scenario = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    lib = _abi.load()
    t0 = time.time()
    box = xgmi.connect(dist, max_doubles=4096)
    if box is None:
        if rank == 0:
            print(json.dumps({"connected": False, "why": xgmi.last_failure()}), flush=True)
        dist.destroy_process_group()
        return
    out = {"rank": rank, "phase_seconds": {"connect": round(time.time() - t0, 3)}}
    (silent_peer if scenario == 1 else everything)(lib, box, out)
    torch.cuda.synchronize()
    out["seconds"] = time.time() - t0
    reports = [None] * world
    dist.all_gather_object(reports, out)
    dist.barrier()                                      # nobody closes its mailbox while a peer may still touch it
    box.close()
    if rank == 0:
        print(json.dumps({"connected": True, "world": world, "ranks": reports}), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
