#!/usr/bin/env python3
"""Developer tool: the device neighbour-list build (csrc/nlist.hip) at the config-5 system (256 000-particle noisy fcc crystal).

  bench_nlist.py [--r-list 1.4] [--builds 30] [--steps 200] [--pairs 5] [--trace DIR]

Reports
  * the time of one rebuild: device events around mtd_nlist_build, median of --builds after warm-up, full and half, and its share
    of the compulsory traffic ((N_local + N_ghost) * 32 B read + entries * 4 B written) at 8 TB/s;
  * the host path it replaces, cv.nlist_cell(device=False).update() (KD-tree + host symmetry walk + upload): wall clock, median of 5;
  * the per-step time of context.run with a cv.steinhardt on a device-built list, check_period 1 and 10, static particles, against
    device=False with a static list: A/B/C alternating, --pairs rounds, the range of each;
  * with --trace DIR: the nlist kernels' rows of one `rocprofv3 --kernel-trace --stats` run of this script's --child mode (a few
    rebuilds and checks), profiler output under DIR."""
import argparse
import ctypes as C
import glob
import os
import subprocess
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np
import torch
import util
from metadynamics import _abi, context, cv, integrate

ap = argparse.ArgumentParser()
ap.add_argument("--r-list", type=float, default=1.4)
ap.add_argument("--builds", type=int, default=30)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--trace", default=None)
ap.add_argument("--child", action="store_true")
ap.add_argument("--skip-host", action="store_true")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_nlist.py needs a GPU")

pos, L = util.fcc_lattice(40)
pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
N = len(pos)
types = np.zeros(N, dtype=np.int32)
lib = _abi.load()
box = _abi.Box.make(L)
d_pos = torch.from_numpy(util.pack_postype(pos, types, np.float64)).cuda()
h = C.c_void_p()
_abi.check(lib.mtd_nlist_create(C.byref(h)))


def build(half):
    p = [C.c_void_p() for _ in range(3)]
    n = C.c_size_t()
    _abi.check(lib.mtd_nlist_build(h, N, 0, d_pos.data_ptr(), _abi.MTD_F64, C.byref(box), args.r_list, int(half), -1, C.byref(p[0]),
                                   C.byref(p[1]), C.byref(p[2]), C.byref(n), None))
    return n.value


def check():
    needs = C.c_int()
    _abi.check(lib.mtd_nlist_check(h, d_pos.data_ptr(), _abi.MTD_F64, C.byref(box), 0.4, C.byref(needs), None))
    return needs.value


if args.child:                       # under the profiler: a few rebuilds and checks, nothing else
    for _ in range(5):
        build(False)
        check()
    torch.cuda.synchronize()
    sys.exit(0)

for half in (False, True):
    for _ in range(5):
        entries = build(half)
    times = []
    for _ in range(max(20, args.builds)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        build(half)
        e1.record()
        e1.synchronize()
        times.append(1e3 * e0.elapsed_time(e1))
    times = np.array(times)
    floor_us = (N * 32 + entries * 4) / 8e12 * 1e6
    print("rebuild (%s, r_list %.2f): %d entries, median %.1f us (min %.1f, max %.1f, n = %d); compulsory traffic %.2f MB = %.2f us at 8 TB/s: share %.3f"
          % ("half" if half else "full", args.r_list, entries, np.median(times), times.min(), times.max(), len(times),
             (N * 32 + entries * 4) / 1e6, floor_us, floor_us / np.median(times)))
build(False)
times = []
for _ in range(50):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    check()
    times.append(1e6 * (time.perf_counter() - t0))
print("displacement check alone (launch + synchronise, host clock): median %.1f us (min %.1f)" % (np.median(times), min(times)))
device_us = None


def make(device, check_period, hi, sigma):
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=args.r_list, r_buff=0.0, check_period=check_period, device=device)
    if not device:
        nl.update()
    st = cv.steinhardt(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=[0, 0, 0, 0, 1, 0, 1], nlist=nl, type="A", sigma=sigma)
    st.set_grid(0.0, hi, 512)
    return context.current, meta, nl, st


if not args.skip_host:
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    nl = cv.nlist_cell(r_cut=args.r_list)
    host = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nl.update()
        torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
    nl_dev = cv.nlist_cell(r_cut=args.r_list, r_buff=0.0, device=True)
    dev = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nl_dev.cpp_nlist.forceRebuild()
        nl_dev.cpp_nlist.compute(0)
        torch.cuda.synchronize()
        dev.append(time.perf_counter() - t0)
    print("host path, nlist_cell(device=False).update(): median of 5 %.3f s (%s)" % (np.median(host), " ".join("%.3f" % x for x in host)))
    print("device path through NeighborList.compute (wall clock, warm): median %.1f us -> ratio %.0f x"
          % (1e6 * np.median(dev[2:]), np.median(host) / np.median(dev[2:])))
    context.current = None

# per-step cost of the check: the same step on a static list (device=False) and on a device-built one, r_buff 0 so that both
# lists hold the same pairs
ctx0, meta0, nl0, st0 = make(False, 1, 1.0, 1.0)
context.run(1)
s0 = st0.cpp_force.getCurrentValue(1)
context.current = None
variants = [("device=False (static list)", False, 1), ("device=True check_period=1", True, 1), ("device=True check_period=10", True, 10)]
built = []
for name, device, period in variants:
    ctx, meta, nl, st = make(device, period, 2.0 * s0, 0.02 * s0)
    context.run(20)
    built.append((name, ctx, nl))
results = {name: [] for name, _, _ in variants}
for _ in range(args.pairs):
    for name, ctx, nl in built:
        context.current = ctx
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.system.run(args.steps)
        torch.cuda.synchronize()
        results[name].append(1e6 * (time.perf_counter() - t0) / args.steps)
for name, ctx, nl in built:
    r = results[name]
    print("%-30s %s us/step: range %.1f - %.1f%s" % (name, " ".join("%.1f" % x for x in r), min(r), max(r),
                                                    "" if not nl.device else "  (rebuilds so far: %d)" % nl.cpp_nlist.getNumRebuilds()))
context.current = None
_abi.check(lib.mtd_nlist_destroy(h))

if args.trace:
    os.makedirs(args.trace, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.trace, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
           "--child", "--r-list", str(args.r_list)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("rocprofv3 failed:\n" + r.stderr[-3000:])
    for f in sorted(glob.glob(os.path.join(args.trace, "**", "*kernel_stats.csv"), recursive=True)):
        print("kernel table (%s), nlist kernels:" % os.path.basename(f).split("_", 1)[-1])
        lines = open(f).read().splitlines()
        print(lines[0])
        for line in lines[1:]:
            if "k_nl_" in line:
                print(line)
