#!/usr/bin/env python3
"""Developer tool: mtd_cluster_largest alone (csrc/cluster.hip) on the config 5 snapshot of tools/bench_ql_local.py (256 000-particle noisy
fcc crystal, list at 1.4, r_link 1.2) for three masks of solid particles: every particle (one cluster of 256 000: the worst case for the
link pass), a spherical nucleus of the given radii in an otherwise non-solid box (what the option is for), and nothing; prints us per
call and the summary.  usage: tools/bench_cluster.py [calls] [radius ...] [--r-list R]   (--r-list: the reach of the list, default 1.4; 1.5 and
2.4 are the lists of tools/bench_cn.py and tools/bench_tet.py, whose --cluster variants run this pass inside their step)
Run under rocprofv3 --kernel-trace --stats for the per-kernel table."""
import ctypes as C
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np
import torch
import util
from metadynamics import _abi as abi

argv = sys.argv[1:]
r_list = 1.4
if "--r-list" in argv:
    k = argv.index("--r-list")
    r_list = float(argv[k + 1])
    del argv[k:k + 2]
calls = int(argv[0]) if len(argv) > 0 else 200
radii = [float(x) for x in argv[1:]] or [6.0, 12.0]
pos, L = util.fcc_lattice(40)
pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
N = len(pos)
nl = util.build_nlist(pos, L, r_list)
lib = abi.load()
box = abi.Box.make(L)
d_pos = torch.from_numpy(util.pack_postype(pos, np.zeros(N, dtype=np.int32), np.float64)).cuda()
d_head, d_nn, d_nl = (torch.from_numpy(np.asarray(x).astype(np.int32)).cuda() for x in nl)
scratch = torch.zeros(lib.mtd_cluster_scratch_bytes(N), dtype=torch.uint8, device="cuda")
p = abi.ClusterParams.make((0.5, 1.2))
r = np.sqrt((pos * pos).sum(axis=1))
masks = [("every particle solid", np.ones(N))] + [("a nucleus of radius %g" % R, (r < R).astype(np.float64)) for R in radii] + [("nothing solid", np.zeros(N))]
print("N = %d, %.1f list entries per particle, %d calls each" % (N, len(nl[2]) / N, calls))
for name, v in masks:
    d_v = torch.from_numpy(v).cuda()
    ptrs = [C.c_void_p() for _ in range(4)]

    def call():
        abi.check(lib.mtd_cluster_largest(N, abi.ptr(d_pos), abi.MTD_F64, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), 0,
                                          abi.ptr(d_v), C.byref(p), abi.ptr(scratch), *[C.byref(x) for x in ptrs], None))
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        call()
    t1.record()
    torch.cuda.synchronize()
    at = ptrs[3].value - scratch.data_ptr()
    summary = scratch[at:at + 16].cpu().numpy().view(np.uint32)
    print("%-28s %8.1f us per call   (root, members, clusters, nodes) = %s" % (name, 1e3 * t0.elapsed_time(t1) / calls, tuple(int(x) for x in summary)))
