"""Worker of tests/test_gpu_probe_volume_dd.py: one rank of a DOMAIN-DECOMPOSED evaluation of the probe volume, two ranks as separate
processes on cuda:0, no ghosts (the variable needs none).

Part "abi": the entry points with the mailbox's all-reduce between accumulate and finalize (tests/test_gpu_probe_volume.py: run_gpu with
its `reduce` hook), for two splits of one snapshot: "cut", the particles left and right of a plane through the region's centre, and
"empty", everything on rank 0 and n_particles = 0 on rank 1.  Value and count of every rank, and the force and virial rows of its local
particles, against the SINGLE-DOMAIN result of the same kernels on the whole snapshot in this process.
Part "api": cv.probe_volume in a metadynamics run of two steps on the "cut" split; the value, the count and the rows of the force array
at the bias factor the integrator reports.
Prints one JSON line on rank 0.   RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT from the environment.
"""
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "metadynamics-plugin_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch
import torch.distributed as dist

import probe_volume_ref as pv
from metadynamics import _abi, context, cv, integrate, xgmi
from test_gpu_probe_volume import run_gpu

KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
L = (16.0, 18.5, 15.0)
WEIGHTS = dict(A=1.0, B=-0.5, C=0.0)
COEFF = [1.0, -0.5, 0.0]
CENTRE = [0.4, -0.3, 0.2]
N = 3001


def bits_of(x):
    return [struct.unpack("<q", struct.pack("<d", float(v)))[0] for v in np.atleast_1d(x)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def gather(values, world, dtype=torch.float64):
    t = torch.tensor(values, dtype=dtype)
    out = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return [o.tolist() for o in out]


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {"world": world}
    box = xgmi.connect(dist, max_doubles=512)
    out["connected"] = box is not None
    if box is not None:
        rng = np.random.default_rng(21)
        pos = (rng.random((N, 3)) - 0.5) * np.array(L)
        pos[: N // 2] = np.array(CENTRE) + (rng.random((N // 2, 3)) - 0.5) * 7.0      # half of them around the region
        types = rng.integers(0, 3, N).astype(np.int32)
        reg = pv.region("box", CENTRE, 0.3, w=[2.0, 2.5, 1.5])
        bias = -1.7
        single = run_gpu(_abi, pos, types, L, reg, COEFF, np.float64, bias=bias, bias_on_device=False)
        sum_abs = float(np.abs(np.array(COEFF)[types]).sum())
        left = pos[:, 0] < CENTRE[0]
        splits = {"cut": np.flatnonzero(left) if rank == 0 else np.flatnonzero(~left),
                  "empty": np.arange(N) if rank == 0 else np.arange(0)}
        res = {}
        for name, mine in splits.items():
            g = run_gpu(_abi, pos[mine], types[mine], L, reg, COEFF, np.float64, bias=bias, bias_on_device=False, n_global=N,
                        reduce=box.all_reduce)
            ok = [same_bits(g["F"], single["F"][mine]), same_bits(g["virial"], single["virial"][:, mine]), same_bits(g["h"], single["h"][mine])]
            rows = gather([float(g["s"] - single["s"]), float(g["count"] - single["count"]), float(len(mine))] + [float(x) for x in ok], world)
            bits = gather(bits_of(g["s"]) + bits_of(g["count"]), world, torch.int64)
            res[name] = dict(value_diff=[r[0] for r in rows], count_diff=[r[1] for r in rows], locals=[int(r[2]) for r in rows],
                             rows_same_bits=[bool(r[3] and r[4] and r[5]) for r in rows], value_bits=[b[0] for b in bits], count_bits=[b[1] for b in bits],
                             value_same_bits_as_single=bits[0][0] == bits_of(single["s"])[0], value=float(g["s"]), count=float(g["count"]))
        out["abi"] = dict(res, sum_abs=sum_abs, single_value=single["s"], single_count=single["count"],
                          straddling=int(((single["h"] > 0) & left).sum()), straddling_right=int(((single["h"] > 0) & ~left).sum()))

        # the host class and the Python API on the "cut" split
        mine = splits["cut"]
        context.initialize(pos[mine], types[mine], ["A", "B", "C"], L, dtype=np.float64, n_global=N)
        xgmi.attach(dist, context.exec_conf, box)
        meta = integrate.mode_metadynamics(**KW)
        var = cv.probe_volume("box", CENTRE, 0.3, half_widths=[2.0, 2.5, 1.5], weights=WEIGHTS, sigma=0.5)
        var.set_grid(single["s"] - 20.0, single["s"] + 20.0, 128)
        context.run(1)
        moved = pos + np.random.default_rng(5).normal(0, 0.08, pos.shape)             # the same move on every rank
        moved -= np.rint(moved / np.array(L)) * np.array(L)
        context.set_positions(moved[mine], types[mine])
        context.run(1)
        integ = meta.cpp_integrator
        s, b = integ.getCurrentValues()[0], integ.getBiasFactors()[0]
        one = run_gpu(_abi, moved, types, L, reg, COEFF, np.float64, bias=b, bias_on_device=False)
        F = var.cpp_force.getForceArray().astype(np.float64)
        rows = gather([float(s - one["s"]), float(var.get_count() - one["count"]), float(same_bits(F, one["F"][mine])),
                       float(b), float(np.abs(F).max())], world)
        bits = gather(bits_of(var.cpp_force.getCurrentValue(2)), world, torch.int64)
        out["api"] = dict(value_diff=[r[0] for r in rows], count_diff=[r[1] for r in rows], force_same_bits=[bool(r[2]) for r in rows],
                          bias=[r[3] for r in rows], max_force=[r[4] for r in rows],
                          value_bits=[x[0] for x in bits], value_same_bits_as_single=bits[0][0] == bits_of(one["s"])[0],
                          route=integ.lastStepRoute(), timeouts=box.timeouts(), sum_abs=sum_abs)
        context.current = None
        dist.barrier()
        torch.cuda.synchronize()
        dist.barrier()
        box.close()
    if rank == 0:
        print(json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
