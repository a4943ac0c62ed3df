"""Worker of tests/test_gpu_bragg_dd.py: one rank of a DOMAIN-DECOMPOSED run of cv.bragg through the reference-shaped API.  The particles
are split 1 : 2 between two ranks by index — no slabs and no ghosts: the variable needs neither — the ranks separate processes on cuda:0, a
harmonic umbrella so that the bias factor is of order one.  Both forms of the variable sit on one 2-d grid.  Every rank's value and the
rows of its local particles in the force array against the SINGLE-DOMAIN GPU result: the same kernels on the whole snapshot through the C
ABI (tests/test_gpu_bragg.py: run_gpu), in this process, at the bias factor the integrator reports plus the umbrella's.
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

from metadynamics import _abi, context, cv, integrate, xgmi
from test_gpu_bragg import run_gpu

KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
HKL = [(0, 0, 3), (1, -1, 0), (2, 1, -1)]
MODE = dict(A=1.0, B=-0.5, C=0.0)
COEFF = [1.0, -0.5, 0.0]
KAPPA = 35.0
N = 3001


def bits_of(x):
    return [struct.unpack("<q", struct.pack("<d", float(v)))[0] for v in np.atleast_1d(x)]


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {"world": world}
    box = xgmi.connect(dist, max_doubles=512)
    out["connected"] = box is not None
    if box is not None:
        # three types, one without an amplitude, in layers along (0, 0, 3) as tests/test_gpu_bragg.py: make_snapshot builds them
        rng = np.random.default_rng(21)
        L = (12.0, 12.0, 12.0)
        f = rng.random((N, 3)) - 0.5
        types = rng.integers(0, 3, N).astype(np.int32)
        f[:, 2] += 0.05 * np.sign(np.array(COEFF)[types]) * np.sin(2 * np.pi * 3 * f[:, 2])
        f[:, 2] -= np.rint(f[:, 2])
        pos = f * np.array(L)
        cut = N // 3 if world == 2 else 0                                 # 1 : 2
        mine = np.arange(0, cut) if rank == 0 else np.arange(cut, N)
        context.initialize(pos[mine], types[mine], ["A", "B", "C"], L, dtype=np.float64, n_global=N)
        xgmi.attach(dist, context.exec_conf, box)
        meta = integrate.mode_metadynamics(**KW)
        single = {m: run_gpu(_abi, pos, types, L, HKL, COEFF, np.float64, None, m, 0, bias=1.0, bias_on_device=False) for m in (False, True)}
        variables, cv0 = [], []
        for m in (False, True):
            val = single[m]["s"]
            var = cv.bragg(MODE, HKL, modulus=m, name="m" if m else None, sigma=0.02 * val)
            var.set_grid(0.4 * val, 1.6 * val, 64)
            cv0.append(0.8 * val)
            var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0[-1])
            variables.append(var)
        context.run(2)
        integ = meta.cpp_integrator
        values, factors = integ.getCurrentValues(), integ.getBiasFactors()
        err, bits, totals = [], [], []
        for c, m in enumerate((False, True)):
            total = factors[c] + KAPPA * (values[c] - cv0[c])
            totals.append(float(total))
            # the whole snapshot once more, at this very bias factor as a host scalar (the umbrella's route): the same fp32 coefficients
            F_single = run_gpu(_abi, pos, types, L, HKL, COEFF, np.float64, None, m, 0, bias=total, bias_on_device=False)["F"][:, :3]
            F = variables[c].cpp_force.getForceArray().astype(np.float64)
            err += [abs(values[c] - single[m]["s"]) / abs(single[m]["s"]), np.abs(F[:, :3] - F_single[mine]).max() / np.abs(F_single).max(),
                    float(np.abs(F[:, 3]).max())]
            bits += bits_of(variables[c].cpp_force.getCurrentValue(2))
        err = torch.tensor(err, dtype=torch.float64)
        dist.all_reduce(err, op=dist.ReduceOp.MAX)
        bits = torch.tensor(bits, dtype=torch.int64)
        all_bits = [torch.zeros_like(bits) for _ in range(world)]
        dist.all_gather(all_bits, bits)
        n_loc = torch.tensor([len(mine)])
        all_n = [torch.zeros_like(n_loc) for _ in range(world)]
        dist.all_gather(all_n, n_loc)
        out["bragg"] = dict(cv_rel=[float(err[0]), float(err[3])], force_rel=[float(err[1]), float(err[4])], force_w=[float(err[2]), float(err[5])],
                            value_bits=[[int(b[c]) for b in all_bits] for c in range(2)], values=[float(v) for v in values], bias=totals,
                            umbrella_part=[float(KAPPA * (values[c] - cv0[c])) for c in range(2)], locals=[int(n[0]) for n in all_n], n_global=N,
                            route=integ.lastStepRoute(), timeouts=box.timeouts())
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
