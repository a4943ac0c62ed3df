"""Worker of tests/test_gpu_coordination_dd.py: one rank of a DOMAIN-DECOMPOSED constant-pressure run of the plain A-B cv.coordination
through the reference-shaped API — z slabs with ghost particles as in tests/_dsf_dd_worker.py, the ranks separate processes on cuda:0, the
pressure flag set, a harmonic umbrella so that the bias factor is of order one.  Every rank's value, the rows of its local particles in
the force array, in get_local() and in get_virial(per_particle=True) against the restatement on the WHOLE snapshot
(tests/coordination_ref.py, at the bias factor the integrator reports plus the umbrella's), and the sum of the virial over the ranks
against the single-domain sums.  Then a switch is set: the variable raises on every rank, before any exchange.
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

import coordination_ref as cn
import util
from metadynamics import context, cv, integrate, xgmi

KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
R0, R_CUT = 1.15, 2.0
KAPPA = 35.0


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
        pos, L = util.fcc_lattice(5)
        pos = pos + np.random.default_rng(12).normal(0, 0.05, pos.shape)
        pos = np.mod(pos + L / 2, L) - L / 2
        N = len(pos)
        types = (np.arange(N) % 2).astype(np.int32)
        r_list = 2.05
        owner = np.minimum((np.mod(pos[:, 2] + L / 2, L) / L * world).astype(int), world - 1)
        mine = np.where(owner == rank)[0]
        lo, hi = -L / 2 + rank * L / world, -L / 2 + (rank + 1) * L / world
        z = pos[:, 2]
        zdist = lambda a, b: np.minimum(np.abs(a - b), L - np.abs(a - b))
        ghosts = np.where((owner != rank) & ((zdist(z, lo) <= r_list) | (zdist(z, hi) <= r_list)))[0]
        context.initialize(pos[mine], types[mine], ["A", "B"], L, dtype=np.float64, n_global=N, ghost_positions=pos[ghosts], ghost_types=types[ghosts])
        xgmi.attach(dist, context.exec_conf, box)
        context.current.system_definition.getParticleData().setPressureFlag(True)
        meta = integrate.mode_metadynamics(**KW)
        nl = cv.nlist_cell(r_cut=r_list)
        nl.update()
        full = util.build_nlist(pos, L, r_list)
        par = cn.params(0, 1, R0, R_CUT)
        val = cn.compute(pos, types, L, full, par)["s"]
        var = cv.coordination(R0, nl, "A", partner="B", r_cut=R_CUT, sigma=0.02 * abs(val))
        var.set_grid(0.4 * val, 1.6 * val, 64)
        cv0 = 0.8 * val
        var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
        context.run(2)
        integ = meta.cpp_integrator
        s = integ.getCurrentValues()[0]
        total = integ.getBiasFactors()[0] + KAPPA * (s - cv0)
        r = cn.compute(pos, types, L, full, par, bias=total)
        per = var.get_virial(per_particle=True)                          # (6, local particles)
        F = var.cpp_force.getForceArray().astype(np.float64)
        F_ref = -total * r["grad"]
        top, w_top, f_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max(), np.abs(F_ref).max()
        loc = np.asarray(var.get_local())
        err = torch.tensor([np.abs(per.T - r["virial"][mine]).max() / top, np.abs(F[:, :3] - F_ref[mine]).max() / f_top,
                            np.abs(loc - r["local"][mine]).max() / np.abs(r["local"]).max()], dtype=torch.float64)
        dist.all_reduce(err, op=dist.ReduceOp.MAX)
        W = torch.from_numpy(var.get_virial().copy())
        dist.all_reduce(W)
        n_loc = torch.tensor([len(mine), len(ghosts), per.shape[1]])
        dist.all_reduce(n_loc)
        bits = torch.tensor(bits_of(var.cpp_force.getCurrentValue(2)), dtype=torch.int64)
        all_bits = [torch.zeros_like(bits) for _ in range(world)]
        dist.all_gather(all_bits, bits)
        # a switch: g'(n_j) of a ghost would have to be exchanged, so the variable raises — on every rank, ahead of its all-reduce
        var.set_switch(dict(c0=5.0, p=8))
        try:
            var.cpp_force.getCurrentValue(2)
            raised = ""
        except RuntimeError as e:
            raised = str(e)
        refused = torch.tensor([1 if "domain-decomposed" in raised else 0])
        dist.all_reduce(refused)
        out["cn"] = dict(per_particle_rel=float(err[0]), force_rel=float(err[1]), local_rel=float(err[2]),
                         sum_rel=float(np.abs(W.numpy() - r["virial_sum"]).max() / w_top),
                         max_W=float(w_top), bias=float(total), umbrella_part=float(KAPPA * (s - cv0)), cv_rel=abs(s - val) / abs(val),
                         value_bits=[int(b[0]) for b in all_bits], switch_refused_on=int(refused[0]),
                         locals_total=int(n_loc[0]), ghosts_total=int(n_loc[1]), rows_total=int(n_loc[2]), n_global=N,
                         timeouts=box.timeouts())
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
