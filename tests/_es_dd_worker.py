"""Worker of tests/test_gpu_env_similarity_dd.py: one rank of a DOMAIN-DECOMPOSED constant-pressure run of cv.environment_similarity
through the reference-shaped API — z slabs with ghost particles as in tests/_pe_dd_worker.py, the ranks separate processes on cuda:0, the
pressure flag set, a harmonic umbrella so that the bias factor is of order one.  The plain variable (fcc template, no switch): every
rank's value, the rows of its local particles in the force array and in get_virial(per_particle=True) against the restatement on the WHOLE
snapshot (tests/env_similarity_ref.py, at the bias factor the integrator reports plus the umbrella's).  Then the same variable with a
switch: it must throw on every rank.
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

import env_similarity_ref as es
import util
from metadynamics import context, cv, integrate, xgmi

KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
PAR = (0.12, 1.3, 1.5)                # sigma_env, r_on, r_cut
KAPPA = 35.0


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
        types = np.zeros(N, dtype=np.int32)
        r_list = 1.55
        owner = np.minimum((np.mod(pos[:, 2] + L / 2, L) / L * world).astype(int), world - 1)
        mine = np.where(owner == rank)[0]
        lo, hi = -L / 2 + rank * L / world, -L / 2 + (rank + 1) * L / world
        z = pos[:, 2]
        zdist = lambda a, b: np.minimum(np.abs(a - b), L - np.abs(a - b))
        ghosts = np.where((owner != rank) & ((zdist(z, lo) <= r_list) | (zdist(z, hi) <= r_list)))[0]
        context.initialize(pos[mine], types[mine], ["A"], L, dtype=np.float64, n_global=N, ghost_positions=pos[ghosts], ghost_types=types[ghosts])
        xgmi.attach(dist, context.exec_conf, box)
        context.current.system_definition.getParticleData().setPressureFlag(True)
        meta = integrate.mode_metadynamics(**KW)
        nl = cv.nlist_cell(r_cut=r_list)
        nl.update()
        full = util.build_nlist(pos, L, r_list)
        T = cv.environment_templates("fcc", np.sqrt(2.0))
        val = es.compute(pos, types, L, full, T, *PAR, 0)["s"]
        var = cv.environment_similarity(T, PAR[0], PAR[2], PAR[1], nl, "A", sigma=0.02)
        var.set_grid(0.0, 1.0, 64)
        cv0 = 0.7 * val
        var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
        context.run(2)
        integ = meta.cpp_integrator
        s = integ.getCurrentValues()[0]
        total = integ.getBiasFactors()[0] + KAPPA * (s - cv0)
        r = es.compute(pos, types, L, full, T, *PAR, 0, bias=total)
        per = var.get_virial(per_particle=True)                          # (6, local particles)
        F = var.cpp_force.getForceArray().astype(np.float64)
        F_ref = -total * r["grad"]
        top, w_top, f_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max(), np.abs(F_ref).max()
        k_err = np.abs(var.get_local() - r["k"][mine]).max() / np.abs(r["k"]).max()
        err = torch.tensor([np.abs(per.T - r["virial"][mine]).max() / top, np.abs(F[:, :3] - F_ref[mine]).max() / f_top, k_err], dtype=torch.float64)
        dist.all_reduce(err, op=dist.ReduceOp.MAX)
        W = torch.from_numpy(var.get_virial().copy())
        dist.all_reduce(W)
        n_loc = torch.tensor([len(mine), len(ghosts), per.shape[1]])
        dist.all_reduce(n_loc)
        bits = torch.tensor([struct.unpack("<q", struct.pack("<d", var.cpp_force.getCurrentValue(2)))[0]], dtype=torch.int64)
        all_bits = [torch.zeros_like(bits) for _ in range(world)]
        dist.all_gather(all_bits, bits)
        # with a switch beta of a ghost neighbour would be needed: refused on every rank, before any launch
        sw = cv.environment_similarity(T, PAR[0], PAR[2], PAR[1], nl, "A", switch=dict(c0=0.5, p=6), name="sw")
        try:
            sw.cpp_force.getCurrentValue(2)
            refused = 0
        except RuntimeError as e:
            refused = int("domain-decomposed runs are not supported" in str(e))
        flag = torch.tensor([refused])
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        out["es"] = dict(per_particle_rel=float(err[0]), force_rel=float(err[1]), k_rel=float(err[2]),
                         sum_rel=float(np.abs(W.numpy() - r["virial_sum"]).max() / w_top), max_W=float(w_top), bias=float(total),
                         umbrella_part=float(KAPPA * (s - cv0)), cv_rel=abs(s - val) / abs(val), value_bits=[int(b[0]) for b in all_bits],
                         locals_total=int(n_loc[0]), ghosts_total=int(n_loc[1]), rows_total=int(n_loc[2]), n_global=N,
                         switch_refused_everywhere=int(flag[0]), timeouts=box.timeouts())
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
