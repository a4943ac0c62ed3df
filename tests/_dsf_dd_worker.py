"""Worker of tests/test_gpu_debye_dd.py: one rank of a DOMAIN-DECOMPOSED constant-pressure run of cv.debye_structure_factor through the
reference-shaped API — z slabs with ghost particles as in tests/_pe_dd_worker.py, the ranks separate processes on cuda:0, the pressure
flag set, a harmonic umbrella so that the bias factor is of order one.  Every rank's value, the rows of its local particles in the force
array and in get_virial(per_particle=True) against the restatement on the WHOLE snapshot (tests/debye_ref.py, at the bias factor the
integrator reports plus the umbrella's), the sum of the virial over the ranks against the single-domain sums, and the spectrum (all-reduced
like the value) on both ranks.
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

import debye_ref as dsf
import util
from metadynamics import context, cv, integrate, xgmi

KW = dict(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
Q, WEIGHTS, R_CUT = (7.695, 8.886), (1.0, -0.5), 2.4
SPECTRUM = (2.0, 14.0, 64)
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
        types = np.zeros(N, dtype=np.int32)
        r_list = 2.45
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
        val = dsf.compute(pos, types, L, full, Q, R_CUT, 0, c=WEIGHTS)["s"]
        var = cv.debye_structure_factor(Q, R_CUT, nl, "A", weights=WEIGHTS, sigma=0.02 * abs(val))
        var.set_grid(0.4 * val, 1.6 * val, 64)
        cv0 = 0.8 * val
        var.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
        context.run(2)
        integ = meta.cpp_integrator
        s = integ.getCurrentValues()[0]
        total = integ.getBiasFactors()[0] + KAPPA * (s - cv0)
        r = dsf.compute(pos, types, L, full, Q, R_CUT, 0, c=WEIGHTS, bias=total)
        per = var.get_virial(per_particle=True)                          # (6, local particles)
        F = var.cpp_force.getForceArray().astype(np.float64)
        F_ref = -total * r["grad"]
        top, w_top, f_top = np.abs(r["virial"]).max(), np.abs(r["virial_sum"]).max(), np.abs(F_ref).max()
        loc = np.asarray(var.get_local())
        Qm, spec = var.get_spectrum(*SPECTRUM)
        _, spec_ref = dsf.spectrum(pos, types, L, full, R_CUT, 0, *SPECTRUM)
        err = torch.tensor([np.abs(per.T - r["virial"][mine]).max() / top, np.abs(F[:, :3] - F_ref[mine]).max() / f_top,
                            np.abs(loc - r["local"][mine]).max() / np.abs(r["local"]).max(),
                            np.abs(spec - spec_ref).max() / np.abs(spec_ref).max(),
                            np.abs(np.asarray(var.get_intensities()) - r["I"]).max() / np.abs(r["I"]).max()], dtype=torch.float64)
        dist.all_reduce(err, op=dist.ReduceOp.MAX)
        W = torch.from_numpy(var.get_virial().copy())
        dist.all_reduce(W)
        n_loc = torch.tensor([len(mine), len(ghosts), per.shape[1]])
        dist.all_reduce(n_loc)
        bits = torch.tensor(bits_of(var.cpp_force.getCurrentValue(2)) + bits_of(spec), dtype=torch.int64)
        all_bits = [torch.zeros_like(bits) for _ in range(world)]
        dist.all_gather(all_bits, bits)
        out["dsf"] = dict(per_particle_rel=float(err[0]), force_rel=float(err[1]), local_rel=float(err[2]), spectrum_rel=float(err[3]),
                          intensity_rel=float(err[4]), sum_rel=float(np.abs(W.numpy() - r["virial_sum"]).max() / w_top),
                          max_W=float(w_top), bias=float(total), umbrella_part=float(KAPPA * (s - cv0)), cv_rel=abs(s - val) / abs(val),
                          value_bits=[int(b[0]) for b in all_bits], spectrum_equal=all(torch.equal(b[1:], all_bits[0][1:]) for b in all_bits),
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
