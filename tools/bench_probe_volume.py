#!/usr/bin/env python3
"""Developer tool: bench.py's configuration (10^6 random particles of two types in a box of 100) with cv.probe_volume as the only variable
of a 512-point well-tempered grid — a slab holding about 10 % of the particles, a box, a sphere of about 10^3 particles, each with and
without the pressure flag (with it the force pass writes six more scalars per particle) — and cv.bragg with ONE lattice vector as the
yardstick, in one process: the variants alternate over several rounds, every round times several blocks of steps, and the table gives the
median, the smallest and the largest block of each variant in us/step.  With --only NAME a process runs one variant.
usage: tools/bench_probe_volume.py [steps] [f32|f64] [--rounds R] [--blocks B] [--only NAME[,NAME]] [--particles N]
(defaults: 200 steps per block, 5 blocks, 3 rounds, f32.  Variants: slab, slab_virial, box, box_virial, sphere, sphere_virial, bragg_1.)
Both variables read 16 bytes and write 16 bytes per particle and step (fp32 arrays); the probe volume does its arithmetic in fp64 and
evaluates erf and exp only for the lanes inside the shell of a face.
Run under rocprofv3 --kernel-trace --stats for the per-kernel table (k_probe_sums, k_probe_forces against k_bragg_sums, k_bragg_forces)."""
import json, os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np, torch
import util
from metadynamics import context, cv, integrate
argv = sys.argv[1:]
par = {"--rounds": 3, "--blocks": 5, "--only": "", "--particles": 1_000_000}
for flag in list(par):
    if flag in argv:
        k = argv.index(flag)
        par[flag] = type(par[flag])(argv[k + 1])
        del argv[k:k + 2]
rounds, blocks, N = par["--rounds"], par["--blocks"], par["--particles"]
args = [a for a in argv if not a.startswith("--")]
steps = int(args[0]) if len(args) > 0 else 200
dtype = np.float64 if (len(args) > 1 and args[1] == "f64") else np.float32
VARIANTS = ["slab", "slab_virial", "box", "box_virial", "sphere", "sphere_virial", "bragg_1"]
names = [v for v in VARIANTS if not par["--only"] or v in par["--only"].split(",")]
L = 100.0 * (N / 1_000_000) ** (1.0 / 3.0)                               # bench.py's density: one particle per unit volume
pos, types = util.snapshot_random(N, L, seed=12345, dtype=np.float32)
INF = float("inf")
CENTRE = [0.1 * L, -0.2 * L, 0.05 * L]
REGIONS = {"slab": dict(shape="box", half_widths=[INF, INF, 0.05 * L]),                      # a tenth of the box
           "box": dict(shape="box", half_widths=[0.15 * L, 0.1 * L, 0.2 * L]),
           "sphere": dict(shape="sphere", radius=(1000.0 * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0))}  # 10^3 particles at unit density
SIGMA_S = 0.3


def build(name, lo, hi, sigma):
    context.initialize(pos, types, ["A", "B"], L, dtype=dtype)
    context.current.system_definition.getParticleData().setPressureFlag(name.endswith("_virial"))
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    if name == "bragg_1":
        var = cv.bragg(dict(A=1.0, B=-1.0), util.CV1_VECTORS[:1], sigma=sigma)
    else:
        var = cv.probe_volume(centre=CENTRE, sigma_s=SIGMA_S, weights=dict(A=1.0, B=0.0), sigma=sigma, **REGIONS[name.split("_")[0]])
    var.set_grid(lo, hi, 512)
    return meta, var


# one untimed evaluation per variant supplies the value the grid is laid around
value = {}
for name in names:
    meta, var = build(name, -1.0, 1.0, 1.0)
    context.run(1)
    value[name] = var.cpp_force.getCurrentValue(1)
    context.current = None
times = {v: [] for v in names}
route = {}
for rnd in range(rounds):
    for name in names:
        s0 = value[name]
        w = max(abs(s0), 1e-6)
        meta, var = build(name, s0 - 8 * w, s0 + 8 * w, 0.2 * w)
        context.run(6)
        for b in range(blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            context.current.system.run(steps)
            torch.cuda.synchronize()
            times[name].append(1e6 * (time.perf_counter() - t0) / steps)
        route[name] = meta.cpp_integrator.lastStepRoute()
        if rnd == 0:
            extra = "" if name == "bragg_1" else ", N_v = %.6g" % var.get_count()
            print("%-14s cv = %.9g%s, hills %d, route: %s" % (name, s0, extra, meta.cpp_integrator.getNumGaussians(), route[name]))
        context.current = None
print("N = %d, L = %.1f, %s: %d rounds x %d blocks of %d steps, us/step" % (N, L, np.dtype(dtype).name, rounds, blocks, steps))
for name in names:
    t = np.array(times[name])
    print("  %-14s median %8.1f   min %8.1f   max %8.1f" % (name, np.median(t), t.min(), t.max()))
print(json.dumps(dict(particles=N, dtype=np.dtype(dtype).name, steps=steps, blocks=blocks, rounds=rounds,
                      us_per_step={v: dict(median=float(np.median(times[v])), min=float(min(times[v])), max=float(max(times[v])), route=route[v])
                                   for v in names})))
