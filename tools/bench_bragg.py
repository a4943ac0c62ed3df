#!/usr/bin/env python3
"""Developer tool: bench.py's configuration (10^6 random particles of two types in a box of 100, amplitudes +1 / -1) with cv.bragg as the
only variable of a 512-point well-tempered grid, and cv.lamellar with the SAME lattice vectors off the fused path (setFusedPath(False):
its stand-alone sums and force kernels and the engine's own launch) as the yardstick, in one process: the variants alternate over several
rounds, every round times several blocks of steps, and the table gives the median, the smallest and the largest block of each variant in
us/step.  With --only NAME a process runs one variant: a job script alternates such processes.
usage: tools/bench_bragg.py [steps] [f32|f64] [--modes K[,K]] [--rounds R] [--blocks B] [--only NAME[,NAME]] [--particles N]
(defaults: 200 steps per block, 5 blocks, 3 rounds, f32, K = 1, 3 and 8: the first K of the headline's first vector set.  Variants, per K:
bragg_K, bragg_modulus_K, lamellar_unfused_K, and lamellar_fused_K, the two-launch step that cv.lamellar takes by default.)
cv.bragg forms a sine AND a cosine per particle and mode in both passes where cv.lamellar forms one of them, adds in fp64, and its step
has two launches more (the reduction of the block sums and finalize).
Run under rocprofv3 --kernel-trace --stats for the per-kernel table (k_bragg_sums, k_bragg_finalize, k_bragg_forces)."""
import json, os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np, torch
import util
from metadynamics import context, cv, integrate
argv = sys.argv[1:]
par = {"--modes": "1,3,8", "--rounds": 3, "--blocks": 5, "--only": "", "--particles": 1_000_000}
for flag in list(par):
    if flag in argv:
        k = argv.index(flag)
        par[flag] = type(par[flag])(argv[k + 1])
        del argv[k:k + 2]
rounds, blocks, N = par["--rounds"], par["--blocks"], par["--particles"]
args = [a for a in argv if not a.startswith("--")]
steps = int(args[0]) if len(args) > 0 else 200
dtype = np.float64 if (len(args) > 1 and args[1] == "f64") else np.float32
modes = [int(k) for k in par["--modes"].split(",")]
VARIANTS = [(kind, K) for K in modes for kind in ("bragg", "bragg_modulus", "lamellar_unfused", "lamellar_fused")]
names = [v for v in VARIANTS if not par["--only"] or "%s_%d" % v in par["--only"].split(",")]
L = 100.0 * (N / 1_000_000) ** (1.0 / 3.0)                               # bench.py's density
pos, types = util.snapshot_random(N, L, seed=12345, dtype=np.float32)
MODE = dict(A=1.0, B=-1.0)


def build(kind, K, lo, hi, sigma):
    context.initialize(pos, types, ["A", "B"], L, dtype=dtype)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    vec = util.CV1_VECTORS[:K]
    if kind.startswith("bragg"):
        var = cv.bragg(MODE, vec, modulus=kind == "bragg_modulus", sigma=sigma)
    else:
        var = cv.lamellar(MODE, vec, sigma=sigma)
        meta.cpp_integrator.setFusedPath(kind == "lamellar_fused")
    var.set_grid(lo, hi, 512)
    return meta, var


# one untimed evaluation per variant supplies the value the grid is laid around
value = {}
for kind, K in names:
    meta, var = build(kind, K, -1.0, 1.0, 1.0)
    context.run(1)
    value[kind, K] = var.cpp_force.getCurrentValue(1)
    context.current = None
times = {v: [] for v in names}
route = {}
for rnd in range(rounds):
    for kind, K in names:
        s0 = value[kind, K]
        w = max(abs(s0), 1e-6)
        meta, var = build(kind, K, s0 - 8 * w, s0 + 8 * w, 0.2 * w)
        context.run(6)
        for b in range(blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            context.current.system.run(steps)
            torch.cuda.synchronize()
            times[kind, K].append(1e6 * (time.perf_counter() - t0) / steps)
        t_now = context.current.system.getCurrentTimeStep()
        route[kind, K] = meta.cpp_integrator.lastStepRoute()
        if rnd == 0:
            print("%-19s cv = %.9g, on grid: %s, hills %d, route: %s" % ("%s_%d" % (kind, K), s0, s0 - 8 * w <= var.cpp_force.getCurrentValue(t_now) < s0 + 8 * w,
                                                                        meta.cpp_integrator.getNumGaussians(), route[kind, K]))
        context.current = None
print("N = %d, L = %.1f, %s: %d rounds x %d blocks of %d steps, us/step" % (N, L, np.dtype(dtype).name, rounds, blocks, steps))
for kind, K in names:
    t = np.array(times[kind, K])
    print("  %-19s median %8.1f   min %8.1f   max %8.1f   (%.3e particle-modes/s incl. CV + force pass)"
          % ("%s_%d" % (kind, K), np.median(t), t.min(), t.max(), 2.0 * N * K / (1e-6 * np.median(t))))
print(json.dumps(dict(particles=N, dtype=np.dtype(dtype).name, steps=steps, blocks=blocks, rounds=rounds,
                      us_per_step={"%s_%d" % v: dict(median=float(np.median(times[v])), min=float(min(times[v])), max=float(max(times[v])), route=route[v])
                                   for v in names})))
