#!/usr/bin/env python3
"""Developer tool: the config 5 snapshot of tools/bench_ql.py (256 000-particle noisy fcc crystal) with cv.pair_entropy_local as the only
variable of a 512-point well-tempered grid; prints us/step.
usage: tools/bench_pel.py [steps] [f32|f64] [--r-max R] [--sigma-r S] [--bins B] [--plain | --switch-only | --average-only] [--pressure]
                          [--cv pair_entropy | steinhardt_local]
(defaults r_max 2.0, sigma_r 0.1, 40 bins, the average over 1.2 .. 1.5 and the switch (c0 3, p 6): a list that reaches 2.4, ~80 entries
per particle, built on the device with r_buff 0; --pressure: sets the pressure flag before the run, as a barostat would: the force pass
also writes the per-particle virial; --cv pair_entropy / steinhardt_local: the global pair entropy with the same histogram, or
cv.steinhardt_local (r_cut 1.4, r_on 1.2, degrees 4 and 6), on the SAME list instead: the yardsticks the step time is read against — run
them in alternating processes)
Run under rocprofv3 --kernel-trace --stats for the per-kernel table."""
import os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np, torch
import util
from metadynamics import context, cv, integrate
argv = sys.argv[1:]
par = {"--r-max": 2.0, "--sigma-r": 0.1, "--bins": 40, "--cv": "pair_entropy_local"}
for flag in list(par):
    if flag in argv:
        k = argv.index(flag)
        par[flag] = type(par[flag])(argv[k + 1])
        del argv[k:k + 2]
r_max, sigma_r, n_bins, which = par["--r-max"], par["--sigma-r"], par["--bins"], par["--cv"]
args = [a for a in argv if not a.startswith("--")]
pressure = "--pressure" in argv
options = dict(average=dict(r_on=1.2, r_cut=1.5), switch=dict(c0=3.0, p=6))
if "--plain" in argv:
    options = dict()
elif "--switch-only" in argv:
    del options["average"]
elif "--average-only" in argv:
    del options["switch"]
steps = int(args[0]) if len(args) > 0 else 100
dtype = np.float32 if (len(args) > 1 and args[1] == "f32") else np.float64
pos, L = util.fcc_lattice(40)
pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
N = len(pos)
r_list = r_max + 4.0 * sigma_r


def build(lo, hi, sigma):
    context.initialize(pos, np.zeros(N, dtype=np.int32), ["A"], L, dtype=dtype)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=r_list, r_buff=0.0, check_period=1 << 30, device=True)   # (nothing moves: no displacement checks)
    if which == "steinhardt_local":
        var = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=[0, 0, 0, 0, 1, 0, 1], nlist=nl, type="A", sigma=sigma)
    elif which == "pair_entropy":
        var = cv.pair_entropy(r_max=r_max, sigma_r=sigma_r, n_bins=n_bins, nlist=nl, type="A", sigma=sigma)
    else:
        var = cv.pair_entropy_local(r_max=r_max, sigma_r=sigma_r, n_bins=n_bins, nlist=nl, type="A", sigma=sigma, **options)
    var.set_grid(lo, hi, 512)
    return meta, var, nl


# grid around the value, sigma 1 % of the range — one untimed evaluation supplies the value
t0 = time.perf_counter()
meta, var, nl = build(-1.0, 1.0, 1.0)
context.run(1)
s0 = var.cpp_force.getCurrentValue(1)
print("N = %d, set up in %.1f s, neighbour list built on the device" % (N, time.perf_counter() - t0))
context.current = None
lo, hi = min(0.0, 2.0 * s0), max(0.0, 2.0 * s0)
meta, var, nl = build(lo, hi, 0.02 * abs(s0))
context.run(1)
entries = nl.cpp_nlist.getNumEntries()
print("%s %s cv =" % (which, sorted(options) if which == "pair_entropy_local" else ""), s0, "grid", (lo, hi),
      "list entries per particle %.1f" % (entries / N))
context.run(5)
torch.cuda.synchronize()
t0 = time.perf_counter()
context.current.system.run(steps)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
t_now = context.current.system.getCurrentTimeStep()
print("on grid: %s, hills %d, bias factors %s, V = %g"
      % (lo <= var.cpp_force.getCurrentValue(t_now) < hi, meta.cpp_integrator.getNumGaussians(), list(meta.cpp_integrator.getBiasFactors()),
         meta.cpp_integrator.getLogValue("bias", t_now)))
if pressure:
    print("virial of the bias force (xx xy xz yy yz zz): %s" % " ".join("%.6e" % w for w in var.get_virial()))
if which == "pair_entropy_local":
    s = var.get_local()
    print("s_i: median %.3f, min %.3f, max %.3f" % (np.median(s), s.min(), s.max()))
print("config 5 %s (%s%s, list to %.2f): %.1f us/step  (%.3e list entries/s incl. CV + force pass)"
      % (which, np.dtype(dtype).name, ", virial" if pressure else "", r_list, 1e6 * dt / steps, 2 * entries * steps / dt))
