#!/usr/bin/env python3
"""Developer tool: the config 5 snapshot of tools/bench_ql.py (256 000-particle noisy fcc crystal) with cv.debye_structure_factor as the
only variable of a 512-point well-tempered grid; prints us/step.
usage: tools/bench_dsf.py [steps] [f32|f64] [--peaks P] [--r-cut R] [--walk-twice] [--pressure] [--spectrum] [--cv pair_entropy]
(defaults: one peak, Q111 = 7.695; --peaks 2 adds Q200 = 8.886 with weight -0.5, up to 8 peaks; r_cut 2.4, a list that reaches it with
~80 entries per particle, built on the device with r_buff 0; --r-cut 3.5 is the second record, ~250 entries per particle;
--walk-twice: mtd_dsf_set_store_gradient(0), the force call walks the rows again instead of scaling the stored gradient — the A/B of
profiles/r24/README.md; --pressure: sets the pressure flag before the run, as a barostat would: the force call also writes the
per-particle virial; --spectrum: times get_spectrum(2, 14, 256) once at the end; --cv pair_entropy: the global pair entropy (r_max =
r_cut - 0.4, sigma_r 0.1, 40 bins) on the SAME list instead: the yardstick the step time is read against — run them in alternating
processes)
Run under rocprofv3 --kernel-trace --stats for the per-kernel table."""
import os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np, torch
import util
from metadynamics import _abi, context, cv, integrate
argv = sys.argv[1:]
par = {"--peaks": 1, "--r-cut": 2.4, "--cv": "debye_structure_factor"}
for flag in list(par):
    if flag in argv:
        k = argv.index(flag)
        par[flag] = type(par[flag])(argv[k + 1])
        del argv[k:k + 2]
n_peaks, r_cut, which = par["--peaks"], par["--r-cut"], par["--cv"]
args = [a for a in argv if not a.startswith("--")]
pressure, walk_twice = "--pressure" in argv, "--walk-twice" in argv
steps = int(args[0]) if len(args) > 0 else 100
dtype = np.float32 if (len(args) > 1 and args[1] == "f32") else np.float64
Q = (7.695, 8.886, 12.57, 14.74, 3.1, 5.2, 17.77, 10.4)[:n_peaks]
WEIGHTS = (1.0, -0.5, 0.25, 0.3, -0.2, 0.1, 0.7, -1.1)[:n_peaks]
pos, L = util.fcc_lattice(40)
pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
N = len(pos)
if which == "debye_structure_factor":
    _abi.check(_abi.load().mtd_dsf_set_store_gradient(0 if walk_twice else 1))


def build(lo, hi, sigma):
    context.initialize(pos, np.zeros(N, dtype=np.int32), ["A"], L, dtype=dtype)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=r_cut, r_buff=0.0, check_period=1 << 30, device=True)   # (nothing moves: no displacement checks)
    if which == "pair_entropy":
        var = cv.pair_entropy(r_max=r_cut - 0.4, sigma_r=0.1, n_bins=40, nlist=nl, type="A", sigma=sigma)
    else:
        var = cv.debye_structure_factor(Q, r_cut, nl, "A", weights=WEIGHTS, sigma=sigma)
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
print("%s cv =" % which, s0, "grid", (lo, hi), "list entries per particle %.1f" % (entries / N))
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
label = which
if which == "debye_structure_factor":
    print("I_p: %s" % " ".join("%.4f" % v for v in var.get_intensities()))
    label = "%s P = %d, %s" % (which, n_peaks, "second walk" if walk_twice else "stored gradient")
    if "--spectrum" in argv:
        var.get_spectrum(2.0, 14.0, 256)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        Qm, I = var.get_spectrum(2.0, 14.0, 256)
        print("spectrum of 256 points, read back: %.2f ms; tallest beyond Q = 5 at Q = %.3f" % (1e3 * (time.perf_counter() - t1),
                                                                                              Qm[Qm > 5.0][np.argmax(I[Qm > 5.0])]))
print("config 5 %s (%s%s, list to %.2f): %.1f us/step  (%.3e list entries/s incl. CV + force pass)"
      % (label, np.dtype(dtype).name, ", virial" if pressure else "", r_cut, 1e6 * dt / steps, 2 * entries * steps / dt))
