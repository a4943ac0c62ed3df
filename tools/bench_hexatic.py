#!/usr/bin/env python3
"""Developer tool: the config 5 snapshot of tools/bench_cn.py (256 000-particle noisy fcc crystal) with cv.hexatic as the only variable
of a 512-point well-tempered grid, and cv.tetrahedral and cv.coordination with a switch on the SAME list as the yardsticks, in one
process: the variants alternate over several rounds, every round times several blocks of steps, and the table gives the median, the
smallest and the largest block of each variant in us/step.  With --only NAME a process runs one variant.
usage: tools/bench_hexatic.py [steps] [f32|f64] [--r-list R] [--rounds K] [--blocks B] [--k K] [--axis x|y|z] [--pressure] [--only NAME[,NAME]]
(defaults: 200 steps per block, 5 blocks, 3 rounds, f64, k = 6 about z; the list, built on the device with r_buff 0, reaches 1.5 — ~17
entries per particle, the first shell, the variable's own use; --r-list 2.4 gives ~80 entries per particle, of which the variables
still take the first shell.  Variants: plain, switch_gate (switch (0.05, 2), gate (6, 11)), global (global_order=True), tetrahedral
(plain), coordination (r_0 = 1.15, (6, 12), r_cut = the list's reach, switch (c0 = its mean, 8)).  The window of the hexatic and of the
tetrahedral order is 1.3 .. 1.5.
--pressure: sets the pressure flag before the run, as a barostat would: the force call also writes the per-particle virial)
Run under rocprofv3 --kernel-trace --stats for the per-kernel table."""
import json, os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np, torch
import util
from metadynamics import context, cv, integrate
argv = sys.argv[1:]
par = {"--r-list": 1.5, "--rounds": 3, "--blocks": 5, "--k": 6, "--axis": "z", "--only": ""}
for flag in list(par):
    if flag in argv:
        k = argv.index(flag)
        par[flag] = type(par[flag])(argv[k + 1])
        del argv[k:k + 2]
r_list, rounds, blocks, fold, axis = par["--r-list"], par["--rounds"], par["--blocks"], par["--k"], par["--axis"]
args = [a for a in argv if not a.startswith("--")]
pressure = "--pressure" in argv
steps = int(args[0]) if len(args) > 0 else 200
dtype = np.float32 if (len(args) > 1 and args[1] == "f32") else np.float64
R_ON, R_CUT = 1.3, 1.5
VARIANTS = ("plain", "switch_gate", "global", "tetrahedral", "coordination")
names = [v for v in VARIANTS if not par["--only"] or v in par["--only"].split(",")]
pos, L = util.fcc_lattice(40)
pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
N = len(pos)
types = np.zeros(N, dtype=np.int32)


def build(name, lo, hi, sigma, c0):
    context.initialize(pos, types, ["A", "B"], L, dtype=dtype)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=r_list, r_buff=0.0, check_period=1 << 30, device=True)   # (nothing moves: no displacement checks)
    if name == "coordination":
        var = cv.coordination(1.15, nl, "A", r_cut=r_list, sigma=sigma, switch=dict(c0=c0, p=8))
    elif name == "tetrahedral":
        var = cv.tetrahedral(R_CUT, R_ON, nl, "A", sigma=sigma)
    else:
        var = cv.hexatic(R_CUT, R_ON, nl, "A", k=fold, axis=axis, global_order=name == "global", sigma=sigma,
                         switch=dict(c0=0.05, p=2) if name == "switch_gate" else None,
                         gate=dict(n_lo=6.0, n_hi=11.0) if name == "switch_gate" else None)
    var.set_grid(lo, hi, 512)
    return meta, var, nl


# one untimed evaluation per variant supplies the value the grid is laid around (sigma 2 % of it) and, for the coordination number's
# switch, c0: its mean, so that h is on its slope
value = {}
for name in names:
    c0 = 1.0
    if name == "coordination":
        meta, var, nl = build(name, -1.0, 1.0, 1.0, 1e9)                 # (h ~ 0: only get_local is read)
        context.run(1)
        c0 = float(np.mean(var.get_local()))
        context.current = None
        value["c0"] = c0
    meta, var, nl = build(name, -1.0, 1.0, 1.0, c0)
    context.run(1)
    value[name] = var.cpp_force.getCurrentValue(1)
    context.current = None
times = {name: [] for name in names}
entries = {}
for rnd in range(rounds):
    for name in names:
        s0 = value[name]
        lo, hi = min(0.0, 2.0 * s0), max(0.0, 2.0 * s0)
        if s0 == 0.0:
            lo, hi, s0 = -1.0, 1.0, 1.0
        meta, var, nl = build(name, lo, hi, 0.02 * abs(s0), value.get("c0", 1.0))
        context.run(6)
        entries[name] = nl.cpp_nlist.getNumEntries()
        for b in range(blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            context.current.system.run(steps)
            torch.cuda.synchronize()
            times[name].append(1e6 * (time.perf_counter() - t0) / steps)
        t_now = context.current.system.getCurrentTimeStep()
        if rnd == 0:
            print("%-13s cv = %.9g, on grid: %s, hills %d, list entries per particle %.1f"
                  % (name, value[name], lo <= var.cpp_force.getCurrentValue(t_now) < hi, meta.cpp_integrator.getNumGaussians(), entries[name] / N))
        context.current = None
print("config 5, N = %d, %s%s, k = %d about %s, list to %.2f: %d rounds x %d blocks of %d steps, us/step"
      % (N, np.dtype(dtype).name, ", virial" if pressure else "", fold, axis, r_list, rounds, blocks, steps))
for name in names:
    t = np.array(times[name])
    print("  %-15s median %8.1f   min %8.1f   max %8.1f   (%.3e list entries/s incl. CV + force pass)"
          % (name, np.median(t), t.min(), t.max(), entries[name] / (1e-6 * np.median(t))))
print(json.dumps(dict(r_list=r_list, k=fold, axis=axis, dtype=np.dtype(dtype).name, virial=pressure, steps=steps, blocks=blocks, rounds=rounds,
                      us_per_step={n: dict(median=float(np.median(times[n])), min=float(min(times[n])), max=float(max(times[n]))) for n in names})))
