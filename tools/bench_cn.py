#!/usr/bin/env python3
"""Developer tool: the config 5 snapshot of tools/bench_dsf.py (256 000-particle noisy fcc crystal) with cv.coordination as the only
variable of a 512-point well-tempered grid, and cv.debye_structure_factor with one peak on the SAME list as the yardstick, in one
process: the variants alternate over several rounds, every round times several blocks of steps, and the table gives the median, the
smallest and the largest block of each variant in us/step.
usage: tools/bench_cn.py [steps] [f32|f64] [--r-cut R] [--rounds K] [--blocks B] [--pressure] [--only NAME[,NAME]] [--cluster V_MIN R_LINK]
(defaults: 200 steps per block, 5 blocks, 3 rounds, f64; r_cut 2.4 — a list that reaches it with ~80 entries per particle, built on the
device with r_buff 0; --r-cut 1.5 is the short list, ~17 entries per particle.  Variants: plain (A = B, every particle of one type),
general (the same with (6, 12) sent through the general Horner loop, mtd_coord_set_compiled_pair(0): the A/B of the compiled pair term),
plain_ab (two types interleaved, A != B: the list holds all pairs and half of its entries play no role), switch (A = B with
switch=dict(c0, p): the second walk), debye (one peak, Q111).  r_0 = 1.15, (n, m) = (6, 12), d_0 = 0.
--pressure: sets the pressure flag before the run, as a barostat would: the force call also writes the per-particle virial
--cluster V_MIN R_LINK: adds the variant switch_cluster, the switch with set_cluster(dict(v_min=V_MIN, r_link=R_LINK)): the largest cluster
of particles with v_i >= V_MIN; its summary (root, members, clusters, nodes) is printed, because the cost of the link pass depends on the
size of the nucleus.  c0 is the mean coordination number, so v_i scatters around 1/2)
Run under rocprofv3 --kernel-trace --stats for the per-kernel table."""
import json, os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np, torch
import util
from metadynamics import _abi, context, cv, integrate
argv = sys.argv[1:]
cluster = None
if "--cluster" in argv:                                                 # (first: V_MIN may be negative and must not be taken for an argument)
    k = argv.index("--cluster")
    cluster = dict(v_min=float(argv[k + 1]), r_link=float(argv[k + 2]))
    del argv[k:k + 3]
par = {"--r-cut": 2.4, "--rounds": 3, "--blocks": 5, "--only": ""}
for flag in list(par):
    if flag in argv:
        k = argv.index(flag)
        par[flag] = type(par[flag])(argv[k + 1])
        del argv[k:k + 2]
r_cut, rounds, blocks = par["--r-cut"], par["--rounds"], par["--blocks"]
args = [a for a in argv if not a.startswith("--")]
pressure = "--pressure" in argv
steps = int(args[0]) if len(args) > 0 else 200
dtype = np.float32 if (len(args) > 1 and args[1] == "f32") else np.float64
VARIANTS = ("plain", "general", "plain_ab", "switch", "debye") + (("switch_cluster",) if cluster else ())
names = [v for v in VARIANTS if not par["--only"] or v in par["--only"].split(",")]
pos, L = util.fcc_lattice(40)
pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
N = len(pos)
ONE, TWO = np.zeros(N, dtype=np.int32), (np.arange(N) % 2).astype(np.int32)


def build(name, lo, hi, sigma, c0):
    _abi.check(_abi.load().mtd_coord_set_compiled_pair(0 if name == "general" else 1))      # process-wide: set for the variant that runs
    context.initialize(pos, TWO if name == "plain_ab" else ONE, ["A", "B"], L, dtype=dtype)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=r_cut, r_buff=0.0, check_period=1 << 30, device=True)   # (nothing moves: no displacement checks)
    if name == "debye":
        var = cv.debye_structure_factor(7.695, r_cut, nl, "A", sigma=sigma)
    else:
        var = cv.coordination(1.15, nl, "A", partner="B" if name == "plain_ab" else None, r_cut=r_cut, sigma=sigma,
                              switch=dict(c0=c0, p=8) if name.startswith("switch") else None)
        if name == "switch_cluster":
            var.set_cluster(cluster)
    var.set_grid(lo, hi, 512)
    return meta, var, nl


# one untimed evaluation per variant supplies the value the grid is laid around (sigma 1 % of the range) and, for the switch, c0: the mean
# coordination number, so that h is on its slope
value, c0 = {}, 1.0
for name in [v for v in VARIANTS if v in names or (v == "plain" and ("switch" in names or "switch_cluster" in names))]:
    meta, var, nl = build(name, -1.0, 1.0, 1.0, c0)
    context.run(1)
    value[name] = var.cpp_force.getCurrentValue(1)
    if name == "plain":
        c0 = value[name]
    context.current = None
times = {name: [] for name in names}
entries = {}
for rnd in range(rounds):
    for name in names:
        s0 = value[name]
        lo, hi = min(0.0, 2.0 * s0), max(0.0, 2.0 * s0)
        if s0 == 0.0:                                                   # (a cluster option that leaves nothing solid: any grid will do)
            lo, hi, s0 = -1.0, 1.0, 1.0
        meta, var, nl = build(name, lo, hi, 0.02 * abs(s0), c0)
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
            print("%-9s cv = %.9g, on grid: %s, hills %d, list entries per particle %.1f"
                  % (name, value[name], lo <= var.cpp_force.getCurrentValue(t_now) < hi, meta.cpp_integrator.getNumGaussians(), entries[name] / N))
            if name == "switch_cluster":
                print("%-9s v_min %g, r_link %g: (root, members, clusters, nodes) = %s" % ("", cluster["v_min"], cluster["r_link"], var.get_largest_cluster()))
        context.current = None
print("config 5, N = %d, %s%s, list to %.2f: %d rounds x %d blocks of %d steps, us/step" % (N, np.dtype(dtype).name, ", virial" if pressure else "",
                                                                                         r_cut, rounds, blocks, steps))
for name in names:
    t = np.array(times[name])
    print("  %-14s median %8.1f   min %8.1f   max %8.1f   (%.3e list entries/s incl. CV + force pass)"
          % (name, np.median(t), t.min(), t.max(), entries[name] / (1e-6 * np.median(t))))
print(json.dumps(dict(r_cut=r_cut, cluster=cluster, dtype=np.dtype(dtype).name, virial=pressure, steps=steps, blocks=blocks, rounds=rounds,
                      us_per_step={n: dict(median=float(np.median(times[n])), min=float(min(times[n])), max=float(max(times[n]))) for n in names})))
