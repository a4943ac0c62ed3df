#!/usr/bin/env python3
"""Developer tool: the config 5 snapshot of tools/bench_cn.py (256 000-particle noisy fcc crystal) with cv.tetrahedral as the only
variable of a 512-point well-tempered grid, and cv.coordination with a switch, cv.environment_similarity("fcc") and cv.steinhardt_local
on the SAME list as the yardsticks, in one process: the variants alternate over several rounds, every round times several blocks of
steps, and the table gives the median, the smallest and the largest block of each variant in us/step.  With --only NAME a process runs
one variant: a job script alternates such processes.
usage: tools/bench_tet.py [steps] [f32|f64] [--r-list R] [--rounds K] [--blocks B] [--pressure] [--only NAME[,NAME]] [--cluster V_MIN R_LINK]
(defaults: 200 steps per block, 5 blocks, 3 rounds, f64; the list, built on the device with r_buff 0, reaches 1.5 — ~17 entries per
particle, the first shell, the variable's own use; --r-list 2.4 gives ~80 entries per particle, of which the variables still take the
first shell.  Variants: plain, switch_gate (switch (0.3, 6), gate (6, 11)), penalty (normalise=False), coordination (r_0 = 1.15, (6, 12),
r_cut = the list's reach, switch (c0 = its mean, 8)), env_fcc (sigma_env 0.12), steinhardt_local (lmax 6, degrees 4 and 6).  The window
of the tetrahedral order, of the environment similarity and of the local Steinhardt variable is 1.3 .. 1.5.
--pressure: sets the pressure flag before the run, as a barostat would: the force call also writes the per-particle virial
--cluster V_MIN R_LINK: adds the variants plain_cluster and switch_gate_cluster, those two with set_cluster(dict(v_min=V_MIN,
r_link=R_LINK)): the largest cluster of particles with v_i >= V_MIN; the summary (root, members, clusters, nodes) is printed, because the
cost of the link pass depends on the size of the nucleus.  t_i of the noisy fcc crystal scatters around 3/11)
Run under rocprofv3 --kernel-trace --stats for the per-kernel table."""
import json, os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np, torch
import util
from metadynamics import context, cv, integrate
argv = sys.argv[1:]
cluster = None
if "--cluster" in argv:                                                 # (first: V_MIN may be negative and must not be taken for an argument)
    k = argv.index("--cluster")
    cluster = dict(v_min=float(argv[k + 1]), r_link=float(argv[k + 2]))
    del argv[k:k + 3]
par = {"--r-list": 1.5, "--rounds": 3, "--blocks": 5, "--only": ""}
for flag in list(par):
    if flag in argv:
        k = argv.index(flag)
        par[flag] = type(par[flag])(argv[k + 1])
        del argv[k:k + 2]
r_list, rounds, blocks = par["--r-list"], par["--rounds"], par["--blocks"]
args = [a for a in argv if not a.startswith("--")]
pressure = "--pressure" in argv
steps = int(args[0]) if len(args) > 0 else 200
dtype = np.float32 if (len(args) > 1 and args[1] == "f32") else np.float64
R_ON, R_CUT = 1.3, 1.5
VARIANTS = ("plain", "switch_gate", "penalty", "coordination", "env_fcc", "steinhardt_local") + (("plain_cluster", "switch_gate_cluster") if cluster else ())
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
    elif name == "env_fcc":
        var = cv.environment_similarity(cv.environment_templates("fcc", np.sqrt(2.0)), 0.12, R_CUT, R_ON, nl, "A", sigma=sigma)
    elif name == "steinhardt_local":
        var = cv.steinhardt_local(r_cut=R_CUT, r_on=R_ON, lmax=6, Ql_ref=[0, 0, 0, 0, 1, 0, 1], nlist=nl, type="A", sigma=sigma)
    else:
        var = cv.tetrahedral(R_CUT, R_ON, nl, "A", normalise=name != "penalty", sigma=sigma,
                             switch=dict(c0=0.3, p=6) if name.startswith("switch_gate") else None,
                             gate=dict(n_lo=6.0, n_hi=11.0) if name.startswith("switch_gate") else None)
        if name.endswith("_cluster"):
            var.set_cluster(cluster)
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
        if s0 == 0.0:                                                   # (a cluster option that leaves nothing solid: any grid will do)
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
            print("%-17s cv = %.9g, on grid: %s, hills %d, list entries per particle %.1f"
                  % (name, value[name], lo <= var.cpp_force.getCurrentValue(t_now) < hi, meta.cpp_integrator.getNumGaussians(), entries[name] / N))
            if name.endswith("_cluster"):
                print("%-17s v_min %g, r_link %g: (root, members, clusters, nodes) = %s" % ("", cluster["v_min"], cluster["r_link"], var.get_largest_cluster()))
        context.current = None
print("config 5, N = %d, %s%s, list to %.2f: %d rounds x %d blocks of %d steps, us/step" % (N, np.dtype(dtype).name, ", virial" if pressure else "",
                                                                                         r_list, rounds, blocks, steps))
for name in names:
    t = np.array(times[name])
    print("  %-19s median %8.1f   min %8.1f   max %8.1f   (%.3e list entries/s incl. CV + force pass)"
          % (name, np.median(t), t.min(), t.max(), entries[name] / (1e-6 * np.median(t))))
print(json.dumps(dict(r_list=r_list, cluster=cluster, dtype=np.dtype(dtype).name, virial=pressure, steps=steps, blocks=blocks, rounds=rounds,
                      us_per_step={n: dict(median=float(np.median(times[n])), min=float(min(times[n])), max=float(max(times[n]))) for n in names})))
