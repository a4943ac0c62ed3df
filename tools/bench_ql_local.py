#!/usr/bin/env python3
"""Developer tool: the config 5 snapshot of tools/bench_ql.py (256 000-particle noisy fcc crystal, lmax 6, degrees 4 and 6,
r_cut 1.4, 512-point grid) with cv.steinhardt_local instead of the global variable; prints us/step.
usage: tools/bench_ql_local.py [steps] [f32|f64] [--device-nlist] [--average] [--switch c0,p] [--gate lo,hi] [--bonds lo,hi] [--cluster v_min,r_link] [--lmax L --ql-ref a,b,...] [--pressure]
(--pressure: sets the pressure flag before the run, as a barostat would: the force pass also writes the per-particle virial;
--device-nlist: cv.nlist_cell(device=True), r_buff 0.4; the next four: the options of cv.steinhardt_local, e.g. --average --switch 0.12,3,
or the solid-bond count --bonds 0.5,0.7 --switch 6.5,12 --ql-ref 0,0,0,0,0,0,1, and with --cluster 0.5,1.2 its largest cluster;
--lmax 12 --ql-ref 0,0,0,0,1,0,1,0,0,0,0.5,0.3,0.25: table rows of 784 bytes, which take the direct force pass instead of the LDS tiles)
Run under rocprofv3 --kernel-trace --stats for the per-kernel table."""
import os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]
import numpy as np, torch
import util
from metadynamics import context, cv, integrate
argv = sys.argv[1:]
options = {}
for flag, keys, kinds in (("--switch", ("c0", "p"), (float, int)), ("--gate", ("n_lo", "n_hi"), (float, float)),
                          ("--bonds", ("d_lo", "d_hi"), (float, float)), ("--cluster", ("v_min", "r_link"), (float, float))):
    if flag in argv:
        k = argv.index(flag)
        options[flag[2:]] = {key: kind(v) for key, kind, v in zip(keys, kinds, argv[k + 1].split(","))}
        del argv[k:k + 2]
lmax, ql_ref = 6, [0, 0, 0, 0, 1, 0, 1]
if "--lmax" in argv:
    k = argv.index("--lmax")
    lmax = int(argv[k + 1])
    del argv[k:k + 2]
if "--ql-ref" in argv:
    k = argv.index("--ql-ref")
    ql_ref = [float(v) for v in argv[k + 1].split(",")]
    del argv[k:k + 2]
if len(ql_ref) != lmax + 1:
    sys.exit("--ql-ref needs lmax + 1 = %d values" % (lmax + 1))
if "--average" in argv:
    options["average"] = True
args = [a for a in argv if not a.startswith("--")]
device_nlist = "--device-nlist" in argv
pressure = "--pressure" in argv
steps = int(args[0]) if len(args) > 0 else 100
dtype = np.float32 if (len(args) > 1 and args[1] == "f32") else np.float64
pos, L = util.fcc_lattice(40)
pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
N = len(pos)


def build(lo, hi, sigma):
    context.initialize(pos, np.zeros(N, dtype=np.int32), ["A"], L, dtype=dtype)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.4, device=device_nlist)
    entries = None if device_nlist else len(nl.update()[2])
    st = cv.steinhardt_local(r_cut=1.4, r_on=1.2, lmax=lmax, Ql_ref=ql_ref, nlist=nl, type="A", sigma=sigma, **options)
    st.set_grid(lo, hi, 512)
    return meta, st, nl, entries


# grid [0, 2 s] x 512, sigma 1 % of the range — one untimed evaluation supplies s
t0 = time.perf_counter()
meta, st, nl, entries = build(0.0, 1.0, 1.0)
context.run(1)
s0 = st.cpp_force.getCurrentValue(1)
print("N = %d, set up in %.1f s, neighbour list %s" % (N, time.perf_counter() - t0, "built on the device" if device_nlist else "built on the host"))
context.current = None
meta, st, nl, entries = build(0.0, 2.0 * s0, 0.02 * s0)
context.run(1)
entries = nl.cpp_nlist.getNumEntries() if entries is None else entries
print("steinhardt_local cv =", s0, "grid", (0.0, 2.0 * s0), "list entries per particle %.1f" % (entries / N))
context.run(5)
torch.cuda.synchronize()
t0 = time.perf_counter()
context.current.system.run(steps)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
t_now = context.current.system.getCurrentTimeStep()
c = st.get_local()
print("on grid: %s, hills %d, bias factors %s, V = %g, mean c_i %.6f, mean n_i %.3f"
      % (0.0 <= st.cpp_force.getCurrentValue(t_now) < 2.0 * s0, meta.cpp_integrator.getNumGaussians(), list(meta.cpp_integrator.getBiasFactors()),
         meta.cpp_integrator.getLogValue("bias", t_now), c.mean(), st.get_coordination().mean()))
if pressure:
    print("virial of the bias force (xx xy xz yy yz zz): %s" % " ".join("%.6e" % w for w in st.get_virial()))
if options:
    print("options %s: mean v_i %.6f" % (options, st.get_switched().mean()))
if "bonds" in options:
    print("mean b_i %.6f" % st.get_bonds().mean())
if "cluster" in options:
    print("largest cluster (root, members, clusters, nodes): %s" % (st.get_largest_cluster(),))
print("config 5 local (%s%s%s): %.1f us/step  (%.3e particle-CV-evals/s, %.3e list entries/s incl. CV + force pass)"
      % (np.dtype(dtype).name + (", virial" if pressure else ""), ", device list" if device_nlist else "", "" if lmax == 6 else ", lmax %d" % lmax, 1e6 * dt / steps, N * steps / dt, 2 * entries * steps / dt))
