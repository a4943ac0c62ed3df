#!/usr/bin/env python3
"""Developer tool: did a step of the host classes move a bit between two trees?  One small run through the Python API for every route
IntegratorMetaDynamics::updateBiasPotential can take (ROWS below: pure and mixed lamellar sets, the mesh alone / beside lamellar
variables / twice, the pressure flag, cv.steinhardt alone and beside a lamellar variable, walkers, adaptive widths, box variables),
fp32 and fp64 particle arrays, 6 steps of stride 2.  The package is imported from the tree this file lies in: copied into an export
of another revision it dumps that revision's values.
usage: tools/host_bits.py dump <out.npz>         CV values, bias factors, hill count, the bias / weight log values, every variable's
                                                 force array and the engine's grid arrays of every row
       tools/host_bits.py compare <a.npz> <b.npz>   np.array_equal on every array; exit status 1 when one differs
tests/test_gpu_step_routes.py runs the same rows and asserts the route of every step (lastStepRoute)."""
import ctypes as C
import os
import sys

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]

AB = dict(A=1.0, B=-1.0)
_probed = {}


def _probe(key, make):
    """the value of a variable whose grid has to be laid around it: one step with the variable alone on a dummy grid"""
    from metadynamics import context, integrate
    if key not in _probed:
        make_system, make_cv = make
        make_system()
        integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
        x = make_cv()
        x.set_grid(0.0, 1.0, 8)
        context.run(1)
        _probed[key] = x.cpp_force.getCurrentValue(1)
        context.current = None
    return _probed[key]


def _integrator(**kw):
    from metadynamics import integrate
    args = dict(dt=0.005, stride=2, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    args.update(kw)
    return integrate.mode_metadynamics(**args)


def _lamellar_system(dtype):
    import util
    from metadynamics import context
    pos, types = util.snapshot_random(5003, 14.0, seed=8, modulated=True, dtype=np.float32)
    context.initialize(pos, types, ["A", "B"], 14.0, dtype=dtype)


def _lamellar(vectors, name, points=32):
    from metadynamics import cv
    x = cv.lamellar(sigma=0.05, mode=AB, lattice_vectors=vectors, name=name)
    x.set_grid(-1.0, 1.0, points)
    return x


def _mesh_system(dtype):
    import util
    from metadynamics import context
    pos, types = util.snapshot_random(8000, 20.0, seed=21, modulated=True, dtype=np.float64)
    context.initialize(pos, types, ["A", "B"], 20.0, dtype=dtype)


def _mesh_value(dtype):
    from metadynamics import cv
    return _probe(("mesh", dtype), (lambda: _mesh_system(dtype), lambda: cv.mesh(nx=16, mode=AB)))


def _mesh(s, points=40):
    from metadynamics import cv
    x = cv.mesh(nx=16, mode=AB, sigma=0.05 * abs(s))
    x.set_grid(0.25 * s, 1.6 * s, points)        # (the value must not sit symmetrically between two nodes: dV/ds pure rounding noise)
    return x


def _fcc_system(dtype):
    import util
    from metadynamics import context
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(12).normal(0, 0.05, pos.shape)
    context.initialize(pos, np.zeros(len(pos), dtype=np.int32), ["A"], L, dtype=dtype)


def _steinhardt(s=None):
    from metadynamics import cv
    nl = cv.nlist_cell(r_cut=1.5)
    nl.update()                                   # a full list built on the host
    x = cv.steinhardt(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=[0, 0, 0, 0, 1, 0, 1], nlist=nl, type="A")
    if s is None:
        return x
    x.sigma = 0.02 * abs(s)
    x.set_grid(0.55 * s, 1.3 * s, 64)
    return x


# every row: build(dtype) -> (integrator, variables), on a fresh context
def row_one_lamellar(dtype, fused=True, **params):
    import util
    _lamellar_system(dtype)
    meta = _integrator()
    lam = _lamellar(util.CV1_VECTORS, "one")
    meta.cpp_integrator.setFusedPath(fused)
    if params:
        meta.set_params(**params)
    return meta, [lam]


def row_four_lamellar(dtype):
    import util
    _lamellar_system(dtype)
    meta = _integrator()
    sets = [util.CV1_VECTORS, util.CV2_VECTORS, [(0, 0, 4)], [(0, 4, 0), (4, 0, 0)]]
    return meta, [_lamellar(v, "v%d" % i, points=6) for i, v in enumerate(sets)]


def row_lamellar_and_umbrella(dtype):
    import util
    _lamellar_system(dtype)
    meta = _integrator()
    one, two = _lamellar(util.CV1_VECTORS, "one"), _lamellar(util.CV2_VECTORS, "two", points=36)
    two.set_params(umbrella="harmonic", kappa=2.0, cv0=0.1)
    return meta, [one, two]


def row_lamellar_and_mesh(dtype, pressure=False, meshes=1):
    import util
    from metadynamics import context
    s = _mesh_value(dtype)                        # (probed on a context of its own)
    _mesh_system(dtype)
    meta = _integrator()
    cvs = [_lamellar(util.CV1_VECTORS, "one", points=12 if meshes > 1 else 32)]
    cvs += [_mesh(s, points=40 if meshes == 1 else 14) for _ in range(meshes)]
    if pressure:
        context.current.system_definition.getParticleData().setPressureFlag(True)
    return meta, cvs


def row_mesh_alone(dtype, fused=True):
    s = _mesh_value(dtype)
    _mesh_system(dtype)
    meta = _integrator()
    meta.cpp_integrator.setFusedPath(fused)
    return meta, [_mesh(s)]


def row_steinhardt(dtype, lamellar=False):
    s = _probe(("steinhardt", dtype), (lambda: _fcc_system(dtype), _steinhardt))
    _fcc_system(dtype)
    meta = _integrator()
    cvs = [_steinhardt(s)]
    if lamellar:
        from metadynamics import cv
        lam = cv.lamellar(sigma=0.05, mode=dict(A=1.0), lattice_vectors=[(0, 0, 3), (3, 0, 0)], name="one")
        lam.set_grid(-1.0, 1.0, 32)
        cvs.append(lam)
    return meta, cvs


def row_box_variables(dtype):
    """test/test_2d.py's set: one particle, density and aspect ratio"""
    from metadynamics import context, cv
    context.initialize(np.zeros((1, 3)), [0], ["A"], 10 ** (1.0 / 3.0), dtype=dtype)
    meta = _integrator(deltaT=1.0)
    density = cv.density(sigma=0.25)
    density.set_grid(cv_min=0, cv_max=1, num_points=20)
    aspect = cv.aspect_ratio(sigma=0.1, dir1=0, dir2=1)
    aspect.set_grid(cv_min=0, cv_max=2, num_points=30)
    return meta, [density, aspect]


ROWS = {
    "one_lamellar": row_one_lamellar,
    "four_lamellar": row_four_lamellar,
    "one_lamellar_unfused": lambda dtype: row_one_lamellar(dtype, fused=False),
    "lamellar_and_umbrella": row_lamellar_and_umbrella,
    "lamellar_and_mesh": row_lamellar_and_mesh,
    "lamellar_and_mesh_pressure": lambda dtype: row_lamellar_and_mesh(dtype, pressure=True),
    "lamellar_and_two_meshes": lambda dtype: row_lamellar_and_mesh(dtype, meshes=2),
    "mesh_alone": row_mesh_alone,
    "mesh_alone_unfused": lambda dtype: row_mesh_alone(dtype, fused=False),
    "steinhardt_alone": row_steinhardt,
    "steinhardt_and_lamellar": lambda dtype: row_steinhardt(dtype, lamellar=True),
    "one_lamellar_walkers": lambda dtype: row_one_lamellar(dtype, multiple_walkers=True),
    "one_lamellar_adaptive": lambda dtype: row_one_lamellar(dtype, adaptive=True, sigma_g=0.02),
    "box_variables": row_box_variables,
}


def state(meta, cvs):
    """everything a step leaves behind that a caller can read"""
    from metadynamics import _abi, context
    lib = _abi.load()
    integ = meta.cpp_integrator
    t = context.current.system.getCurrentTimeStep()
    out = dict(cv=np.array(integ.getCurrentValues()), bias_factors=np.array(integ.getBiasFactors()), n=np.array([integ.getNumGaussians()]),
               V=np.array([integ.getLogValue("bias", t)]), w=np.array([integ.getLogValue("weight", t)]))
    for i, c in enumerate(cvs):
        out["force%d" % i] = np.array(c.cpp_force.getForceArray())
    h = C.c_void_p(integ.getEngineHandle())
    G = lib.mtd_metad_num_elements(h)
    for which, name in enumerate(_abi.ARRAY_NAMES):
        a = np.zeros(G, dtype=np.float64 if which < 6 else np.uint32)
        _abi.check(lib.mtd_metad_get_array(h, which, a.ctypes.data, None))
        out["grid_" + name] = a
    return out


def dump(path):
    import torch  # noqa: F401  (one HIP runtime: torch's, loaded first)
    from metadynamics import context
    out = {}
    for name, build in ROWS.items():
        for dtype in (np.float32, np.float64):
            meta, cvs = build(dtype)
            context.run(6)
            s = state(meta, cvs)
            context.current = None
            for k, v in s.items():
                out["%s/%s/%s" % (name, np.dtype(dtype).name, k)] = v
            print("%-28s %s: cv %s, %d hills, max |F| %.6g" % (name, np.dtype(dtype).name, s["cv"], s["n"][0],
                                                              max(np.abs(s["force%d" % i]).max() for i in range(len(cvs)))))
    np.savez(path, **out)
    print("tree %s -> %s" % (root, path))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    same = sorted(A.files) == sorted(B.files)
    for k in sorted(A.files):
        eq = k in B.files and np.array_equal(A[k], B[k], equal_nan=A[k].dtype.kind == "f")
        same = same and eq
        print("%-56s %s" % (k, "identical bits" if eq else "DIFFERS"))
    print("all identical" if same else "NOT identical")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
