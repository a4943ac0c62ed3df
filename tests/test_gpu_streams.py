"""GPU: the stream contract of include/mtd_abi.h — every kernel family on a non-blocking stream of the caller's, through the gate of
tests/stream_gate.py (read its header first).

Every case runs one call sequence three times: on the NULL stream for snapshot B (the warm-up that builds lazy tables, the expected
result, the host time that sizes the delay), on the NULL stream for snapshot A (A's result must differ from B's in every compared
output), and on a stream S behind a delay kernel while the input buffers still hold A and B arrives on S.  The result must be B's NULL
stream result bit for bit: all these paths sum in a fixed order.  The one exception is the third-law half-list force pass of the global
Steinhardt variable with mtd_ql_set_half_list_exact(0), floating-point atomics: it is held to the bound its own parity test uses
(tests/test_gpu_steinhardt.py:122, test_ql_half_list_forces_bitwise_reproducible: 1e-12 of max|F| with fp64 arrays, 2e-6 with fp32).

The call sequences are the runners of the families' own test modules (run_gpu of test_gpu_pair_entropy, test_gpu_env_similarity,
test_gpu_steinhardt, test_gpu_ql_virial, test_gpu_ql_local_avg / _bonds / _virial / _cluster, test_gpu_cluster; GpuMetad, Fused, GpuMesh
and the neighbour list's Handle with a stream); the sequences that had no runner yet are the run_* functions below.

-s prints the calibrated rate of the delay kernel and one line per case: the delay, the host time it was sized from, event pending.
The multi-process paths (mailbox, RCCL, slab mesh) are not run here: a delay kernel in front of a cross-process wait meets
MTD_COMM_TIMEOUT_MS."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_paths
import list_layouts as ll
import stream_gate as sg
import util
from test_gpu_cluster import run_gpu as run_gpu_cluster
from test_gpu_env_similarity import run_gpu as run_gpu_es
from test_gpu_fused import Fused
from test_gpu_mesh import GpuMesh, assign_info
from test_gpu_metad import GpuMetad
from test_gpu_nlist import Handle
from test_gpu_pair_entropy import run_gpu as run_gpu_pe
from test_gpu_ql_local_avg import run_gpu as run_gpu_opt
from test_gpu_ql_local_bonds import run_gpu as run_gpu_bonds
from test_gpu_ql_local_cluster import API_OPT, COMBO, _kw
from test_gpu_ql_local_cluster import reference as cluster_reference
from test_gpu_ql_local_cluster import run_gpu as run_gpu_ql_cluster
from test_gpu_ql_local_cluster import system as cluster_system
from test_gpu_ql_local_virial import run_gpu as run_gpu_local_virial
from test_gpu_ql_virial import run_gpu as run_gpu_ql_virial
from test_gpu_steinhardt import run_gpu as run_gpu_ql

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N = 4099                                                                 # no multiple of 64 or 256: 17 blocks of 256 with a ragged last one
DTYPES = [np.float32, np.float64]
CVS = [(util.CV1_VECTORS, util.MODE_AB), (util.CV2_VECTORS, util.MODE_AB)]
QL_46 = [0, 0, 0, 0, 1, 0, 1]


def _dt(abi, dtype):
    return abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64


def _tdt(dtype):
    return torch.float32 if dtype == np.float32 else torch.float64


# ---- snapshots: built once, shared, never changed ---------------------------------------------------------------------------------------

_cache = {}


def lamellar_snapshots(dtype, n=N, L=30.0):
    """(A, B): two modulated random snapshots (util.snapshot_random) as packed postype arrays, every particle wrapped into the box"""
    key = ("lam", np.dtype(dtype).name, n)
    if key not in _cache:
        out = []
        for seed in (101, 202):
            pos, types = util.snapshot_random(n, L, seed=seed, modulated=True, dtype=dtype)
            pos = (np.mod(pos.astype(np.float64) + L / 2, L) - L / 2).astype(dtype)
            pos = np.clip(pos, -L / 2, np.nextafter(dtype(L / 2), dtype(0)))
            out.append(dict(pos=pos, types=types, L=L, postype=util.pack_postype(pos, types, dtype)))
        _cache[key] = tuple(out)
    return _cache[key]


def liquid_snapshots(dtype, n=N, r_list=1.55, seeds=(303, 404)):
    """(A, B): two random snapshots at density 0.8, all of type 0, rounded to the dtype, with their full lists at r_list.  A is the one
    with the shorter list array: stale rows of A, read with the sizes of B, stay inside every buffer sized for B"""
    key = ("liq", np.dtype(dtype).name, n, r_list, seeds)
    if key not in _cache:
        L = (n / 0.8) ** (1.0 / 3.0)
        out = []
        for seed in seeds:
            pos, _ = util.snapshot_random(n, L, seed=seed, dtype=dtype)
            pos = pos.astype(np.float64)
            out.append(dict(pos=pos, types=np.zeros(n, dtype=np.int32), L=L, nl=util.build_nlist(pos, L, r_list)))
        out.sort(key=lambda s: len(s["nl"][2]))
        assert len(out[0]["nl"][2]) < len(out[1]["nl"][2])
        _cache[key] = tuple(out)
    return _cache[key]


def crystal_snapshots(dtype, cells=10, r_list=1.55):
    """(A, B): fcc crystals of cells^3 x 4 particles with noise 0.08 and 0.05 (different seeds) and their full lists, A's the shorter"""
    key = ("fcc", np.dtype(dtype).name, cells, r_list)
    if key not in _cache:
        out = []
        for seed, noise in ((5, 0.08), (6, 0.05)):
            pos, L = util.fcc_lattice(cells)
            pos = (pos + np.random.default_rng(seed).normal(0, noise, pos.shape)).astype(dtype).astype(np.float64)
            out.append(dict(pos=pos, types=np.zeros(len(pos), dtype=np.int32), L=L, nl=util.build_nlist(pos, L, r_list)))
        out.sort(key=lambda s: len(s["nl"][2]))
        _cache[key] = tuple(out)
    return _cache[key]


def listed(s, **more):
    """the positional part of the list runners' arguments as keywords"""
    return dict(pos=s["pos"], types=s["types"], L=s["L"], nl=s["nl"], **more)


# ---- runners of the sequences that had none ---------------------------------------------------------------------------------------------

def run_lamellar(abi, postype, L, dtype, bias, gate=None):
    """mtd_lamellar_cv_partials -> mtd_reduce_partials -> mtd_lamellar_forces, the bias factors read from device doubles: dict(cv, F0, F1)"""
    lib = abi.load()
    gate = gate or sg.Plain()
    n = len(postype)
    box, lset, dt = abi.Box.make(L), abi.LamellarSet.make(CVS), _dt(abi, dtype)
    d_pos = gate.inp(postype)
    d_bias = gate.inp(np.asarray(bias, dtype=np.float64))
    scratch = torch.full((lib.mtd_lamellar_scratch_doubles(n),), float("nan"), dtype=torch.float64, device="cuda")
    cv = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    forces = [torch.full((n, 4), float("nan"), dtype=_tdt(dtype), device="cuda") for _ in CVS]
    fptr = (C.c_void_p * 2)(*[f.data_ptr() for f in forces])
    n_part = C.c_uint()
    stream = gate.arm()
    abi.check(lib.mtd_lamellar_cv_partials(C.byref(lset), n, abi.ptr(d_pos), dt, C.byref(box), abi.ptr(scratch), C.byref(n_part), stream))
    abi.check(lib.mtd_reduce_partials(abi.ptr(scratch), n_part.value, 2, 2, 1.0 / n, 0.0, abi.ptr(cv), stream))
    abi.check(lib.mtd_lamellar_forces(C.byref(lset), n, abi.ptr(d_pos), fptr, dt, n, abi.ptr(d_bias), C.byref(box), stream))
    return gate.done(lambda: dict(cv=cv.cpu().numpy(), F0=forces[0].cpu().numpy(), F1=forces[1].cpu().numpy()))


def run_lamellar_cv(abi, postype, L, dtype, gate=None):
    """mtd_lamellar_cv_partials -> mtd_reduce_partials alone: dict(cv)"""
    lib = abi.load()
    gate = gate or sg.Plain()
    n = len(postype)
    box, lset, dt = abi.Box.make(L), abi.LamellarSet.make(CVS), _dt(abi, dtype)
    d_pos = gate.inp(postype)
    scratch = torch.full((lib.mtd_lamellar_scratch_doubles(n),), float("nan"), dtype=torch.float64, device="cuda")
    cv = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    n_part = C.c_uint()
    stream = gate.arm()
    abi.check(lib.mtd_lamellar_cv_partials(C.byref(lset), n, abi.ptr(d_pos), dt, C.byref(box), abi.ptr(scratch), C.byref(n_part), stream))
    abi.check(lib.mtd_reduce_partials(abi.ptr(scratch), n_part.value, 2, 2, 1.0 / n, 0.0, abi.ptr(cv), stream))
    return gate.done(lambda: dict(cv=cv.cpu().numpy()))


def run_dropin(abi, postype, L, dtype, gate=None):
    """mtd_calculate_fourier_modes / mtd_compute_sq_forces (one CV, 12 modes, host bias): dict(modes, F)"""
    lib = abi.load()
    gate = gate or sg.Plain()
    n = len(postype)
    lat = util.CV1_VECTORS + [(1, 1, 1), (2, -1, 0), (0, 1, -2), (5, 0, 1)]
    mode = [1.0, -0.5]
    box, dt = abi.Box.make(L), _dt(abi, dtype)
    d_pos = gate.inp(postype)
    scratch = torch.full((lib.mtd_lamellar_scratch_doubles(n),), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((2 * len(lat),), float("nan"), dtype=torch.float64, device="cuda")
    force = torch.full((n, 4), float("nan"), dtype=_tdt(dtype), device="cuda")
    stream = gate.arm()
    abi.check(lib.mtd_calculate_fourier_modes(len(lat), util.flat_lattice(lat), n, abi.ptr(d_pos), dt, util.dbl_array(mode), 2, abi.ptr(out),
                                              abi.ptr(scratch), C.byref(box), stream))
    abi.check(lib.mtd_compute_sq_forces(n, abi.ptr(d_pos), abi.ptr(force), dt, len(lat), util.flat_lattice(lat), util.dbl_array(mode), 2, n, 2.5,
                                        C.byref(box), stream))
    return gate.done(lambda: dict(modes=out.cpu().numpy(), F=force.cpu().numpy()))


def run_wte(abi, nf, nt, nv, dtype, bias, which, gate=None):
    """which = "energy": mtd_wte_energy_partials + mtd_reduce_partials -> dict(pe); "wte" / "wrapper": mtd_wte_scale_netforce /
    mtd_wrapper_scale_forces with the bias factor in device memory -> dict(f, t, v), the arrays scaled in place"""
    lib = abi.load()
    gate = gate or sg.Plain()
    n, pitch, dt = len(nf), nv.shape[1], _dt(abi, dtype)
    d_nf, d_nt, d_nv = gate.inp(nf), gate.inp(nt), gate.inp(nv)
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    parts = torch.full((lib.mtd_wte_scratch_doubles(n),), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    n_part = C.c_uint()
    stream = gate.arm()
    if which == "energy":
        abi.check(lib.mtd_wte_energy_partials(n, abi.ptr(d_nf), dt, abi.ptr(parts), C.byref(n_part), stream))
        abi.check(lib.mtd_reduce_partials(abi.ptr(parts), n_part.value, 1, 1, 1.0, 3.5, abi.ptr(out), stream))
        return gate.done(lambda: dict(pe=out.cpu().numpy()))
    fn = lib.mtd_wte_scale_netforce if which == "wte" else lib.mtd_wrapper_scale_forces
    abi.check(fn(n, abi.ptr(d_nf), abi.ptr(d_nt), abi.ptr(d_nv), pitch, dt, abi.ptr(d_bias), 0.0, 1, stream))
    return gate.done(lambda: dict(f=d_nf.cpu().numpy(), t=d_nt.cpu().numpy(), v=d_nv.cpu().numpy()))


def run_update_grid(abi, cur, gate=None):
    """mtd_update_grid (the drop-in of gpu_update_grid) on a 20 x 30 grid, the current value in device memory: dict(delta)"""
    lib = abi.load()
    gate = gate or sg.Plain()
    d_cur = gate.inp(np.asarray(cur, dtype=np.float64))
    d_delta = torch.full((600,), 0.25, dtype=torch.float64, device="cuda")
    stream = gate.arm()
    abi.check(lib.mtd_update_grid(600, util.uint_array([20, 30]), 2, abi.ptr(d_cur), abi.ptr(d_delta), util.dbl_array([0.0, 0.0]),
                                  util.dbl_array([1.0, 2.0]), util.dbl_array([4.0, 0.0, 0.0, 10.0]), 0.8, 1.5, stream))
    return gate.done(lambda: dict(delta=d_delta.cpu().numpy()))


def run_sigma(abi, forces, dtype, gate=None):
    """mtd_sigma_products with three variables, the middle one without derivatives; SYNCHRONISES: dict(sigmasq)"""
    lib = abi.load()
    gate = gate or sg.Plain()
    n = len(forces[0])
    d_f = [gate.inp(f) for f in forces]
    scratch = torch.full((lib.mtd_sigma_scratch_doubles(),), float("nan"), dtype=torch.float64, device="cuda")
    fptr = (C.c_void_p * 3)(d_f[0].data_ptr(), None, d_f[1].data_ptr())
    sigmasq = (C.c_double * 9)(*([float("nan")] * 9))
    stream = gate.arm()
    abi.check(lib.mtd_sigma_products(3, fptr, n, _dt(abi, dtype), 0.7, abi.ptr(scratch), sigmasq, stream))
    gate.synced()
    host = np.array(sigmasq[:])
    return gate.done(lambda: dict(sigmasq=host))


def closing(read, *handles):
    """read() followed by close() of the handles: a runner's handles live until its outputs are read, which a deferred read (two
    streams) does after the runner has returned"""
    def wrapped():
        try:
            return read()
        finally:
            for h in handles:
                h.close()
    return wrapped


GRID = dict(sigma=[0.05, 0.05], cv_min=[-1.0, -1.0], cv_max=[1.0, 1.0], num_points=[64, 64], W=1.0, T_shift=7.0, T=1.0, stride=2, mode="well_tempered")


def grid_trajectory(seed, steps=8, n_part=5):
    """[steps, n_part, 2] partial sums whose column sums walk over the 64 x 64 grid of GRID: CV c of step t is the sum over the rows"""
    rng = np.random.default_rng(seed)
    target = np.cumsum(rng.normal(0, 0.06, (steps, 2)), axis=0) + rng.uniform(-0.3, 0.3, 2)
    parts = rng.normal(0, 0.2, (steps, n_part, 2))
    parts[:, 0, :] += target - parts.sum(axis=1)
    assert np.abs(parts.sum(axis=1)).max() < 0.9
    return parts


def _engine_result(g, abi, more=None):
    st = g.state()
    out = dict(cv=st["cv"], bias=st["bias"], V=st["V"], w=st["w"], num_gaussians=st["num_gaussians"])
    out.update({name: g.array(name) for name in abi.ARRAY_NAMES})
    out.update(more or {})
    return out


def run_grid(abi, traj, variant="plain", late=False, gate=None):
    """eight mtd_metad_update_bias steps on the 64 x 64 well-tempered grid, both CV values from device partial sums that are rewritten
    on the stream before every step, no host synchronise inside; then mtd_metad_get_state and every mtd_metad_get_array, which must
    have waited.  variant "reset+set": mtd_metad_reset_histogram behind step 3 and mtd_metad_set_array(grid) behind step 5;
    "touched": a device write into the bias grid through mtd_metad_device_array(0) behind step 5, followed by mtd_metad_grid_touched;
    "phases": every step as mtd_metad_update_phase_a + mtd_metad_update_phase_b, mtd_metad_set_num_gaussians(40) behind step 3;
    "walkers": every step as mtd_metad_update_bias_walkers without a communicator (one walker).
    late: state and arrays are read in the runner's read-back instead (nothing synchronises before it)"""
    gate = gate or sg.Plain()
    d_traj = gate.inp(traj)
    steps, n_part, n_cv = traj.shape
    parts = torch.zeros((n_part, n_cv), dtype=torch.float64, device="cuda")
    tmp = torch.zeros(1, dtype=torch.float64, device="cuda")
    g = GpuMetad(abi, **GRID)
    lib = g.lib
    try:
        d_grid = lib.mtd_metad_device_array(g.h, 0)                     # before the first step: only grid_touched tells of the write
        for c in range(n_cv):
            abi.check(lib.mtd_metad_set_cv_source(g.h, c, abi.ptr(parts), n_part, n_cv, c, 1.0, 0.0))
        bump = np.zeros(g.len)
        bump[32 * 64 + 30:32 * 64 + 34] = 2.5
        g.stream = gate.arm()
        for t in range(steps):
            parts.copy_(d_traj[t])                                       # on the current stream: S in a gated run
            if variant == "phases":
                dep = C.c_int(-1)
                abi.check(lib.mtd_metad_update_phase_a(g.h, t, C.byref(dep), g.stream))
                assert dep.value == (1 if t % 2 == 0 else 0)
                abi.check(lib.mtd_metad_update_phase_b(g.h, dep.value, g.stream))
                if t == 3:                                               # synchronises like mtd_metad_set_array (the header's block on the raw arrays)
                    gate.queued()
                    abi.check(lib.mtd_metad_set_num_gaussians(g.h, 40, g.stream))
                    gate.synced()
            elif variant == "walkers":
                abi.check(lib.mtd_metad_update_bias_walkers(g.h, None, t, g.stream))
            else:
                abi.check(lib.mtd_metad_update_bias(g.h, t, g.stream))
            if variant == "reset+set" and t == 3:
                abi.check(lib.mtd_metad_reset_histogram(g.h, g.stream))
            if variant == "reset+set" and t == 5:
                gate.queued()
                abi.check(lib.mtd_metad_set_array(g.h, 0, bump.ctypes.data, g.stream))
                gate.synced()
            if variant == "touched" and t == 5:
                for k, idx in enumerate((31 * 64 + 31, 32 * 64 + 32, 33 * 64 + 31)):
                    abi.check(lib.mtd_reduce_partials(d_grid + 8 * idx, 1, 1, 1, 1.0, 0.75 + 0.5 * k, tmp.data_ptr(), g.stream))
                    abi.check(lib.mtd_reduce_partials(tmp.data_ptr(), 1, 1, 1, 1.0, 0.0, d_grid + 8 * idx, g.stream))
                abi.check(lib.mtd_metad_grid_touched(g.h, g.stream))
        if late:
            return gate.done(closing(lambda: _engine_result(g, abi), g))
        if variant not in ("reset+set", "phases"):
            gate.queued()
        st = g.state()
        gate.synced()
        arrays = {name: g.array(name) for name in abi.ARRAY_NAMES}
        gate.synced()
        out = dict(cv=st["cv"], bias=st["bias"], V=st["V"], w=st["w"], num_gaussians=st["num_gaussians"], **arrays)
        return gate.done(closing(lambda: out, g))
    except BaseException:
        g.close()
        raise


def run_touched_on_path(abi, shift, gate=None):
    """the cached patch hit right behind a device write: eight `hit` steps of tests/grid_paths.py on its 2-d grid, a write of `shift`
    (a device double) into the cell of the walk's centre through mtd_metad_device_array(0), mtd_metad_grid_touched on the same
    stream, six more `hit` steps: the bias factors of every step (copied out by a kernel), then state and grid"""
    gate = gate or sg.Plain()
    kw = grid_paths.settings(2)
    walk = grid_paths.values(grid_paths.hit_walk(2, 14), 2)
    assert all(label == "hit" for _, label in walk[1:])
    d_shift = gate.inp(np.array([shift], dtype=np.float64))
    d_vals = torch.tensor([v for v, _ in walk], dtype=torch.float64, device="cuda")
    rows = torch.full((len(walk), 2), float("nan"), dtype=torch.float64, device="cuda")
    val = torch.zeros(2, dtype=torch.float64, device="cuda")
    g = GpuMetad(abi, **kw)
    lib = g.lib
    try:
        d_grid = lib.mtd_metad_device_array(g.h, 0)
        n, c0 = kw["num_points"], grid_paths.centre(2)
        idx = c0[0] + n[0] * c0[1]
        for c in range(2):
            abi.check(lib.mtd_metad_set_cv_source(g.h, c, abi.ptr(val), 1, 2, c, 1.0, 0.0))
        g.stream = gate.arm()
        for t in range(len(walk)):
            val.copy_(d_vals[t])
            if t == 8:                                                   # grid[idx] <- grid[idx] + shift, as two kernels on the stream
                abi.check(lib.mtd_reduce_partials(d_grid + 8 * idx, 1, 1, 1, 1.0, 0.0, val.data_ptr(), g.stream))
                val[0:1].add_(d_shift)
                abi.check(lib.mtd_reduce_partials(val.data_ptr(), 1, 1, 1, 1.0, 0.0, d_grid + 8 * idx, g.stream))
                abi.check(lib.mtd_metad_grid_touched(g.h, g.stream))
                val.copy_(d_vals[t])
            abi.check(lib.mtd_metad_update_bias(g.h, t, g.stream))
            abi.check(lib.mtd_reduce_partials(lib.mtd_metad_bias_device(g.h), 1, 2, 2, 1.0, 0.0, rows.data_ptr() + 16 * t, g.stream))
        return gate.done(closing(lambda: dict(rows=rows.cpu().numpy(), **_engine_result(g, abi)), g))
    except BaseException:
        g.close()
        raise


def fused_trajectory(dtype, seed, steps=6, L=30.0):
    """[steps, N, 4] packed postype arrays: a modulated snapshot whose modulation grows from step to step"""
    key = ("traj", np.dtype(dtype).name, seed, steps)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        base = rng.random((N, 3)) * L - L / 2
        types = (np.arange(N) % 2).astype(np.int32)
        a = np.where(types == 0, 1.0, -1.0)
        out = []
        for t in range(steps):
            pos = base.copy()
            pos[:, 2] += (1.0 + 0.15 * t) * a * np.sin(2 * np.pi * 3 * pos[:, 2] / L)
            pos[:, 0] += (0.4 + 0.1 * t) * a * np.sin(2 * np.pi * (pos[:, 0] + pos[:, 1] + pos[:, 2]) / L)
            out.append(util.pack_postype(pos.astype(dtype), types, dtype))
        _cache[key] = np.stack(out)
    return _cache[key]


FUSED_GRID = dict(sigma=[0.05, 0.05], cv_min=[-1.0, -1.0], cv_max=[1.0, 1.0], num_points=[64, 64], W=1.0, T_shift=7.0, T=1.0, stride=2,
                  mode="well_tempered")


def run_fused(abi, traj, dtype, form, L=30.0, gate=None):
    """six bias steps of 2 lamellar CVs x 8 modes on 4 099 particles, the positions replaced on the stream between the steps.
    form "passes": mtd_fused_cv_pass + mtd_fused_force_pass; "step0" / "step1": mtd_fused_step in the two-launch form and as the
    persistent kernel; "slots": mtd_fused_force_pass_slots with the permuted slot map (1, 0).  The forces of every step are kept by a
    device copy; the engine's state and arrays are read at the end"""
    gate = gate or sg.Plain()
    lib = abi.load()
    d_traj = gate.inp(traj)
    steps = len(traj)
    box = abi.Box.make(L)
    d_pos = torch.zeros((N, 4), dtype=_tdt(dtype), device="cuda")
    kept = torch.full((steps, 2, N, 4), float("nan"), dtype=_tdt(dtype), device="cuda")
    g = GpuMetad(abi, **FUSED_GRID)
    try:
        cvs = CVS if form != "slots" else [CVS[1], CVS[0]]
        f = Fused(abi, g, N, dtype, one_launch=form == "step1", cvs=cvs)
        slots = util.uint_array([1, 0])
        n_part = C.c_uint()
        if form == "step0":
            abi.check(lib.mtd_fused_step_set_mode(g.h, 0))
        g.stream = f.stream = gate.arm()
        for t in range(steps):
            d_pos.copy_(d_traj[t])
            if form == "passes" or form == "step1":
                f.step(t, d_pos, box)
            elif form == "step0":
                abi.check(lib.mtd_fused_step(g.h, C.byref(f.lset), N, abi.ptr(d_pos), f.fptr, f.dt, N, C.byref(box), abi.ptr(f.scratch), t, f.stream))
                assert lib.mtd_fused_step_launches(g.h) == 2
            else:
                abi.check(lib.mtd_fused_cv_pass(g.h, C.byref(f.lset), N, abi.ptr(d_pos), f.dt, C.byref(box), abi.ptr(f.scratch), C.byref(n_part),
                                                f.stream))
                if t == 0:
                    for c in range(2):
                        abi.check(lib.mtd_metad_set_cv_source(g.h, slots[c], abi.ptr(f.scratch), n_part.value, 2, c, 1.0 / N, 0.0))
                abi.check(lib.mtd_fused_force_pass_slots(g.h, C.byref(f.lset), slots, N, abi.ptr(d_pos), f.fptr, f.dt, N, C.byref(box), t, f.stream))
            for c in range(2):
                kept[t, c].copy_(f.forces[c])
        return gate.done(closing(lambda: dict(F=kept.cpu().numpy(), **_engine_result(g, abi)), g))
    except BaseException:
        g.close()
        raise


MESH_MODE = [1.0, -1.0]


def run_mesh(abi, two, dims, dtype, variant, s_mesh=None, new_table=True, L=30.0, gate=None):
    """two: [2, N, 4] packed postype arrays, the second a displaced copy of the first.  mtd_mesh_compute_cv on the first (the counting
    pipeline) and, with the displaced snapshot arriving on the stream in between, on the second (the bin pipeline), each reduced to a
    device double; then by variant
      "forces"   mtd_mesh_forces with the bias factor in device memory, then the synchronising calls mtd_mesh_assign_info,
                 mtd_mesh_qmax, mtd_mesh_virial (with a table in use) and mtd_mesh_get_array(0)
      "setters"  a first table in use from the start; between the two evaluations mtd_mesh_set_table with a second table (new_table =
                 False: the first one again) and mtd_mesh_set_bug_compat(0), both documented to synchronise the device, the table first
                 so that it is the call that meets the queued evaluation; forces and mtd_mesh_virial, the one reader of the table,
                 behind the second evaluation.  (mtd_mesh_virial synchronises itself: no reader of a table can be left queued.)
      "setters2" the same with mtd_mesh_set_bug_compat first: each setter in turn is the one that meets the queued evaluation
      "merged"   mtd_mesh_set_lamellar_rider in front of the second evaluation and mtd_mesh_forces_update_bias (one lamellar rider,
                 a 2-d grid of 16 x 12 points: one 256-cell grid block; the mesh variable's range is laid around s_mesh) behind it
      "split"    the second evaluation as mtd_mesh_assign + mtd_mesh_spectral; forces behind it
      "plain"    mtd_mesh_forces alone"""
    gate = gate or sg.Plain()
    lib = abi.load()
    d_two = gate.inp(two)
    d_bias = gate.inp(np.array([0.8], dtype=np.float64))
    box, dt = abi.Box.make(L), _dt(abi, dtype)
    d_pos = torch.zeros((N, 4), dtype=_tdt(dtype), device="cuda")
    cv = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    f_mesh = torch.full((N, 4), float("nan"), dtype=_tdt(dtype), device="cuda")
    f_lam = torch.full((N, 4), float("nan"), dtype=_tdt(dtype), device="cuda")
    K = np.linspace(1.0, 0.2, 32)
    dK = np.linspace(-0.5, -0.1, 32)
    m = GpuMesh(abi, dims, MESH_MODE, N)
    g = None
    try:
        setters = variant in ("setters", "setters2")
        if variant == "forces" or setters:
            abi.check(lib.mtd_mesh_set_table(m.h, util.dbl_array(K), util.dbl_array(dK), 32, 0.0, 20.0))
            abi.check(lib.mtd_mesh_set_use_table(m.h, 1))
        if variant == "merged":
            kw = dict(FUSED_GRID, cv_min=[-1.0, 0.0], cv_max=[1.0, 2.0 * s_mesh], sigma=[0.05, 0.05 * s_mesh], num_points=[16, 12], stride=1)
            g = GpuMetad(abi, **kw)
            lset = abi.LamellarSet.make(CVS[:1])
            lam_parts = torch.full((lib.mtd_lamellar_scratch_doubles(N),), float("nan"), dtype=torch.float64, device="cuda")
            n_lam = C.c_uint()
            fptr = (C.c_void_p * 1)(f_lam.data_ptr())
        m.stream = gate.arm()
        if g is not None:
            g.stream = m.stream
        d_pos.copy_(d_two[0])
        m.enqueue_cv(d_pos, dt, box, N, cv[0:1])
        if setters:
            K2, dK2 = (np.linspace(0.7, 0.4, 24), np.linspace(-0.2, -0.9, 24)) if new_table else (K, dK)
            gate.queued()
            if variant == "setters2":
                abi.check(lib.mtd_mesh_set_bug_compat(m.h, 0))
                gate.synced()                                            # the first evaluation has run: with the old tables
            abi.check(lib.mtd_mesh_set_table(m.h, util.dbl_array(K2), util.dbl_array(dK2), len(K2), 0.0, 20.0))
            gate.synced()
            if variant == "setters":
                abi.check(lib.mtd_mesh_set_bug_compat(m.h, 0))
                gate.synced()
        d_pos.copy_(d_two[1])
        if variant == "merged":
            abi.check(lib.mtd_mesh_set_lamellar_rider(m.h, g.h, C.byref(lset), C.byref(box), N, abi.ptr(lam_parts), C.byref(n_lam), m.stream))
        parts, n_parts = C.c_void_p(), C.c_uint()
        if variant == "split":
            abi.check(lib.mtd_mesh_assign(m.h, N, abi.ptr(d_pos), dt, C.byref(box), m.stream))
            abi.check(lib.mtd_mesh_spectral(m.h, C.byref(box), N, C.byref(parts), C.byref(n_parts), m.stream))
        else:
            abi.check(lib.mtd_mesh_compute_cv(m.h, N, abi.ptr(d_pos), dt, C.byref(box), N, C.byref(parts), C.byref(n_parts), m.stream))
        abi.check(lib.mtd_reduce_partials(parts.value, n_parts.value, 1, 1, 0.5, 0.0, abi.ptr(cv[1:2]), m.stream))
        more = {}
        if variant == "merged":
            abi.check(lib.mtd_metad_set_cv_source(g.h, 0, abi.ptr(lam_parts), n_lam.value, 1, 0, 1.0 / N, 0.0))
            abi.check(lib.mtd_metad_set_cv_source(g.h, 1, parts.value, n_parts.value, 1, 0, 0.5, 0.0))
            slots = util.uint_array([0])
            abi.check(lib.mtd_mesh_forces_update_bias(m.h, g.h, 1, C.byref(lset), slots, N, abi.ptr(d_pos), abi.ptr(f_mesh), fptr, dt, N,
                                                      C.byref(box), 0, m.stream))
        else:
            m.enqueue_forces(d_pos, dt, box, N, f_mesh, d_bias)
        if variant == "forces":
            gate.queued()
            more["pipeline"] = np.array(assign_info(abi, m))
            gate.synced()
            q = (C.c_double * 4)()
            abi.check(lib.mtd_mesh_qmax(m.h, C.byref(box), N, q, m.stream))
            gate.synced()
            vir = (C.c_double * 6)()
            abi.check(lib.mtd_mesh_virial(m.h, C.byref(box), N, 0.8, vir, m.stream))
            gate.synced()
            more.update(qmax=np.array(q[:]), virial=np.array(vir[:]), mesh=m.array(0))
            gate.synced()

        if setters:
            vir = (C.c_double * 6)()
            abi.check(lib.mtd_mesh_virial(m.h, C.byref(box), N, 0.8, vir, m.stream))
            gate.synced()
            more["virial"] = np.array(vir[:])

        def read():
            out = dict(cv=cv.cpu().numpy(), F=f_mesh.cpu().numpy(), **more)
            if variant == "merged":
                out.update(F_lam=f_lam.cpu().numpy(), **{"engine_" + k: v for k, v in _engine_result(g, abi).items()})
            return out
        return gate.done(closing(read, m, *([g] if g is not None else [])))
    except BaseException:
        m.close()
        if g is not None:
            g.close()
        raise


def mesh_pair(dtype, seeds=(101, 202)):
    """(A, B): [2, N, 4] arrays of two snapshots each followed by a copy displaced by up to 0.3, wrapped into the box"""
    key = ("mesh", np.dtype(dtype).name, seeds)
    if key not in _cache:
        out = []
        for s in lamellar_snapshots(dtype):
            rng = np.random.default_rng(len(out) + 7)
            L = s["L"]
            moved = s["pos"].astype(np.float64) + rng.uniform(-0.3, 0.3, s["pos"].shape)
            moved = (np.mod(moved + L / 2, L) - L / 2).astype(dtype)
            moved = np.clip(moved, -L / 2, np.nextafter(dtype(L / 2), dtype(0)))
            out.append(np.stack([s["postype"], util.pack_postype(moved, s["types"], dtype)]))
        _cache[key] = tuple(out)
    return _cache[key]


def run_nlist(abi, two, L, dtype, r_list=1.5, r_buff=0.4, gate=None):
    """two: [2, N, 4], the second a displaced copy of the first.  mtd_nlist_build on the first (synchronises once, for the entry count),
    mtd_nlist_check after the displacement has arrived on the stream (synchronises), the rebuild that follows: both lists as sorted rows,
    the verdict of the check"""
    gate = gate or sg.Plain()
    d_two = gate.inp(two)
    n = two.shape[1]
    box, dt = abi.Box.make(L), _dt(abi, dtype)
    d_pos = torch.zeros((n, 4), dtype=_tdt(dtype), device="cuda")
    stream = gate.arm()
    h = Handle(abi, stream=stream, wait=torch.cuda.current_stream())
    try:
        d_pos.copy_(d_two[0])
        rc, first = h.build_device(d_pos, dt, n, n, box, r_list, after_build=gate.synced)
        abi.check(rc)
        d_pos.copy_(d_two[1])
        needs = h.check_device(d_pos, dt, box, r_buff)
        gate.synced()
        rc, second = h.build_device(d_pos, dt, n, n, box, r_list, after_build=gate.synced)
        abi.check(rc)
        rows = lambda lists: np.concatenate([np.sort(r) for r in ll.as_rows(lists)] + [np.asarray(lists[1]).astype(np.int64)])
        out = dict(first=rows(first), second=rows(second), needs=np.array([needs]), n_first=np.array([len(first[2])]),
                   n_second=np.array([len(second[2])]))
        return gate.done(closing(lambda: out, h))
    except BaseException:
        h.close()
        raise


def run_symmetrize(abi, half, n, workspace=True, gate=None):
    """mtd_ql_symmetrize_half_list_ws (one synchronisation, for the entry count; the fill is stream-ordered), or without a workspace
    mtd_ql_symmetrize_half_list (synchronous): the full list's arrays"""
    lib = abi.load()
    gate = gate or sg.Plain()
    fn = abi.bind("mtd_ql_symmetrize_half_list_ws", C.c_int, [C.c_uint] + [C.c_void_p] * 6 + [C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p])
    ws_uints = abi.bind("mtd_ql_symmetrize_workspace_uints", C.c_size_t, [C.c_uint])
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in half)
    cap = 2 * len(half[2]) + 64
    f_head = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    f_nn = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    f_nl = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(ws_uints(n), dtype=torch.int32, device="cuda")
    n_full = C.c_size_t()
    stream = gate.arm()
    if workspace:
        abi.check(fn(n, abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), abi.ptr(f_head), abi.ptr(f_nn), abi.ptr(f_nl), cap, C.byref(n_full),
                     abi.ptr(ws), stream))
    else:
        abi.check(lib.mtd_ql_symmetrize_half_list(n, abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), abi.ptr(f_head), abi.ptr(f_nn), abi.ptr(f_nl),
                                                  cap, C.byref(n_full), stream))
    gate.synced()
    count = n_full.value
    return gate.done(lambda: dict(head=f_head.cpu().numpy(), nn=f_nn.cpu().numpy(), lst=f_nl.cpu().numpy()[:count], count=np.array([count])))


def run_ql_merged(abi, pos, types, L, nl, dtype, virial=False, gate=None):
    """mtd_ql_accumulate_local -> mtd_ql_finalize_update_bias on a 1-d grid -> mtd_ql_forces with the engine's device bias factor (the
    deferred pass of the deposit rides in it), two steps; virial: mtd_ql_finalize + mtd_metad_update_bias + mtd_ql_forces_virial instead"""
    lib = abi.load()
    gate = gate or sg.Plain()
    n = len(pos)
    box, dt = abi.Box.make(L), _dt(abi, dtype)
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    scratch = torch.zeros(lib.mtd_ql_scratch_doubles(6), dtype=torch.float64, device="cuda")
    force = torch.full((n, 4), float("nan"), dtype=_tdt(dtype), device="cuda")
    vir = torch.full((6, n), float("nan"), dtype=_tdt(dtype), device="cuda")
    ql = util.dbl_array(QL_46)
    g = GpuMetad(abi, sigma=[0.5], cv_min=[0.0], cv_max=[60.0], num_points=[96], W=1.3, T_shift=5.0, T=1.0, stride=1, mode="well_tempered")
    try:
        geo = (n, abi.ptr(d_pos), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), 0, 1.4, 1.2, 6, 0)
        p_val, sums, n_sums = C.c_void_p(), C.c_void_p(), C.c_uint()
        g.stream = stream = gate.arm()
        for t in range(2):
            abi.check(lib.mtd_ql_accumulate_local(*geo, n, abi.ptr(scratch), C.byref(sums), C.byref(n_sums), stream))
            if virial:
                abi.check(lib.mtd_ql_finalize(0, 6, ql, n, abi.ptr(scratch), C.byref(p_val), None, None, stream))
                abi.check(lib.mtd_metad_set_cv_source(g.h, 0, p_val.value, 1, 1, 0, 1.0, 0.0))
                abi.check(lib.mtd_metad_update_bias(g.h, t, stream))
                abi.check(lib.mtd_ql_forces_virial(n, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl),
                                                   0, 1.4, 1.2, 6, 0, ql, n, abi.ptr(scratch), lib.mtd_metad_bias_device(g.h), 0.0, stream,
                                                   abi.ptr(vir), n))
            else:
                abi.check(lib.mtd_ql_finalize_update_bias(g.h, 0, 6, ql, n, abi.ptr(scratch), t, C.byref(p_val), None, None, stream))
                abi.check(lib.mtd_ql_forces(n, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), 0,
                                            1.4, 1.2, 6, 0, ql, n, abi.ptr(scratch), lib.mtd_metad_bias_device(g.h), 0.0, stream))

        def read():
            out = dict(F=force.cpu().numpy(), **_engine_result(g, abi))
            if virial:
                out["virial"] = vir.cpu().numpy()
            return out
        return gate.done(closing(read, g))
    except BaseException:
        g.close()
        raise


def unlist(run, abi):
    """a list runner (abi, pos, types, L, nl, ...) as a function of keywords"""
    def wrapped(pos, types, L, nl, gate=None, args=(), **kw):
        out = run(abi, pos, types, L, nl, *args, gate=gate, **kw)
        return out
    return wrapped


# ---- 1. negative controls: the gate fails for real NULL-stream work -----------------------------------------------------------------------

def test_control_cv_on_the_null_stream_gives_the_stale_result(abi):
    """the caller's mistake, made here and not in the library: mtd_lamellar_cv_partials + mtd_reduce_partials with stream = NULL while B
    arrives on S behind the delay.  The calls run at once, on A: the result is A's, bit for bit, and not B's"""
    a, b = lamellar_snapshots(np.float32)
    run = lambda postype, gate=None: run_lamellar_cv(abi, postype, 30.0, np.float32, gate=gate)
    want, stale, arr_b, arr_a, host_ms = sg.expected(run, dict(postype=a["postype"]), dict(postype=b["postype"]), "control 1")
    gate = sg.Gated(arr_a, arr_b, sg.delay_ms(host_ms), misuse="null_stream")
    got = sg.run_gated(run, gate, dict(postype=b["postype"]))
    print(gate.line("control: cv on the NULL stream", host_ms))
    assert gate.pending
    assert not sg.differing_keys(stale, got) and sg.differing_keys(want, got) == ["cv"]
    with pytest.raises(AssertionError, match="differ from the NULL-stream result"):
        sg.assert_same_bits(got, want, "control 1")


def test_control_scale_on_the_null_stream_leaves_b_unscaled(abi):
    """mtd_wte_scale_netforce with stream = NULL while B arrives on S: A is scaled at once, then B overwrites it: what is read on S is
    B, unscaled"""
    rng = np.random.default_rng(1)
    mk = lambda: dict(nf=rng.normal(size=(N, 4)).astype(np.float32), nt=rng.normal(size=(N, 4)).astype(np.float32),
                      nv=rng.normal(size=(6, N + 5)).astype(np.float32), bias=float(rng.uniform(0.2, 0.6)))
    a, b = mk(), mk()
    run = lambda gate=None, **kw: run_wte(abi, dtype=np.float32, which="wte", gate=gate, **kw)
    want, stale, arr_b, arr_a, host_ms = sg.expected(run, a, b, "control 2")
    gate = sg.Gated(arr_a, arr_b, sg.delay_ms(host_ms), misuse="null_stream")
    got = sg.run_gated(run, gate, b)
    print(gate.line("control: scale on the NULL stream", host_ms))
    assert gate.pending
    assert np.array_equal(got["f"], b["nf"]) and np.array_equal(got["t"], b["nt"]) and np.array_equal(got["v"], b["nv"])
    assert sorted(sg.differing_keys(want, got)) == ["f", "t", "v"]


def test_control_read_on_the_null_stream_sees_the_prefill(abi):
    """the output read on the NULL stream by a device-side clone instead of on S, while the call is queued on S behind the delay: the
    clone holds the NaN the output was filled with"""
    lib = abi.load()
    _, b = lamellar_snapshots(np.float32)
    box, lset = abi.Box.make(30.0), abi.LamellarSet.make(CVS)
    d_pos = torch.from_numpy(b["postype"]).cuda()
    scratch = torch.zeros(lib.mtd_lamellar_scratch_doubles(N), dtype=torch.float64, device="cuda")
    cv = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    n_part = C.c_uint()
    torch.cuda.synchronize()
    S, ev = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(S):
        sg._delay(sg.delay_units(sg.MIN_MS, sg.rate()))
        ev.record(S)
    abi.check(lib.mtd_lamellar_cv_partials(C.byref(lset), N, abi.ptr(d_pos), abi.MTD_F32, C.byref(box), abi.ptr(scratch), C.byref(n_part), S.cuda_stream))
    abi.check(lib.mtd_reduce_partials(abi.ptr(scratch), n_part.value, 2, 2, 1.0 / N, 0.0, abi.ptr(cv), S.cuda_stream))
    early = cv.clone()                                                   # on the NULL stream: not ordered with S
    pending = not ev.query()
    with torch.cuda.stream(S):
        late = cv.clone()
    S.synchronize()
    torch.cuda.synchronize()
    print("stream gate: control: read on the NULL stream           delay %6.1f ms  event pending: %s" % (sg.MIN_MS, "yes" if pending else "NO"))
    assert pending
    assert torch.isnan(early).all() and torch.isfinite(late).all() and (late != 0).all()


# ---- 2. lamellar, WTE, wrapper, adaptive ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_lamellar_partials_reduce_forces(abi, dtype):
    a, b = lamellar_snapshots(dtype)
    run = lambda gate=None, **kw: run_lamellar(abi, L=30.0, dtype=dtype, gate=gate, **kw)
    got, _, _ = sg.check("lamellar %s" % np.dtype(dtype).name, run, dict(postype=a["postype"], bias=[0.3, -0.2]),
                         dict(postype=b["postype"], bias=[-0.45, 0.7]))
    assert np.isfinite(got["F0"]).all() and np.abs(got["F0"][:, :3]).max() > 0 and np.abs(got["F1"][:, :3]).max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_lamellar_dropin_pair(abi, dtype):
    a, b = lamellar_snapshots(dtype)
    run = lambda gate=None, **kw: run_dropin(abi, L=30.0, dtype=dtype, gate=gate, **kw)
    got, _, _ = sg.check("lamellar drop-in %s" % np.dtype(dtype).name, run, dict(postype=a["postype"]), dict(postype=b["postype"]))
    assert np.isfinite(got["modes"]).all() and np.abs(got["F"][:, :3]).max() > 0


def _wte_inputs(dtype, seed):
    rng = np.random.default_rng(seed)
    return dict(nf=rng.normal(size=(N, 4)).astype(dtype), nt=rng.normal(size=(N, 4)).astype(dtype), nv=rng.normal(size=(6, N + 5)).astype(dtype),
                bias=float(rng.uniform(0.2, 0.6)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["energy", "wte", "wrapper"])
def test_wte_and_wrapper(abi, dtype, which):
    """mtd_wte_energy_partials + mtd_reduce_partials; mtd_wte_scale_netforce and mtd_wrapper_scale_forces with the bias in device memory"""
    a, b = _wte_inputs(dtype, 11), _wte_inputs(dtype, 12)
    run = lambda gate=None, **kw: run_wte(abi, dtype=dtype, which=which, gate=gate, **kw)
    got, _, _ = sg.check("%s %s" % (which, np.dtype(dtype).name), run, a, b)
    if which != "energy":
        fac = (1.0 + b["bias"]) if which == "wte" else b["bias"]
        assert np.allclose(got["f"][:, :3], fac * b["nf"][:, :3], rtol=1e-6) and np.array_equal(got["v"][:, N:], b["nv"][:, N:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_sigma_products_waits_for_the_stream(abi, dtype):
    """mtd_sigma_products (3 variables, one without derivatives) is synchronous: when it returns the stream has passed the delay and the
    host array holds B's products"""
    rng = np.random.default_rng(3)
    mk = lambda: dict(forces=[rng.normal(size=(N, 4)).astype(dtype) for _ in range(2)])
    a, b = mk(), mk()
    run = lambda gate=None, **kw: run_sigma(abi, dtype=dtype, gate=gate, **kw)
    got, _, _ = sg.check("sigma products %s" % np.dtype(dtype).name, run, a, b, synchronising=True)
    s = got["sigmasq"].reshape(3, 3)
    assert s[0, 0] > 0 and s[2, 2] > 0 and s[0, 2] == s[2, 0] != 0 and not s[1].any() and not s[:, 1].any()


# ---- 3. the bias grid ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["plain", "reset+set", "touched", "phases", "walkers"])
def test_grid_eight_steps_from_device_partials(abi, variant):
    run = lambda gate=None, **kw: run_grid(abi, variant=variant, gate=gate, **kw)
    keys = ["cv", "bias", "V", "grid", "hist", "reweighted"]
    got, _, _ = sg.check("grid 64x64 %s" % variant, run, dict(traj=grid_trajectory(1)), dict(traj=grid_trajectory(2)), keys=keys, synchronising=True)
    assert got["num_gaussians"] == (42 if variant == "phases" else 4) and got["grid"].max() > 0 and np.isfinite(got["reweighted"]).all()
    if variant == "reset+set":
        assert got["hist"].sum() + got["hist_delta"].sum() == 4          # steps 4 .. 7 behind the reset (hist_delta: not yet accumulated)


def test_update_grid_dropin(abi):
    got, _, _ = sg.check("update_grid drop-in", lambda gate=None, **kw: run_update_grid(abi, gate=gate, **kw), dict(cur=[0.37, 1.21]),
                         dict(cur=[0.62, 0.4]))
    assert got["delta"].max() > 0.25 and got["delta"].min() >= 0.25


def test_grid_patch_hit_behind_a_device_write(abi):
    """mtd_metad_device_array(0) + mtd_metad_grid_touched(m, S) as the header prescribes, on a `hit` path of tests/grid_paths.py: the
    step behind the write must see it, and through the patch"""
    run = lambda gate=None, **kw: run_touched_on_path(abi, gate=gate, **kw)
    keys = ["rows", "bias", "V", "grid", "reweighted"]
    got, want, _ = sg.check("grid patch behind a device write", run, dict(shift=1.25), dict(shift=3.5), keys=keys)
    plain = run(shift=0.0)
    assert np.array_equal(plain["rows"][:8], got["rows"][:8]) and not np.array_equal(plain["rows"][8], got["rows"][8])


# ---- 4. the fused step ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["passes", "step0", "step1", "slots"])
def test_fused_six_steps(abi, dtype, form):
    run = lambda gate=None, **kw: run_fused(abi, dtype=dtype, form=form, gate=gate, **kw)
    keys = ["F", "cv", "bias", "V", "grid", "hist", "reweighted"]
    got, _, _ = sg.check("fused %s %s" % (form, np.dtype(dtype).name), run, dict(traj=fused_trajectory(dtype, 42)), dict(traj=fused_trajectory(dtype, 43)),
                         keys=keys)
    assert got["num_gaussians"] == 3 and np.isfinite(got["F"]).all() and np.abs(got["F"][-1, :, :, :3]).max() > 0


# ---- 5. the mesh ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims,variant", [((16, 16, 16), "forces"), ((16, 16, 16), "setters"), ((16, 16, 16), "setters2"), ((16, 16, 16), "merged"), ((16, 16, 16), "split"),
                                          ((128, 64, 8), "forces"), ((128, 64, 8), "split")],
                         ids=["16-forces", "16-setters", "16-setters2", "16-merged", "16-split", "128x64x8-forces", "128x64x8-split"])
def test_mesh(abi, dtype, dims, variant):
    a, b = mesh_pair(dtype)
    s_mesh = float(run_mesh(abi, b, dims, dtype, "plain")["cv"][1]) if variant == "merged" else None      # the grid is laid around B's value
    run = lambda gate=None, **kw: run_mesh(abi, dims=dims, dtype=dtype, variant=variant, s_mesh=s_mesh, gate=gate, **kw)
    keys = ["cv", "F"] + {"forces": ["qmax", "virial", "mesh"], "setters": ["virial"], "setters2": ["virial"], "split": [], "merged": ["F_lam", "engine_cv", "engine_bias", "engine_grid"]}[variant]
    got, _, _ = sg.check("mesh %s %s %s" % ("x".join(map(str, dims)), variant, np.dtype(dtype).name), run, dict(two=a), dict(two=b), keys=keys,
                         synchronising=variant in ("forces", "setters", "setters2"))
    assert np.isfinite(got["F"]).all() and np.abs(got["F"][:, :3]).max() > 0 and got["cv"][0] != got["cv"][1]
    if variant in ("setters", "setters2"):                               # what follows the setters sees the NEW tables
        old = run(two=b, new_table=False)
        assert np.abs(got["virial"]).max() > 0 and sg.differing_keys(old, got, ["cv", "virial"]) == ["virial"]
        m = GpuMesh(abi, dims, MESH_MODE, N)                             # ... and the first evaluation saw the old ones: bug_compat = 1
        try:
            d = torch.from_numpy(b[0]).cuda()
            assert m.cv(d, _dt(abi, dtype), abi.Box.make(30.0), N) == got["cv"][0]
            abi.check(abi.load().mtd_mesh_set_bug_compat(m.h, 0))
            assert m.cv(d, _dt(abi, dtype), abi.Box.make(30.0), N) != got["cv"][0]
        finally:
            m.close()
    if variant == "forces":
        assert got["pipeline"][0] == 2 and np.abs(got["virial"]).max() > 0      # the second evaluation took the bin pipeline


# ---- 6. neighbour-row variables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_entropy(abi, dtype):
    a, b = liquid_snapshots(dtype, r_list=2.45)
    run = unlist(run_gpu_pe, abi)
    kw = dict(args=(2.0, 0.1, 40, 0, dtype), virial=True)
    got, _, _ = sg.check("pair entropy %s" % np.dtype(dtype).name, run, listed(a, bias=0.7, **kw), listed(b, bias=0.9, **kw))
    assert np.isfinite(got["F"]).all() and np.abs(got["F"]).max() > 0 and np.abs(got["virial"]).max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["fcc", "two_switch"])
def test_environment_similarity(abi, dtype, variant):
    a, b = crystal_snapshots(dtype)
    t, lam, sw = ll.es_variants()[variant]
    run = unlist(run_gpu_es, abi)
    kw = dict(args=(t, dtype), lam=lam, sw=sw, virial=True)
    keys = ["sum_v", "s", "ke", "k", "v", "F", "virial"]
    got, _, _ = sg.check("environment similarity %s %s" % (variant, np.dtype(dtype).name), run, listed(a, bias=0.7, **kw), listed(b, bias=0.9, **kw),
                         keys=keys)
    assert np.isfinite(got["F"]).all() and np.abs(got["F"]).max() > 0 and got["s"] > 0.1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["full", "half-exact", "half-atomic", "virial", "merged", "merged-virial"])
def test_global_steinhardt(abi, dtype, mode):
    """mtd_ql_accumulate -> (mtd_ql_finalize) -> mtd_ql_forces on a full list, on a half list with the exact integer sums (the pooled
    stream-ordered allocation) and with floating-point atomics, mtd_ql_forces_virial, and mtd_ql_finalize_update_bias with a 1-d grid"""
    a, b = crystal_snapshots(dtype)
    name = "steinhardt %s %s" % (mode, np.dtype(dtype).name)
    lib = abi.load()
    if mode in ("merged", "merged-virial"):
        run = lambda gate=None, **kw: run_ql_merged(abi, dtype=dtype, virial=mode == "merged-virial", gate=gate, **kw)
        keys = ["F", "cv", "bias", "V", "grid"] + (["virial"] if mode == "merged-virial" else [])
        got, _, _ = sg.check(name, run, listed(a), listed(b), keys=keys)
        assert got["num_gaussians"] == 2 and np.abs(got["F"][:, :3]).max() > 0
        return
    if mode == "virial":
        run = unlist(run_gpu_ql_virial, abi)
        kw = dict(args=(6, QL_46, dtype), pitch=len(a["pos"]) + 3)
        got, _, _ = sg.check(name, run, listed(a, bias=0.7, **kw), listed(b, bias=0.9, **kw))
        assert np.array_equal(got["F"], got["F_plain"]) and np.abs(got["raw"][:, :len(a["pos"])]).max() > 0
        return
    run = unlist(run_gpu_ql, abi)
    args = (1.4, 1.2, 6, 0, QL_46, dtype)
    if mode == "full":
        sg.check(name, run, listed(a, args=args, bias=0.7), listed(b, args=args, bias=0.9))
        return
    half_a, half_b = (dict(s, nl=ll.half_of(s["nl"])) for s in (a, b))
    abi.check(lib.mtd_ql_set_half_list_exact(1 if mode == "half-exact" else 0))
    try:
        close = None
        if mode == "half-atomic":
            def close(got, want):
                sg.assert_same_bits(got, want, name, keys=[0, 1, 2])    # the CV pass has no atomics
                tol = 1e-12 if dtype == np.float64 else 2e-6             # tests/test_gpu_steinhardt.py:122 (test_ql_half_list_forces_bitwise_reproducible)
                assert np.abs(got[3][:, :3] - want[3][:, :3]).max() <= tol * np.abs(want[3][:, :3]).max()
        sg.check(name, run, listed(half_a, args=args, bias=0.7, half=True), listed(half_b, args=args, bias=0.9, half=True), close=close)
    finally:
        abi.check(lib.mtd_ql_set_half_list_exact(1))


def first_exact_call(abi):
    """the exact half-list force pass as the FIRST such call of a process: its pool of stream-ordered allocations does not exist yet
    (steinhardt.hip creates one per device at the first call).  The warm-up that loads the kernels and sizes the delay therefore runs
    on the full list, which never enters that pass; the gated call comes next, the NULL-stream runs it is compared with come last"""
    a, b = crystal_snapshots(np.float64, cells=7)
    args = (1.4, 1.2, 6, 0, QL_46, np.float64)
    run = unlist(run_gpu_ql, abi)
    warm = sg.Plain()
    run(gate=warm, **listed(b, args=args, bias=0.9))
    half = [dict(s, nl=ll.half_of(s["nl"])) for s in (a, b)]
    arrays = [[util.pack_postype(s["pos"], s["types"], np.float64)] + [np.asarray(x).astype(np.int32) for x in s["nl"]] +
              [np.array([bias], dtype=np.float64)] for s, bias in zip(half, (0.7, 0.9))]
    kw_a, kw_b = (listed(s, args=args, bias=bias, half=True) for s, bias in zip(half, (0.7, 0.9)))
    gate = sg.Gated(arrays[0], arrays[1], sg.delay_ms(warm.host_ms))
    got = sg.run_gated(run, gate, kw_b)
    print(gate.line("steinhardt half-exact, first call", warm.host_ms))
    assert gate.pending, "the delay was over before the calls were queued: the case proved nothing"
    want, stale = run(**kw_b), run(**kw_a)
    sg.assert_all_differ(stale, want, "first exact call")
    sg.assert_same_bits(got, want, "first exact call")
    assert np.abs(got[3][:, :3]).max() > 0
    print("FIRST_EXACT_OK")


def test_exact_half_list_pass_first_call_in_a_process():
    """first_exact_call() in a fresh process: in this one some earlier test has created the pool already"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "first-exact"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "FIRST_EXACT_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("workspace", [True, False], ids=["ws", "plain"])
def test_symmetrize_half_list(abi, workspace):
    a, b = crystal_snapshots(np.float64)
    run = lambda gate=None, **kw: run_symmetrize(abi, n=len(a["pos"]), workspace=workspace, gate=gate, **kw)
    got, _, _ = sg.check("symmetrize half list (%s)" % ("ws" if workspace else "plain"), run, dict(half=ll.half_of(a["nl"])), dict(half=ll.half_of(b["nl"])), synchronising=True)
    full = b["nl"]
    assert got["count"][0] == len(full[2]) and np.array_equal(got["head"], np.asarray(full[0]).astype(np.int32))
    assert np.array_equal(got["lst"], np.asarray(full[2]).astype(np.int32))


LOCAL = {"switch+gate": dict(switch=(0.25, 3), gate=(10, 16)), "average": dict(average=True)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["plain", "switch+gate", "average", "bonds", "virial", "cluster"])
def test_local_steinhardt(abi, dtype, name):
    """mtd_ql_local_accumulate_opt / forces_opt with switch + gate and with `average`; the bonds pair; mtd_ql_local_forces_virial;
    mtd_ql_local_accumulate_cluster (mtd_cluster_largest inside), its summary read on the stream"""
    a, b = crystal_snapshots(dtype)
    what = "local steinhardt %s %s" % (name, np.dtype(dtype).name)
    args = (1.4, 1.2, 6, 0, QL_46, dtype)
    if name == "plain":                                                  # mtd_ql_local_accumulate / mtd_ql_local_forces, the entry points without options
        run = unlist(run_gpu_opt, abi)
        got, _, _ = sg.check(what, run, listed(a, args=args, entry="old", bias=0.7), listed(b, args=args, entry="old", bias=0.9),
                             keys=["s", "c", "n", "F", "partials"])
    elif name in LOCAL:
        run = unlist(run_gpu_opt, abi)
        got, _, _ = sg.check(what, run, listed(a, args=args, opt=LOCAL[name], bias=0.7), listed(b, args=args, opt=LOCAL[name], bias=0.9))
    elif name == "bonds":
        run = unlist(run_gpu_bonds, abi)
        opt = dict(bonds=(0.3, 0.8), switch=(6.5, 6), gate=(10, 16))
        got, _, _ = sg.check(what, run, listed(a, args=args, opt=opt, bias=0.7), listed(b, args=args, opt=opt, bias=0.9))
    elif name == "virial":
        run = unlist(run_gpu_local_virial, abi)
        kw = dict(args=args, opt=LOCAL["switch+gate"], pitch=len(a["pos"]) + 3)
        got, _, _ = sg.check(what, run, listed(a, bias=0.7, **kw), listed(b, bias=0.9, **kw))
        assert np.array_equal(got["F"], got["F_opt"])
    else:
        opt = dict(bonds=(0.3, 0.8), switch=(6.5, 6))
        # v_min: the median of B's v_i (a first run with every particle a node), r_link: the nearest-neighbour distance
        first = run_gpu_ql_cluster(abi, b["pos"], b["types"], b["L"], b["nl"], dtype, opt=opt, cluster=(-1.0, 1.0), args=args[:5])
        cluster = (float(np.median(first["v"])), 1.0)
        run2 = lambda pos, types, L, nl, gate=None, **k: run_gpu_ql_cluster(abi, pos, types, L, nl, dtype, gate=gate, args=args[:5], **k)
        kw = dict(opt=opt, cluster=cluster)
        keys = ["s", "c", "n", "v", "b", "partials", "F", "F_vir", "raw", "w", "label", "summary"]
        got, _, _ = sg.check(what, run2, listed(a, bias=0.7, **kw), listed(b, bias=0.9, **kw), keys=keys)
        assert 1 < got["summary"][1] < got["summary"][3] and got["summary"][2] > 1
    assert np.isfinite(got["F"]).all() and np.abs(got["F"][:, :3]).max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_largest(abi, dtype):
    a, b = liquid_snapshots(dtype, r_list=1.5)
    rng = np.random.default_rng(9)
    run = lambda pos, types, L, nl, v, gate=None: run_gpu_cluster(abi, pos, types, L, nl, 0, v, (0.5, 1.05), dtype, gate=gate)[0]
    got, _, _ = sg.check("cluster largest %s" % np.dtype(dtype).name, run, listed(a, v=rng.random(N)), listed(b, v=rng.random(N)))
    assert got["summary"][2] > 10 and 0.4 * N < got["summary"][3] < 0.6 * N


# ---- 7. the neighbour list -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_nlist_build_check_rebuild(abi, dtype):
    """mtd_nlist_build on B arriving behind the delay (it synchronises once, for the entry count), mtd_nlist_check after a displacement
    that arrives on the stream, the rebuild: both lists are B's, as sorted rows"""
    out = []
    L = (N / 0.8) ** (1.0 / 3.0)
    for seed, move in ((31, 0.05), (32, 0.35)):                          # A moves by less than r_buff / 2, B by more: the verdicts differ
        pos, types = util.snapshot_random(N, L, seed=seed, dtype=dtype)
        rng = np.random.default_rng(seed)
        d = rng.normal(size=pos.shape)
        moved = pos.astype(np.float64) + move * d / np.linalg.norm(d, axis=1)[:, None]
        moved = np.clip((np.mod(moved + L / 2, L) - L / 2).astype(dtype), -L / 2, np.nextafter(dtype(L / 2), dtype(0)))
        out.append(np.stack([util.pack_postype(pos, types, dtype), util.pack_postype(moved, types, dtype)]))
    run = lambda gate=None, **kw: run_nlist(abi, L=L, dtype=dtype, gate=gate, **kw)
    got, _, _ = sg.check("nlist %s" % np.dtype(dtype).name, run, dict(two=out[0]), dict(two=out[1]), synchronising=True)
    assert got["needs"][0] == 1 and got["n_first"][0] > 0 and not np.array_equal(got["first"], got["second"])
    want = util.build_nlist(out[1][0][:, :3].astype(np.float64), L, 1.5)
    assert got["n_first"][0] == len(want[2])


# ---- 8. two streams at once ----------------------------------------------------------------------------------------------------------------

def test_two_streams_handle_less_families(abi):
    """two independent problems with different N and different lists on two streams, queued one behind the other with a delay of its
    own length in front of each and no host synchronise until both are queued: each result is its solo NULL-stream result bit for bit.
    This is the case for scratch, lazy tables or caches shared behind the caller's back (the per-device maps of the Steinhardt units)"""
    big_a, big_b = crystal_snapshots(np.float64)
    small_a, small_b = crystal_snapshots(np.float64, cells=7)
    liq_a, liq_b = liquid_snapshots(np.float64, r_list=2.45)
    lam_a, lam_b = lamellar_snapshots(np.float32)
    lam2_a, lam2_b = lamellar_snapshots(np.float32, n=2999)
    args = (1.4, 1.2, 6, 0, QL_46, np.float64)
    t, lam, sw = ll.es_variants()["two_switch"]
    pairs = {
        "lamellar": (lambda gate=None, **kw: run_lamellar(abi, L=30.0, dtype=np.float32, gate=gate, **kw),
                     dict(postype=lam_a["postype"], bias=[0.3, -0.2]), dict(postype=lam_b["postype"], bias=[-0.45, 0.7]),
                     dict(postype=lam2_a["postype"], bias=[0.1, 0.2]), dict(postype=lam2_b["postype"], bias=[0.5, -0.6]), None),
        "steinhardt": (unlist(run_gpu_ql, abi), listed(big_a, args=args, bias=0.7), listed(big_b, args=args, bias=0.9),
                       listed(small_a, args=args, bias=0.6), listed(small_b, args=args, bias=0.8), None),
        "steinhardt half": (unlist(run_gpu_ql, abi), listed(dict(big_a, nl=ll.half_of(big_a["nl"])), args=args, bias=0.7, half=True),
                            listed(dict(big_b, nl=ll.half_of(big_b["nl"])), args=args, bias=0.9, half=True),
                            listed(dict(small_a, nl=ll.half_of(small_a["nl"])), args=args, bias=0.6, half=True),
                            listed(dict(small_b, nl=ll.half_of(small_b["nl"])), args=args, bias=0.8, half=True), None),
        "local steinhardt": (unlist(run_gpu_bonds, abi), listed(big_a, args=args, opt=dict(bonds=(0.3, 0.8), switch=(6.5, 6)), bias=0.7),
                             listed(big_b, args=args, opt=dict(bonds=(0.3, 0.8), switch=(6.5, 6)), bias=0.9),
                             listed(small_a, args=args, opt=dict(bonds=(0.3, 0.8), switch=(6.5, 6)), bias=0.6),
                             listed(small_b, args=args, opt=dict(bonds=(0.3, 0.8), switch=(6.5, 6)), bias=0.8), None),
        "local average": (unlist(run_gpu_opt, abi), listed(big_a, args=args, opt=dict(average=True), bias=0.7),
                          listed(big_b, args=args, opt=dict(average=True), bias=0.9), listed(small_a, args=args, opt=dict(average=True), bias=0.6),
                          listed(small_b, args=args, opt=dict(average=True), bias=0.8), None),
        "pair entropy": (unlist(run_gpu_pe, abi), listed(liq_a, args=(2.0, 0.1, 40, 0, np.float64), bias=0.7),
                         listed(liq_b, args=(2.0, 0.1, 40, 0, np.float64), bias=0.9), listed(small_a, args=(1.2, 0.08, 24, 0, np.float64), bias=0.6),
                         listed(small_b, args=(1.2, 0.08, 24, 0, np.float64), bias=0.8), ["S", "g", "sums", "F"]),
        "environment similarity": (unlist(run_gpu_es, abi), listed(big_a, args=(t, np.float64), lam=lam, sw=sw, bias=0.7),
                                   listed(big_b, args=(t, np.float64), lam=lam, sw=sw, bias=0.9),
                                   listed(small_a, args=(t, np.float64), lam=lam, sw=sw, bias=0.6),
                                   listed(small_b, args=(t, np.float64), lam=lam, sw=sw, bias=0.8), ["sum_v", "s", "ke", "k", "v", "F"]),
    }
    for name, (run, a1, b1, a2, b2, keys) in pairs.items():
        sg.check_pair("two streams: " + name, run, a1, b1, run, a2, b2, keys1=keys, keys2=keys)
    a, b = _wte_inputs(np.float64, 21), _wte_inputs(np.float64, 22)
    small = lambda d: dict(nf=d["nf"][:1777], nt=d["nt"][:1777], nv=d["nv"][:, :1782].copy(), bias=d["bias"] + 0.1)
    run = lambda gate=None, **kw: run_wte(abi, dtype=np.float64, which="wte", gate=gate, **kw)
    run_e = lambda gate=None, **kw: run_wte(abi, dtype=np.float64, which="energy", gate=gate, **kw)
    sg.check_pair("two streams: wte scale", run, a, b, run, small(a), small(b))
    sg.check_pair("two streams: wte energy", run_e, a, b, run_e, small(a), small(b))


def test_two_streams_two_engines_and_two_meshes(abi):
    """two mtd_metad engines and two mtd_mesh handles, one per stream"""
    run = lambda gate=None, **kw: run_grid(abi, late=True, gate=gate, **kw)
    keys = ["cv", "bias", "V", "grid", "hist", "reweighted"]
    sg.check_pair("two streams: engines", run, dict(traj=grid_trajectory(1)), dict(traj=grid_trajectory(2)),
                  run, dict(traj=grid_trajectory(3, n_part=9), variant="touched"), dict(traj=grid_trajectory(4, n_part=9), variant="touched"),
                  keys1=keys, keys2=keys)
    a, b = mesh_pair(np.float32)
    s1 = float(run_mesh(abi, b, (16, 16, 16), np.float32, "plain")["cv"][1])
    s2 = float(run_mesh(abi, a[::-1].copy(), (128, 64, 8), np.float32, "plain")["cv"][1])
    run1 = lambda gate=None, **kw: run_mesh(abi, dims=(16, 16, 16), dtype=np.float32, variant="merged", s_mesh=s1, gate=gate, **kw)
    run2 = lambda gate=None, **kw: run_mesh(abi, dims=(128, 64, 8), dtype=np.float32, variant="merged", s_mesh=s2, gate=gate, **kw)
    keys = ["cv", "F", "F_lam", "engine_cv", "engine_bias", "engine_grid"]
    sg.check_pair("two streams: meshes", run1, dict(two=a), dict(two=b), run2, dict(two=b[::-1].copy()), dict(two=a[::-1].copy()), keys1=keys, keys2=keys)


# ---- 9. the host classes -------------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


def _host_run(api, abi, kind, stream):
    """12 steps of System::run from a fresh context with the execution configuration's stream set to `stream` (None: the default):
    CV values, bias factors, V, the weight, every grid array and every force array"""
    context, cv, integrate = api
    lib = abi.load()
    if kind == "steinhardt_local":                                       # the two crystallites of tests/test_gpu_ql_local_cluster.py
        s = cluster_system(np.float64)
        context.initialize(s["pos"], s["types"], ["A", "B"], s["L"], dtype=np.float64)
    else:
        s = lamellar_snapshots(np.float32)[1]
        if kind == "mesh+lamellar" and "s_mesh" not in _cache:           # one evaluation supplies the value the grid is laid around
            context.initialize(s["pos"], s["types"], ["A", "B"], s["L"], dtype=np.float32)
            integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
            probe = cv.mesh(nx=16, mode={"A": 1.0, "B": -1.0})
            probe.set_grid(0.0, 1.0, 8)
            context.run(1)
            _cache["s_mesh"] = probe.cpp_force.getCurrentValue(1)
            context.current = None
        context.initialize(s["pos"], s["types"], ["A", "B"], s["L"], dtype=np.float32)
    if stream is not None:
        context.exec_conf.setStream(stream.cuda_stream)
    meta = integrate.mode_metadynamics(dt=0.005, stride=2, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    if kind in ("two_lamellar", "umbrella"):
        cvs = [cv.lamellar(sigma=0.05, mode=dict(A=1.0, B=-1.0), lattice_vectors=v) for v in (util.CV1_VECTORS, util.CV2_VECTORS)]
        for c in cvs:
            c.set_grid(-1.0, 1.0, 64)
        if kind == "umbrella":                                           # the generic path: the umbrella adds to a bias factor read back from the device
            cvs[0].set_params(umbrella="harmonic", kappa=2.0, cv0=0.1)
    elif kind == "mesh+lamellar":
        lam = cv.lamellar(sigma=0.02, mode=dict(A=1.0, B=-1.0), lattice_vectors=util.CV1_VECTORS)
        lam.set_grid(-1.0, 1.0, 48)
        sm = _cache["s_mesh"]
        mesh = cv.mesh(nx=16, mode={"A": 1.0, "B": -1.0}, sigma=0.05 * abs(sm))
        mesh.set_grid(0.25 * sm, 1.6 * sm, 40)
        cvs = [lam, mesh]
    else:
        nl = cv.nlist_cell(r_cut=1.5, r_buff=0.4, device=True)           # built on the device: mtd_nlist_build on the same stream
        _, cluster, r = cluster_reference(COMBO, np.float64)
        st = cv.steinhardt_local(**_kw(nl), sigma=0.02 * r["s"], cluster=dict(v_min=cluster[0], r_link=cluster[1]), **API_OPT)
        st.set_grid(0.55 * r["s"], 1.3 * r["s"], 64)
        cvs = [st]
    context.run(12)
    integ = meta.cpp_integrator
    t = context.current.system.getCurrentTimeStep()
    h = C.c_void_p(integ.getEngineHandle())
    G = lib.mtd_metad_num_elements(h)
    res = dict(cv=np.array(integ.getCurrentValues()), bias=np.array(integ.getBiasFactors()), V=integ.getLogValue("bias", t),
               w=integ.getLogValue("weight", t), n=integ.getNumGaussians())
    for which, name in enumerate(abi.ARRAY_NAMES):
        out = np.zeros(G, dtype=np.float64 if which < 6 else np.uint32)
        abi.check(lib.mtd_metad_get_array(h, which, out.ctypes.data, None if stream is None else stream.cuda_stream))
        res[name] = out
    for k, c in enumerate(cvs):
        res["F%d" % k] = c.cpp_force.getForceArray().copy()
    context.current = None
    return res


@pytest.mark.parametrize("kind", ["two_lamellar", "umbrella", "mesh+lamellar", "steinhardt_local"])
def test_host_classes_on_a_stream_of_their_own(api, abi, kind):
    """exec_conf.setStream(S): 12 steps of System::run mix uploads, kernels and read-backs; nothing may depend on the NULL stream's
    implicit ordering: every value, grid array and force array is that of the run on the default stream, bit for bit"""
    plain = _host_run(api, abi, kind, None)
    S = torch.cuda.Stream()
    own = _host_run(api, abi, kind, S)
    S.synchronize()
    assert plain["n"] == own["n"] >= 6 and np.abs(plain["bias"]).max() > 0
    bad = sg.differing_keys(plain, own)
    assert not bad, "%s on a stream of its own: %s differ from the run on the default stream" % (kind, bad)
    for k in [k for k in plain if k.startswith("F")]:
        assert np.isfinite(plain[k]).all() and np.abs(plain[k][:, :3]).max() > 0


def _host_run_energy_or_box(api, abi, kind, stream):
    """the host classes that read the device-resident bias factor back to the host inside a step: cv.potential_energy with an external
    virial (WellTemperedEnsemble scales it on the host) and cv.density + cv.aspect_ratio (box-shape variables: their bias forces are
    host numbers).  Two steps, then the value is moved (the external energy by 30, the box scaled by 0.9: hills deposited at one
    place have no slope there) and two more; the engine's state and grid, and what the variables left behind"""
    context, cv, integrate = api
    lib = abi.load()
    rng = np.random.default_rng(4)
    n = 1777
    context.initialize(rng.random((n, 3)) * 10 - 5, np.zeros(n, dtype=int), ["A"], 10.0, dtype=np.float64)
    if stream is not None:
        context.exec_conf.setStream(stream.cuda_stream)
    pdata = context.current.system_definition.getParticleData()
    if kind == "potential_energy":
        nf = rng.normal(size=(n, 4))
        nf[:, 3] = rng.normal(-2.0, 0.5, n)
        pdata.setNetForce(nf)
        pdata.setNetTorque(rng.normal(size=(n, 4)))
        pdata.setNetVirial(rng.normal(size=(6, n)))
        pdata.setExternalEnergy(12.5)
        for i in range(6):
            pdata.setExternalVirial(i, float(i + 1))
        pe0 = nf[:, 3].sum() + 12.5
        meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=2.0, deltaT=50.0, T=1.0)
        pe = cv.potential_energy(sigma=40.0)
        pe.set_grid(cv_min=pe0 - 300.0, cv_max=pe0 + 300.0, num_points=64)
    else:
        meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=1.0, T=1.0)
        density = cv.density(sigma=0.25)
        density.set_grid(cv_min=0.0, cv_max=4.0, num_points=20)
        aspect = cv.aspect_ratio(sigma=0.1, dir1=0, dir2=1)
        aspect.set_grid(cv_min=0.0, cv_max=2.0, num_points=30)
    context.run(2)
    if kind == "potential_energy":
        pdata.setExternalEnergy(42.5)
    else:
        pdata.setGlobalBox(pdata.getGlobalBox().scale(0.9))
    context.run(2)
    integ = meta.cpp_integrator
    t = context.current.system.getCurrentTimeStep()
    h = C.c_void_p(integ.getEngineHandle())
    G = lib.mtd_metad_num_elements(h)
    grid = np.zeros(G)
    abi.check(lib.mtd_metad_get_array(h, 0, grid.ctypes.data, None if stream is None else stream.cuda_stream))
    res = dict(cv=np.array(integ.getCurrentValues()), bias=np.array(integ.getBiasFactors()), V=integ.getLogValue("bias", t), grid=grid)
    if kind == "box":
        res.update(external_virial=np.array([[c.cpp_force.getExternalVirial(i) for i in range(6)] for c in (density, aspect)]))
    else:
        res.update(external_virial=np.array([pdata.getExternalVirial(i) for i in range(6)]), net_force=pdata.getNetForce().copy(), net_torque=pdata.getNetTorque().copy(), net_virial=pdata.getNetVirial().copy())
    context.current = None
    return res


@pytest.mark.parametrize("kind", ["potential_energy", "box"])
def test_host_read_backs_of_the_bias_factor_wait_for_the_stream(api, abi, kind):
    """the variables whose step reads dV/ds back from the device (a plain copy is not ordered with a non-blocking stream: they wait for
    the execution configuration's stream first) give on a stream of their own what they give on the default stream, bit for bit"""
    plain = _host_run_energy_or_box(api, abi, kind, None)
    S = torch.cuda.Stream()
    own = _host_run_energy_or_box(api, abi, kind, S)
    S.synchronize()
    assert np.abs(plain["bias"]).max() > 0 and np.abs(plain["external_virial"]).max() > 0 and plain["grid"].max() > 0
    bad = sg.differing_keys(plain, own)
    assert not bad, "%s on a stream of its own: %s differ from the run on the default stream" % (kind, bad)


if __name__ == "__main__":                                               # the child of test_exact_half_list_pass_first_call_in_a_process
    import conftest  # noqa: F401  (the import paths of the suite, torch ahead of the library)
    from metadynamics import _abi
    assert sys.argv[1:] == ["first-exact"], sys.argv
    _abi.load().mtd_lamellar_set_fast_trig(0)
    first_exact_call(_abi)
