"""GPU parity: the virial of the global Steinhardt variable's bias force (mtd_ql_forces_virial, cv.steinhardt.get_virial) against
the fp64 numpy restatement in the scatter form (tests/ql_virial_ref.py, itself checked on the CPU against the oracle's forces and
against strain differences in tests/test_ql_virial_ref.py), with the Q_lm of the oracle's ql_compute_cv.  Tolerances are the project's
own for the force of this variable (test_ql_parity) — the virial is the same arithmetic plus one product and one halving: per-particle
virial within 1e-9 of max|virial_i| with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store, 2^-24, with a margin of 3; the
fp32 snapshot is the rounded array, on both sides), the six sums in fp64 within 1e-9 of max|W|.  Through the Python API the restatement
is evaluated with the bias factor the integrator itself reports (plus the umbrella's kappa (s - cv0) at the value it reports), so the
same 1e-9 holds there.
Every call also runs mtd_ql_forces on the same table: the force array of the virial call must be that one bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ql_virial_ref as vir_ref
import stream_gate
import util
from test_gpu_ql_local_avg import brute_nlist, noisy_fcc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

QL_46 = [0, 0, 0, 0, 1, 0, 1]
DEGREES = {6: QL_46, 4: [0.2, 0, 1.0, 0.5, 1.0], 12: [0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0.5, 0, 0.25]}     # those of test_ql_parity
R_CUT, R_ON = 1.4, 1.2
SENTINEL = -7.25
BIAS = 0.9


def symmetrize(abi, N, half):
    """the symmetric full list a half list stands for, built on the device (mtd_ql_symmetrize_half_list)"""
    lib = abi.load()
    d_head, d_nn, d_nl = (torch.from_numpy(np.ascontiguousarray(x).astype(np.int32)).cuda() for x in half)
    cap = 2 * len(half[2])
    f_head = torch.zeros(N, dtype=torch.int32, device="cuda")
    f_nn = torch.zeros(N, dtype=torch.int32, device="cuda")
    f_nl = torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda")
    n_full = C.c_size_t()
    abi.check(lib.mtd_ql_symmetrize_half_list(N, abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), abi.ptr(f_head), abi.ptr(f_nn), abi.ptr(f_nl), cap,
                                              C.byref(n_full), None))
    torch.cuda.synchronize()
    assert n_full.value == cap
    return f_head.cpu().numpy().astype(np.uint32), f_nn.cpu().numpy().astype(np.uint32), f_nl.cpu().numpy().astype(np.uint32)


_snapshots = {}


def snapshot(abi, cells, dtype):
    """noisy fcc, rounded to the dtype, with its lists at r_cut + 0.15: {0: full, 1: half, 2: the half list symmetrised on the device};
    built once per size and dtype"""
    key = (cells, np.dtype(dtype).name)
    if key not in _snapshots:
        pos, L = noisy_fcc(cells)
        pos = pos.astype(dtype).astype(np.float64)
        half = util.build_nlist(pos, L, R_CUT + 0.15, half=True)
        lists = {0: util.build_nlist(pos, L, R_CUT + 0.15), 1: half, 2: symmetrize(abi, len(pos), half)}
        _snapshots[key] = (pos, L, np.zeros(len(pos), dtype=np.int32), lists)
    return _snapshots[key]


def run_gpu(abi, pos, types, L, nl, lmax, Ql_ref, dtype, mode=0, rcut=R_CUT, ron=R_ON, type_id=0, n_global=None, bias=BIAS, tilt=None,
            bias_on_device=True, pitch=None, pass_virial=True, gate=None):
    """mtd_ql_accumulate, then mtd_ql_forces and mtd_ql_forces_virial on the same table.  Returns dict(F_plain, F, raw): the two force
    arrays (N, 4) as stored and the whole virial buffer (6, pitch), which starts as SENTINEL.  gate: the stream the calls run on and how
    their inputs arrive (tests/stream_gate.py; None: the NULL stream)."""
    lib = abi.load()
    gate = gate or stream_gate.Plain()
    N = len(pos)
    n_global = N if n_global is None else n_global
    pitch = N if pitch is None else pitch
    box = abi.Box.make(L, **(tilt or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn, d_nl = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl)
    assert int(np.asarray(nl[0]).astype(np.int64)[-1] + np.asarray(nl[1]).astype(np.int64)[-1]) <= len(nl[2])
    scratch = torch.zeros(lib.mtd_ql_scratch_doubles(lmax), dtype=torch.float64, device="cuda")
    ql = util.dbl_array(Ql_ref)
    geo = (C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), mode, rcut, ron, lmax, type_id, ql, n_global, abi.ptr(scratch))
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    f_plain = torch.full((N, 4), 3.0, dtype=tdt, device="cuda")
    f_vir = torch.full((N, 4), 5.0, dtype=tdt, device="cuda")
    virial = torch.full((6, pitch), SENTINEL, dtype=tdt, device="cuda")
    stream = gate.arm()
    abi.check(lib.mtd_ql_accumulate(N, abi.ptr(d_pos), dt, *geo, None, None, None, stream))
    b_args = (abi.ptr(d_bias) if bias_on_device else None, 0.0 if bias_on_device else bias, stream)
    abi.check(lib.mtd_ql_forces(N, abi.ptr(d_pos), abi.ptr(f_plain), dt, *geo, *b_args))
    abi.check(lib.mtd_ql_forces_virial(N, abi.ptr(d_pos), abi.ptr(f_vir), dt, *geo, *b_args, abi.ptr(virial) if pass_virial else None, pitch))
    return gate.done(lambda: dict(F_plain=f_plain.cpu().numpy(), F=f_vir.cpu().numpy(), raw=virial.cpu().numpy()))


_refs = {}


def reference(key, ref, pos, types, L, nl, lmax, Ql_ref, bias=BIAS, rcut=R_CUT, ron=R_ON, type_id=0, n_global=None, tilt=None, half=False):
    """the restatement's answer with the oracle's Q_lm (nl: the list the ORACLE reads — the half list itself for modes 1 and 2), computed
    once per key and left unchanged"""
    if key not in _refs:
        case = dict(pos=pos, types=types, L=L, nl=nl, r_cut=rcut, r_on=ron, lmax=lmax, type_id=type_id, Ql_ref=Ql_ref, n_global=n_global, tilt=tilt,
                    half=half)
        _, Qlm = vir_ref.oracle_cv(ref, **case)
        _refs[key] = vir_ref.compute(**case, Qlm=Qlm, bias=bias)
    return _refs[key]


def compare(g, r, dtype, N, rows=None, types=None, type_id=0):
    """per-particle virial (the first N columns of the buffer) and, with fp64 arrays, the six sums against the restatement (its rows
    `rows` when given); the force array against that of mtd_ql_forces, bit for bit"""
    vg = g["raw"][:, :N].astype(np.float64).T                           # (N, 6) like the reference
    vr = r["virial"] if rows is None else r["virial"][rows]
    top = np.abs(r["virial"]).max()
    err = np.abs(vg - vr).max()
    w_top = np.abs(r["W"]).max()
    w_err = np.abs(vg.sum(axis=0) - vr.sum(axis=0)).max()
    print("virial: max |d| %.3e of max |virial_i| %.3e (%.3e relative); sums: %.3e of max |W| %.3e (%.3e relative)"
          % (err, top, err / top if top else 0.0, w_err, w_top, w_err / w_top if w_top else 0.0))
    assert np.isfinite(g["raw"]).all() and np.isfinite(g["F"]).all()    # (no NaN and no sentinel arithmetic)
    assert top > 0
    assert err <= (1e-9 if dtype == np.float64 else 2e-7) * top
    if dtype == np.float64:
        assert w_err <= 1e-9 * w_top
    assert np.array_equal(g["F"], g["F_plain"])                         # the virial must not perturb the force sums
    assert np.abs(g["F"][:, :3]).max() > 0 and np.all(g["F"][:, 3] == 0.0)
    if types is not None:
        assert np.all(vg[types != type_id] == 0.0)
    return vg


# ---- 1. parity and force bits ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cells", [3, 5])                               # N = 108: one full chunk of 64 and a partial one; N = 500
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("lmax", [6, 4, 12])                            # 12: the instantiation with two blocks per compute unit already
def test_virial_parity(abi, ref, dtype, cells, mode, lmax):
    pos, L, types, lists = snapshot(abi, cells, dtype)
    g = run_gpu(abi, pos, types, L, lists[mode], lmax, DEGREES[lmax], dtype, mode=mode)
    r = reference(("parity", cells, np.dtype(dtype).name, mode, lmax), ref, pos, types, L, lists[1 if mode else 0], lmax, DEGREES[lmax], half=mode != 0)
    compare(g, r, dtype, len(pos))


def test_modes_0_and_2_give_the_same_per_particle_values(abi):
    """even degrees only: the Q_lm of the two CV passes agree to rounding, and the force pass treats 2 like 0"""
    pos, L, types, lists = snapshot(abi, 5, np.float64)
    assert all(np.array_equal(a, b) for a, b in zip(lists[0], lists[2]))   # (the symmetrised half list IS the full list, partners ascending)
    a = run_gpu(abi, pos, types, L, lists[0], 6, QL_46, np.float64, mode=0)
    b = run_gpu(abi, pos, types, L, lists[2], 6, QL_46, np.float64, mode=2)
    assert np.abs(a["raw"] - b["raw"]).max() <= 1e-12 * np.abs(a["raw"]).max()


# ---- 2. d_virial == NULL, pitch, the third-law pass -----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_null_virial_is_the_force_entry_point(abi, dtype, mode):
    """the same kernels, the same bits, any list mode (the third-law pass included: exact integer sums); the virial buffer is never
    passed and stays as it was"""
    pos, L, types, lists = snapshot(abi, 5, dtype)
    g = run_gpu(abi, pos, types, L, lists[mode], 6, QL_46, dtype, mode=mode, pass_virial=False)
    assert np.array_equal(g["F"], g["F_plain"])
    assert np.abs(g["F"][:, :3]).max() > 0
    assert np.all(g["raw"] == SENTINEL)


def test_third_law_pass_with_a_virial_array_is_refused_and_writes_nothing(abi):
    lib = abi.load()
    pos, L, types, lists = snapshot(abi, 3, np.float64)
    N = len(pos)
    box = abi.Box.make(L)
    d_pos = torch.from_numpy(util.pack_postype(pos, types, np.float64)).cuda()
    d_head, d_nn, d_nl = (torch.from_numpy(np.asarray(x).astype(np.int32)).cuda() for x in lists[1])
    scratch = torch.zeros(lib.mtd_ql_scratch_doubles(6), dtype=torch.float64, device="cuda")
    force = torch.full((N, 4), 5.0, dtype=torch.float64, device="cuda")
    virial = torch.full((6, N), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.mtd_ql_forces_virial(N, abi.ptr(d_pos), abi.ptr(force), abi.MTD_F64, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), 1, R_CUT,
                                  R_ON, 6, 0, util.dbl_array(QL_46), N, abi.ptr(scratch), None, BIAS, None, abi.ptr(virial), N)
    torch.cuda.synchronize()
    assert rc == -2
    assert torch.all(force == 5.0).item() and torch.all(virial == SENTINEL).item()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pitch_beyond_the_particles(abi, ref, dtype):
    pos, L, types, lists = snapshot(abi, 3, dtype)
    N = len(pos)
    g = run_gpu(abi, pos, types, L, lists[0], 6, QL_46, dtype, pitch=N + 37)
    r = reference(("parity", 3, np.dtype(dtype).name, 0, 6), ref, pos, types, L, lists[0], 6, QL_46)
    compare(g, r, dtype, N)
    assert g["raw"].shape == (6, N + 37)
    assert np.all(g["raw"][:, N:] == SENTINEL)                          # the padding of every component is left alone


# ---- 3. two types and a shard ---------------------------------------------------------------------------------------------------

def test_two_types_and_shard(abi, ref):
    """only particles of `type` take part; N_global != N (the set-up of test_ql_two_types_and_shard)"""
    pos, L = noisy_fcc(4, seed=5)
    N = len(pos)
    types = (np.random.default_rng(1).random(N) < 0.3).astype(np.int32)
    nl = util.build_nlist(pos, L, 1.6)
    kw = dict(rcut=1.45, ron=1.1, n_global=3 * N)
    Ql_ref = [0.5, 0, 0.25, 0, 1, 0, 1]
    for type_id in (0, 1):
        g = run_gpu(abi, pos, types, L, nl, 6, Ql_ref, np.float64, type_id=type_id, **kw)
        r = reference(("types", type_id), ref, pos, types, L, nl, 6, Ql_ref, type_id=type_id, **kw)
        compare(g, r, np.float64, N, types=types, type_id=type_id)


# ---- 4. ghost particles ---------------------------------------------------------------------------------------------------------

def test_two_slabs_with_ghosts(abi, ref):
    """the snapshot cut into two z slabs the way tests/_host_dd_worker.py::steinhardt_set cuts it, in one process: every slab holds its
    local particles, then its ghosts; mtd_ql_accumulate_local per slab, the sums added on the host, mtd_ql_finalize, then the virial call
    with n_particles = the slab's local particles.  The rows of the local particles are the single-domain rows."""
    lib = abi.load()
    pos, L, types, lists = snapshot(abi, 5, np.float64)
    pos = np.mod(pos + L / 2, L) - L / 2
    N, world, r_list, lmax = len(pos), 2, R_CUT + 0.15, 6
    r = reference(("slabs",), ref, pos, types, L, lists[0], lmax, QL_46)
    head, nn, lst = (np.asarray(a).astype(np.int64) for a in lists[0])
    owner = np.minimum((np.mod(pos[:, 2] + L / 2, L) / L * world).astype(int), world - 1)
    z = pos[:, 2]
    zdist = lambda a, b: np.minimum(np.abs(a - b), L - np.abs(a - b))
    box = abi.Box.make(L)
    ql = util.dbl_array(QL_46)
    slabs, total = [], None
    for rank in range(world):
        mine = np.where(owner == rank)[0]
        lo, hi = -L / 2 + rank * L / world, -L / 2 + (rank + 1) * L / world
        ghosts = np.where((owner != rank) & ((zdist(z, lo) <= r_list) | (zdist(z, hi) <= r_list)))[0]
        index = np.full(N, -1, dtype=np.int64)
        index[mine] = np.arange(len(mine))
        index[ghosts] = len(mine) + np.arange(len(ghosts))
        rows = [index[lst[head[i]:head[i] + nn[i]]] for i in mine]
        assert all((row >= 0).all() for row in rows) and any((row >= len(mine)).any() for row in rows)       # every partner is held; some are ghosts
        s_nn = np.array([len(row) for row in rows], dtype=np.uint32)
        s_head = np.zeros(len(mine), dtype=np.uint32)
        s_head[1:] = np.cumsum(s_nn)[:-1]
        order = np.concatenate([mine, ghosts])
        d_pos = torch.from_numpy(util.pack_postype(pos[order], types[order], np.float64)).cuda()
        d_lists = [torch.from_numpy(x.astype(np.int32)).cuda() for x in (s_head, s_nn, np.concatenate(rows))]
        scratch = torch.zeros(lib.mtd_ql_scratch_doubles(lmax), dtype=torch.float64, device="cuda")
        sums, n_sums = C.c_void_p(), C.c_uint()
        abi.check(lib.mtd_ql_accumulate_local(len(mine), abi.ptr(d_pos), abi.MTD_F64, C.byref(box), *[abi.ptr(x) for x in d_lists], 0, R_CUT, R_ON, lmax,
                                              0, N, abi.ptr(scratch), C.byref(sums), C.byref(n_sums), None))
        torch.cuda.synchronize()
        off = (sums.value - scratch.data_ptr()) // 8
        part = scratch[off:off + n_sums.value].cpu().numpy().copy()
        total = part if total is None else total + part
        slabs.append(dict(mine=mine, d_pos=d_pos, d_lists=d_lists, scratch=scratch, off=off, n=n_sums.value))
    assert sum(len(s["mine"]) for s in slabs) == N
    seen = np.zeros((N, 6))
    for s in slabs:
        n_loc = len(s["mine"])
        s["scratch"][s["off"]:s["off"] + s["n"]] = torch.from_numpy(total).cuda()                        # the all-reduce of the ranks
        abi.check(lib.mtd_ql_finalize(0, lmax, ql, N, abi.ptr(s["scratch"]), None, None, None, None))
        geo = (C.byref(box), *[abi.ptr(x) for x in s["d_lists"]], 0, R_CUT, R_ON, lmax, 0, ql, N, abi.ptr(s["scratch"]), None, BIAS, None)
        f_plain = torch.full((n_loc, 4), 3.0, dtype=torch.float64, device="cuda")
        f_vir = torch.full((n_loc, 4), 5.0, dtype=torch.float64, device="cuda")
        virial = torch.full((6, n_loc), SENTINEL, dtype=torch.float64, device="cuda")
        abi.check(lib.mtd_ql_forces(n_loc, abi.ptr(s["d_pos"]), abi.ptr(f_plain), abi.MTD_F64, *geo))
        abi.check(lib.mtd_ql_forces_virial(n_loc, abi.ptr(s["d_pos"]), abi.ptr(f_vir), abi.MTD_F64, *geo, abi.ptr(virial), n_loc))
        torch.cuda.synchronize()
        g = dict(F_plain=f_plain.cpu().numpy(), F=f_vir.cpu().numpy(), raw=virial.cpu().numpy())
        seen[s["mine"]] = compare(g, r, np.float64, n_loc, rows=s["mine"])
    assert np.abs(seen.sum(axis=0) - r["W"]).max() <= 1e-9 * np.abs(r["W"]).max()          # the slabs' sums add up to the single-domain sum


# ---- 5. triclinic box -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_triclinic_box(abi, ref, dtype):
    """a sheared fcc crystal in the sheared box: d_kj is HOOMD's minimum image with tilt factors"""
    pos, L = noisy_fcc(4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = ((pos / L) @ h.T).astype(dtype).astype(np.float64)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = brute_nlist(pos, h, 1.6)
    kw = dict(rcut=1.45, ron=1.15)
    Ql_ref = [0, 0, 0.3, 0, 1, 0, 1]
    g = run_gpu(abi, pos, types, L, nl, 6, Ql_ref, dtype, tilt=tilt, **kw)
    r = reference(("triclinic", np.dtype(dtype).name), ref, pos, types, L, nl, 6, Ql_ref, tilt=tilt, **kw)
    compare(g, r, dtype, len(pos))
    # the pair vectors did cross the tilted faces: without the tilt in the minimum image the restatement gives another virial
    flat = vir_ref.compute(pos, types, L, nl, 1.45, 1.15, 6, 0, Ql_ref, vir_ref.oracle_cv(ref, pos, types, L, nl, 1.45, 1.15, 6, 0, Ql_ref, tilt=tilt)[1], BIAS)
    assert np.abs(flat["virial"] - r["virial"]).max() > 1e-3 * np.abs(r["virial"]).max()


# ---- 6. dilute case -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dilated_box_with_empty_rows(abi, ref, dtype):
    """the crystal and its box dilated by 1.7: 51 of the 500 particles have no list entry at all and many more none inside the cut-off;
    everything finite, those rows exactly 0"""
    pos, L = util.fcc_lattice(5)
    pos = (1.7 * pos + np.random.default_rng(31).normal(0, 0.12, pos.shape)).astype(dtype).astype(np.float64)
    L = 1.7 * L
    N = len(pos)
    types = np.zeros(N, dtype=np.int32)
    nl = util.build_nlist(pos, L, R_CUT + 0.15)
    inside = np.asarray(util.build_nlist(pos, L, R_CUT * (1 - 1e-6))[1])
    empty = np.asarray(nl[1]) == 0
    assert empty.sum() >= 20 and (inside > 0).sum() >= 100
    g = run_gpu(abi, pos, types, L, nl, 6, QL_46, dtype)
    r = reference(("dilated", np.dtype(dtype).name), ref, pos, types, L, nl, 6, QL_46)
    vg = compare(g, r, dtype, N)
    assert np.all(vg[empty] == 0.0) and np.all(g["F"][empty] == 0.0)
    assert np.all(vg[inside == 0] == 0.0)                               # entries beyond the cut-off add exact zeros


# ---- 7. bias --------------------------------------------------------------------------------------------------------------------

def test_bias_from_device_and_host_zero_bias_and_reproducible_bits(abi, ref):
    pos, L, types, lists = snapshot(abi, 5, np.float64)
    call = lambda **kw: run_gpu(abi, pos, types, L, lists[0], 6, QL_46, np.float64, **kw)
    dev = call(bias=-1.7, bias_on_device=True)
    host = call(bias=-1.7, bias_on_device=False)
    again = call(bias=-1.7, bias_on_device=True)
    assert np.array_equal(dev["raw"], host["raw"]) and np.array_equal(dev["F"], host["F"])
    assert np.array_equal(dev["raw"], again["raw"]) and np.array_equal(dev["F"], again["F"])     # no atomics, fixed orders
    r = reference(("bias",), ref, pos, types, L, lists[0], 6, QL_46, bias=-1.7)
    compare(dev, r, np.float64, len(pos))
    zero = call(bias=0.0, bias_on_device=False)
    assert np.all(zero["raw"] == 0.0) and np.all(zero["F"] == 0.0)


# ---- 8. a deferred grid pass is waiting -----------------------------------------------------------------------------------------

def test_virial_call_with_a_pending_grid_pass(abi, ref):
    """mtd_ql_finalize_update_bias leaves the engine's deferred pass pending on the stream; the force call that follows is the plain
    one in one run and the virial call in the other.  Every grid array, V, w and the bias factor after every step are the same BITS
    (whether the pass rides in the launch or runs on its own), the forces too, and the virial is that of a stand-alone call (nothing
    pending) with the same bias factor."""
    from test_gpu_metad import GpuMetad
    lib = abi.load()
    pos0, L = noisy_fcc(5, seed=3)
    N = len(pos0)
    types = np.zeros(N, dtype=np.int32)
    lmax = 6
    box = abi.Box.make(L)
    rng = np.random.default_rng(8)
    snaps = [pos0 + rng.normal(0, 0.01 * k, pos0.shape) for k in range(4)]
    nls = [util.build_nlist(p, L, R_CUT + 0.15) for p in snaps]
    val0 = vir_ref.oracle_cv(ref, snaps[0], types, L, nls[0], R_CUT, R_ON, lmax, 0, QL_46)[0]
    kw = dict(sigma=[0.01 * val0], cv_min=[0.6 * val0], cv_max=[1.2 * val0], num_points=[96], W=1.3, T_shift=5.0, T=1.0, stride=1, mode="well_tempered")
    ql = util.dbl_array(QL_46)

    def run(with_virial):
        g = GpuMetad(abi, **kw)
        scratch = torch.zeros(lib.mtd_ql_scratch_doubles(lmax), dtype=torch.float64, device="cuda")
        force = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
        out = []
        try:
            for t, (p, nl) in enumerate(zip(snaps, nls)):
                d_pos = torch.from_numpy(util.pack_postype(p, types, np.float64)).cuda()
                d_head, d_nn, d_nl = (torch.from_numpy(x.astype(np.int32)).cuda() for x in nl)
                lists = (abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), 0, R_CUT, R_ON, lmax, 0)
                sums, n_sums = C.c_void_p(), C.c_uint()
                abi.check(lib.mtd_ql_accumulate_local(N, abi.ptr(d_pos), abi.MTD_F64, C.byref(box), *lists, N, abi.ptr(scratch), C.byref(sums),
                                                      C.byref(n_sums), None))
                abi.check(lib.mtd_ql_finalize_update_bias(g.h, 0, lmax, ql, N, abi.ptr(scratch), t, None, None, None, None))
                tail = (ql, N, abi.ptr(scratch), lib.mtd_metad_bias_device(g.h), 0.0, None)
                virial = torch.full((6, N), SENTINEL, dtype=torch.float64, device="cuda")
                if with_virial:
                    abi.check(lib.mtd_ql_forces_virial(N, abi.ptr(d_pos), abi.ptr(force), abi.MTD_F64, C.byref(box), *lists, *tail, abi.ptr(virial), N))
                else:
                    abi.check(lib.mtd_ql_forces(N, abi.ptr(d_pos), abi.ptr(force), abi.MTD_F64, C.byref(box), *lists, *tail))
                torch.cuda.synchronize()
                rec = dict(F=force.cpu().numpy().copy(), arrays={n: g.array(n) for n in abi.ARRAY_NAMES}, virial=virial.cpu().numpy())
                if with_virial:        # g.array has flushed what nobody took: nothing is pending now, and the bias factor on the device
                    # is still this step's (g.state() below re-evaluates it on the grid that now holds the step's hill)
                    alone = torch.full((6, N), SENTINEL, dtype=torch.float64, device="cuda")
                    f2 = torch.zeros((N, 4), dtype=torch.float64, device="cuda")
                    abi.check(lib.mtd_ql_forces_virial(N, abi.ptr(d_pos), abi.ptr(f2), abi.MTD_F64, C.byref(box), *lists, *tail, abi.ptr(alone), N))
                    torch.cuda.synchronize()
                    rec.update(alone=alone.cpu().numpy(), F_alone=f2.cpu().numpy())
                rec["st"] = g.state()
                out.append(rec)
        finally:
            g.close()
        return out

    a, b = run(True), run(False)
    for t, (x, y) in enumerate(zip(a, b)):
        for k in ("cv", "bias"):
            assert np.array_equal(x["st"][k], y["st"][k], equal_nan=True), (t, k, x["st"][k], y["st"][k])
        for k in ("V", "w", "num_gaussians", "oob"):
            assert x["st"][k] == y["st"][k] or (np.isnan(x["st"][k]) and np.isnan(y["st"][k])), (t, k, x["st"][k], y["st"][k])
        for n in abi.ARRAY_NAMES:
            assert np.array_equal(x["arrays"][n], y["arrays"][n], equal_nan=True), (t, n)
        assert np.array_equal(x["F"], y["F"]), t
        assert np.array_equal(x["virial"], x["alone"]) and np.array_equal(x["F"], x["F_alone"]), t
        assert np.all(y["virial"] == SENTINEL)
    assert a[-1]["st"]["num_gaussians"] == len(snaps)
    # (the stand-alone call is held against the restatement in test_virial_parity; here: it was not a comparison of zeros)
    assert np.isfinite(a[-1]["virial"]).all() and np.abs(a[-1]["virial"]).max() > 0 and np.abs(a[-1]["F"][:, :3]).max() > 0


# ---- 9. through the Python API --------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


API_TOL = 1e-9                                                          # the bias factor is the integrator's own: see the module docstring
KAPPA = 35.0


def _umbrella_run(api, ref, pressure, steps=3, half=False):
    """cv.steinhardt as the only grid variable under a harmonic umbrella; returns (st, meta, pos, types, L, oracle list, val, cv0)"""
    context, cv, integrate = api
    from metadynamics import _metadynamics
    pos, L = util.fcc_lattice(5)
    pos = pos + np.random.default_rng(15).normal(0, 0.05, pos.shape)
    types = np.zeros(len(pos), dtype=np.int32)
    context.initialize(pos, types, ["A"], L, dtype=np.float64)
    context.current.system_definition.getParticleData().setPressureFlag(pressure)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=1.5)
    lists = util.build_nlist(pos, L, 1.5, half=half)
    val = vir_ref.oracle_cv(ref, pos, types, L, lists, R_CUT, R_ON, 6, 0, QL_46, half=half)[0]
    st = cv.steinhardt(r_cut=R_CUT, r_on=R_ON, lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=0.02 * val)
    if half:                                                            # (as a C++ caller would: cv.steinhardt asks for full storage)
        nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
        nl.set_lists(*lists)
    else:
        assert all(np.array_equal(a, b) for a, b in zip(nl.update(), lists))
    st.set_grid(0.55 * val, 1.3 * val, 512)
    cv0 = 0.8 * val
    st.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(steps)
    return st, meta, pos, types, L, lists, val, cv0


def _api_compare(st, meta, ref, pos, types, L, lists, cv0, half):
    """get_virial() against the restatement at the bias factor the integrator reports plus the umbrella's"""
    integ = meta.cpp_integrator
    s = integ.getCurrentValues()[0]
    total = integ.getBiasFactors()[0] + KAPPA * (s - cv0)
    assert abs(KAPPA * (s - cv0)) > 0.1 * abs(total)
    case = dict(pos=pos, types=types, L=L, nl=lists, r_cut=R_CUT, r_on=R_ON, lmax=6, type_id=0, Ql_ref=QL_46, half=half)
    r = vir_ref.compute(**case, Qlm=vir_ref.oracle_cv(ref, **case)[1], bias=total)
    N = len(pos)
    per, raw, W = st.get_virial(per_particle=True), st.cpp_force.getVirial(), st.get_virial()
    assert per.shape == (6, N) and per.dtype == np.float64 and W.shape == (6,) and W.dtype == np.float64
    assert raw.shape == (6, st.cpp_force.getVirialPitch()) and np.array_equal(raw[:, :N], per)
    top, w_top = np.abs(r["virial"]).max(), np.abs(r["W"]).max()
    print("per particle: %.3e of %.3e; sums %.3e of %.3e" % (np.abs(per.T - r["virial"]).max(), top, np.abs(W - r["W"]).max(), w_top))
    assert w_top > 0.05
    assert np.abs(per.T - r["virial"]).max() <= API_TOL * top
    assert np.abs(W - r["W"]).max() <= API_TOL * w_top
    F = st.cpp_force.getForceArray()
    assert np.abs(F[:, :3] - r["F"]).max() <= API_TOL * np.abs(r["F"]).max()
    return per, F.copy()


def test_api_virial_with_umbrella_and_flag_off(api, ref):
    """(a) pressure flag set: get_virial() and cpp_force.getVirial() against the restatement; (b) flag off: get_virial() raises and the
    force array is that of (a) bit for bit"""
    context, cv, integrate = api
    st, meta, pos, types, L, lists, val, cv0 = _umbrella_run(api, ref, True)
    _, F_on = _api_compare(st, meta, ref, pos, types, L, lists, cv0, False)
    context.current = None
    st, meta = _umbrella_run(api, ref, False)[:2]
    with pytest.raises(RuntimeError):
        st.get_virial()
    with pytest.raises(RuntimeError):
        st.get_virial(per_particle=True)
    assert np.array_equal(st.cpp_force.getForceArray(), F_on)


def test_api_flag_on_then_off_leaves_no_stale_virial(api, ref):
    """flag on for one run, off for the next: the array the first run filled reads back as zeros after the second"""
    context, cv, integrate = api
    st = _umbrella_run(api, ref, True, steps=2)[0]
    assert np.abs(st.cpp_force.getVirial()).max() > 0
    context.current.system_definition.getParticleData().setPressureFlag(False)
    context.run(1)
    assert np.all(st.cpp_force.getVirial() == 0.0)
    with pytest.raises(RuntimeError):
        st.get_virial()
    context.current.system_definition.getParticleData().setPressureFlag(True)
    context.run(1)
    assert np.abs(st.get_virial()).max() > 0


def test_api_half_list_gives_the_full_list_virial(api, ref):
    """a NeighborList in half storage: the host class hands the pass the symmetric full list (mode 2), so the virial is there — the
    half-list restatement's (scatter form), which is the full-list virial of the same Q_lm"""
    context, cv, integrate = api
    st, meta, pos, types, L, half, val, cv0 = _umbrella_run(api, ref, True, half=True)
    per, _ = _api_compare(st, meta, ref, pos, types, L, half, cv0, True)
    context.current = None
    full = _umbrella_run(api, ref, True)[0].get_virial(per_particle=True)
    assert np.abs(per - full).max() <= 1e-7 * np.abs(full).max()       # (two runs with bias factors of their own grids: 1e-7, as the oracle's grid)


CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
for p in ("metadynamics-plugin_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(root, p))
import torch
import mtd_ref
import ql_virial_ref
import util
from metadynamics import _metadynamics, context, cv, integrate
pos, L = util.fcc_lattice(3)
pos = pos + np.random.default_rng(15).normal(0, 0.05, pos.shape)
context.initialize(pos, np.zeros(len(pos), dtype=np.int32), ["A"], L, dtype=np.float64)
context.current.system_definition.getParticleData().setPressureFlag(sys.argv[2] == "on")
meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
nl = cv.nlist_cell(r_cut=1.5)
half = util.build_nlist(pos, L, 1.5, half=True)
val = ql_virial_ref.oracle_cv(mtd_ref, pos, np.zeros(len(pos), dtype=np.int32), L, half, 1.4, 1.2, 6, 0, [0, 0, 0, 0, 1, 0, 1], half=True)[0]
st = cv.steinhardt(r_cut=1.4, r_on=1.2, lmax=6, Ql_ref=[0, 0, 0, 0, 1, 0, 1], nlist=nl, type="A", sigma=0.02 * val)
nl.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.half)
nl.set_lists(*half)
st.set_grid(0.55 * val, 1.3 * val, 64)
try:
    context.run(1)
    print("RESULT ran")
except RuntimeError as e:
    print("RESULT raised: %s" % e)
"""


@pytest.mark.parametrize("flag", ["on", "off"])
def test_third_law_diagnostic_with_the_pressure_flag_throws(flag):
    """MTD_QL_HALF_THIRD_LAW=1 keeps the third-law pass of a half list, which forms no virial: with the pressure flag the step throws a
    clear runtime_error, without it the step runs.  In a fresh child process: the variable is read once."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MTD_QL_HALF_THIRD_LAW="1")
    p = subprocess.run([sys.executable, "-c", CHILD, root, flag], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    if flag == "on":
        assert line.startswith("RESULT raised") and "third-law" in line and "virial" in line, line
    else:
        assert line == "RESULT ran", line
