"""The runner and the comparisons the GPU tests of the largest-cluster entry points share (helper, no test):
mtd_coord_accumulate_cluster and mtd_tetrahedral_accumulate_cluster through the C ABI, then the unit's own _finalize and _forces, with BOTH
scratches pre-filled with garbage (NaN doubles in the unit's, 0xAB bytes in the cluster pass's).

Tolerances, those of tests/test_gpu_coordination.py and tests/test_gpu_tetrahedral.py: value 1e-9 relative; n_i, t_i and v_i 1e-9 of
their maximum; forces and per-particle virial 1e-9 of their maximum with fp64 arrays and 2e-7 with fp32 arrays (one rounding on store),
the six virial sums to the same figure relative.  Mask, labels and summary are compared EXACTLY: the fixtures keep every v_i and every pair
distance at least 1e-6 (relative, for r) from the thresholds, and the GPU's v_i and r^2 are good to 1e-9 and a few ulp."""
import ctypes as C

import numpy as np

import stream_gate
import util

UNITS = {
    "coordination": dict(scratch="mtd_coord_scratch_doubles", plain="mtd_coord_accumulate", cluster="mtd_coord_accumulate_cluster",
                         finalize="mtd_coord_finalize", forces="mtd_coord_forces", per_particle=("local", "switched")),
    "tetrahedral": dict(scratch="mtd_tet_scratch_doubles", plain="mtd_tet_accumulate", cluster="mtd_tetrahedral_accumulate_cluster",
                        finalize="mtd_tet_finalize", forces="mtd_tet_forces", per_particle=("local", "switched", "coordination")),
}
OUTPUTS = ("s", "sums", "local", "switched", "F", "virial", "w", "label", "summary")


def _params(abi, kind, par):
    if kind == "coordination":
        return abi.CoordParams.make(par["type_a"], par["type_b"], par["r_0"], par["r_cut"], d_0=par["d_0"], n=par["n"], m=par["m"], switch=par["switch"])
    return abi.TetParams.make(par["type"], par["r_cut"], par["r_on"], cos0=par["cos0"], normalise=par["normalise"], switch=par["switch"],
                              gate=par["gate"])


def run(abi, kind, pos, types, L, nl, par, dtype, cluster=None, entry="cluster", off="null", bias=0.9, virial=True, gate=None, expect=0):
    """One step.  cluster: (v_min, r_link), or None — then entry = "plain" calls the unit's plain accumulate and entry = "cluster" the new
    one with cluster == NULL (off = "null") or an all-zero struct (off = "zero") and no cluster scratch.  Returns dict(s, sums, local,
    switched[, coordination], F, virial, w, label, summary (None when off), scratch (the unit's whole scratch as int64), null (the three
    cluster pointers came back NULL)); expect: the status the accumulate must return (then nothing else is called)"""
    import torch
    lib = abi.load()
    u = UNITS[kind]
    gate = gate or stream_gate.Plain()
    N = len(nl[0])
    box = abi.Box.make(L)
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    d_pos = gate.inp(util.pack_postype(pos.astype(dtype), types, dtype))
    d_head, d_nn = (gate.inp(np.asarray(x).astype(np.int32)) for x in nl[:2])
    d_nl = gate.inp(np.asarray(nl[2]).astype(np.int32) if len(nl[2]) else np.zeros(1, dtype=np.int32))
    d_bias = gate.inp(np.array([bias], dtype=np.float64))
    scratch = torch.full((getattr(lib, u["scratch"])(N),), float("nan"), dtype=torch.float64, device="cuda")
    cscratch = torch.full((lib.mtd_cluster_scratch_bytes(N),), 0xAB, dtype=torch.uint8, device="cuda")
    force = torch.full((max(N, 1), 4), 3.0, dtype=tdt, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=tdt, device="cuda") if virial else None
    cpar = _params(abi, kind, par)
    p_sums, p_value, p_local, p_switched, p_coord = (C.c_void_p() for _ in range(5))
    p_w, p_label, p_summary = (C.c_void_p(1) for _ in range(3))
    n_sums = C.c_uint()
    stream = gate.arm()
    call = abi.RowCall(N, 0, abi.ptr(d_pos), dt, C.pointer(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), abi.ptr(scratch), stream)
    if entry == "plain":
        assert cluster is None
        rc = getattr(lib, u["plain"])(C.byref(cpar), C.byref(call), C.byref(p_sums), C.byref(n_sums))
        p_w = p_label = p_summary = C.c_void_p()
    else:
        cl = abi.ClusterParams.make(cluster)
        rc = getattr(lib, u["cluster"])(C.byref(cpar), C.byref(call), None if cluster is None and off == "null" else C.byref(cl),
                                        abi.ptr(cscratch) if cluster is not None else None, C.byref(p_sums), C.byref(n_sums), C.byref(p_w),
                                        C.byref(p_label), C.byref(p_summary))
    if expect:
        assert rc == expect
        return gate.done(lambda: None)
    abi.check(rc)
    assert n_sums.value == 2
    if kind == "coordination":
        abi.check(lib.mtd_coord_finalize(C.byref(cpar), C.byref(call), C.byref(p_value), C.byref(p_local), C.byref(p_switched)))
    else:
        abi.check(lib.mtd_tet_finalize(C.byref(cpar), C.byref(call), C.byref(p_value), C.byref(p_local), C.byref(p_switched), C.byref(p_coord)))
    abi.check(getattr(lib, u["forces"])(C.byref(cpar), C.byref(call), abi.ptr(force), abi.ptr(d_bias), 0.0, abi.ptr(vir) if virial else None,
                                        pitch if virial else 0))
    null = not (p_w.value or p_label.value or p_summary.value)
    assert null == (cluster is None)

    def read():
        s = scratch.cpu().numpy()
        off_ = lambda p: (p.value - scratch.data_ptr()) // 8
        per = lambda p: s[off_(p):off_(p) + N].copy()
        out = dict(s=float(s[off_(p_value)]), sums=s[off_(p_sums):off_(p_sums) + 2].copy(), local=per(p_local), switched=per(p_switched),
                   F=force.cpu().numpy().astype(np.float64)[:N], virial=None, w=None, label=None, summary=None, scratch=s.view(np.int64).copy(),
                   null=null)
        if kind == "tetrahedral":
            out["coordination"] = per(p_coord)
        if virial:
            v = vir.cpu().numpy().astype(np.float64)
            assert np.all(v[:, N:] == 7.0)                                  # [n_particles, pitch) is left alone
            out["virial"] = v[:, :N].T.copy()
        if cluster is not None:
            raw = cscratch.cpu().numpy()
            at = lambda p: p.value - cscratch.data_ptr()
            assert 0 <= at(p_summary) and at(p_w) + 8 * N <= len(raw) and at(p_label) + 4 * N <= len(raw)
            out["w"] = raw[at(p_w):at(p_w) + 8 * N].view(np.float64).copy()
            out["label"] = raw[at(p_label):at(p_label) + 4 * N].view(np.uint32).copy()
            out["summary"] = raw[at(p_summary):at(p_summary) + 16].view(np.uint32).copy()
        return out
    return gate.done(read)


def compare(kind, g, r, bias, dtype, types, type_id, forces=True):
    """prints every figure, then asserts; r: row_cluster_ref.coordination / .tetrahedral formed with the same bias"""
    assert np.array_equal(g["w"], r["w"]) and np.array_equal(g["label"], r["label"]) and np.array_equal(g["summary"], r["summary"])
    count = r["n_a"] if kind == "coordination" else r["n_t"]
    err_s = abs(g["s"] - r["s"]) / abs(r["s"]) if r["s"] else abs(g["s"])
    keys = UNITS[kind]["per_particle"]
    err = {k: np.abs(g[k] - r[k]).max() / max(np.abs(r[k]).max(), 1e-300) for k in keys}
    F_ref = r["force"]
    fs, err_f = np.abs(F_ref).max(), np.abs(g["F"][:, :3] - F_ref).max()
    print("%s: s %.15g vs %.15g (%.3e rel); %s of their maxima; forces: max |d| %.3e of max |F| %.3e (%.3e rel); summary %s"
          % (kind, g["s"], r["s"], err_s, ", ".join("%s %.3e" % (k, err[k]) for k in keys), err_f, fs, err_f / fs if fs else 0.0, g["summary"]))
    assert np.isfinite(g["F"]).all() and np.isfinite(g["s"]) and all(np.isfinite(g[k]).all() for k in keys)
    assert g["sums"][1] == count                                        # the UNMASKED count
    assert err_s <= 1e-9 and all(e <= 1e-9 for e in err.values())
    tol = 1e-9 if dtype == np.float64 else 2e-7
    if forces:
        assert fs > 0
    assert err_f <= tol * fs
    assert np.all(g["F"][:, 3] == 0.0) and np.all(g["F"][types != type_id] == 0.0)
    top_w = np.abs(r["virial"]).max()
    err_w = np.abs(g["virial"] - r["virial"]).max()
    W, W_ref = g["virial"].sum(axis=0), r["virial"].sum(axis=0)
    err_sum = np.abs(W - W_ref).max() / np.abs(W_ref).max() if top_w else np.abs(W).max()
    print("virial: max |d| %.3e of max |virial_i| %.3e (%.3e rel); sums %.3e rel" % (err_w, top_w, err_w / top_w if top_w else 0.0, err_sum))
    if forces:
        assert top_w > 0
    assert err_w <= tol * top_w and err_sum <= tol
    assert np.all(g["virial"][types != type_id] == 0.0)


def same_bits(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        if x is None or y is None:
            assert x is None and y is None, k
        else:
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), k
