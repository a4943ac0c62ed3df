#!/usr/bin/env python3
"""Developer tool: did cv.pair_entropy, cv.environment_similarity, cv.debye_structure_factor or cv.coordination move a bit between two
builds of libmtd_hip.so?  All four walk the rows of a neighbour list through csrc/row_walk.hpp and share the kernels of
csrc/row_scale.hpp; this goes through the C ABI (mtd_pe_*, mtd_es_*, mtd_dsf_*, mtd_coord_*) with the snapshot builders of tests/util.py
and the parameter values of tests/test_gpu_pair_entropy.py, test_gpu_env_similarity.py, test_gpu_debye.py and test_gpu_coordination.py.
All cases are small:
noisy fcc crystals of N = 500 (a multiple of neither 32 nor 64) and N = 108 (environment similarity: one full chunk of 64 and a partial
one), fp32 and fp64 arrays, with and without the virial.
  pair entropy             n_bins 40 and 256 (the limit) on N = 500, 32 bins on N = 108; two types, so that some rows are empty; a
                           triclinic box; rows that address ghost particles
  environment similarity   every entry of VARIANTS of the test (fcc: the fused single walk; two, two_switch: the closed general path;
                           half_fcc: beta = 1 with an open environment), the diamond templates (open, general path), two types, the
                           ghost-row case, the triclinic case
  Debye structure factor   1, 2, 3 and 8 peaks on N = 500, each with the stored gradient and with the second walk
                           (mtd_dsf_set_store_gradient); a spectrum of 256 points and one of 5; N = 108, two types, the ghost rows (both
                           routes), the triclinic case
  coordination number      plain and switched with (n, m) = (6, 12) and (8, 14) on N = 500; N = 108; two types with A != B and with
                           A = B; the plain variable on the ghost rows (a switch refuses ghosts); the triclinic case
Per case every output array of the entry points: pair entropy sums, value, g, force, virial; environment similarity k^e_i, k_i, v_i, block
sums, force, virial; Debye sums, value, I_p, s_i, spectrum sums, spectrum, force, virial; coordination sums, value, n_i, v_i, force, virial.
usage: MTD_LIB_OVERRIDE=<lib> tools/row_bits.py dump <out.npz>
       tools/row_bits.py compare <a.npz> <b.npz>                         np.array_equal on every array; exit status 1 when one differs"""
import ctypes as C
import os
import sys

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]

TILT = dict(xy=0.15, xz=-0.1, yz=0.2)


def systems():
    """name -> dict(pos, types, L, tilt, n_rows, reach -> list): the snapshots of the tests; the lists are built on demand and kept"""
    import util
    from pair_entropy_ref import brute_nlist

    def noisy_fcc(n, seed=777):
        pos, L = util.fcc_lattice(n)
        return pos + np.random.default_rng(seed).normal(0, 0.05, pos.shape), L

    out = {}
    for name, cells, seed in (("n500", 5, 777), ("n108", 3, 4), ("two_types", 5, 5), ("ghosts", 5, 9)):
        pos, L = noisy_fcc(cells, seed)
        types = np.zeros(len(pos), dtype=np.int32)
        if name == "two_types":
            types = (np.random.default_rng(1).random(len(pos)) < 0.4).astype(np.int32)
        out[name] = dict(pos=pos, types=types, L=L, tilt=None, n_rows=300 if name == "ghosts" else len(pos), lists={},
                         build=lambda p, r, L=L: util.build_nlist(p, L, r))
    pos, L = noisy_fcc(4, 11)
    h = np.array([[L, TILT["xy"] * L, TILT["xz"] * L], [0, L, TILT["yz"] * L], [0, 0, L]])
    out["triclinic"] = dict(pos=(pos / L) @ h.T, types=np.zeros(len(pos), dtype=np.int32), L=L, tilt=TILT, n_rows=len(pos), lists={},
                            build=lambda p, r, h=h: brute_nlist(p, h, r))
    return out


def device_arrays(s, reach, dtype):
    """the positions rounded to dtype, and the list of the rounded snapshot cut to the central rows (the others are ghosts)"""
    import torch
    import util
    pos = s["pos"].astype(dtype).astype(np.float64)
    key = (reach, np.dtype(dtype).name)
    if key not in s["lists"]:
        head, nn, lst = s["build"](pos, reach)
        n = s["n_rows"]
        end = int(head[n]) if n < len(head) else len(lst)
        s["lists"][key] = tuple(torch.from_numpy(np.asarray(x).astype(np.int32)).cuda() for x in (head[:n], nn[:n], lst[:end]))
    return torch.from_numpy(util.pack_postype(pos.astype(dtype), s["types"], dtype)).cuda(), s["lists"][key]


def outputs(abi, force, vir, scratch, N, named):
    import torch
    torch.cuda.synchronize()
    sc = scratch.cpu().numpy()
    out = {name: sc[(p.value - scratch.data_ptr()) // 8:][:n].copy() for name, (p, n) in named.items()}
    out["force"] = force.cpu().numpy()
    if vir is not None:
        out["virial"] = vir.cpu().numpy()
    return out


def run_pe(abi, lib, s, par, type_id, dtype, virial):
    import torch
    r_max, sigma_r, n_bins = par
    d_pos, lists = device_arrays(s, r_max + 4.0 * sigma_r + 1e-9, dtype)
    N = s["n_rows"]
    box = abi.Box.make(s["L"], **(s["tilt"] or {}))
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    scratch = torch.zeros(lib.mtd_pe_scratch_doubles(n_bins), dtype=torch.float64, device="cuda")
    p_sums, p_value, p_g, n_sums = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint()
    lp = tuple(abi.ptr(x) for x in lists)
    abi.check(lib.mtd_pe_accumulate(N, abi.ptr(d_pos), dt, C.byref(box), *lp, r_max, sigma_r, n_bins, type_id, abi.ptr(scratch), C.byref(p_sums),
                                    C.byref(n_sums), None))
    abi.check(lib.mtd_pe_finalize(C.byref(box), r_max, sigma_r, n_bins, abi.ptr(scratch), C.byref(p_value), C.byref(p_g), None))
    force = torch.full((N, 4), 3.0, dtype=d_pos.dtype, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=d_pos.dtype, device="cuda") if virial else None
    d_bias = torch.tensor([0.9], dtype=torch.float64, device="cuda")
    abi.check(lib.mtd_pe_forces(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *lp, r_max, sigma_r, n_bins, type_id, abi.ptr(scratch),
                                abi.ptr(d_bias), 0.0, None, abi.ptr(vir) if virial else None, pitch if virial else 0))
    return outputs(abi, force, vir, scratch, N, dict(sums=(p_sums, n_sums.value), value=(p_value, 1), g=(p_g, n_bins)))


def run_es(abi, lib, s, templates, window, lam, sw, type_id, dtype, virial):
    import torch
    import env_similarity_ref as es
    from test_gpu_env_similarity import SIGMA_ENV
    r_on, r_cut, reach = window
    d_pos, lists = device_arrays(s, reach, dtype)
    N = s["n_rows"]
    n_global = len(s["pos"])
    box = abi.Box.make(s["L"], **(s["tilt"] or {}))
    par = abi.EsParams.make(es.as_environments(templates), SIGMA_ENV, r_on, r_cut, lam, sw)
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    scratch = torch.zeros(lib.mtd_es_scratch_doubles(N), dtype=torch.float64, device="cuda")
    p_part, p_k, p_ke, p_v, n_part = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint()
    lp = tuple(abi.ptr(x) for x in lists)
    abi.check(lib.mtd_es_accumulate(N, n_global - N, abi.ptr(d_pos), dt, C.byref(box), *lp, type_id, C.byref(par), n_global, abi.ptr(scratch),
                                    C.byref(p_part), C.byref(n_part), C.byref(p_k), C.byref(p_ke), C.byref(p_v), None))
    force = torch.full((N, 4), 3.0, dtype=d_pos.dtype, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=d_pos.dtype, device="cuda") if virial else None
    d_bias = torch.tensor([0.9], dtype=torch.float64, device="cuda")
    abi.check(lib.mtd_es_forces(N, n_global - N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *lp, type_id, C.byref(par), n_global,
                                abi.ptr(scratch), abi.ptr(d_bias), 0.0, None, abi.ptr(vir) if virial else None, pitch if virial else 0))
    return outputs(abi, force, vir, scratch, N, dict(partials=(p_part, n_part.value), ke=(p_ke, 4 * N), k=(p_k, N), v=(p_v, N)))


def run_dsf(abi, lib, s, peaks, r_cut, store, spectrum, type_id, dtype, virial):
    import torch
    q, c = peaks
    d_pos, lists = device_arrays(s, r_cut, dtype)
    N = s["n_rows"]
    box = abi.Box.make(s["L"], **(s["tilt"] or {}))
    par = abi.DsfParams.make(type_id, r_cut, q, c=c)
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    scratch = torch.zeros(lib.mtd_dsf_scratch_doubles(N), dtype=torch.float64, device="cuda")
    p_sums, p_value, p_I, p_local, p_ssums, p_spec = (C.c_void_p() for _ in range(6))
    n_sums, n_ssums = C.c_uint(), C.c_uint()
    call = abi.DsfCall(N, len(s["pos"]) - N, abi.ptr(d_pos), dt, C.pointer(box), *(abi.ptr(x) for x in lists), abi.ptr(scratch), None)
    force = torch.full((N, 4), 3.0, dtype=d_pos.dtype, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=d_pos.dtype, device="cuda") if virial else None
    d_bias = torch.tensor([0.9], dtype=torch.float64, device="cuda")
    abi.check(lib.mtd_dsf_set_store_gradient(1 if store else 0))
    try:
        abi.check(lib.mtd_dsf_accumulate(C.byref(par), C.byref(call), C.byref(p_sums), C.byref(n_sums)))
        abi.check(lib.mtd_dsf_finalize(C.byref(par), C.byref(call), C.byref(p_value), C.byref(p_I), C.byref(p_local)))
        abi.check(lib.mtd_dsf_forces(C.byref(par), C.byref(call), abi.ptr(force), abi.ptr(d_bias), 0.0, abi.ptr(vir) if virial else None,
                                     pitch if virial else 0))
        named = dict(sums=(p_sums, n_sums.value), value=(p_value, 1), I=(p_I, len(q)), local=(p_local, N))
        if spectrum is not None:
            abi.check(lib.mtd_dsf_spectrum(C.byref(par), C.byref(call), *spectrum, C.byref(p_ssums), C.byref(n_ssums)))
            abi.check(lib.mtd_dsf_spectrum_finalize(C.byref(call), *spectrum, C.byref(p_spec)))
            named.update(spectrum_sums=(p_ssums, n_ssums.value), spectrum=(p_spec, spectrum[2]))
    finally:
        abi.check(lib.mtd_dsf_set_store_gradient(1))
    return outputs(abi, force, vir, scratch, N, named)


def run_cn(abi, lib, s, pair, nm, r_cut, switch, dtype, virial):
    import torch
    from test_gpu_coordination import R0
    d_pos, lists = device_arrays(s, r_cut, dtype)
    N = s["n_rows"]
    box = abi.Box.make(s["L"], **(s["tilt"] or {}))
    par = abi.CoordParams.make(pair[0], pair[1], R0, r_cut, n=nm[0], m=nm[1], switch=switch)
    dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
    scratch = torch.zeros(lib.mtd_coord_scratch_doubles(N), dtype=torch.float64, device="cuda")
    p_sums, p_value, p_local, p_switched, n_sums = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint()
    call = abi.CoordCall(N, len(s["pos"]) - N, abi.ptr(d_pos), dt, C.pointer(box), *(abi.ptr(x) for x in lists), abi.ptr(scratch), None)
    force = torch.full((N, 4), 3.0, dtype=d_pos.dtype, device="cuda")
    pitch = N + 3
    vir = torch.full((6, pitch), 7.0, dtype=d_pos.dtype, device="cuda") if virial else None
    d_bias = torch.tensor([0.9], dtype=torch.float64, device="cuda")
    abi.check(lib.mtd_coord_accumulate(C.byref(par), C.byref(call), C.byref(p_sums), C.byref(n_sums)))
    abi.check(lib.mtd_coord_finalize(C.byref(par), C.byref(call), C.byref(p_value), C.byref(p_local), C.byref(p_switched)))
    abi.check(lib.mtd_coord_forces(C.byref(par), C.byref(call), abi.ptr(force), abi.ptr(d_bias), 0.0, abi.ptr(vir) if virial else None,
                                   pitch if virial else 0))
    return outputs(abi, force, vir, scratch, N, dict(sums=(p_sums, n_sums.value), value=(p_value, 1), local=(p_local, N), switched=(p_switched, N)))


def cases():
    """(name, runner, system, arguments after the system) — the virial flag and the dtype are added by dump"""
    import env_similarity_ref as es
    from test_gpu_env_similarity import R_CUT, R_ON, SWITCH, VARIANTS
    out = [("pe_n500_b40", run_pe, "n500", ((2.0, 0.1, 40), 0)), ("pe_n500_b256", run_pe, "n500", ((2.0, 0.05, 256), 0)),
           ("pe_n108_b32", run_pe, "n108", ((1.6, 0.1, 32), 0)), ("pe_two_types_t0", run_pe, "two_types", ((2.0, 0.1, 40), 0)),
           ("pe_two_types_t1", run_pe, "two_types", ((2.0, 0.1, 40), 1)), ("pe_ghosts", run_pe, "ghosts", ((2.0, 0.1, 40), 0)),
           ("pe_triclinic", run_pe, "triclinic", ((1.6, 0.1, 32), 0))]
    window = (R_ON, R_CUT, R_CUT)
    for name, (t, lam, sw, _) in VARIANTS.items():
        out.append(("es_n500_" + name, run_es, "n500", (t, window, lam, sw, 0)))
        out.append(("es_n108_" + name, run_es, "n108", (t, window, lam, sw, 0)))
    # two environments that are each other's inverse: neither is closed (the general path with both Gaussians)
    out.append(("es_n500_open_general", run_es, "n500", (es.templates("diamond", 4.0 / np.sqrt(3.0)), window, 100.0, None, 0)))
    out.append(("es_two_types_t1", run_es, "two_types", (VARIANTS["two_switch"][0], window, 20.0, SWITCH, 1)))
    out.append(("es_ghosts", run_es, "ghosts", (VARIANTS["fcc"][0], window, 100.0, None, 0)))
    out.append(("es_triclinic", run_es, "triclinic", (VARIANTS["fcc"][0], (R_ON, R_CUT, 1.55), 100.0, None, 0)))
    from test_gpu_coordination import R_CUT as CN_R_CUT, SWITCHES
    from test_gpu_debye import PEAKS
    peaks = dict(PEAKS)
    peaks[2] = tuple(x[:2] for x in PEAKS[3])
    for P in (1, 2, 3, 8):                                 # (the compiled peak counts are 1, 2, 4, 8: three peaks run the kernel of four)
        for store in (True, False):
            out.append(("dsf_n500_q%d_%s" % (P, "store" if store else "walk"), run_dsf, "n500",
                        (peaks[P], 2.4, store, (2.0, 12.0, 256) if P == 1 and store else None, 0)))
    out.append(("dsf_n108_q3", run_dsf, "n108", (peaks[3], 1.5, True, (2.0, 12.0, 5), 0)))
    out.append(("dsf_two_types_t1", run_dsf, "two_types", (peaks[3], 2.4, True, None, 1)))
    out.append(("dsf_ghosts_q3", run_dsf, "ghosts", (peaks[3], 2.4, True, None, 0)))
    out.append(("dsf_ghosts_q3_walk", run_dsf, "ghosts", (peaks[3], 2.4, False, None, 0)))
    out.append(("dsf_triclinic", run_dsf, "triclinic", (peaks[2], 1.5, True, None, 0)))
    for mode in ("plain", "switch"):
        for nm in ((6, 12), (8, 14)):
            out.append(("cn_n500_%s_%d_%d" % ((mode,) + nm), run_cn, "n500", ((0, 0), nm, CN_R_CUT, SWITCHES[mode])))
            out.append(("cn_two_types_ab_%s_%d_%d" % ((mode,) + nm), run_cn, "two_types", ((0, 1), nm, CN_R_CUT, SWITCHES[mode])))
        out.append(("cn_n108_" + mode, run_cn, "n108", ((0, 0), (6, 12), 1.5, SWITCHES[mode])))
        out.append(("cn_two_types_bb_" + mode, run_cn, "two_types", ((1, 1), (6, 12), CN_R_CUT, SWITCHES[mode])))
        out.append(("cn_triclinic_" + mode, run_cn, "triclinic", ((0, 0), (6, 12), 1.5, SWITCHES[mode])))
    out.append(("cn_two_types_ba_less", run_cn, "two_types", ((1, 0), (6, 12), CN_R_CUT, SWITCHES["less"])))
    for nm in ((6, 12), (8, 14)):                          # (a switch refuses ghosts)
        out.append(("cn_ghosts_plain_%d_%d" % nm, run_cn, "ghosts", ((0, 0), nm, CN_R_CUT, None)))
    return out


def dump(path):
    import torch  # noqa: F401  (first: its HIP runtime is the one the library binds to)
    from metadynamics import _abi as abi
    lib = abi.load()
    sysm, out = systems(), {}
    for name, run, system, args in cases():
        for dtype in (np.float32, np.float64):
            for virial in (False, True):
                key = "%s_%s_%s" % (name, np.dtype(dtype).name, "vir" if virial else "plain")
                res = run(abi, lib, sysm[system], *args, dtype, virial)
                finite = all(np.isfinite(v).all() for v in res.values())
                print("%-44s N %4d: max |F| %.6g, %s%s" % (key, len(res["force"]), np.abs(res["force"][:, :3]).max(),
                                                          ", ".join("%s %d" % (k, v.size) for k, v in res.items()), "" if finite else "  NOT FINITE"))
                for k, v in res.items():
                    out[key + "_" + k] = v
    np.savez(path, **out)
    print("library %s -> %s (%d arrays)" % (abi.LIB_PATH, path, len(out)))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    same = sorted(A.files) == sorted(B.files)
    for k in sorted(A.files):
        eq = k in B.files and np.array_equal(A[k], B[k])
        same = same and eq
        print("%-56s %s" % (k, "identical bits" if eq else "DIFFERS"))
    print("all %d identical" % len(A.files) if same else "NOT identical")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
