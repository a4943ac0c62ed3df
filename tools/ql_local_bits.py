#!/usr/bin/env python3
"""Developer tool: did cv.steinhardt_local move a bit between two builds of libmtd_hip.so?  The config 5 snapshot (256 000-particle noisy
fcc crystal, lmax 6, r_cut 1.4) through mtd_ql_local_accumulate_opt / mtd_ql_local_forces_opt, fp32 and fp64 arrays: the plain variable
and the option paths (average; switch + gate; average + switch + gate); and on a 16^3-cell snapshot of 16 384 particles the direct force
pass (rows longer than 256 bytes), plain and averaged: lmax 12 (rows of 784 bytes, four gather windows) and every degree up to 6 and up to 8
(448 and 720 bytes: the compiled bounds 6 and 8), and the tile force pass under the compiled bounds 8 and 12 (degrees 4 and 6 at lmax 8 and 12).
The four gather passes with something to gather: the 16^3-cell snapshot at noise 0.13, where the products d_ij populate all three parts of
the ramp (0.3, 0.8) (at 0.05 every bond lies above it and the second bonds pass sums zeros): the bond count, bare and with switch and gate,
with rows of 128 bytes (e_6: half a gather window), 208 bytes (degrees 4 and 6: one window) and 784 bytes (lmax 12: four windows, d and
E summed over them), and the average at lmax 12.  Every case goes through mtd_ql_local_accumulate_bonds / mtd_ql_local_forces_bonds, to
which the _opt entry points forward.
usage: MTD_LIB_OVERRIDE=<lib> tools/ql_local_bits.py dump <out.npz>      c_i, n_i, v_i, block sums and the force array of every case, b_i of the bonds cases
       tools/ql_local_bits.py compare <a.npz> <b.npz>                    np.array_equal on every array; exit status 1 when one differs"""
import ctypes as C
import os
import sys

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]

QL_46 = [0, 0, 0, 0, 1, 0, 1]
QL_12 = [0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0.5, 0.3, 0.25]
QL_ALL = [0.1, 0.2, 0.3, 0.4, 1, 0.5, 1, 0.6, 0.7]
QL_6 = [0, 0, 0, 0, 0, 0, 1]
RAMP, SWITCH_GATE = (0.3, 0.8), dict(switch=(6.5, 6), gate=(10, 13))
# (name, fcc cells, lmax, Ql_ref, options[, noise: 0.05 unless given])
CASES = (("plain", 40, 6, QL_46, {}),
         ("average", 40, 6, QL_46, dict(average=True)),
         ("switch+gate", 40, 6, QL_46, dict(switch=(0.25, 3), gate=(4, 8))),
         ("average+switch+gate", 40, 6, QL_46, dict(average=True, switch=(0.12, 3), gate=(4, 8))),
         ("lmax12", 16, 12, QL_12, {}),
         # every degree in use: rows of 448 and 720 bytes, the direct force pass at the compiled bounds 6 and 8, with and without E
         ("lmax6all", 16, 6, QL_ALL[:7], {}),
         ("lmax6all+average", 16, 6, QL_ALL[:7], dict(average=True)),
         ("lmax8all", 16, 8, QL_ALL, {}),
         ("lmax8all+average", 16, 8, QL_ALL, dict(average=True)),
         ("lmax12+average", 16, 12, QL_12, dict(average=True)),
         # degrees 4 and 6 under the compiled bounds 8 and 12: rows of 208 bytes, the tile force pass of those instantiations
         ("lmax8tile", 16, 8, QL_46 + [0] * 2, {}),
         ("lmax8tile+average", 16, 8, QL_46 + [0] * 2, dict(average=True)),
         ("lmax12tile", 16, 12, QL_46 + [0] * 6, {}),
         ("lmax12tile+average", 16, 12, QL_46 + [0] * 6, dict(average=True)),
         # the gather passes at noise 0.13: rows of half a window, one window and four windows
         ("bonds_e6", 16, 6, QL_6, dict(bonds=RAMP), 0.13),
         ("bonds_e6+switch+gate", 16, 6, QL_6, dict(bonds=RAMP, **SWITCH_GATE), 0.13),
         ("bonds_46", 16, 6, QL_46, dict(bonds=RAMP), 0.13),
         ("bonds_46+switch+gate", 16, 6, QL_46, dict(bonds=RAMP, **SWITCH_GATE), 0.13),
         ("bonds_lmax12", 16, 12, QL_12, dict(bonds=RAMP), 0.13),
         ("average_lmax12_noisy", 16, 12, QL_12, dict(average=True), 0.13))


def dump(path):
    import torch
    import util
    from metadynamics import _abi as abi
    lib = abi.load()
    out, systems = {}, {}
    for name, cells, lmax, ql, opt, *noise in CASES:
        noise = noise[0] if noise else 0.05
        if (cells, noise) not in systems:
            pos, L = util.fcc_lattice(cells)
            pos = pos + np.random.default_rng(777).normal(0, noise, pos.shape)
            systems[cells, noise] = (pos, L, [torch.from_numpy(x.astype(np.int32)).cuda() for x in util.build_nlist(pos, L, 1.4)])
        pos, L, (d_head, d_nn, d_nl) = systems[cells, noise]
        N = len(pos)
        types = np.zeros(N, dtype=np.int32)
        box = abi.Box.make(L)
        Ql_ref = util.dbl_array(ql)
        o = abi.QlLocalOptions.make(**{k: v for k, v in opt.items() if k != "bonds"})
        bo = abi.QlLocalBonds.make(opt.get("bonds"))
        for dtype in (np.float32, np.float64):
            dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
            d_pos = torch.from_numpy(util.pack_postype(pos.astype(dtype), types, dtype)).cuda()
            scratch = torch.zeros(lib.mtd_ql_local_scratch_doubles_bonds(N, lmax, d_nl.numel(), C.byref(o), C.byref(bo)), dtype=torch.float64, device="cuda")
            p_part, p_c, p_n, p_v, p_b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            n_part = C.c_uint()
            common = (abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), 1.4, 1.2, lmax, 0, Ql_ref, N, abi.ptr(scratch))
            abi.check(lib.mtd_ql_local_accumulate_bonds(N, abi.ptr(d_pos), dt, C.byref(box), *common, C.byref(p_part), C.byref(n_part), C.byref(p_c),
                                                        C.byref(p_n), None, C.byref(o), C.byref(p_v), C.byref(bo), C.byref(p_b)))
            force = torch.zeros((N, 4), dtype=d_pos.dtype, device="cuda")
            d_bias = torch.tensor([0.9], dtype=torch.float64, device="cuda")
            abi.check(lib.mtd_ql_local_forces_bonds(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), *common, abi.ptr(d_bias), 0.0, None, C.byref(o),
                                                    None, 0, C.byref(bo)))
            torch.cuda.synchronize()
            s = scratch.cpu().numpy()
            off = lambda p: (p.value - scratch.data_ptr()) // 8
            key = name + "_" + np.dtype(dtype).name
            out[key + "_partials"] = s[off(p_part):off(p_part) + n_part.value].copy()
            tags = (("c", p_c), ("n", p_n), ("v", p_v)) + ((("b", p_b),) if bo.on else ())
            for tag, p in tags:
                out[key + "_" + tag] = s[off(p):off(p) + N].copy()
            out[key + "_force"] = force.cpu().numpy()
            finite = all(np.isfinite(out[key + "_" + tag]).all() for tag in ("partials", "force") + tuple(t for t, _ in tags))
            print("%-36s N %6d: s %.17g, max |F| %.6g%s%s" % (key, N, out[key + "_partials"].sum() / N, np.abs(out[key + "_force"]).max(),
                                                           ", mean b %.4f of mean n %.4f" % (out[key + "_b"].mean(), out[key + "_n"].mean()) if bo.on else "",
                                                           "" if finite else "  NOT FINITE"))
            del scratch, force, d_pos
    np.savez(path, **out)
    print("library %s -> %s" % (abi.LIB_PATH, path))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    same = sorted(A.files) == sorted(B.files)
    for k in sorted(A.files):
        eq = k in B.files and np.array_equal(A[k], B[k])
        same = same and eq
        print("%-52s %s" % (k, "identical bits" if eq else "DIFFERS"))
    print("all identical" if same else "NOT identical")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
