#!/usr/bin/env python3
"""Developer tool: did cv.steinhardt move a bit between two builds of libmtd_hip.so?  The config 5 snapshot (256 000-particle noisy
fcc crystal, lmax 6, r_cut 1.4) through mtd_ql_accumulate / mtd_ql_forces, fp32 and fp64 arrays, full and half list.
usage: MTD_LIB_OVERRIDE=<lib> tools/ql_bits.py dump <out.npz>      value, Q_l, Q_lm and the force array of the four cases
       tools/ql_bits.py compare <a.npz> <b.npz>                    np.array_equal on every array; exit status 1 when one differs"""
import ctypes as C
import os
import sys

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "metadynamics-plugin_amd"), os.path.join(root, "tests")]


def dump(path):
    import torch
    import util
    from metadynamics import _abi as abi
    lib = abi.load()
    pos, L = util.fcc_lattice(40)
    pos = pos + np.random.default_rng(777).normal(0, 0.05, pos.shape)
    N = len(pos)
    types = np.zeros(N, dtype=np.int32)
    box = abi.Box.make(L)
    Ql_ref = util.dbl_array([0, 0, 0, 0, 1, 0, 1])
    out = {}
    for half in (0, 1):
        nl = util.build_nlist(pos, L, 1.4, half=bool(half))
        d_head, d_nn, d_nl = (torch.from_numpy(x.astype(np.int32)).cuda() for x in nl)
        for dtype in (np.float32, np.float64):
            dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
            d_pos = torch.from_numpy(util.pack_postype(pos.astype(dtype), types, dtype)).cuda()
            scratch = torch.zeros(lib.mtd_ql_scratch_doubles(6), dtype=torch.float64, device="cuda")
            p_val, p_ql, p_qlm = C.c_void_p(), C.c_void_p(), C.c_void_p()
            abi.check(lib.mtd_ql_accumulate(N, abi.ptr(d_pos), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), half, 1.4, 1.2, 6, 0,
                                            Ql_ref, N, abi.ptr(scratch), C.byref(p_val), C.byref(p_ql), C.byref(p_qlm), None))
            force = torch.zeros((N, 4), dtype=d_pos.dtype, device="cuda")
            d_bias = torch.tensor([0.9], dtype=torch.float64, device="cuda")
            abi.check(lib.mtd_ql_forces(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), half, 1.4,
                                        1.2, 6, 0, Ql_ref, N, abi.ptr(scratch), abi.ptr(d_bias), 0.0, None))
            torch.cuda.synchronize()
            s = scratch.cpu().numpy()
            off = lambda p: (p.value - scratch.data_ptr()) // 8
            key = "%s_%s" % ("half" if half else "full", np.dtype(dtype).name)
            out[key + "_value"] = s[off(p_val):off(p_val) + 1].copy()
            out[key + "_Ql"] = s[off(p_ql):off(p_ql) + 7].copy()
            out[key + "_Qlm"] = s[off(p_qlm):off(p_qlm) + 2 * 49].copy()
            out[key + "_force"] = force.cpu().numpy()
            print("%s: value %.17g, max |F| %.6g" % (key, out[key + "_value"][0], np.abs(out[key + "_force"]).max()))
    np.savez(path, **out)
    print("library %s -> %s" % (abi.LIB_PATH, path))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    same = sorted(A.files) == sorted(B.files)
    for k in sorted(A.files):
        eq = k in B.files and np.array_equal(A[k], B[k])
        same = same and eq
        print("%-24s %s" % (k, "identical bits" if eq else "DIFFERS"))
    print("all identical" if same else "NOT identical")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
