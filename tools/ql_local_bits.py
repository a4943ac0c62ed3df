#!/usr/bin/env python3
"""Developer tool: did the PLAIN cv.steinhardt_local move a bit between two builds of libmtd_hip.so?  The config 5 snapshot
(256 000-particle noisy fcc crystal, lmax 6, r_cut 1.4) through mtd_ql_local_accumulate / mtd_ql_local_forces, fp32 and fp64 arrays.
usage: MTD_LIB_OVERRIDE=<lib> tools/ql_local_bits.py dump <out.npz>      c_i, n_i, block sums and the force array of both cases
       tools/ql_local_bits.py compare <a.npz> <b.npz>                    np.array_equal on every array; exit status 1 when one differs"""
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
    nl = util.build_nlist(pos, L, 1.4)
    d_head, d_nn, d_nl = (torch.from_numpy(x.astype(np.int32)).cuda() for x in nl)
    out = {}
    for dtype in (np.float32, np.float64):
        dt = abi.MTD_F32 if dtype == np.float32 else abi.MTD_F64
        d_pos = torch.from_numpy(util.pack_postype(pos.astype(dtype), types, dtype)).cuda()
        scratch = torch.zeros(lib.mtd_ql_local_scratch_doubles(N, 6), dtype=torch.float64, device="cuda")
        p_part, p_c, p_n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n_part = C.c_uint()
        abi.check(lib.mtd_ql_local_accumulate(N, abi.ptr(d_pos), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), 1.4, 1.2, 6, 0, Ql_ref,
                                              N, abi.ptr(scratch), C.byref(p_part), C.byref(n_part), C.byref(p_c), C.byref(p_n), None))
        force = torch.zeros((N, 4), dtype=d_pos.dtype, device="cuda")
        d_bias = torch.tensor([0.9], dtype=torch.float64, device="cuda")
        abi.check(lib.mtd_ql_local_forces(N, abi.ptr(d_pos), abi.ptr(force), dt, C.byref(box), abi.ptr(d_head), abi.ptr(d_nn), abi.ptr(d_nl), 1.4, 1.2,
                                          6, 0, Ql_ref, N, abi.ptr(scratch), abi.ptr(d_bias), 0.0, None))
        torch.cuda.synchronize()
        s = scratch.cpu().numpy()
        off = lambda p: (p.value - scratch.data_ptr()) // 8
        key = np.dtype(dtype).name
        out[key + "_partials"] = s[off(p_part):off(p_part) + n_part.value].copy()
        out[key + "_c"] = s[off(p_c):off(p_c) + N].copy()
        out[key + "_n"] = s[off(p_n):off(p_n) + N].copy()
        out[key + "_force"] = force.cpu().numpy()
        print("%s: s %.17g, max |F| %.6g" % (key, out[key + "_partials"].sum() / N, np.abs(out[key + "_force"]).max()))
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
