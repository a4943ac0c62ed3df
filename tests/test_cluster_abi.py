"""CPU: the cluster pass (mtd_cluster_*, csrc/cluster.hip) and the entry point of the local Steinhardt variable that uses it
(mtd_ql_local_accumulate_cluster) are exported and declared, and refuse what they do not take before they touch a device.  Nothing here
needs a GPU: every pointer is a small non-null value that is never dereferenced when the arguments are refused."""
import ctypes as C

import util

CLUSTER_SYMBOLS = ("mtd_cluster_scratch_bytes", "mtd_cluster_largest", "mtd_ql_local_accumulate_cluster")
INVALID, UNSUPPORTED = -1, -2
NAN, INF = float("nan"), float("inf")


def test_cluster_symbols_exported_and_declared(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in CLUSTER_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    assert abi.MTD_CLUSTER_NONE == 0xffffffff
    assert C.sizeof(abi.ClusterParams) == 24


def test_cluster_scratch_size(abi):
    lib = abi.load()
    # parent, label and size (4 bytes each), w (8 bytes), the summary and the key of the pick; every segment 16-byte aligned
    for n in (0, 1, 2, 3, 5, 1000, 4099, 256000):
        got = lib.mtd_cluster_scratch_bytes(n)
        assert got % 16 == 0
        assert 20 * n + 24 <= got <= 20 * n + 24 + 5 * 16


def _largest(lib, abi, box, n=4, pos=1, head=1, nn=1, nl=1, v=1, dtype=1, cluster=(0.5, 1.4), scratch=4096, on=None):
    p = abi.ClusterParams.make(cluster) if cluster is not None else None
    if on is not None:
        p.on = on
    out = [C.c_void_p() for _ in range(4)]
    return lib.mtd_cluster_largest(n, pos * 4096 or None, dtype, C.byref(box) if box is not None else None, head * 4096 or None,
                                   nn * 4096 or None, nl * 4096 or None, 0, v * 4096 or None, C.byref(p) if p is not None else None,
                                   scratch or None, *[C.byref(o) for o in out], None)


def test_cluster_largest_refusals_without_gpu(abi):
    """null pointers, an unknown dtype, r_link <= 0 or not finite, v_min not finite, a misaligned scratch, p == NULL and on == 0"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _largest(lib, abi, None) == INVALID
    for key in ("pos", "head", "nn", "nl", "v", "scratch"):
        assert _largest(lib, abi, box, **{key: 0}) == INVALID, key
    assert _largest(lib, abi, box, dtype=7) == INVALID
    assert _largest(lib, abi, box, scratch=4096 + 8) == INVALID
    for r_link in (0.0, -1.0, NAN, INF):
        assert _largest(lib, abi, box, cluster=(0.5, r_link)) == INVALID, r_link
    for v_min in (NAN, INF, -INF):
        assert _largest(lib, abi, box, cluster=(v_min, 1.4)) == INVALID, v_min
    assert _largest(lib, abi, box, cluster=None) == INVALID
    assert _largest(lib, abi, box, on=0) == INVALID


def _acc(lib, abi, box, n=4, cluster=(0.5, 1.4), cscratch=8192, opt=None, bonds=None, on=None, scratch=4096, rcut=1.4):
    p = abi.ClusterParams.make(cluster)
    if on is not None:
        p.on = on
    o = abi.QlLocalOptions.make(**(opt or {}))
    bd = abi.QlLocalBonds.make(bonds)
    partials, n_partials = C.c_void_p(), C.c_uint()
    outs = [C.c_void_p() for _ in range(7)]
    ql_ref = util.dbl_array([0, 0, 0, 0, 0, 0, 1])
    return lib.mtd_ql_local_accumulate_cluster(n, 4096, 1, C.byref(box), 4096, 4096, 4096, rcut, 1.2, 6, 0, ql_ref, 4, scratch or None,
                                               C.byref(partials), C.byref(n_partials), C.byref(outs[0]), C.byref(outs[1]), None, C.byref(o),
                                               C.byref(outs[2]), C.byref(bd), C.byref(outs[3]), C.byref(p), cscratch or None,
                                               C.byref(outs[4]), C.byref(outs[5]), C.byref(outs[6]))


def test_ql_local_accumulate_cluster_refusals_without_gpu(abi):
    """with the option on: the refusals of the cluster pass and `average` (MTD_ERR_UNSUPPORTED), before the first launch; the refusals of
    the variable itself stay what they were"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for r_link in (0.0, -1.0, NAN, INF):
        assert _acc(lib, abi, box, cluster=(0.5, r_link)) == INVALID
    for v_min in (NAN, INF):
        assert _acc(lib, abi, box, cluster=(v_min, 1.4)) == INVALID
    assert _acc(lib, abi, box, cscratch=0) == INVALID
    assert _acc(lib, abi, box, cscratch=8192 + 8) == INVALID
    assert _acc(lib, abi, box, opt=dict(average=True)) == UNSUPPORTED
    assert _acc(lib, abi, box, opt=dict(average=True, switch=(0.1, 3))) == UNSUPPORTED
    assert _acc(lib, abi, box, bonds=(0.7, 0.5)) == INVALID            # the variable's own refusals come first
    assert _acc(lib, abi, box, scratch=0) == INVALID
    assert _acc(lib, abi, box, rcut=-1.0) == INVALID
    assert _acc(lib, abi, box, rcut=-1.0, on=0) == INVALID              # ... with the option off too
