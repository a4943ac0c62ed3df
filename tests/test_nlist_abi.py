"""CPU: the device neighbour-list build (mtd_nlist_*, csrc/nlist.hip) is exported and declared, validates its arguments before it
touches a device, and is reachable from the host classes and the Python API.  Nothing here needs a GPU."""
import ctypes as C
import inspect

import pytest

NLIST_SYMBOLS = ("mtd_nlist_create", "mtd_nlist_destroy", "mtd_nlist_build", "mtd_nlist_check", "mtd_nlist_cells")


def test_nlist_symbols_exported_and_declared(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in NLIST_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s


def _build(lib, abi, h, box, r_list, dtype=1, n_local=0, n_ghost=0, half=0):
    head, nn, nl = C.c_void_p(), C.c_void_p(), C.c_void_p()
    n = C.c_size_t()
    return lib.mtd_nlist_build(h, n_local, n_ghost, None, dtype, C.byref(box), r_list, half, -1, C.byref(head), C.byref(nn), C.byref(nl),
                               C.byref(n), None)


def test_nlist_argument_validation_without_gpu(abi):
    """null handle, r_list <= 0, an unknown dtype and r_list > d_k / 2 are refused before any device call"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _build(lib, abi, None, box, 1.0) == -1
    assert lib.mtd_nlist_create(None) == -1
    assert lib.mtd_nlist_destroy(None) == -1
    h = C.c_void_p()
    assert lib.mtd_nlist_create(C.byref(h)) == 0 and h.value            # (no device is touched: buffers come with the first build)
    try:
        assert _build(lib, abi, h, box, 0.0) == -1
        assert _build(lib, abi, h, box, -1.0) == -1
        assert _build(lib, abi, h, box, float("nan")) == -1
        assert _build(lib, abi, h, box, 1.0, dtype=7) == -1
        assert _build(lib, abi, h, box, 5.0 * (1 + 1e-12)) == -1        # r_list > L / 2
        # the distance between the faces shrinks with the tilt: d_x = L / sqrt(1 + xy^2 + (xy yz - xz)^2)
        tilted = abi.Box.make(10.0, xy=0.4)
        d_x = 10.0 / (1 + 0.4 ** 2) ** 0.5
        assert _build(lib, abi, h, tilted, 0.5 * d_x * (1 + 1e-9)) == -1
        assert _build(lib, abi, h, tilted, 4.99) == -1                   # below L / 2, above d_x / 2
        # positions missing although particles are announced; half list with ghosts
        assert _build(lib, abi, h, box, 1.0, n_local=4) == -1
        assert _build(lib, abi, h, box, 1.0, n_local=4, n_ghost=2, half=1) == -2
        # the check: bad arguments, and "rebuild" without device work as long as nothing was built
        needs = C.c_int(-5)
        assert lib.mtd_nlist_check(None, None, 1, C.byref(box), 0.4, C.byref(needs), None) == -1
        assert lib.mtd_nlist_check(h, None, 9, C.byref(box), 0.4, C.byref(needs), None) == -1
        assert lib.mtd_nlist_check(h, None, 1, C.byref(box), -0.1, C.byref(needs), None) == -1
        assert lib.mtd_nlist_check(h, None, 1, C.byref(box), 0.4, C.byref(needs), None) == 0 and needs.value == 1
        dim = (C.c_uint * 3)()
        assert lib.mtd_nlist_cells(h, dim) == -1                         # nothing built yet
    finally:
        assert lib.mtd_nlist_destroy(h) == 0


def test_nlist_cell_keywords_and_host_methods():
    """cv.nlist_cell(r_cut, r_buff=0.4, check_period=1, device=False); NeighborList gained the device-build methods"""
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.nlist_cell.__init__).parameters.items() if n != "self"]
    assert params == [("r_cut", E), ("r_buff", 0.4), ("check_period", 1), ("device", False)]
    for meth in ("setDeviceBuild", "forceRebuild", "getNumRebuilds", "getVersion", "getLists", "isDeviceBuild",
                 "setLists", "setStorageMode", "getStorageMode", "compute"):
        assert hasattr(mod.NeighborList, meth), meth
    for meth in ("update", "set_lists"):
        assert hasattr(cv.nlist_cell, meth), meth
