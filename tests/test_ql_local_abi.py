"""CPU: the local Steinhardt variable (mtd_ql_local_*, csrc/steinhardt_local.hip) is exported and declared, validates its
arguments before it touches a device, and is reachable from the host classes and the Python API.  Nothing here needs a GPU."""
import ctypes as C
import inspect

import util

QL_LOCAL_SYMBOLS = ("mtd_ql_local_scratch_doubles", "mtd_ql_local_accumulate", "mtd_ql_local_forces")
INVALID, UNSUPPORTED = -1, -2


def test_ql_local_symbols_exported_and_declared(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in QL_LOCAL_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s


def test_ql_local_scratch_size(abi):
    lib = abi.load()
    # block sums + n_i + c_i + a table row of at most (lmax + 1)(lmax + 2) doubles per particle
    for n, lmax in ((0, 6), (1, 0), (108, 6), (256000, 6), (501, 12)):
        got = lib.mtd_ql_local_scratch_doubles(n, lmax)
        assert got >= 2 * n + n * (lmax + 1) * (lmax + 2)
        assert got <= 2 * n + n * (lmax + 1) * (lmax + 2) + 2048
    # config 5: degrees 4 and 6 use 13 of the 28 complex slots; the whole scratch stays below the 256 MiB Infinity Cache
    assert lib.mtd_ql_local_scratch_doubles(256000, 6) * 8 < 256 * 2 ** 20


def _acc(lib, abi, box, n=4, pos=1, head=1, nn=1, dtype=1, rcut=1.4, ron=1.2, lmax=6, ql=True, n_global=4, scratch=4096, out=True):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    partials, c, nv = C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_partials = C.c_uint()
    ql_ref = util.dbl_array([0, 0, 0, 0, 1, 0, 1] + [0] * 6) if ql else None
    return lib.mtd_ql_local_accumulate(n, pos * 4096 or None, dtype, C.byref(box) if box is not None else None, head * 4096 or None,
                                       nn * 4096 or None, 4096, rcut, ron, lmax, 0, ql_ref, n_global, scratch or None,
                                       C.byref(partials) if out else None, C.byref(n_partials) if out else None, C.byref(c), C.byref(nv), None)


def _frc(lib, abi, box, n=4, pos=1, force=1, head=1, nn=1, dtype=1, rcut=1.4, ron=1.2, lmax=6, ql=True, n_global=4, scratch=4096):
    ql_ref = util.dbl_array([0, 0, 0, 0, 1, 0, 1] + [0] * 6) if ql else None
    return lib.mtd_ql_local_forces(n, pos * 4096 or None, force * 4096 or None, dtype, C.byref(box) if box is not None else None,
                                   head * 4096 or None, nn * 4096 or None, 4096, rcut, ron, lmax, 0, ql_ref, n_global, scratch or None,
                                   None, 0.5, None)


def test_ql_local_argument_validation_without_gpu(abi):
    """null pointers, r_on > r_cut, r_cut <= 0, a bad dtype (MTD_ERR_INVALID_ARGUMENT) and lmax > 12 (MTD_ERR_UNSUPPORTED) are refused
    before any device call — this test runs on a machine without a GPU"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _frc):
        assert call(lib, abi, None) == INVALID
        assert call(lib, abi, box, pos=0) == INVALID
        assert call(lib, abi, box, head=0) == INVALID
        assert call(lib, abi, box, nn=0) == INVALID
        assert call(lib, abi, box, ql=False) == INVALID
        assert call(lib, abi, box, scratch=0) == INVALID
        assert call(lib, abi, box, scratch=4096 + 8) == INVALID           # not 16-byte aligned
        assert call(lib, abi, box, rcut=1.0, ron=1.2) == INVALID           # r_on > r_cut
        assert call(lib, abi, box, rcut=0.0, ron=0.0) == INVALID
        assert call(lib, abi, box, rcut=-1.0, ron=0.0) == INVALID
        assert call(lib, abi, box, rcut=float("nan")) == INVALID
        assert call(lib, abi, box, ron=-0.1) == INVALID
        assert call(lib, abi, box, dtype=7) == INVALID
        assert call(lib, abi, box, n_global=0) == INVALID
        assert call(lib, abi, box, lmax=13) == UNSUPPORTED
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID


def test_steinhardt_local_python_surface():
    """cv.steinhardt_local(r_cut, r_on, lmax, Ql_ref, nlist, type, name=None, sigma=1.0) with get_local / get_coordination; the host
    class with its accessors"""
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.steinhardt_local.__init__).parameters.items() if n != "self"]
    assert params == [("r_cut", E), ("r_on", E), ("lmax", E), ("Ql_ref", E), ("nlist", E), ("type", E), ("name", None), ("sigma", 1.0)]
    assert issubclass(cv.steinhardt_local, cv._collective_variable)
    for meth in ("get_local", "get_coordination", "get_rcut", "set_grid", "set_params"):
        assert hasattr(cv.steinhardt_local, meth), meth
    assert issubclass(mod.SteinhardtLocal, mod.CollectiveVariable)
    for meth in ("getLocalValues", "getCoordination", "getCurrentValue", "getForceArray", "getLogValue", "getProvidedLogQuantities"):
        assert hasattr(mod.SteinhardtLocal, meth), meth
