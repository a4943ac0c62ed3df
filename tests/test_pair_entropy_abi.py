"""CPU: the pair entropy (mtd_pe_*, csrc/pair_entropy.hip) is exported, declared and registered, refuses bad arguments before it touches
a device, and is reachable from the host classes and the Python API.  Nothing here needs a GPU."""
import ctypes as C
import inspect

PE_SYMBOLS = ("mtd_pe_scratch_doubles", "mtd_pe_accumulate", "mtd_pe_finalize", "mtd_pe_forces")
INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in PE_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    assert abi._SIGNATURES["mtd_pe_forces"][1][-2:] == [C.c_void_p, C.c_uint]      # void *d_virial, unsigned int virial_pitch


def test_scratch_size(abi):
    lib = abi.load()
    for b in (1, 40, 256):
        n = lib.mtd_pe_scratch_doubles(b)
        assert n >= 3 * b + 4 and n * 8 < 4 * 2 ** 20       # sums, g_b, W_b, the value; a few MB at most whatever the particle number
        assert n % 2 == 0


def _acc(lib, abi, box, n=4, pos=1, head=1, nn=1, dtype=1, r_max=2.0, sigma_r=0.1, n_bins=40, scratch=4096, out=True):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    sums, n_sums = C.c_void_p(), C.c_uint()
    return lib.mtd_pe_accumulate(n, pos * 4096 or None, dtype, C.byref(box) if box is not None else None, head * 4096 or None, nn * 4096 or None,
                                 4096, r_max, sigma_r, n_bins, 0, scratch or None, C.byref(sums) if out else None,
                                 C.byref(n_sums) if out else None, None)


def _fin(lib, abi, box, r_max=2.0, sigma_r=0.1, n_bins=40, scratch=4096, out=True, **_):
    value, g = C.c_void_p(), C.c_void_p()
    return lib.mtd_pe_finalize(C.byref(box) if box is not None else None, r_max, sigma_r, n_bins, scratch or None,
                               C.byref(value) if out else None, C.byref(g), None)


def _frc(lib, abi, box, n=4, pos=1, force=1, head=1, nn=1, dtype=1, r_max=2.0, sigma_r=0.1, n_bins=40, scratch=4096, virial=0, pitch=0):
    return lib.mtd_pe_forces(n, pos * 4096 or None, force * 4096 or None, dtype, C.byref(box) if box is not None else None, head * 4096 or None,
                             nn * 4096 or None, 4096, r_max, sigma_r, n_bins, 0, scratch or None, None, 0.5, None, virial * 4096 or None, pitch)


SHARED = [dict(scratch=0), dict(scratch=4096 + 8), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan")), dict(r_max=float("inf")),
          dict(sigma_r=0.0), dict(sigma_r=-0.1), dict(sigma_r=float("nan")), dict(sigma_r=float("inf")), dict(n_bins=0)]
PARTICLES = [dict(pos=0), dict(head=0), dict(nn=0), dict(dtype=7)]


def test_argument_validation_without_gpu(abi):
    """null pointers, non-finite or non-positive r_max / sigma_r, n_bins = 0, a bad dtype, a misaligned scratch: MTD_ERR_INVALID_ARGUMENT;
    n_bins > 256: MTD_ERR_UNSUPPORTED — all before any device call (this test runs on a machine without a GPU)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _fin, _frc):
        assert call(lib, abi, None) == INVALID
        for kw in SHARED:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
        assert call(lib, abi, box, n_bins=257) == UNSUPPORTED
        assert call(lib, abi, box, n_bins=100000) == UNSUPPORTED
    for call in (_acc, _frc):
        for kw in PARTICLES:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _fin(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID
    assert _frc(lib, abi, box, virial=1, pitch=3) == INVALID            # a virial pitch below the particle count
    flat = abi.Box.make([10.0, 0.0, 10.0])
    assert _fin(lib, abi, flat) == INVALID                               # no volume


def test_no_particles_is_success_in_the_force_pass(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _frc(lib, abi, box, n=0) == SUCCESS
    assert _frc(lib, abi, box, n=0, pos=0, force=0, head=0, nn=0) == SUCCESS
    assert _frc(lib, abi, box, n=0, virial=1, pitch=0) == SUCCESS


def test_python_and_pybind_surface():
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.pair_entropy.__init__).parameters.items() if n != "self"]
    assert params == [("r_max", E), ("sigma_r", E), ("n_bins", E), ("nlist", E), ("type", E), ("name", None), ("sigma", 1.0)]
    assert issubclass(cv.pair_entropy, cv._collective_variable)
    for meth in ("get_rcut", "get_gr", "get_virial", "set_grid", "set_params"):
        assert hasattr(cv.pair_entropy, meth), meth
    assert issubclass(mod.PairEntropy, mod.CollectiveVariable)
    for meth in ("getGr", "getVirial", "getCurrentValue", "getForceArray", "getLogValue", "getProvidedLogQuantities", "getRCut"):
        assert hasattr(mod.PairEntropy, meth), meth
