"""CPU: the local pair entropy (mtd_pel_*, csrc/pair_entropy_local.hip) is exported, declared and registered, its two structures have the
header's layout, it refuses bad arguments before it touches a device, and it is reachable from the host classes and the Python API.
Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re

PEL_SYMBOLS = ("mtd_pel_scratch_doubles", "mtd_pel_accumulate", "mtd_pel_forces")
INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in PEL_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    assert abi._SIGNATURES["mtd_pel_forces"][1][-2:] == [C.c_void_p, C.c_uint]     # void *d_virial, unsigned int virial_pitch
    assert abi.MTD_PEL_MAX_BINS == 128


def _header_fields(name):
    """[(C type, field)] of `typedef struct { ... } name;` in include/mtd_abi.h, comments removed, `a, b` declarations split"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*%s\s*;" % name, text).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *rest = [x.strip() for x in decl.split(",")]
        ctype, field = first.rsplit(" ", 1)
        for f in [field] + rest:
            stars = f.count("*")
            out.append((ctype + " *" * bool(stars), f.replace("*", "").strip()))
    return out


def test_struct_layouts_match_header(abi):
    """the ctypes mirrors field by field against the header's field list: names, order, and a type of the same size and kind"""
    kinds = {"double": C.c_double, "unsigned int": C.c_uint, "int": C.c_int, "mtd_stream_t": C.c_void_p}
    for name, mirror in (("mtd_pel_params", abi.PelParams), ("mtd_pel_call", abi.PelCall)):
        fields = _header_fields(name)
        assert [f for _, f in fields] == [f for f, _ in mirror._fields_], name
        for (ctype, field), (_, mtype) in zip(fields, mirror._fields_):
            want = C.c_void_p if ctype.endswith("*") else kinds[ctype]
            assert C.sizeof(mtype) == C.sizeof(want), (name, field)
            assert issubclass(mtype, C._Pointer) or mtype is want, (name, field)
    assert C.sizeof(abi.PelParams) == 2 * 8 + 2 * 4 + (4 + 4) + 2 * 8 + (4 + 4) + 8 + (4 + 4)       # (ints padded to the next double)
    assert C.sizeof(abi.PelCall) == 2 * 4 + 8 + (4 + 4) + 6 * 8
    assert abi.PelParams.a_on.offset == 32 and abi.PelParams.c0.offset == 56 and abi.PelCall.box.offset == 24


def test_scratch_size(abi):
    lib = abi.load()
    for n, b in ((0, 1), (1, 1), (500, 40), (37044, 128)):
        d = lib.mtd_pel_scratch_doubles(n, b)
        assert d >= n * b + 6 * n + 2 * 1024 and d <= n * b + 6 * (n + 1) + 2 * 1024


def _call(abi, box, n=4, n_global=4, pos=1, head=1, nn=1, dtype=1, scratch=4096, **_):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    return abi.PelCall(n, n_global, pos * 4096 or None, dtype, C.pointer(box) if box is not None else None, head * 4096 or None,
                       nn * 4096 or None, 4096, scratch or None, None)


def _par(abi, r_max=2.0, sigma_r=0.1, n_bins=40, average=None, switch=None, **_):
    return abi.PelParams.make(r_max, sigma_r, n_bins, 0, average=average, switch=switch)


def _acc(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    part, n_part, s = C.c_void_p(), C.c_uint(), C.c_void_p()
    return lib.mtd_pel_accumulate(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(part) if out else None,
                                  C.byref(n_part) if out else None, C.byref(s), None, None)


def _frc(lib, abi, box, force=1, virial=0, pitch=0, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    return lib.mtd_pel_forces(None if no_par else C.byref(par), None if no_call else C.byref(call), force * 4096 or None, None, 0.5,
                              virial * 4096 or None, pitch)


SHARED = [dict(scratch=0), dict(scratch=4096 + 8), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan")), dict(r_max=float("inf")),
          dict(sigma_r=0.0), dict(sigma_r=-0.1), dict(sigma_r=float("nan")), dict(sigma_r=float("inf")), dict(n_bins=0),
          dict(pos=0), dict(head=0), dict(nn=0), dict(dtype=7), dict(n_global=0), dict(no_par=True), dict(no_call=True),
          dict(average=(1.5, 1.2)), dict(average=(1.2, 1.2)), dict(average=(-0.1, 1.2)), dict(average=(1.2, 2.4 + 1e-9)),
          dict(average=(float("nan"), 1.2)), dict(average=(1.2, float("nan"))), dict(average=(1.2, float("inf"))),
          dict(switch=(0.0, 6)), dict(switch=(-1.0, 6)), dict(switch=(float("nan"), 6)), dict(switch=(float("inf"), 6)), dict(switch=(1.0, 0))]


def test_argument_validation_without_gpu(abi):
    """null pointers, non-finite or non-positive r_max / sigma_r, n_bins = 0, a bad dtype, a misaligned scratch, a bad average window or
    switch, n_global = 0: MTD_ERR_INVALID_ARGUMENT; n_bins > 128: MTD_ERR_UNSUPPORTED — all before any device call (this test runs on
    a machine without a GPU)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _frc):
        assert call(lib, abi, None) == INVALID
        for kw in SHARED:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
        assert call(lib, abi, box, n_bins=129) == UNSUPPORTED
        assert call(lib, abi, box, n_bins=100000) == UNSUPPORTED
        assert call(lib, abi, box, n_bins=129, scratch=4096 + 8) == INVALID       # an invalid argument beside the unsupported one
        assert call(lib, abi, abi.Box.make([10.0, 0.0, 10.0])) == INVALID          # no volume
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID
    assert _frc(lib, abi, box, virial=1, pitch=3) == INVALID                       # a virial pitch below the particle count


def test_no_particles_is_success_in_the_force_pass(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _frc(lib, abi, box, n=0) == SUCCESS
    assert _frc(lib, abi, box, n=0, pos=0, force=0, head=0, nn=0) == SUCCESS
    assert _frc(lib, abi, box, n=0, virial=1, pitch=0) == SUCCESS
    assert _frc(lib, abi, box, n=0, average=(1.2, 1.5), switch=(3.0, 6)) == SUCCESS


def test_python_and_pybind_surface():
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.pair_entropy_local.__init__).parameters.items() if n != "self"]
    assert params == [("r_max", E), ("sigma_r", E), ("n_bins", E), ("nlist", E), ("type", E), ("average", None), ("switch", None),
                      ("name", None), ("sigma", 1.0)]
    assert type(cv.pair_entropy_local) is type                                      # no metaclass: help() and inspect show the options
    assert issubclass(cv.pair_entropy_local, cv._neighbour_variable)
    assert [n for n in inspect.signature(cv.pair_entropy_local.set_options).parameters] == ["self", "average", "switch"]
    for meth in ("get_rcut", "get_virial", "get_local", "get_averaged", "get_switched", "set_options", "set_grid", "set_params"):
        assert hasattr(cv.pair_entropy_local, meth), meth
    assert issubclass(mod.PairEntropyLocal, mod.CollectiveVariable)
    for meth in ("getLocalValues", "getAveragedValues", "getSwitchedValues", "setAverage", "clearAverage", "setSwitch", "clearSwitch", "getVirial",
                 "getCurrentValue", "getForceArray", "getLogValue", "getProvidedLogQuantities", "getRCut"):
        assert hasattr(mod.PairEntropyLocal, meth), meth
