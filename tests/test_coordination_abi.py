"""CPU: the coordination number (mtd_coord_*, csrc/coordination.hip) is exported, declared and registered, its two structures have the
header's layout, it refuses bad arguments before it touches a device, and it is reachable from the host classes and the Python API.
Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re

COORD_SYMBOLS = ("mtd_coord_scratch_doubles", "mtd_coord_set_compiled_pair", "mtd_coord_accumulate", "mtd_coord_finalize", "mtd_coord_forces")
INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0
NAN, INF = float("nan"), float("inf")


def _header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in COORD_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    assert abi._SIGNATURES["mtd_coord_forces"][1][-2:] == [C.c_void_p, C.c_uint]   # void *d_virial, unsigned int virial_pitch
    text = _header()
    assert int(re.search(r"#define MTD_COORD_MAX_M (\d+)", text).group(1)) == abi.MTD_COORD_MAX_M == 32
    # the stream travels inside mtd_coord_call: no entry point of the unit takes a bare one (tests/test_stream_gate.py counts those)
    for m in re.finditer(r"\b(mtd_coord_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        assert "mtd_stream_t" not in m.group(2), m.group(1)


def _header_fields(name):
    """[(C type, field)] of `typedef struct { ... } name;` in include/mtd_abi.h, `a, b` declarations split; a name that is
    `typedef other name;` has the fields of `other`"""
    alias = re.search(r"typedef\s+(\w+)\s+%s\s*;" % name, _header())
    if alias:
        return _header_fields(alias.group(1))
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header()).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *rest = [x.strip() for x in decl.split(",")]
        ctype, field = first.rsplit(" ", 1)
        for f in [field] + rest:
            out.append((ctype + " *" * bool(f.count("*")), f.replace("*", "").strip()))
    return out


def test_struct_layouts_match_header(abi):
    """the ctypes mirrors field by field against the header's field list: names, order, and a type of the same size and kind"""
    kinds = {"double": C.c_double, "unsigned int": C.c_uint, "int": C.c_int, "mtd_stream_t": C.c_void_p}
    for name, mirror in (("mtd_coord_params", abi.CoordParams), ("mtd_coord_call", abi.CoordCall)):
        fields = _header_fields(name)
        assert [f for _, f in fields] == [f for f, _ in mirror._fields_], name
        for (ctype, field), (_, mtype) in zip(fields, mirror._fields_):
            want = C.c_void_p if ctype.endswith("*") else kinds[ctype]
            assert C.sizeof(mtype) == C.sizeof(want), (name, field)
            assert issubclass(mtype, C._Pointer) or mtype is want, (name, field)
    # type_a, type_b | r_0 | d_0 | n, m | r_cut | switch_on (+ pad) | c0 | p, less
    assert C.sizeof(abi.CoordParams) == 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8
    assert abi.CoordParams.r_0.offset == 8 and abi.CoordParams.n.offset == 24 and abi.CoordParams.r_cut.offset == 32
    assert abi.CoordParams.switch_on.offset == 40 and abi.CoordParams.c0.offset == 48 and abi.CoordParams.less.offset == 60
    assert [f for f, _ in abi.CoordCall._fields_] == [f for f, _ in abi.DsfCall._fields_]           # "the same fields as mtd_dsf_call"
    assert C.sizeof(abi.CoordCall) == C.sizeof(abi.DsfCall) and abi.CoordCall.stream.offset == 64


def test_scratch_size(abi):
    lib = abi.load()
    base = lib.mtd_coord_scratch_doubles(0)
    assert base >= 2 * 1024 + 4
    for n in (1, 2, 500, 37044):
        d = lib.mtd_coord_scratch_doubles(n)
        assert base + 12 * n <= d <= base + 12 * (n + 1)


def _call(abi, box, n_particles=4, n_ghost=0, pos=1, head=1, nn=1, dtype=1, scratch=4096, **_):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    return abi.CoordCall(n_particles, n_ghost, pos * 4096 or None, dtype, C.pointer(box) if box is not None else None, head * 4096 or None,
                         nn * 4096 or None, 4096, scratch or None, None)


def _par(abi, r_0=1.15, r_cut=2.0, d_0=0.0, n=6, m=12, switch=None, **_):
    return abi.CoordParams.make(0, 1, r_0, r_cut, d_0=d_0, n=n, m=m, switch=switch)


def _acc(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    return lib.mtd_coord_accumulate(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(sums) if out else None,
                                    C.byref(n_sums) if out else None)


def _fin(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    v, l, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
    return lib.mtd_coord_finalize(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(v) if out else None,
                                  C.byref(l), C.byref(s))


def _frc(lib, abi, box, force=1, virial=0, pitch=0, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    return lib.mtd_coord_forces(None if no_par else C.byref(par), None if no_call else C.byref(call), force * 4096 or None, None, 0.5,
                                virial * 4096 or None, pitch)


CALL = [dict(scratch=0), dict(scratch=4096 + 8), dict(no_call=True)]
ARRAYS = [dict(pos=0), dict(head=0), dict(nn=0), dict(dtype=7), dict(no_par=True)]
PARAMS = [dict(r_0=0.0), dict(r_0=-1.0), dict(r_0=NAN), dict(r_0=INF), dict(d_0=-0.1), dict(d_0=NAN), dict(d_0=INF), dict(r_cut=0.0),
          dict(r_cut=NAN), dict(r_cut=INF), dict(d_0=2.0), dict(d_0=2.5), dict(n=0), dict(n=12), dict(n=13), dict(n=6, m=6), dict(n=40, m=33),
          dict(switch=(0.0, 8)), dict(switch=(-1.0, 8)), dict(switch=(NAN, 8)), dict(switch=(INF, 8)), dict(switch=(5.0, 0))]


def test_argument_validation_without_gpu(abi):
    """null pointers, non-finite or out-of-range parameters, a bad dtype, a misaligned scratch, a pitch below n_particles:
    MTD_ERR_INVALID_ARGUMENT; m > 32 and a switch with ghosts: MTD_ERR_UNSUPPORTED — all before any device call (this test runs on a
    machine without a GPU)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _fin, _frc):
        assert call(lib, abi, None) == INVALID
        for kw in CALL + ARRAYS + PARAMS:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
        assert call(lib, abi, box, n=6, m=33) == UNSUPPORTED
        assert call(lib, abi, box, n=32, m=100000) == UNSUPPORTED
        assert call(lib, abi, box, switch=(5.0, 8), n_ghost=3) == UNSUPPORTED
        assert call(lib, abi, box, switch=(5.0, 8, 1), n_ghost=1) == UNSUPPORTED
        assert call(lib, abi, box, n=6, m=33, scratch=4096 + 8) == INVALID              # an invalid argument beside the unsupported one
        assert call(lib, abi, box, switch=(NAN, 8), n_ghost=3) == INVALID
        assert call(lib, abi, box, n=6, m=33, r_0=NAN) == INVALID
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _fin(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID
    assert _frc(lib, abi, box, virial=1, pitch=3) == INVALID                            # a virial pitch below the particle count


def test_no_particles_is_success_in_the_force_pass(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    for switch in (None, (5.0, 8)):
        assert _frc(lib, abi, box, n_particles=0, switch=switch) == SUCCESS
        assert _frc(lib, abi, box, n_particles=0, pos=0, force=0, head=0, nn=0, switch=switch) == SUCCESS
        assert _frc(lib, abi, box, n_particles=0, virial=1, pitch=0, switch=switch) == SUCCESS
    assert lib.mtd_coord_set_compiled_pair(0) == SUCCESS
    assert _frc(lib, abi, box, n_particles=0) == SUCCESS
    assert lib.mtd_coord_set_compiled_pair(1) == SUCCESS


def test_python_and_pybind_surface():
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.coordination.__init__).parameters.items() if n != "self"]
    assert params == [("r_0", E), ("nlist", E), ("type", E), ("partner", None), ("d_0", 0.0), ("n", 6), ("m", 12), ("r_cut", None),
                      ("switch", None), ("name", None), ("sigma", 1.0)]
    assert issubclass(cv.coordination, cv._neighbour_variable)
    for meth in ("get_rcut", "get_virial", "get_local", "get_switched", "set_switch", "set_grid", "set_params"):
        assert hasattr(cv.coordination, meth), meth
    assert "discontinuous" in cv.coordination.__doc__
    assert cv.coordination._switch(dict(c0=5, p=8)) == (5.0, 8, False) and cv.coordination._switch(dict(c0=5, p=8, less=True)) == (5.0, 8, True)
    assert issubclass(mod.CoordinationNumber, mod.CollectiveVariable)
    for meth in ("getLocalValues", "getSwitchedValues", "setSwitch", "clearSwitch", "getVirial", "getCurrentValue", "getForceArray",
                 "getLogValue", "getProvidedLogQuantities", "getRCut"):
        assert hasattr(mod.CoordinationNumber, meth), meth
