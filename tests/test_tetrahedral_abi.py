"""CPU: the tetrahedral order (mtd_tet_*, csrc/tetrahedral.hip) is exported, declared and registered, its two structures have the
header's layout, it refuses bad arguments before it touches a device, and it is reachable from the host classes and the Python API.
Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re

TET_SYMBOLS = ("mtd_tet_scratch_doubles", "mtd_tet_accumulate", "mtd_tet_finalize", "mtd_tet_forces")
INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0
NAN, INF = float("nan"), float("inf")


def _header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in TET_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    assert abi._SIGNATURES["mtd_tet_forces"][1][-2:] == [C.c_void_p, C.c_uint]     # void *d_virial, unsigned int virial_pitch
    text = _header()
    assert float(re.search(r"#define MTD_TET_W_MIN (\S+)", text).group(1)) == abi.MTD_TET_W_MIN == 1e-12
    # the stream travels inside mtd_tet_call: no entry point of the unit takes a bare one (tests/test_stream_gate.py counts those)
    found = 0
    for m in re.finditer(r"\b(mtd_tet_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        assert "mtd_stream_t" not in m.group(2), m.group(1)
        found += 1
    assert found == len(TET_SYMBOLS)


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
    for name, mirror in (("mtd_tet_params", abi.TetParams), ("mtd_tet_call", abi.TetCall)):
        fields = _header_fields(name)
        assert [f for _, f in fields] == [f for f, _ in mirror._fields_], name
        for (ctype, field), (_, mtype) in zip(fields, mirror._fields_):
            want = C.c_void_p if ctype.endswith("*") else kinds[ctype]
            assert C.sizeof(mtype) == C.sizeof(want), (name, field)
            assert issubclass(mtype, C._Pointer) or mtype is want, (name, field)
    # type (+ pad) | r_cut | r_on | cos0 | normalise, switch_on | c0 | p, gate_on | n_lo | n_hi
    assert C.sizeof(abi.TetParams) == 9 * 8
    assert abi.TetParams.r_cut.offset == 8 and abi.TetParams.cos0.offset == 24 and abi.TetParams.normalise.offset == 32
    assert abi.TetParams.switch_on.offset == 36 and abi.TetParams.c0.offset == 40 and abi.TetParams.p.offset == 48
    assert abi.TetParams.gate_on.offset == 52 and abi.TetParams.n_lo.offset == 56 and abi.TetParams.n_hi.offset == 64
    assert abi.TetCall is abi.RowCall and abi.TetCall.stream.offset == 64
    p = abi.TetParams.make(1, 1.3, 0.9)
    assert (p.type, p.r_cut, p.r_on, p.cos0, p.normalise, p.switch_on, p.gate_on) == (1, 1.3, 0.9, -1.0 / 3.0, 1, 0, 0)
    p = abi.TetParams.make(0, 1.3, 0.9, cos0=0.0, normalise=False, switch=(0.5, 6), gate=(1.0, 3.0))
    assert (p.cos0, p.normalise, p.switch_on, p.c0, p.p, p.gate_on, p.n_lo, p.n_hi) == (0.0, 0, 1, 0.5, 6, 1, 1.0, 3.0)


def test_scratch_size(abi):
    """sums, value and two rows of block sums; per particle n_i, t_i, v_i and the twelve doubles of the adjoint row, every part 16-byte
    aligned"""
    lib = abi.load()
    base = lib.mtd_tet_scratch_doubles(0)
    assert base >= 2 * 1024 + 4 and base % 2 == 0
    for n in (1, 2, 500, 37044):
        d = lib.mtd_tet_scratch_doubles(n)
        assert d == base + 15 * (n + n % 2)


def _call(abi, box, n_particles=4, n_ghost=0, pos=1, head=1, nn=1, dtype=1, scratch=4096, **_):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    return abi.TetCall(n_particles, n_ghost, pos * 4096 or None, dtype, C.pointer(box) if box is not None else None, head * 4096 or None,
                       nn * 4096 or None, 4096, scratch or None, None)


def _par(abi, r_cut=1.3, r_on=0.9, cos0=-1.0 / 3.0, normalise=True, switch=None, gate=None, **_):
    return abi.TetParams.make(0, r_cut, r_on, cos0=cos0, normalise=normalise, switch=switch, gate=gate)


def _acc(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    return lib.mtd_tet_accumulate(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(sums) if out else None,
                                  C.byref(n_sums) if out else None)


def _fin(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    v, l, s, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    return lib.mtd_tet_finalize(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(v) if out else None,
                                C.byref(l), C.byref(s), C.byref(n))


def _frc(lib, abi, box, force=1, virial=0, pitch=0, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    return lib.mtd_tet_forces(None if no_par else C.byref(par), None if no_call else C.byref(call), force * 4096 or None, None, 0.5,
                              virial * 4096 or None, pitch)


CALL = [dict(scratch=0), dict(scratch=4096 + 8), dict(no_call=True)]
ARRAYS = [dict(pos=0), dict(head=0), dict(nn=0), dict(dtype=7), dict(no_par=True)]
PARAMS = [dict(r_cut=0.0), dict(r_cut=-1.0), dict(r_cut=NAN), dict(r_cut=INF), dict(r_on=-0.1), dict(r_on=NAN), dict(r_on=1.3), dict(r_on=2.0),
          dict(cos0=-1.01), dict(cos0=1.01), dict(cos0=NAN), dict(cos0=INF),
          dict(switch=(0.0, 6)), dict(switch=(-1.0, 6)), dict(switch=(NAN, 6)), dict(switch=(INF, 6)), dict(switch=(0.5, 0)),
          dict(gate=(0.99, 3.0)), dict(gate=(0.0, 3.0)), dict(gate=(-1.0, 3.0)), dict(gate=(2.0, 2.0)), dict(gate=(3.0, 2.0)), dict(gate=(NAN, 3.0)),
          dict(gate=(1.0, NAN)), dict(gate=(1.0, INF)),
          dict(normalise=False, switch=(0.5, 6)), dict(normalise=False, gate=(1.0, 3.0)), dict(normalise=False, switch=(0.5, 6), gate=(1.0, 3.0))]
ACCEPTED = [dict(), dict(cos0=-1.0), dict(cos0=1.0), dict(cos0=0.0), dict(r_on=0.0), dict(normalise=False), dict(switch=(0.5, 6)),
            dict(gate=(1.0, 3.0)), dict(switch=(0.5, 1), gate=(1.0, 1.5))]


def test_argument_validation_without_gpu(abi):
    """null pointers, non-finite or out-of-range parameters, a switch or a gate without `normalise`, n_lo < 1, a bad dtype, a misaligned
    scratch, a pitch below n_particles: MTD_ERR_INVALID_ARGUMENT; ghosts: MTD_ERR_UNSUPPORTED — all before any device call (this test
    runs on a machine without a GPU)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _fin, _frc):
        assert call(lib, abi, None) == INVALID
        for kw in CALL + ARRAYS + PARAMS:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
        for kw in ACCEPTED:                                              # what is accepted gets as far as the ghosts
            assert call(lib, abi, box, n_ghost=3, **kw) == UNSUPPORTED, (call.__name__, kw)
        assert call(lib, abi, box, n_ghost=1) == UNSUPPORTED
        assert call(lib, abi, box, n_ghost=3, scratch=4096 + 8) == INVALID               # an invalid argument beside the unsupported one
        assert call(lib, abi, box, n_ghost=3, switch=(NAN, 6)) == INVALID
        assert call(lib, abi, box, n_ghost=3, normalise=False, gate=(1.0, 3.0)) == INVALID
        assert call(lib, abi, box, n_ghost=3, dtype=7) == INVALID
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _fin(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID
    assert _frc(lib, abi, box, virial=1, pitch=3) == INVALID                             # a virial pitch below the particle count


def test_no_particles_is_success_in_the_force_pass(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    for kw in ACCEPTED:
        assert _frc(lib, abi, box, n_particles=0, **kw) == SUCCESS
        assert _frc(lib, abi, box, n_particles=0, pos=0, force=0, head=0, nn=0, **kw) == SUCCESS
        assert _frc(lib, abi, box, n_particles=0, virial=1, pitch=0, **kw) == SUCCESS


def test_python_and_pybind_surface():
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.tetrahedral.__init__).parameters.items() if n != "self"]
    assert params == [("r_cut", E), ("r_on", E), ("nlist", E), ("type", E), ("cos0", -1.0 / 3.0), ("normalise", True), ("switch", None),
                      ("gate", None), ("name", None), ("sigma", 1.0)]
    assert [n for n in inspect.signature(cv.tetrahedral.set_options).parameters] == ["self", "switch", "gate"]
    assert issubclass(cv.tetrahedral, cv._neighbour_variable)
    for meth in ("get_rcut", "get_virial", "get_local", "get_switched", "get_coordination", "set_options", "set_grid", "set_params"):
        assert hasattr(cv.tetrahedral, meth), meth
    assert "gate" in cv.tetrahedral.__doc__ and "Dilute" in cv.tetrahedral.__doc__.replace("dilute", "Dilute")
    assert cv.tetrahedral._options(dict(c0=0.5, p=6), dict(n_lo=1, n_hi=3), True) == ((0.5, 6), (1.0, 3.0))
    assert cv.tetrahedral._options(None, None, False) == (None, None)
    assert issubclass(mod.TetrahedralOrder, mod.CollectiveVariable)
    for meth in ("getLocalValues", "getSwitchedValues", "getCoordination", "setSwitch", "clearSwitch", "setGate", "clearGate", "getVirial",
                 "getCurrentValue", "getForceArray", "getLogValue", "getProvidedLogQuantities", "getRCut"):
        assert hasattr(mod.TetrahedralOrder, meth), meth
