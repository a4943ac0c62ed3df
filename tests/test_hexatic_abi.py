"""CPU: the bond-orientational order (mtd_hex_*, csrc/hexatic.hip) is exported, declared and registered, its two structures have the
header's layout, it refuses bad arguments before it touches a device, and it is reachable from the host classes and the Python API.
Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re

HEX_SYMBOLS = ("mtd_hex_scratch_doubles", "mtd_hex_accumulate", "mtd_hex_finalize", "mtd_hex_forces")
INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0
NAN, INF = float("nan"), float("inf")


def _header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in HEX_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    assert abi._SIGNATURES["mtd_hex_forces"][1][-2:] == [C.c_void_p, C.c_uint]     # void *d_virial, unsigned int virial_pitch
    assert len(abi._SIGNATURES["mtd_hex_finalize"][1]) == 7                         # value, c_i, v_i, n_i, psi_i
    text = _header()
    assert float(re.search(r"#define MTD_HEX_N_MIN (\S+)", text).group(1)) == abi.MTD_HEX_N_MIN == 1e-12
    assert int(re.search(r"#define MTD_HEX_MAX_K (\S+)", text).group(1)) == abi.MTD_HEX_MAX_K == 12
    # the stream travels inside mtd_hex_call: no entry point of the unit takes a bare one (tests/test_stream_gate.py counts those)
    found = 0
    for m in re.finditer(r"\b(mtd_hex_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        assert "mtd_stream_t" not in m.group(2), m.group(1)
        found += 1
    assert found == len(HEX_SYMBOLS)


def test_header_states_the_definition():
    """the block sits between "Tetrahedral order" and the next unit, says that the sectoral form IS the definition and that |psi_i| < 1
    on a rippled layer is intended"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    tet, hexa, bragg = text.index("* Tetrahedral order (cv.tetrahedral)"), text.index("* Bond-orientational order (cv.hexatic)"), \
        text.index("* Bragg intensity (cv.bragg)")
    assert tet < hexa < bragg
    block = " ".join(text[hexa:bragg].split())
    assert "THIS IS THE DEFINITION" in block and "sectoral harmonic" in block
    assert "|psi_i| < 1 on a rippled but perfect layer is therefore INTENDED" in block


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
    for name, mirror in (("mtd_hex_params", abi.HexParams), ("mtd_hex_call", abi.HexCall)):
        fields = _header_fields(name)
        assert [f for _, f in fields] == [f for f, _ in mirror._fields_], name
        for (ctype, field), (_, mtype) in zip(fields, mirror._fields_):
            want = C.c_void_p if ctype.endswith("*") else kinds[ctype]
            assert C.sizeof(mtype) == C.sizeof(want), (name, field)
            assert issubclass(mtype, C._Pointer) or mtype is want, (name, field)
    assert [f for f, _ in abi.HexParams._fields_] == ["type", "k", "axis", "r_cut", "r_on", "global_order", "switch_on", "c0", "p", "gate_on",
                                                      "n_lo", "n_hi"]
    # type, k | axis (+ pad) | r_cut | r_on | global_order, switch_on | c0 | p, gate_on | n_lo | n_hi
    assert C.sizeof(abi.HexParams) == 9 * 8
    assert abi.HexParams.k.offset == 4 and abi.HexParams.axis.offset == 8 and abi.HexParams.r_cut.offset == 16 and abi.HexParams.r_on.offset == 24
    assert abi.HexParams.global_order.offset == 32 and abi.HexParams.switch_on.offset == 36 and abi.HexParams.c0.offset == 40
    assert abi.HexParams.p.offset == 48 and abi.HexParams.gate_on.offset == 52 and abi.HexParams.n_lo.offset == 56 and abi.HexParams.n_hi.offset == 64
    assert abi.HexCall is abi.RowCall and abi.HexCall.stream.offset == 64
    p = abi.HexParams.make(1, 1.3, 0.9)
    assert (p.type, p.k, p.axis, p.r_cut, p.r_on, p.global_order, p.switch_on, p.gate_on) == (1, 6, 2, 1.3, 0.9, 0, 0, 0)
    p = abi.HexParams.make(0, 1.3, 0.9, k=4, axis=0, switch=(0.5, 6), gate=(0.0, 3.0))
    assert (p.k, p.axis, p.switch_on, p.c0, p.p, p.gate_on, p.n_lo, p.n_hi) == (4, 0, 1, 0.5, 6, 1, 0.0, 3.0)
    assert abi.HexParams.make(0, 1.3, 0.9, global_order=True).global_order == 1


def test_scratch_size(abi):
    """sums, value and four rows of block sums; per particle n_i, c_i, v_i, the two doubles of psi_i and the four of the adjoint row,
    every part 16-byte aligned"""
    lib = abi.load()
    base = lib.mtd_hex_scratch_doubles(0)
    assert base >= 4 * 1024 + 8 and base % 2 == 0
    for n in (1, 2, 500, 33124):
        d = lib.mtd_hex_scratch_doubles(n)
        assert d == base + 9 * (n + n % 2)


def _call(abi, box, n_particles=4, n_ghost=0, pos=1, head=1, nn=1, dtype=1, scratch=4096, **_):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    return abi.HexCall(n_particles, n_ghost, pos * 4096 or None, dtype, C.pointer(box) if box is not None else None, head * 4096 or None,
                       nn * 4096 or None, 4096, scratch or None, None)


def _par(abi, r_cut=1.3, r_on=0.9, k=6, axis=2, global_order=False, switch=None, gate=None, **_):
    return abi.HexParams.make(0, r_cut, r_on, k=k, axis=axis, global_order=global_order, switch=switch, gate=gate)


def _acc(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    return lib.mtd_hex_accumulate(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(sums) if out else None,
                                  C.byref(n_sums) if out else None)


def _fin(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    v, l, s, n, psi = (C.c_void_p() for _ in range(5))
    return lib.mtd_hex_finalize(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(v) if out else None,
                                C.byref(l), C.byref(s), C.byref(n), C.byref(psi))


def _frc(lib, abi, box, force=1, virial=0, pitch=0, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    return lib.mtd_hex_forces(None if no_par else C.byref(par), None if no_call else C.byref(call), force * 4096 or None, None, 0.5,
                              virial * 4096 or None, pitch)


CALL = [dict(scratch=0), dict(scratch=4096 + 8), dict(no_call=True)]
ARRAYS = [dict(pos=0), dict(head=0), dict(nn=0), dict(dtype=7), dict(no_par=True)]
PARAMS = [dict(r_cut=0.0), dict(r_cut=-1.0), dict(r_cut=NAN), dict(r_cut=INF), dict(r_on=-0.1), dict(r_on=NAN), dict(r_on=1.3), dict(r_on=2.0),
          dict(k=0), dict(axis=3), dict(axis=7),
          dict(switch=(0.0, 6)), dict(switch=(-1.0, 6)), dict(switch=(NAN, 6)), dict(switch=(INF, 6)), dict(switch=(0.5, 0)),
          dict(gate=(-0.01, 3.0)), dict(gate=(-1.0, 3.0)), dict(gate=(2.0, 2.0)), dict(gate=(3.0, 2.0)), dict(gate=(NAN, 3.0)),
          dict(gate=(1.0, NAN)), dict(gate=(1.0, INF)),
          dict(global_order=True, switch=(NAN, 6)), dict(global_order=True, gate=(3.0, 2.0)), dict(k=13, axis=3), dict(k=13, r_on=NAN)]
NOT_BUILT = [dict(k=13), dict(k=1000), dict(global_order=True, switch=(0.5, 6)), dict(global_order=True, gate=(1.0, 3.0)),
             dict(global_order=True, switch=(0.5, 6), gate=(0.0, 3.0))]
ACCEPTED = [dict(), dict(k=1), dict(k=12), dict(axis=0), dict(axis=1), dict(r_on=0.0), dict(global_order=True), dict(switch=(0.5, 6)),
            dict(gate=(0.0, 3.0)), dict(switch=(0.5, 1), gate=(1.0, 1.5)), dict(k=4, axis=0, global_order=True)]


def test_argument_validation_without_gpu(abi):
    """null pointers, a non-finite or out-of-range window, k = 0, axis > 2, a bad switch or gate, a bad dtype, a misaligned scratch, a
    pitch below n_particles: MTD_ERR_INVALID_ARGUMENT; k > MTD_HEX_MAX_K, a switch or a gate with global_order, ghosts:
    MTD_ERR_UNSUPPORTED — all with device pointers that cannot be dereferenced and before any device call (this test runs on a
    machine without a GPU)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _fin, _frc):
        assert call(lib, abi, None) == INVALID
        for kw in CALL + ARRAYS + PARAMS:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
        for kw in NOT_BUILT:
            assert call(lib, abi, box, **kw) == UNSUPPORTED, (call.__name__, kw)
            assert call(lib, abi, box, scratch=4096 + 8, **kw) == INVALID, (call.__name__, kw)   # an invalid argument beside it
        for kw in ACCEPTED:                                              # what is accepted gets as far as the ghosts
            assert call(lib, abi, box, n_ghost=3, **kw) == UNSUPPORTED, (call.__name__, kw)
        assert call(lib, abi, box, n_ghost=1) == UNSUPPORTED
        assert call(lib, abi, box, n_ghost=3, scratch=4096 + 8) == INVALID               # an invalid argument beside the unsupported one
        assert call(lib, abi, box, n_ghost=3, switch=(NAN, 6)) == INVALID
        assert call(lib, abi, box, n_ghost=3, k=0) == INVALID
        assert call(lib, abi, box, n_ghost=3, dtype=7) == INVALID
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _fin(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID
    assert _frc(lib, abi, box, virial=1, pitch=3) == INVALID                             # a virial pitch below the particle count
    assert _frc(lib, abi, box, virial=1, pitch=3, n_ghost=2) == INVALID
    assert _frc(lib, abi, box, force=0, k=13) == INVALID


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
    params = [(n, p.default) for n, p in inspect.signature(cv.hexatic.__init__).parameters.items() if n != "self"]
    assert params == [("r_cut", E), ("r_on", E), ("nlist", E), ("type", E), ("k", 6), ("axis", "z"), ("global_order", False), ("switch", None),
                      ("gate", None), ("name", None), ("sigma", 1.0)]
    assert [n for n in inspect.signature(cv.hexatic.set_options).parameters] == ["self", "switch", "gate"]
    assert issubclass(cv.hexatic, cv._neighbour_variable)
    for meth in ("get_rcut", "get_virial", "get_local", "get_switched", "get_coordination", "get_psi", "get_global_psi", "set_options",
                 "set_grid", "set_params"):
        assert hasattr(cv.hexatic, meth), meth
    doc = " ".join(cv.hexatic.__doc__.split())
    for word in ("sectoral", "layer normal", "gate", "steep", "single-domain"):
        assert word in doc.lower(), word
    assert cv.hexatic._options(dict(c0=0.5, p=6), dict(n_lo=0, n_hi=3), False) == ((0.5, 6), (0.0, 3.0))
    assert cv.hexatic._options(None, None, True) == (None, None)
    assert issubclass(mod.HexaticOrder, mod.CollectiveVariable)
    for meth in ("getLocalValues", "getSwitchedValues", "getCoordination", "getPsi", "getGlobalPsi", "setSwitch", "clearSwitch", "setGate",
                 "clearGate", "getVirial", "getCurrentValue", "getForceArray", "getLogValue", "getProvidedLogQuantities", "getRCut"):
        assert hasattr(mod.HexaticOrder, meth), meth
