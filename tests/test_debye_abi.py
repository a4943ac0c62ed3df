"""CPU: the Debye structure factor (mtd_dsf_*, csrc/debye.hip) is exported, declared and registered, its two structures have the header's
layout, it refuses bad arguments before it touches a device, and it is reachable from the host classes and the Python API.  Nothing here
needs a GPU."""
import ctypes as C
import inspect
import os
import re

DSF_SYMBOLS = ("mtd_dsf_scratch_doubles", "mtd_dsf_set_store_gradient", "mtd_dsf_accumulate", "mtd_dsf_finalize", "mtd_dsf_forces",
               "mtd_dsf_spectrum", "mtd_dsf_spectrum_finalize")
INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0
NAN, INF = float("nan"), float("inf")


def _header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in DSF_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    assert abi._SIGNATURES["mtd_dsf_forces"][1][-2:] == [C.c_void_p, C.c_uint]     # void *d_virial, unsigned int virial_pitch
    text = _header()
    assert int(re.search(r"#define MTD_DSF_MAX_Q (\d+)", text).group(1)) == abi.MTD_DSF_MAX_Q == 8
    assert int(re.search(r"#define MTD_DSF_MAX_SPECTRUM (\d+)", text).group(1)) == abi.MTD_DSF_MAX_SPECTRUM == 256
    # the stream travels inside mtd_dsf_call: no entry point of the unit takes a bare one (tests/test_stream_gate.py counts those)
    for m in re.finditer(r"\b(mtd_dsf_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        assert "mtd_stream_t" not in m.group(2), m.group(1)


def _header_fields(name):
    """[(C type, field, array length)] of `typedef struct { ... } name;` in include/mtd_abi.h, `a, b` declarations split; a name that
    is `typedef other name;` has the fields of `other`"""
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
            arr = re.search(r"\[(\w+)\]", f)
            f = re.sub(r"\[\w+\]", "", f)
            out.append((ctype + " *" * bool(f.count("*")), f.replace("*", "").strip(), arr.group(1) if arr else None))
    return out


def test_struct_layouts_match_header(abi):
    """the ctypes mirrors field by field against the header's field list: names, order, and a type of the same size and kind"""
    kinds = {"double": C.c_double, "unsigned int": C.c_uint, "int": C.c_int, "mtd_stream_t": C.c_void_p}
    for name, mirror in (("mtd_dsf_params", abi.DsfParams), ("mtd_dsf_call", abi.DsfCall)):
        fields = _header_fields(name)
        assert [f for _, f, _ in fields] == [f for f, _ in mirror._fields_], name
        for (ctype, field, arr), (_, mtype) in zip(fields, mirror._fields_):
            want = C.c_void_p if ctype.endswith("*") else kinds[ctype]
            if arr:
                assert arr == "MTD_DSF_MAX_Q" and mtype._length_ == 8 and mtype._type_ is want, (name, field)
                continue
            assert C.sizeof(mtype) == C.sizeof(want), (name, field)
            assert issubclass(mtype, C._Pointer) or mtype is want, (name, field)
    assert C.sizeof(abi.DsfParams) == (4 + 4) + 8 + (4 + 4) + 2 * 8 * 8                 # (ints padded to the next double)
    assert abi.DsfParams.r_cut.offset == 8 and abi.DsfParams.q.offset == 24 and abi.DsfParams.c.offset == 24 + 64
    assert C.sizeof(abi.DsfCall) == 2 * 4 + 8 + (4 + 4) + 6 * 8
    assert abi.DsfCall.box.offset == 24 and abi.DsfCall.stream.offset == 64


def test_scratch_size(abi):
    lib = abi.load()
    base = lib.mtd_dsf_scratch_doubles(0)
    assert base >= (256 + 1) * 1024 + 2 * 258 + 16
    for n in (1, 2, 500, 37044):
        d = lib.mtd_dsf_scratch_doubles(n)
        assert base + 10 * n <= d <= base + 10 * (n + 1)


def _call(abi, box, n=4, n_ghost=0, pos=1, head=1, nn=1, dtype=1, scratch=4096, **_):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    return abi.DsfCall(n, n_ghost, pos * 4096 or None, dtype, C.pointer(box) if box is not None else None, head * 4096 or None,
                       nn * 4096 or None, 4096, scratch or None, None)


def _par(abi, r_cut=2.4, q=(7.7, 8.9), c=None, n_q=None, **_):
    return abi.DsfParams.make(0, r_cut, q, c=c, n_q=n_q)


def _acc(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    return lib.mtd_dsf_accumulate(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(sums) if out else None,
                                  C.byref(n_sums) if out else None)


def _fin(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    v, i, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
    return lib.mtd_dsf_finalize(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(v) if out else None,
                                C.byref(i) if out else None, C.byref(s))


def _frc(lib, abi, box, force=1, virial=0, pitch=0, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    return lib.mtd_dsf_forces(None if no_par else C.byref(par), None if no_call else C.byref(call), force * 4096 or None, None, 0.5,
                              virial * 4096 or None, pitch)


def _spc(lib, abi, box, q_min=2.0, q_max=12.0, m=64, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    return lib.mtd_dsf_spectrum(None if no_par else C.byref(par), None if no_call else C.byref(call), q_min, q_max, m,
                                C.byref(sums) if out else None, C.byref(n_sums) if out else None)


def _spf(lib, abi, box, q_min=2.0, q_max=12.0, m=64, out=True, no_call=False, **kw):
    call = _call(abi, box, **kw)
    spec = C.c_void_p()
    return lib.mtd_dsf_spectrum_finalize(None if no_call else C.byref(call), q_min, q_max, m, C.byref(spec) if out else None)


CALL = [dict(scratch=0), dict(scratch=4096 + 8), dict(no_call=True)]
ARRAYS = [dict(pos=0), dict(head=0), dict(nn=0), dict(dtype=7), dict(no_par=True), dict(r_cut=0.0), dict(r_cut=-1.0), dict(r_cut=NAN),
          dict(r_cut=INF)]
PEAKS = [dict(q=()), dict(q=(0.0,)), dict(q=(-1.0,)), dict(q=(NAN,)), dict(q=(INF,)), dict(q=(7.7, 0.0)), dict(q=(7.7,), c=(NAN,)),
         dict(q=(7.7,), c=(INF,)), dict(q=(7.7, 8.9), c=(1.0, -INF)), dict(q=(1.0,) * 8, c=(1.0,) * 7 + (NAN,))]
SPECTRUM = [dict(q_min=0.0), dict(q_min=-1.0), dict(q_min=NAN), dict(q_min=INF), dict(q_max=NAN), dict(q_max=INF), dict(q_min=3.0, q_max=2.0),
            dict(m=0)]


def test_argument_validation_without_gpu(abi):
    """null pointers, a non-finite or non-positive r_cut or Q, a non-finite weight, n_q = 0, a bad dtype, a misaligned scratch, a pitch
    below n_particles, q_min > q_max: MTD_ERR_INVALID_ARGUMENT; n_q above the two capacities: MTD_ERR_UNSUPPORTED — all before any
    device call (this test runs on a machine without a GPU)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _fin, _frc):
        assert call(lib, abi, None) == INVALID
        for kw in CALL + ARRAYS + PEAKS:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
        assert call(lib, abi, box, q=(1.0,) * 8, n_q=9) == UNSUPPORTED
        assert call(lib, abi, box, q=(1.0,) * 8, n_q=100000) == UNSUPPORTED
        assert call(lib, abi, box, q=(1.0,) * 8, n_q=9, scratch=4096 + 8) == INVALID     # an invalid argument beside the unsupported one
        assert call(lib, abi, box, q=(1.0,) * 7 + (NAN,), n_q=9) == INVALID
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _fin(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID
    assert _frc(lib, abi, box, virial=1, pitch=3) == INVALID                             # a virial pitch below the particle count
    assert _spc(lib, abi, None) == INVALID
    for kw in CALL + ARRAYS + SPECTRUM:
        assert _spc(lib, abi, box, **kw) == INVALID, kw
    for kw in CALL + SPECTRUM:
        assert _spf(lib, abi, box, **kw) == INVALID, kw
    for call in (_spc, _spf):
        assert call(lib, abi, box, out=False) == INVALID
        assert call(lib, abi, box, m=257) == UNSUPPORTED
        assert call(lib, abi, box, m=257, q_min=3.0, q_max=2.0) == INVALID
        assert call(lib, abi, box, m=257, scratch=4096 + 8) == INVALID


def test_no_particles_is_success_in_the_force_pass(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _frc(lib, abi, box, n=0) == SUCCESS
    assert _frc(lib, abi, box, n=0, pos=0, force=0, head=0, nn=0) == SUCCESS
    assert _frc(lib, abi, box, n=0, virial=1, pitch=0) == SUCCESS
    assert lib.mtd_dsf_set_store_gradient(0) == SUCCESS
    assert _frc(lib, abi, box, n=0) == SUCCESS
    assert lib.mtd_dsf_set_store_gradient(1) == SUCCESS


def test_python_and_pybind_surface():
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.debye_structure_factor.__init__).parameters.items() if n != "self"]
    assert params == [("q", E), ("r_cut", E), ("nlist", E), ("type", E), ("weights", None), ("name", None), ("sigma", 1.0)]
    assert issubclass(cv.debye_structure_factor, cv._neighbour_variable)
    assert [n for n in inspect.signature(cv.debye_structure_factor.get_spectrum).parameters] == ["self", "q_min", "q_max", "n_q"]
    for meth in ("get_rcut", "get_virial", "get_local", "get_intensities", "get_spectrum", "set_grid", "set_params"):
        assert hasattr(cv.debye_structure_factor, meth), meth
    assert "discontinuous" in cv.debye_structure_factor.__doc__
    assert issubclass(mod.DebyeStructureFactor, mod.CollectiveVariable)
    for meth in ("getLocalValues", "getIntensities", "getSpectrum", "getVirial", "getCurrentValue", "getForceArray", "getLogValue",
                 "getProvidedLogQuantities", "getRCut"):
        assert hasattr(mod.DebyeStructureFactor, meth), meth
