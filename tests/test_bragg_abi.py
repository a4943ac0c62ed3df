"""CPU: the Bragg intensity (mtd_bragg_*, csrc/bragg.hip) is exported, declared and registered, its two structures have the header's
layout, it refuses bad arguments before it touches a device, and it is reachable from the host classes and the Python API.
Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re

BRAGG_SYMBOLS = ("mtd_bragg_scratch_doubles", "mtd_bragg_accumulate", "mtd_bragg_finalize", "mtd_bragg_forces")
INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0
NAN, INF = float("nan"), float("inf")


def _header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in BRAGG_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    text = _header()
    assert int(re.search(r"#define MTD_BRAGG_MAX_MODES (\d+)", text).group(1)) == abi.MTD_BRAGG_MAX_MODES == 16
    # the stream travels inside mtd_bragg_call: no entry point of the unit takes a bare one (tests/test_stream_gate.py counts those)
    found = 0
    for m in re.finditer(r"\b(mtd_bragg_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        assert "mtd_stream_t" not in m.group(2), m.group(1)
        found += 1
    assert found == len(BRAGG_SYMBOLS)


def _header_fields(name):
    """[(C type, field, array suffix)] of `typedef struct { ... } name;` in include/mtd_abi.h"""
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header()).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, field = decl.rsplit(" ", 1)
        dims = re.findall(r"\[(\w+)\]", field)
        out.append((ctype + " *" * bool(field.count("*")), re.sub(r"\[.*", "", field).replace("*", ""), dims))
    return out


def test_struct_layouts_match_header(abi):
    """the ctypes mirrors field by field against the header's field list: names, order, element type and array extents"""
    kinds = {"double": C.c_double, "unsigned int": C.c_uint, "int": C.c_int, "mtd_stream_t": C.c_void_p}
    extents = {"MTD_BRAGG_MAX_MODES": 16, "MTD_MAX_TYPES": 16, "3": 3}
    for name, mirror in (("mtd_bragg_params", abi.BraggParams), ("mtd_bragg_call", abi.BraggCall)):
        fields = _header_fields(name)
        assert [f for _, f, _ in fields] == [f for f, _ in mirror._fields_], name
        for (ctype, field, dims), (_, mtype) in zip(fields, mirror._fields_):
            want = C.c_void_p if ctype.endswith("*") else kinds[ctype]
            n = 1
            for d in dims:
                n *= extents[d]
            assert C.sizeof(mtype) == n * C.sizeof(want), (name, field)
    # n_modes | hkl[16][3] | n_types (+ pad) | coeff[16] | weights[16] | modulus, trig_mode
    P = abi.BraggParams
    assert (P.hkl.offset, P.n_types.offset, P.coeff.offset, P.weights.offset, P.modulus.offset, P.trig_mode.offset) == (4, 196, 200, 328, 456, 460)
    assert C.sizeof(P) == 464
    c = abi.BraggCall
    assert (c.d_postype.offset, c.dtype.offset, c.global_box.offset, c.n_global.offset, c.d_scratch.offset, c.stream.offset) == (8, 16, 24, 32, 40, 48)
    p = P.make([(0, 0, 2), (1, -1, 0)], [1.0, -0.5, 0.0])
    assert (p.n_modes, p.n_types, p.modulus, p.trig_mode) == (2, 3, 0, 0) and list(p.hkl[1]) == [1, -1, 0]
    assert list(p.weights[:3]) == [0.5, 0.5, 0.0] and list(p.coeff[:4]) == [1.0, -0.5, 0.0, 0.0]


def test_scratch_size(abi):
    """the same for every particle count: sums, value, S_k, coefficients and 256 rows of 34 block sums"""
    lib = abi.load()
    base = lib.mtd_bragg_scratch_doubles(0)
    assert base >= 256 * 34 + 34 + 1 + 16 + 32 and base % 2 == 0
    for n in (1, 4097, 1 << 20, 0xffffffff):
        assert lib.mtd_bragg_scratch_doubles(n) == base


def _call(abi, box, n_particles=4, pos=1, dtype=0, n_global=4, scratch=4096, **_):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    return abi.BraggCall(n_particles, pos * 4096 or None, dtype, C.pointer(box) if box is not None else None, n_global, scratch or None, None)


def _par(abi, hkl=((0, 0, 2), (1, 0, 0)), coeff=(1.0, -1.0), weights=None, modulus=False, trig_mode=0, n_modes=None, n_types=None, **_):
    return abi.BraggParams.make(list(hkl), list(coeff), weights, modulus, trig_mode, n_modes, n_types)


def _acc(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    return lib.mtd_bragg_accumulate(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(sums) if out else None,
                                    C.byref(n_sums) if out else None)


def _fin(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    v, s, a, g = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    return lib.mtd_bragg_finalize(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(v) if out else None, C.byref(s),
                                  C.byref(a), C.byref(g))


def _frc(lib, abi, box, force=1, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    return lib.mtd_bragg_forces(None if no_par else C.byref(par), None if no_call else C.byref(call), force * 4096 or None, None, 0.5)


SEVENTEEN = [(1, 0, k) for k in range(17)]
REFUSED = [dict(no_par=True), dict(no_call=True), dict(scratch=0), dict(scratch=4096 + 8), dict(pos=0), dict(dtype=7), dict(dtype=-1),
           dict(n_global=0), dict(n_modes=0), dict(n_types=0), dict(n_types=17), dict(trig_mode=3), dict(trig_mode=-1),
           dict(weights=[NAN, 1.0]), dict(weights=[1.0, INF]), dict(weights=[-INF, 1.0]), dict(coeff=[NAN, 1.0]), dict(coeff=[1.0, INF])]
ACCEPTED = [dict(), dict(modulus=True), dict(trig_mode=1), dict(trig_mode=2), dict(weights=[-1.0, 0.0]), dict(coeff=[0.0, 0.0]),
            dict(hkl=SEVENTEEN[:16]), dict(hkl=[(0, 0, 0)]), dict(dtype=1)]


def test_argument_validation_without_gpu(abi):
    """null pointers, K = 0, non-finite weights or amplitudes, an unknown dtype or trig mode, a misaligned scratch, n_global = 0:
    MTD_ERR_INVALID_ARGUMENT; K > 16: MTD_ERR_UNSUPPORTED — all before any device call (this test runs on a machine without a GPU)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _fin, _frc):
        assert call(lib, abi, None) == INVALID                                           # no box
        assert call(lib, abi, abi.Box.make([10.0, 0.0, 10.0])) == INVALID                # a box without volume
        for kw in REFUSED:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
        for kw in ACCEPTED:                                                              # what is accepted gets as far as the capacity
            kw = dict(kw, hkl=SEVENTEEN) if "hkl" not in kw else dict(kw, n_modes=17)
            if "weights" in kw:
                kw["weights"] = list(kw["weights"]) + [1.0] * 15
            assert call(lib, abi, box, **kw) == UNSUPPORTED, (call.__name__, kw)
        assert call(lib, abi, box, n_modes=1000) == UNSUPPORTED
        for kw in (dict(scratch=4096 + 8), dict(dtype=7), dict(n_global=0), dict(coeff=[NAN, 1.0]), dict(trig_mode=5)):
            assert call(lib, abi, box, hkl=SEVENTEEN, **kw) == INVALID, (call.__name__, kw)   # an invalid argument beside the unsupported one
        assert call(lib, abi, box, hkl=SEVENTEEN, weights=[NAN] + [1.0] * 16) == INVALID
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _fin(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID


def test_no_particles_is_success_in_the_force_pass(abi):
    """a rank that holds no particle of a system that has some"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for kw in ACCEPTED:
        assert _frc(lib, abi, box, n_particles=0, **kw) == SUCCESS
        assert _frc(lib, abi, box, n_particles=0, pos=0, force=0, **kw) == SUCCESS
    assert _frc(lib, abi, box, n_particles=0, n_global=0) == INVALID


def test_python_and_pybind_surface():
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.bragg.__init__).parameters.items() if n != "self"]
    assert params == [("mode", E), ("lattice_vectors", E), ("weights", None), ("modulus", False), ("name", None), ("sigma", 1.0)]
    assert issubclass(cv.bragg, cv._collective_variable) and not issubclass(cv.bragg, (cv.lamellar, cv._neighbour_variable))
    for meth in ("get_structure_factors", "get_amplitudes", "set_weights", "set_trig_mode", "set_grid", "set_params"):
        assert hasattr(cv.bragg, meth), meth
    assert "virial" in cv.bragg.__doc__.lower()
    assert cv.bragg._weights(None, 4) == [0.25] * 4 and cv.bragg._weights([1, 2], 2) == [1.0, 2.0] and cv.bragg._weights(3, 1) == [3.0]
    # the integrator picks its routes by class: this one must be neither a lamellar nor a neighbour-row variable
    assert issubclass(mod.BraggIntensity, mod.CollectiveVariable)
    assert not issubclass(mod.BraggIntensity, mod.LamellarOrderParameterGPU)
    for meth in ("getStructureFactors", "getAmplitudes", "setWeights", "getWeights", "getModulus", "setTrigMode", "getTrigMode",
                 "getCurrentValue", "getForceArray", "getLogValue", "getProvidedLogQuantities", "setUmbrella", "computeDerivatives"):
        assert hasattr(mod.BraggIntensity, meth), meth
