"""CPU: the probe volume (mtd_probe_*, csrc/probe_volume.hip) is exported, declared and registered, its two structures have the header's
layout, it refuses bad arguments — the fit rule included — before it touches a device, and it is reachable from the host classes and the
Python API.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re

import probe_volume_ref as pv

PROBE_SYMBOLS = ("mtd_probe_scratch_doubles", "mtd_probe_accumulate", "mtd_probe_finalize", "mtd_probe_forces", "mtd_probe_local")
INVALID, SUCCESS = -1, 0
NAN, INF = float("nan"), float("inf")


def _header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in PROBE_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    text = _header()
    m = re.search(r"enum mtd_probe_shape \{ MTD_PROBE_BOX = (\d), MTD_PROBE_SPHERE = (\d), MTD_PROBE_CYLINDER = (\d) \}", text)
    assert tuple(int(x) for x in m.groups()) == (abi.MTD_PROBE_BOX, abi.MTD_PROBE_SPHERE, abi.MTD_PROBE_CYLINDER) == (0, 1, 2)
    # the stream travels inside mtd_probe_call: no entry point of the unit takes a bare one (tests/test_stream_gate.py counts those)
    found = 0
    for m in re.finditer(r"\b(mtd_probe_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        assert "mtd_stream_t" not in m.group(2), m.group(1)
        found += 1
    assert found == len(PROBE_SYMBOLS)


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
    extents = {"MTD_MAX_TYPES": 16, "3": 3}
    for name, mirror in (("mtd_probe_params", abi.ProbeParams), ("mtd_probe_call", abi.ProbeCall)):
        fields = _header_fields(name)
        assert [f for _, f, _ in fields] == [f for f, _ in mirror._fields_], name
        for (ctype, field, dims), (_, mtype) in zip(fields, mirror._fields_):
            want = C.c_void_p if ctype.endswith("*") else kinds[ctype]
            n = 1
            for d in dims:
                n *= extents[d]
            assert C.sizeof(mtype) == n * C.sizeof(want), (name, field)
    # shape, axis | centre[3] | half_width[3] | radius | sigma_s | r_c | n_types (+ pad) | coeff[16]
    P = abi.ProbeParams
    assert (P.axis.offset, P.centre.offset, P.half_width.offset, P.radius.offset, P.sigma_s.offset, P.r_c.offset, P.n_types.offset,
            P.coeff.offset) == (4, 8, 32, 56, 64, 72, 80, 88)
    assert C.sizeof(P) == 216
    c = abi.ProbeCall
    assert (c.d_postype.offset, c.dtype.offset, c.global_box.offset, c.n_global.offset, c.d_scratch.offset, c.stream.offset) == (8, 16, 24, 32, 40, 48)
    assert C.sizeof(c) == 56
    p = P.make("cylinder", [0.5, 0.25, 0.5], 0.3, radius=2.0, axis=1, half_width=1.5, coeff=[1.0, 0.0, -1.0])
    assert (p.shape, p.axis, p.n_types, p.r_c, p.radius) == (2, 1, 3, 0.6, 2.0) and list(p.half_width) == [INF, 1.5, INF]
    assert list(p.coeff[:4]) == [1.0, 0.0, -1.0, 0.0] and list(p.centre) == [0.5, 0.25, 0.5]
    box = abi.Box.make([10.0, 12.0, 8.0], xy=0.3, xz=-0.2, yz=0.15)
    f = P.fractional([1.0, -2.0, 3.0], box)
    A = pv.lattice([10.0, 12.0, 8.0], xy=0.3, xz=-0.2, yz=0.15)
    back = [box.lo[d] + sum(f[i] * A[i][d] for i in range(3)) for d in range(3)]
    assert max(abs(b - w) for b, w in zip(back, [1.0, -2.0, 3.0])) <= 1e-14


def test_scratch_size(abi):
    """the same for every particle count: two sums and 256 rows of two block sums"""
    lib = abi.load()
    base = lib.mtd_probe_scratch_doubles(0)
    assert base >= 256 * 2 + 2 and base % 2 == 0
    for n in (1, 4097, 1 << 20, 0xffffffff):
        assert lib.mtd_probe_scratch_doubles(n) == base


def _call(abi, box, n_particles=4, pos=1, dtype=0, n_global=4, scratch=4096, **_):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    return abi.ProbeCall(n_particles, pos * 4096 or None, dtype, C.pointer(box) if box is not None else None, n_global, scratch or None, None)


def _par(abi, shape="box", centre=(0.5, 0.5, 0.5), sigma_s=0.3, r_c=None, half_width=(1.0, 2.0, INF), radius=0.0, axis=0, coeff=(1.0, -1.0),
         n_types=None, **_):
    return abi.ProbeParams.make(shape, centre, sigma_s, r_c, half_width, radius, axis, list(coeff), n_types)


def _acc(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    return lib.mtd_probe_accumulate(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(sums) if out else None,
                                    C.byref(n_sums) if out else None)


def _fin(lib, abi, box, out=True, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    v, n = C.c_void_p(), C.c_void_p()
    return lib.mtd_probe_finalize(None if no_par else C.byref(par), None if no_call else C.byref(call), C.byref(v) if out else None, C.byref(n))


def _frc(lib, abi, box, force=1, virial=0, pitch=0, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    return lib.mtd_probe_forces(None if no_par else C.byref(par), None if no_call else C.byref(call), force * 4096 or None, None, 0.5,
                                virial * 4096 or None, pitch)


def _loc(lib, abi, box, out=1, no_par=False, no_call=False, **kw):
    par, call = _par(abi, **kw), _call(abi, box, **kw)
    return lib.mtd_probe_local(None if no_par else C.byref(par), None if no_call else C.byref(call), out * 4096 or None)


SPHERE = dict(shape="sphere", half_width=None, radius=2.0)
CYL = dict(shape="cylinder", half_width=1.5, radius=2.0, axis=2)
REFUSED = [dict(no_par=True), dict(no_call=True), dict(scratch=0), dict(scratch=4096 + 8), dict(pos=0), dict(dtype=7), dict(dtype=-1),
           dict(n_global=0), dict(n_types=0), dict(n_types=17), dict(shape=3), dict(shape=-1),
           dict(sigma_s=0.0), dict(sigma_s=-0.3), dict(sigma_s=NAN), dict(sigma_s=INF), dict(r_c=0.0), dict(r_c=-1.0), dict(r_c=NAN), dict(r_c=INF),
           dict(half_width=(0.0, 2.0, INF)), dict(half_width=(1.0, -2.0, INF)), dict(half_width=(1.0, NAN, INF)), dict(half_width=(1.0, 2.0, -INF)),
           dict(half_width=(INF, INF, INF)),                                                   # no bounded axis
           dict(centre=(NAN, 0.5, 0.5)), dict(centre=(0.5, INF, 0.5)), dict(coeff=[NAN, 1.0]), dict(coeff=[1.0, INF]),
           dict(SPHERE, radius=0.6), dict(SPHERE, radius=0.5), dict(SPHERE, radius=NAN), dict(SPHERE, radius=INF), dict(SPHERE, radius=-2.0),
           dict(CYL, radius=0.6), dict(CYL, axis=3), dict(CYL, axis=-1), dict(CYL, half_width=0.0), dict(CYL, half_width=NAN), dict(CYL, radius=INF)]
ACCEPTED = [dict(), dict(dtype=1), dict(half_width=(INF, INF, 1.0)), dict(half_width=(0.01, 0.01, 0.01)), dict(coeff=[0.0, 0.0]),
            dict(coeff=[-1.0, 2.5]), dict(r_c=1.5), dict(sigma_s=1.0, r_c=0.25), dict(SPHERE), dict(SPHERE, radius=0.6000001), dict(CYL),
            dict(CYL, half_width=INF), dict(CYL, axis=0), dict(centre=(7.25, -3.0, 0.0)), dict(n_types=16, coeff=[1.0] * 16)]


def test_argument_validation_without_gpu(abi):
    """everything the header lists, all before any device call (this test runs on a machine without a GPU).  What is accepted is seen
    through mtd_probe_finalize, which launches nothing, and through the force pass of a rank without particles"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for call in (_acc, _fin, _frc, _loc):
        assert call(lib, abi, None) == INVALID                                           # no box
        assert call(lib, abi, abi.Box.make([10.0, 0.0, 10.0])) == INVALID                # a box without volume
        assert call(lib, abi, abi.Box.make([10.0, NAN, 10.0])) == INVALID
        for kw in REFUSED:
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
    for kw in ACCEPTED:
        assert _fin(lib, abi, box, **kw) == SUCCESS, kw
        assert _frc(lib, abi, box, n_particles=0, **kw) == SUCCESS, kw
        assert _loc(lib, abi, box, n_particles=0, **kw) == SUCCESS, kw
    assert _acc(lib, abi, box, out=False) == INVALID
    assert _fin(lib, abi, box, out=False) == INVALID
    assert _frc(lib, abi, box, force=0) == INVALID
    assert _loc(lib, abi, box, out=0) == INVALID
    assert _frc(lib, abi, box, virial=1, pitch=3) == INVALID                              # a virial pitch below n_particles = 4


def test_no_particles_is_success(abi):
    """a rank that holds no particle of a system that has some; an empty system is refused"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _frc(lib, abi, box, n_particles=0, pos=0, force=0) == SUCCESS
    assert _frc(lib, abi, box, n_particles=0, pos=0, force=0, virial=1, pitch=0) == SUCCESS
    assert _loc(lib, abi, box, n_particles=0, pos=0, out=0) == SUCCESS
    assert _fin(lib, abi, box, n_particles=0, pos=0) == SUCCESS
    for call in (_acc, _fin, _frc, _loc):
        assert call(lib, abi, box, n_particles=0, n_global=0) == INVALID


def test_fit_rule_orthorhombic(abi):
    """e = w + r_c (R + r_c) against L / 2 on every bounded axis: accepted AT L / 2, refused just above"""
    lib = abi.load()
    box = abi.Box.make([10.0, 12.0, 8.0])
    up = lambda x: x * (1.0 + 2.0 ** -50)                                # a few ulp: w + r_c still rounds above L / 2
    # r_c = 0.5 (exact in binary): the sums below are exact
    ok = [dict(half_width=(4.5, 5.5, 3.5)), dict(half_width=(INF, INF, 3.5)), dict(half_width=(4.5, INF, INF)),
          dict(SPHERE, radius=3.5), dict(CYL, radius=4.5, half_width=3.5), dict(CYL, radius=4.5, half_width=INF),
          dict(CYL, axis=1, radius=3.5, half_width=5.5), dict(CYL, axis=0, radius=3.5, half_width=4.5)]
    bad = [dict(half_width=(up(4.5), 5.5, 3.5)), dict(half_width=(4.5, up(5.5), 3.5)), dict(half_width=(4.5, 5.5, up(3.5))),
           dict(half_width=(INF, INF, 3.6)), dict(SPHERE, radius=up(3.5)), dict(SPHERE, radius=4.0), dict(CYL, radius=up(4.5), half_width=3.5),
           dict(CYL, radius=4.5, half_width=up(3.5)), dict(CYL, axis=1, radius=up(3.5), half_width=5.5), dict(CYL, axis=0, radius=3.5, half_width=4.6)]
    for kw in ok:
        kw = dict(kw, sigma_s=0.25, r_c=0.5)
        assert _fin(lib, abi, box, **kw) == SUCCESS, kw
        assert _frc(lib, abi, box, n_particles=0, **kw) == SUCCESS and _loc(lib, abi, box, n_particles=0, **kw) == SUCCESS, kw
    for kw in bad:
        kw = dict(kw, sigma_s=0.25, r_c=0.5)
        for call in (_acc, _fin, _frc, _loc):
            assert call(lib, abi, box, **kw) == INVALID, (call.__name__, kw)
    # the same region in a box that has shrunk: the rule is applied to the box of the call
    kw = dict(half_width=(4.5, 5.5, 3.5), sigma_s=0.25, r_c=0.5)
    assert _fin(lib, abi, abi.Box.make([10.0, 12.0, 8.0]), **kw) == SUCCESS and _fin(lib, abi, abi.Box.make([10.0, 12.0, 7.99]), **kw) == INVALID


def test_fit_rule_tilted(abi):
    """the header's rule, against its restatement (tests/probe_volume_ref.py::fits) and at hand-computed limits"""
    lib = abi.load()
    L, tilt = (17.0, 18.5, 16.25), dict(xy=0.3, xz=-0.2, yz=0.15)
    box = abi.Box.make(L, **tilt)
    # bounded along z only: a_3 alone has a z component, its coordinate is z / Lz: e <= Lz / 2 (within the 1e-12 of the rule)
    assert _fin(lib, abi, box, half_width=(INF, INF, 7.5), sigma_s=0.25, r_c=0.5) == SUCCESS
    assert _fin(lib, abi, box, half_width=(INF, INF, 7.7), sigma_s=0.25, r_c=0.5) == INVALID
    # bounded along x only: a_2 and a_3 have x components and their coordinates depend on y and z, which are unbounded
    assert _fin(lib, abi, box, half_width=(1.0, INF, INF)) == INVALID
    assert _fin(lib, abi, abi.Box.make(L, yz=0.15), half_width=(1.0, INF, INF)) == SUCCESS   # a_1 alone has an x component here
    assert _fin(lib, abi, abi.Box.make(L, yz=0.15), half_width=(INF, 1.0, INF)) == INVALID   # a_3 has a y component; it depends on z
    # a cylinder without ends along z: a_3 must not lean (its images along a_3 would be shifted sideways)
    assert _fin(lib, abi, box, **dict(CYL, half_width=INF)) == INVALID
    assert _fin(lib, abi, abi.Box.make(L, xy=0.3), **dict(CYL, half_width=INF)) == SUCCESS
    assert _fin(lib, abi, abi.Box.make(L, xy=0.3), **dict(CYL, axis=0, half_width=INF)) == SUCCESS     # a_2 leans ALONG this axis: harmless
    assert _fin(lib, abi, abi.Box.make(L, xy=0.3), **dict(CYL, axis=1, half_width=INF)) == INVALID
    # a sphere: row 0 of the inverse is (1, -xy, xy yz - xz) / Lx, the strictest: e (1 + 0.3 + 0.245) / 17 <= 1 / 2
    e_max = 0.5 * 17.0 / (1.0 + 0.3 + (0.3 * 0.15 + 0.2))
    assert _fin(lib, abi, box, **dict(SPHERE, radius=e_max - 0.5 - 1e-9, sigma_s=0.25, r_c=0.5)) == SUCCESS
    assert _fin(lib, abi, box, **dict(SPHERE, radius=e_max - 0.5 + 1e-9, sigma_s=0.25, r_c=0.5)) == INVALID
    # and a sweep against the restatement
    n_ok = n_bad = 0
    for shape, sizes in (("box", [(w, 1.3 * w, 0.8 * w) for w in (1.0, 3.0, 4.5, 5.0, 5.5, 6.5, 8.0)]), ("sphere", [2.0, 4.0, 4.9, 5.1, 6.0, 7.0]),
                         ("cylinder", [(R, w, ax) for R in (2.0, 4.5, 5.2, 6.5) for w in (1.0, 6.0, 8.0) for ax in (0, 1, 2)])):
        for size in sizes:
            if shape == "box":
                reg, kw = pv.region("box", [0, 0, 0], 0.25, 0.5, w=size), dict(half_width=size)
            elif shape == "sphere":
                reg, kw = pv.region("sphere", [0, 0, 0], 0.25, 0.5, R=size), dict(SPHERE, radius=size)
            else:
                reg, kw = pv.region("cylinder", [0, 0, 0], 0.25, 0.5, R=size[0], w=size[1], axis=size[2]), dict(CYL, radius=size[0], half_width=size[1], axis=size[2])
            want = pv.fits(reg, L, tilt)
            n_ok, n_bad = n_ok + want, n_bad + (not want)
            assert _fin(lib, abi, box, **dict(kw, sigma_s=0.25, r_c=0.5)) == (SUCCESS if want else INVALID), (shape, size)
    assert n_ok >= 10 and n_bad >= 10


def test_python_and_pybind_surface():
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.probe_volume.__init__).parameters.items() if n != "self"]
    assert params == [("shape", E), ("centre", E), ("sigma_s", E), ("r_c", None), ("half_widths", None), ("radius", None), ("axis", None),
                      ("half_length", None), ("weights", None), ("name", None), ("sigma", 1.0)]
    assert issubclass(cv.probe_volume, cv._collective_variable) and not issubclass(cv.probe_volume, (cv.lamellar, cv._neighbour_variable))
    for meth in ("set_region", "set_weights", "get_count", "get_local", "get_virial", "set_grid", "set_params"):
        assert hasattr(cv.probe_volume, meth), meth
    doc = cv.probe_volume.__doc__.lower()
    assert "virial" in doc and "do not sum to zero" in doc and "radially" in doc
    # the shape's own arguments, and nothing else
    R = cv.probe_volume._region
    assert R("box", [0, 0, 0], 0.3, None, [1, 2, INF], None, None, None) == (0, [0.0, 0.0, 0.0], [1.0, 2.0, INF], 0.0, 0, 0.3, 0.6)
    assert R("sphere", [0, 0, 1], 0.3, 0.9, None, 2, None, None) == (1, [0.0, 0.0, 1.0], [INF] * 3, 2.0, 0, 0.3, 0.9)
    assert R("cylinder", [0, 0, 0], 0.3, None, None, 2.0, "y", 1.5) == (2, [0.0, 0.0, 0.0], [INF, 1.5, INF], 2.0, 1, 0.3, 0.6)
    assert R("cylinder", [0, 0, 0], 0.3, None, None, 2.0, "z", None)[2] == [INF] * 3
    for bad in (("box", [0, 0, 0], 0.3, None, None, None, None, None), ("box", [0, 0, 0], 0.3, None, [1, 2, 3], 2.0, None, None),
                ("box", [0, 0, 0], 0.3, None, [1, 2, 3], None, "x", None), ("box", [0, 0, 0], 0.3, None, [1, 2, 3], None, None, 1.0),
                ("box", [0, 0, 0], 0.3, None, [1, 2], None, None, None), ("box", [0, 0], 0.3, None, [1, 2, 3], None, None, None),
                ("sphere", [0, 0, 0], 0.3, None, None, None, None, None), ("sphere", [0, 0, 0], 0.3, None, [1, 2, 3], 2.0, None, None),
                ("sphere", [0, 0, 0], 0.3, None, None, 2.0, "x", None), ("sphere", [0, 0, 0], 0.3, None, None, 2.0, None, 1.0),
                ("cylinder", [0, 0, 0], 0.3, None, None, 2.0, None, 1.0), ("cylinder", [0, 0, 0], 0.3, None, None, None, "x", 1.0),
                ("cylinder", [0, 0, 0], 0.3, None, [1, 2, 3], 2.0, "x", None), ("cylinder", [0, 0, 0], 0.3, None, None, 2.0, "w", None),
                ("ellipsoid", [0, 0, 0], 0.3, None, None, 2.0, None, None)):
        try:
            R(*bad)
        except (ValueError, KeyError):
            continue
        raise AssertionError(bad)
    # the integrator picks its routes by class: this one must be neither a lamellar nor a Bragg variable
    assert issubclass(mod.ProbeVolume, mod.CollectiveVariable)
    assert not issubclass(mod.ProbeVolume, (mod.LamellarOrderParameterGPU, mod.BraggIntensity))
    for meth in ("setRegion", "setWeights", "getWeights", "getFractionalCentre", "getCount", "getLocal", "getVirial", "getVirialPitch",
                 "getCurrentValue", "getForceArray", "getLogValue", "getProvidedLogQuantities", "setUmbrella", "computeDerivatives"):
        assert hasattr(mod.ProbeVolume, meth), meth
