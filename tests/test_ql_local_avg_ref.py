"""CPU: the yardstick of the options of cv.steinhardt_local (tests/ql_local_avg_ref.py: neighbour average, switch, gate) is checked
before anything is held against it — against the restatement of the plain variable with the options off, against known answers,
and its analytic gradient against central differences of its own s.  Then the C ABI of the options: exported, declared, mirrored in
ctypes field by field, and validated before a device is touched.  Nothing here needs a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import ql_local_avg_ref as avg_ref
import ql_local_ref
import util

# computed for the issue that introduced the options (fp64, checked there against finite differences); reproduced here, not fitted
KNOWN = {
    "average": 0.205134494125319,
    "switch": 0.518075509113396,
    "average+switch": 0.720412449710603,
    "average+switch+gate": 0.715644379269685,
    "switch+gate": 0.513793491441936,
}
DILUTE_S = 0.29674341030178875


def test_options_off_is_the_plain_variable():
    case = ql_local_ref.issue_case()
    plain = ql_local_ref.compute(**case)
    off = avg_ref.compute(**case)
    assert off["s"] == plain["s"]
    assert np.array_equal(off["c"], plain["c"]) and np.array_equal(off["n"], plain["n"]) and np.array_equal(off["v"], plain["c"])
    print("gradients: largest difference %.3e" % np.abs(off["grad"] - plain["grad"]).max())
    assert np.abs(off["grad"] - plain["grad"]).max() <= 1e-16


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    out = avg_ref.compute(gradient=False, **ql_local_ref.issue_case(), **avg_ref.COMBINATIONS[name])
    print("%s: s = %.15g, expected %.15g" % (name, out["s"], KNOWN[name]))
    assert out["s"] == pytest.approx(KNOWN[name], rel=1e-12)


def central_difference_check(case, opt, n_coordinates=12, seed=0, step=1e-6):
    out = avg_ref.compute(**case, **opt)
    g = out["grad"]
    assert np.isfinite(g).all()
    scale = np.abs(g).max()
    assert scale > 0
    rng = np.random.default_rng(seed)
    coords = [(int(rng.integers(len(g))), int(rng.integers(3))) for _ in range(n_coordinates)]
    worst = 0.0
    for k, a in coords:
        sp = []
        for sign in (1.0, -1.0):
            p = case["pos"].copy()
            p[k, a] += sign * step
            sp.append(avg_ref.compute(**{**case, "pos": p}, gradient=False, **opt)["s"])
        worst = max(worst, abs((sp[0] - sp[1]) / (2 * step) - g[k, a]))
    print("max |ds/dr| %.4g, largest difference on %d coordinates %.3e (%.3e of it)" % (scale, n_coordinates, worst, worst / scale))
    assert worst <= 1e-7 * scale
    return out


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_analytic_gradient_against_central_differences(name):
    case = ql_local_ref.issue_case()
    out = central_difference_check(case, avg_ref.COMBINATIONS[name], n_coordinates=14)
    # translation invariance, and particles of the other type
    assert np.abs(out["grad"].sum(axis=0)).max() <= 1e-15
    other = case["types"] == 1
    assert np.all(out["grad"][other] == 0.0) and np.all(out["v"][other] == 0.0) and np.all(out["c"][other] == 0.0)


def test_dilute_edge_case():
    """particles without a neighbour, with less than one, and inside the gate's ramp: finite, and the same difference check"""
    case = avg_ref.dilute_case()
    opt = {k: case.pop(k) for k in ("average", "switch", "gate")}
    out = central_difference_check(case, opt, n_coordinates=16, seed=1)
    n = out["n"]
    assert ((n == 0).sum(), ((n > 0) & (n < 2)).sum(), ((n > 2) & (n < 6)).sum()) == (6, 41, 20)
    print("s = %.17g" % out["s"])
    assert out["s"] == pytest.approx(DILUTE_S, rel=1e-12)
    assert np.all(out["v"][n == 0] == 0.0) and np.all(out["grad"][n == 0] == 0.0)
    assert np.abs(out["grad"].sum(axis=0)).max() <= 1e-15


# ---- the C ABI of the options -------------------------------------------------------------------------------------------------

OPT_SYMBOLS = ("mtd_ql_local_scratch_doubles_opt", "mtd_ql_local_accumulate_opt", "mtd_ql_local_forces_opt")
INVALID = -1


def test_option_symbols_exported_and_declared(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in OPT_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s


def test_options_struct_mirrors_the_header(abi):
    """the ctypes mirror has the header's fields, in the header's order and types; 40 bytes under the C layout rules"""
    text = open(abi.HEADER_PATH).read()
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*mtd_ql_local_options;", text)
    assert m, "mtd_ql_local_options is not declared"
    ctype = {"int": C.c_int, "unsigned int": C.c_uint, "double": C.c_double}
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            t = re.match(r"(unsigned int|int|double)\s", decl).group(1)
            for name in decl[len(t):].split(","):
                fields.append((name.strip(), ctype[t]))
    assert fields == list(abi.QlLocalOptions._fields_)
    assert C.sizeof(abi.QlLocalOptions) == 40
    assert abi.QlLocalOptions.c0.offset == 8 and abi.QlLocalOptions.p.offset == 16 and abi.QlLocalOptions.n_lo.offset == 24
    o = abi.QlLocalOptions.make(average=True, switch=(0.12, 3), gate=(2, 6))
    assert (o.average, o.switch_on, o.c0, o.p, o.gate_on, o.n_lo, o.n_hi) == (1, 1, 0.12, 3, 1, 2.0, 6.0)
    assert bytes(abi.QlLocalOptions.make()) == bytes(40)


def _calls(lib, abi, box, opt, n=4):
    """the two passes with small non-null pointers that are never dereferenced when the arguments are refused"""
    ql_ref = util.dbl_array([0, 0, 0, 0, 1, 0, 1])
    partials, c, nv, v = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_partials = C.c_uint()
    o = C.byref(opt) if opt is not None else None
    acc = lib.mtd_ql_local_accumulate_opt(n, 4096, 1, C.byref(box), 4096, 4096, 4096, 1.4, 1.2, 6, 0, ql_ref, 4, 4096, C.byref(partials),
                                          C.byref(n_partials), C.byref(c), C.byref(nv), None, o, C.byref(v))
    frc = lib.mtd_ql_local_forces_opt(n, 4096, 4096, 1, C.byref(box), 4096, 4096, 4096, 1.4, 1.2, 6, 0, ql_ref, 4, 4096, None, 0.5, None, o)
    return acc, frc


def test_option_validation_without_gpu(abi):
    """c0 <= 0, p == 0 and a gate without 0 <= n_lo < n_hi are MTD_ERR_INVALID_ARGUMENT before any device call; with n_particles = 0 the
    force pass has nothing to launch and returns success for valid options: the fields are read where the header puts them.
    (A scratch sized for fewer list entries than the list holds is not among the refusals: the entry points are told neither the size
    of the scratch nor the length of the list, so it cannot be known there; the header says so, and SteinhardtLocal sizes its scratch
    from the list at every step — test_options_on_a_device_list_follow_the_particles.)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    make = abi.QlLocalOptions.make
    nan = float("nan")
    bad = [make(switch=(0.0, 3)), make(switch=(-0.1, 3)), make(switch=(nan, 3)), make(switch=(0.25, 0)), make(gate=(-1.0, 4.0)),
           make(gate=(4.0, 4.0)), make(gate=(6.0, 2.0)), make(gate=(nan, 4.0)), make(gate=(1.0, nan)),
           make(average=True, switch=(0.0, 1)), make(average=True, switch=(0.12, 3), gate=(3.0, 1.0))]
    for opt in bad:
        assert _calls(lib, abi, box, opt) == (INVALID, INVALID)
        assert _calls(lib, abi, box, opt, n=0)[1] == INVALID
    good = [None, make(), make(average=True), make(switch=(0.25, 3)), make(gate=(0.0, 1.0)), make(average=True, switch=(0.12, 1), gate=(4, 8))]
    for opt in good:
        assert _calls(lib, abi, box, opt, n=0)[1] == 0
    # fields of an option that is off are not looked at
    off = make()
    off.c0, off.p, off.n_lo, off.n_hi = -1.0, 0, 5.0, 1.0
    assert _calls(lib, abi, box, off, n=0)[1] == 0
    # the checks of the plain entry points still come first
    ql_ref = util.dbl_array([0, 0, 0, 0, 1, 0, 1])
    assert lib.mtd_ql_local_forces_opt(4, 4096, 4096, 1, C.byref(box), 4096, 4096, 4096, 1.0, 1.2, 6, 0, ql_ref, 4, 4096, None, 0.5, None,
                                       C.byref(make(average=True))) == INVALID


def test_option_scratch_sizes(abi):
    lib = abi.load()
    make = abi.QlLocalOptions.make
    for n, lmax, entries in ((0, 6, 0), (1, 0, 0), (108, 6, 1300), (256000, 6, 256000 * 12), (501, 12, 9000)):
        plain = lib.mtd_ql_local_scratch_doubles(n, lmax)
        rows = n * (lmax + 1) * (lmax + 2)
        assert lib.mtd_ql_local_scratch_doubles_opt(n, lmax, entries, None) == plain
        assert lib.mtd_ql_local_scratch_doubles_opt(n, lmax, entries, C.byref(make())) == plain
        sw = lib.mtd_ql_local_scratch_doubles_opt(n, lmax, entries, C.byref(make(switch=(0.25, 3))))
        assert plain + n <= sw <= plain + n + 2                                   # v_i, padded to 16 bytes
        assert lib.mtd_ql_local_scratch_doubles_opt(n, lmax, entries, C.byref(make(gate=(1, 2)))) == sw
        av = lib.mtd_ql_local_scratch_doubles_opt(n, lmax, entries, C.byref(make(average=True)))
        # v_i, a0_i, slot weights, two more tables of rows and one double per list entry
        assert av >= plain + 2 * n + 2 * rows + entries
        assert av <= plain + 2 * n + 2 * rows + entries + (lmax + 1) * (lmax + 2) // 2 + 6
        assert av % 2 == entries % 2                                              # everything before E keeps rows 16-byte aligned
        assert lib.mtd_ql_local_scratch_doubles_opt(n, lmax, entries + 10, C.byref(make(average=True))) == av + 10


def test_python_surface_of_the_options():
    """cv.steinhardt_local takes average / switch / gate as keyword arguments of the call and has get_switched / set_options; the host
    class has the setters"""
    import inspect
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    call = inspect.signature(type(cv.steinhardt_local).__call__).parameters
    assert [(n, call[n].default) for n in ("average", "switch", "gate")] == [("average", False), ("switch", None), ("gate", None)]
    assert all(call[n].kind == inspect.Parameter.KEYWORD_ONLY for n in ("average", "switch", "gate"))
    for meth in ("get_switched", "set_options", "get_local", "get_coordination"):
        assert hasattr(cv.steinhardt_local, meth), meth
    for meth in ("setAverage", "setSwitch", "clearSwitch", "setGate", "clearGate", "getSwitchedValues"):
        assert hasattr(mod.SteinhardtLocal, meth), meth


def test_switch_limit_of_a_huge_power():
    """x^p beyond the range of a double: h is its limit 1 and h' is 0, not inf * 0"""
    h, dh = avg_ref.switch_fn(np.array([0.0, 0.05, 0.1, 0.2, 5.0]), (0.1, 2000))
    assert np.isfinite(h).all() and np.isfinite(dh).all()
    assert h[0] == 0.0 and h[1] == 0.0 and h[2] == 0.5 and h[3] == 1.0 and h[4] == 1.0 and dh[3] == 0.0 and dh[4] == 0.0
