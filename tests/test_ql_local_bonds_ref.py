"""CPU: the yardstick of the solid-bond count of cv.steinhardt_local (tests/ql_local_bonds_ref.py) is checked before anything is held
against it — with bonds off against ql_local_avg_ref bit for bit, against known answers, its analytic gradient against central
differences of its own s (the bound of tests/test_ql_local_avg_ref.py), its summed virial against strain differences (the bound of
tests/test_ql_local_virial_ref.py).  Then the C ABI of the bonds: exported, declared, mirrored in ctypes field by field, validated
before a device is touched, and the size of its scratch.  Nothing here needs a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import ql_local_avg_ref as avg_ref
import ql_local_bonds_ref as bonds_ref
import ql_local_ref
import util

# computed for the issue that introduced the bond count (fp64, checked there against finite differences); reproduced here, not fitted.
# The first is known to the 13 digits the issue printed; the restatement, which passes the difference check below, gives the rest.
KNOWN = {
    "bonds(0.5,0.7)": (7.945620996786, 1e-12),
    "bonds": (7.90058730367782, 1e-12),
    "bonds+switch": (0.712799889154498, 1e-12),
    "bonds+switch+gate": (0.710073369647509, 1e-12),
    "own-degrees+bonds+switch": (0.664665335978127, 1e-12),
}
DILUTE_S = 0.24648936191120521
BIAS = 0.9


@pytest.mark.parametrize("opt", [dict(), dict(switch=(0.25, 3)), dict(switch=(0.25, 3), gate=(4, 8)), dict(gate=(10, 13))])
def test_bonds_off_is_the_variable_without_them(opt):
    case = ql_local_ref.issue_case()
    a = avg_ref.compute(**case, **opt)
    b = bonds_ref.compute(**case, **opt)
    assert b["s"] == a["s"]
    for key in ("c", "n", "v"):
        assert np.array_equal(a[key], b[key]), key
    assert b["b"] is None and b["dent"] is None
    print("gradients: largest difference %.3e of %.3e" % (np.abs(a["grad"] - b["grad"]).max(), np.abs(a["grad"]).max()))
    assert np.abs(a["grad"] - b["grad"]).max() <= 1e-16


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    case, opt = bonds_ref.issue_case(name)
    out = bonds_ref.compute(gradient=False, **case, **opt)
    print("%s: s = %.17g, expected %.15g" % (name, out["s"], KNOWN[name][0]))
    assert out["s"] == pytest.approx(KNOWN[name][0], rel=KNOWN[name][1])
    # the plain local value is untouched by the bonds; d lies in [-1, 1] and is symmetric in the two ends of a bond
    assert np.array_equal(out["c"], ql_local_ref.compute(**case, gradient=False)["c"])
    d = out["dent"]
    assert np.abs(d).max() <= 1.0 + 1e-14
    pair = {(int(i), int(j)): x for i, j, x in zip(out["i"], out["j"], d)}
    assert max(abs(x - pair[(j, i)]) for (i, j), x in pair.items()) <= 1e-15


def central_difference_check(case, opt, n_coordinates=14, seed=0, step=1e-6):
    out = bonds_ref.compute(**case, **opt)
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
            sp.append(bonds_ref.compute(**{**case, "pos": p}, gradient=False, **opt)["s"])
        worst = max(worst, abs((sp[0] - sp[1]) / (2 * step) - g[k, a]))
    print("max |ds/dr| %.4g, largest difference on %d coordinates %.3e (%.3e of it)" % (scale, n_coordinates, worst, worst / scale))
    assert worst <= 1e-7 * scale
    return out


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_analytic_gradient_against_central_differences(name):
    case, opt = bonds_ref.issue_case(name)
    out = central_difference_check(case, opt, n_coordinates=14)
    # translation invariance, and particles of the other type
    assert np.abs(out["grad"].sum(axis=0)).max() <= 1e-15
    other = case["types"] == 1
    assert other.sum() > 0
    for key in ("grad", "v", "c", "b", "n"):
        assert np.all(out[key][other] == 0.0), key


def test_dilute_edge_case():
    """particles without a neighbour, with less than one, and inside the gate's ramp; products d from -0.30 to 1 with most of them inside
    the ramp of the bonds: finite, and the same difference check"""
    case, opt = bonds_ref.dilute_case()
    out = central_difference_check(case, opt, n_coordinates=16, seed=1)
    n, d = out["n"], out["dent"]
    assert ((n == 0).sum(), ((n > 0) & (n < 2)).sum(), ((n > 2) & (n < 6)).sum()) == (6, 41, 20)
    print("s = %.17g; d from %.4f to %.4f, %d of %d entries inside the ramp" % (out["s"], d.min(), d.max(), ((d > 0.0) & (d < 0.9)).sum(), len(d)))
    assert out["s"] == pytest.approx(DILUTE_S, rel=1e-12)
    assert (len(d), ((d > 0.0) & (d < 0.9)).sum()) == (406, 300) and -0.31 < d.min() < -0.30
    assert not ((n > 0) & (out["c"] == 0)).any()
    assert np.all(out["v"][n == 0] == 0.0) and np.all(out["b"][n == 0] == 0.0) and np.all(out["grad"][n == 0] == 0.0)
    assert np.abs(out["grad"].sum(axis=0)).max() <= 1e-15


@pytest.mark.parametrize("cells,counts", [(3, (426, 1006, 180)), (5, (2000, 4952, 548))])
def test_parity_snapshot_populates_the_ramp(cells, counts):
    """the snapshot the GPU tests are held against: each of below, inside and above the ramp (0.3, 0.8) holds at least 5 % of the entries"""
    case = bonds_ref.noisy_fcc(cells)
    d = bonds_ref.compute(**case, bonds=(0.3, 0.8), gradient=False)["dent"]
    got = ((d <= 0.3).sum(), ((d > 0.3) & (d < 0.8)).sum(), (d >= 0.8).sum())
    print("N = %d: below %d, inside %d, above %d of %d" % (len(case["pos"]), *got, len(d)))
    assert got == counts
    assert min(got) >= 0.05 * len(d)


# ---- the virial ---------------------------------------------------------------------------------------------------------------

def _dense(**kw):
    case = bonds_ref.noisy_fcc(3)
    case.update(kw)
    return case


VIRIAL_CASES = {
    "bonds": lambda: (_dense(), dict(bonds=(0.3, 0.8))),
    "bonds+switch": lambda: (_dense(), dict(bonds=(0.3, 0.8), switch=(6.5, 6))),
    "bonds+switch+gate": lambda: (_dense(), dict(bonds=(0.3, 0.8), switch=(6.5, 6), gate=(10, 13))),
    "l0-and-odd": lambda: (_dense(lmax=4, Ql_ref=[0.2, 0, 1, 0.5, 1]), dict(bonds=(0.3, 0.8), switch=(6.5, 6))),
    "dilute": bonds_ref.dilute_case,
}

_results = {}


def result(name):
    """the restatement's answer for a case, computed once and left unchanged"""
    if name not in _results:
        case, opt = VIRIAL_CASES[name]()
        _results[name] = (case, opt, bonds_ref.compute(**case, bias=BIAS, **opt))
    return _results[name]


@pytest.mark.parametrize("name", sorted(VIRIAL_CASES))
def test_summed_virial_against_strain_differences(name):
    case, opt, out = result(name)
    W = out["W"]
    top = np.abs(W).max()
    fd = -BIAS * bonds_ref.strain_derivative(**case, eps=1e-6, **opt)
    err = np.abs(fd - W).max()
    print("%s: W = %s\n  -bias ds/d eps = %s\n  largest difference %.3e (%.3e of max|W| = %.4g)" % (name, W, fd, err, err / top, top))
    assert top > 0.05
    assert err <= 1e-8 * top
    T = out["tensor"]
    assert np.abs(T - T.T).max() / 2 <= 1e-12 * top
    assert np.abs(np.array([T[a, b] for a, b in bonds_ref.COMPONENTS]) - W).max() <= 1e-13 * top
    assert np.isfinite(out["virial"]).all() and out["virial"].shape == (len(case["pos"]), 6)


def test_gate_is_populated_where_it_is_tested():
    n = result("bonds+switch+gate")[2]["n"]
    assert ((n > 10) & (n < 13)).sum() > 10


# ---- the C ABI of the bonds ---------------------------------------------------------------------------------------------------

BOND_SYMBOLS = ("mtd_ql_local_scratch_doubles_bonds", "mtd_ql_local_accumulate_bonds", "mtd_ql_local_forces_bonds")
INVALID, UNSUPPORTED = -1, -2


def test_bond_symbols_exported_and_declared(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in BOND_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s


def test_bonds_struct_mirrors_the_header(abi):
    """the ctypes mirror has the header's fields, in the header's order and types; 24 bytes with d_lo at offset 8"""
    text = open(abi.HEADER_PATH).read()
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*mtd_ql_local_bonds;", text)
    assert m, "mtd_ql_local_bonds is not declared"
    ctype = {"int": C.c_int, "unsigned int": C.c_uint, "double": C.c_double}
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            t = re.match(r"(unsigned int|int|double)\s", decl).group(1)
            for name in decl[len(t):].split(","):
                fields.append((name.strip(), ctype[t]))
    assert fields == list(abi.QlLocalBonds._fields_)
    assert C.sizeof(abi.QlLocalBonds) == 24
    assert abi.QlLocalBonds.d_lo.offset == 8 and abi.QlLocalBonds.d_hi.offset == 16
    o = abi.QlLocalBonds.make((0.5, 0.7))
    assert (o.on, o.d_lo, o.d_hi) == (1, 0.5, 0.7)
    assert bytes(abi.QlLocalBonds.make()) == bytes(24)
    assert C.sizeof(abi.QlLocalOptions) == 40                      # the options stay as they are


def _calls(lib, abi, box, opt, bonds, n=4, ql=(0, 0, 0, 0, 1, 0, 1), rcut=1.4):
    """the two passes with small non-null pointers that are never dereferenced when the arguments are refused"""
    ql_ref = util.dbl_array(list(ql))
    partials, c, nv, v, b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_partials = C.c_uint()
    o = C.byref(opt) if opt is not None else None
    bd = C.byref(bonds) if bonds is not None else None
    acc = lib.mtd_ql_local_accumulate_bonds(n, 4096, 1, C.byref(box), 4096, 4096, 4096, rcut, 1.2, 6, 0, ql_ref, 4, 4096, C.byref(partials),
                                            C.byref(n_partials), C.byref(c), C.byref(nv), None, o, C.byref(v), bd, C.byref(b))
    frc = lib.mtd_ql_local_forces_bonds(n, 4096, 4096, 1, C.byref(box), 4096, 4096, 4096, rcut, 1.2, 6, 0, ql_ref, 4, 4096, None, 0.5, None, o,
                                        None, 0, bd)
    return acc, frc


def test_bond_validation_without_gpu(abi):
    """bonds without -1 <= d_lo < d_hi <= 1 (NaN included), a negative Ql_ref[l] with bonds on and everything the _opt calls refuse are
    MTD_ERR_INVALID_ARGUMENT, `average` with bonds is MTD_ERR_UNSUPPORTED, all before any device call; with n_particles = 0 the force
    pass has nothing to launch and returns success for valid bonds: the fields are read where the header puts them"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    opts, bonds = abi.QlLocalOptions.make, abi.QlLocalBonds.make
    nan = float("nan")
    for bad in ((-1.5, 0.5), (0.5, 0.5), (0.7, 0.5), (0.5, 1.5), (nan, 0.5), (0.5, nan), (-2.0, 2.0)):
        for opt in (None, opts(), opts(switch=(6.5, 6)), opts(average=True)):
            assert _calls(lib, abi, box, opt, bonds(bad)) == (INVALID, INVALID), bad
            assert _calls(lib, abi, box, opt, bonds(bad), n=0)[1] == INVALID, bad
    assert _calls(lib, abi, box, None, bonds((0.5, 0.7)), ql=(0, 0, 0, 0, -0.5, 0, 1)) == (INVALID, INVALID)
    assert _calls(lib, abi, box, None, bonds((0.5, 0.7)), ql=(0, 0, 0, 0, nan, 0, 1)) == (INVALID, INVALID)
    assert _calls(lib, abi, box, None, bonds((0.5, 0.7)), ql=(0, 0, 0, 0, -0.5, 0, 1), n=0)[1] == INVALID
    assert _calls(lib, abi, box, None, None, ql=(0, 0, 0, 0, -0.5, 0, 1), n=0)[1] == 0          # without bonds a negative weight is allowed
    assert _calls(lib, abi, box, None, bonds(), ql=(0, 0, 0, 0, -0.5, 0, 1), n=0)[1] == 0
    # what the _opt calls refuse
    for opt in (opts(switch=(0.0, 3)), opts(switch=(6.5, 0)), opts(gate=(4.0, 4.0)), opts(gate=(nan, 4.0))):
        assert _calls(lib, abi, box, opt, bonds((0.5, 0.7))) == (INVALID, INVALID)
        assert _calls(lib, abi, box, opt, None) == (INVALID, INVALID)
    assert _calls(lib, abi, box, None, bonds((0.5, 0.7)), rcut=1.0) == (INVALID, INVALID)      # r_on >= r_cut
    # the average
    for opt in (opts(average=True), opts(average=True, switch=(0.12, 3), gate=(4, 8))):
        assert _calls(lib, abi, box, opt, bonds((0.5, 0.7))) == (UNSUPPORTED, UNSUPPORTED)
        assert _calls(lib, abi, box, opt, bonds((0.5, 0.7)), n=0)[1] == UNSUPPORTED
        assert _calls(lib, abi, box, opt, None, n=0)[1] == 0
        assert _calls(lib, abi, box, opt, bonds(), n=0)[1] == 0
    for good in ((0.5, 0.7), (-1.0, 1.0), (0.0, 0.9), (-1.0, -0.5)):
        for opt in (None, opts(), opts(switch=(6.5, 12)), opts(switch=(6.5, 12), gate=(4, 8))):
            assert _calls(lib, abi, box, opt, bonds(good), n=0)[1] == 0
    # fields of bonds that are off are not looked at
    off = bonds()
    off.d_lo, off.d_hi = 3.0, -3.0
    assert _calls(lib, abi, box, None, off, n=0)[1] == 0


def test_bond_scratch_sizes(abi):
    lib = abi.load()
    opts, bonds = abi.QlLocalOptions.make, abi.QlLocalBonds.make
    on = bonds((0.5, 0.7))
    for n, lmax, entries in ((0, 6, 0), (1, 0, 0), (108, 6, 1300), (256000, 6, 256000 * 12), (501, 12, 9000)):
        plain = lib.mtd_ql_local_scratch_doubles(n, lmax)
        rows = n * (lmax + 1) * (lmax + 2)
        for opt in (None, opts(), opts(switch=(0.25, 3)), opts(average=True), opts(average=True, switch=(0.12, 3), gate=(4, 8))):
            o = C.byref(opt) if opt is not None else None
            want = lib.mtd_ql_local_scratch_doubles_opt(n, lmax, entries, o)
            assert lib.mtd_ql_local_scratch_doubles_bonds(n, lmax, entries, o, None) == want
            assert lib.mtd_ql_local_scratch_doubles_bonds(n, lmax, entries, o, C.byref(bonds())) == want
        for opt in (None, opts(switch=(6.5, 12)), opts(switch=(6.5, 12), gate=(4, 8))):
            o = C.byref(opt) if opt is not None else None
            bd = lib.mtd_ql_local_scratch_doubles_bonds(n, lmax, entries, o, C.byref(on))
            # v_i, b_i, beta_i (and a_k), slot weights, one more table of rows and one double per list entry
            assert bd >= plain + 3 * n + rows + entries
            assert bd <= plain + 4 * n + rows + entries + (lmax + 1) * (lmax + 2) // 2 + 8
            assert bd % 2 == entries % 2                                          # everything before the entries keeps rows 16-byte aligned
            assert lib.mtd_ql_local_scratch_doubles_bonds(n, lmax, entries + 10, o, C.byref(on)) == bd + 10


def test_python_surface_of_the_bonds():
    """cv.steinhardt_local takes bonds as a fourth keyword-only argument of the call and has get_bonds; the host class has the setters"""
    import inspect
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    call = inspect.signature(type(cv.steinhardt_local).__call__).parameters
    assert [(n, call[n].default) for n in ("average", "switch", "gate", "bonds")] == [("average", False), ("switch", None), ("gate", None),
                                                                                      ("bonds", None)]
    assert all(call[n].kind == inspect.Parameter.KEYWORD_ONLY for n in ("average", "switch", "gate", "bonds"))
    assert list(inspect.signature(cv.steinhardt_local.set_options).parameters) == ["self", "average", "switch", "gate", "bonds"]
    for meth in ("get_bonds", "get_switched", "set_options", "get_local", "get_coordination"):
        assert hasattr(cv.steinhardt_local, meth), meth
    for meth in ("setBonds", "clearBonds", "getBondCounts"):
        assert hasattr(mod.SteinhardtLocal, meth), meth
