"""GPU parity ON and NEXT TO the z axis: every entry point whose force pass goes through ql_pair_force (steinhardt_device.hpp) on
crystals whose columns put hundreds of bonds exactly on the axis of the box (util.columns: bcc_columns with 256 of 1792 entries,
sc_columns with 250 of 752) and on the same crystals with the columns bent by 1e-14 ... 1e-2 (util.near_axis), against the fp64
restatements evaluated in a ROTATED frame (frame=, checked on the CPU in tests/test_ql_axis_ref.py): in the lab frame the
restatements divide by sin(theta) and return NaN there, as the kernels did before the pair gradient was written without 1 / rho.

Bounds are the project's own, none is new:
    forces                      1e-5 of max|F| (BASELINE.json; tests/test_gpu_ql_local.py, test_ql_local_config5_size)
    c_i, n_i, v_i, b_i          1e-11 of their largest value; s 1e-10 relative   (the parity asserts of the file of each variable)
    per-particle virial         1e-9 of max|virial_i| with fp64 arrays, 2e-7 with fp32 arrays; its six sums 1e-9 of max|W| in fp64
    sum of the forces           1e-4 max|F| sqrt(N)                              (tests/test_gpu_ql_local.py, symmetric lists)
and every force and virial entry is finite.  Each case prints its number of on-axis entries and the errors it measured.

Which force kernel of the local variable a case runs (rows of rs16 = 1 + sum over the active degrees of (l + 1) slots of 16 bytes;
k_qll_forces_tile up to QLL_TILE_MAX16 = 16 slots, k_qll_forces beyond) is stated at LOCAL_CASES."""
import ctypes as C

import numpy as np
import pytest

import ql_local_avg_ref as avg_ref
import ql_local_bonds_ref as bonds_ref
import ql_local_ref as loc_ref
import ql_local_virial_ref as lvir_ref
import ql_virial_ref as gvir_ref
import util
from test_gpu_ql_local import run_gpu as run_local
from test_gpu_ql_local_avg import run_gpu as run_opt
from test_gpu_ql_local_bonds import run_gpu as run_bonds
from test_gpu_ql_local_virial import run_gpu as run_lvir
from test_gpu_ql_virial import run_gpu as run_global
from test_gpu_ql_virial import symmetrize

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

BIAS = 0.9
FRAME = util.random_rotation(1)
QL_46 = [0, 0, 0, 0, 1, 0, 1]
E6 = [0, 0, 0, 0, 0, 0, 1]
DTYPES = [np.float64, np.float32]
SNAPS = sorted(util.COLUMNS)

# (lmax, Ql_ref, slots of a row, kernel): every compiled bound of dispatch_lmax (4, 6, 8, 12), each with the sets of the issue, and further
# sets so that every bound that can reach both kernels does (lmax 4 holds 15 slots at most: the tile form only)
LOCAL_CASES = [
    (4, [0, 0, 0, 0, 1], 6, "tile"),
    (6, QL_46, 13, "tile"),
    (6, [0, 0.4, 0.2, 0.6, 1, 0.7, 1], 28, "row"),
    (8, [0, 0, 0, 0, 0, 0, 0, 0, 1], 10, "tile"),
    (8, [0, 0, 0, 0, 0, 0, 1, 0, 1], 17, "row"),
    (12, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], 14, "tile"),
    (12, [0.5, 0.3, 0.2, 0.4, 1, 0.7, 1, 0.6, 0.5, 0.3, 0.5, 0.3, 0.25], 91, "row"),
]


def slots(Ql_ref):
    return 1 + sum(l + 1 for l, w in enumerate(Ql_ref) if w != 0.0 and l > 0)


_cases = {}


def snapshot(name, dtype, near=False):
    """(case, n_on) built once per name and dtype: util.columns or util.near_axis, positions rounded to the dtype"""
    key = (name, np.dtype(dtype).name, near)
    if key not in _cases:
        _cases[key] = (util.near_axis if near else util.columns)(name, dtype=dtype)
    return _cases[key]


_refs = {}


def reference(key, fn):
    """a restatement's answer, computed once per key and left unchanged"""
    if key not in _refs:
        _refs[key] = fn()
    return _refs[key]


def geometry(case):
    return case["pos"], case["types"], case["L"], case["nl"], case["r_cut"], case["r_on"]


def check_forces(label, n_on, F, F_ref):
    """F (N, 4) as stored against F_ref (N, 3): finite, 1e-5 of max|F|, w == 0, sum 0"""
    F = np.asarray(F, dtype=np.float64)
    N = len(F)
    fs = np.abs(F_ref).max()
    assert np.isfinite(F).all(), "%s: %d of %d force entries are not finite" % (label, (~np.isfinite(F)).sum(), F.size)
    err = np.abs(F[:, :3] - F_ref).max() / fs
    total = np.abs(F[:, :3].sum(axis=0)).max()
    print("%s: %d entries on the axis; forces %.3e of max|F| %.4g; |sum F| %.3e" % (label, n_on, err, fs, total))
    assert fs > 0
    assert err <= 1e-5
    assert np.all(F[:, 3] == 0.0)
    assert total <= 1e-4 * fs * np.sqrt(N)


def check_virial(label, raw, r_virial, r_W, dtype):
    """raw (6, pitch) as stored against the restatement's (N, 6) and its six sums"""
    N = len(r_virial)
    vg = np.asarray(raw, dtype=np.float64)[:, :N].T
    assert np.isfinite(vg).all(), "%s: %d virial entries are not finite" % (label, (~np.isfinite(vg)).sum())
    top, w_top = np.abs(r_virial).max(), np.abs(r_W).max()
    err, w_err = np.abs(vg - r_virial).max() / top, np.abs(vg.sum(axis=0) - r_W).max() / w_top
    print("%s: virial %.3e of max|virial_i| %.4g; sums %.3e of max|W| %.4g" % (label, err, top, w_err, w_top))
    assert top > 0 and w_top > 0
    assert err <= (1e-9 if dtype == np.float64 else 2e-7)
    if dtype == np.float64:
        assert w_err <= 1e-9


def check_values(label, g, r, keys):
    for k in keys:
        assert np.isfinite(g[k]).all(), (label, k)
        err, top = np.abs(g[k] - r[k]).max(), np.abs(r[k]).max()
        print("%s: %s_i %.3e of %.4g" % (label, k, err, top))
        assert err <= 1e-11 * top, (label, k)
    assert g["s"] == pytest.approx(r["s"], rel=1e-10)


# ---- 1. mtd_ql_local_accumulate + mtd_ql_local_forces: every compiled bound, both force kernels ---------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("snap", SNAPS)
@pytest.mark.parametrize("lmax,Ql_ref,n_slots,kernel", LOCAL_CASES, ids=["lmax%d-%dslots-%s" % (c[0], c[2], c[3]) for c in LOCAL_CASES])
def test_local_forces_on_the_axis(abi, dtype, snap, lmax, Ql_ref, n_slots, kernel):
    assert slots(Ql_ref) == n_slots and (n_slots <= 16) == (kernel == "tile")
    case, n_on = snapshot(snap, dtype)
    label = "%s %s lmax %d (%s)" % (snap, np.dtype(dtype).name, lmax, kernel)
    g = run_local(abi, *geometry(case), lmax, 0, Ql_ref, dtype, bias=BIAS)
    r = reference(("local", snap, np.dtype(dtype).name, lmax, n_slots),
                  lambda: loc_ref.compute(**case, lmax=lmax, Ql_ref=Ql_ref, frame=FRAME))
    check_values(label, g, r, ("c", "n"))
    check_forces(label, n_on, g["F"], -BIAS * r["grad"])


# ---- 2. the options, each against its own restatement ------------------------------------------------------------------------------------

OPTIONS = {
    "switch": dict(switch=(0.5, 3)),                                   # c_i is about 0.26 on bcc: the switch is not saturated
    "gate": dict(gate=(12.5, 14.5)),                                   # n_i: 14 neighbours, the second shell inside the smoothing: on the ramp
    "average": dict(average=True),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_local_options_on_the_axis(abi, dtype, name):
    case, n_on = snapshot("bcc_columns", dtype)
    opt = OPTIONS[name]
    label = "bcc_columns %s %s" % (np.dtype(dtype).name, name)
    g = run_opt(abi, *geometry(case), 6, 0, QL_46, dtype, opt=opt, bias=BIAS)
    r = reference(("opt", np.dtype(dtype).name, name), lambda: avg_ref.compute(**case, lmax=6, Ql_ref=QL_46, frame=FRAME, **opt))
    if name == "gate":
        assert ((r["n"] > 12.5) & (r["n"] < 14.5)).sum() > 64               # the ramp is populated
    check_values(label, g, r, ("c", "n", "v"))
    check_forces(label, n_on, g["F"], -BIAS * r["grad"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_local_bonds_on_the_axis(abi, dtype):
    """bonds=(0.5, 0.7) with a switch: value, b_i, forces (with and without the virial: the same bits) and the virial"""
    case, n_on = snapshot("bcc_columns", dtype)
    opt = dict(bonds=(0.5, 0.7), switch=(6.5, 6))
    label = "bcc_columns %s bonds" % np.dtype(dtype).name
    g = run_bonds(abi, *geometry(case), 6, 0, E6, dtype, opt=opt, bias=BIAS)
    r = reference(("bonds", np.dtype(dtype).name), lambda: bonds_ref.compute(**case, lmax=6, Ql_ref=E6, bias=BIAS, frame=FRAME, **opt))
    check_values(label, g, r, ("c", "n", "b", "v"))
    check_forces(label, n_on, g["F"], -BIAS * r["grad"])
    check_virial(label, g["raw"], r["virial"], r["W"], dtype)
    assert np.array_equal(g["F"], g["F_vir"])


# ---- 3. the virial variants: per-particle virial and its sums; forces bit-equal to the call without the virial ------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("snap", SNAPS)
@pytest.mark.parametrize("average", [False, True], ids=["plain", "average"])
def test_local_virial_on_the_axis(abi, dtype, snap, average):
    case, n_on = snapshot(snap, dtype)
    opt = dict(average=True, switch=(0.5, 3)) if average else dict()
    label = "%s %s local virial%s" % (snap, np.dtype(dtype).name, " average+switch" if average else "")
    g = run_lvir(abi, *geometry(case), 6, 0, QL_46, dtype, opt=opt, bias=BIAS)
    r = reference(("lvir", snap, np.dtype(dtype).name, average),
                  lambda: lvir_ref.compute(**case, lmax=6, Ql_ref=QL_46, bias=BIAS, frame=FRAME, **opt))
    check_forces(label, n_on, g["F"], -BIAS * r["grad"])
    check_virial(label, g["raw"], r["virial"], r["W"], dtype)
    assert np.array_equal(g["F"], g["F_opt"])


def global_reference(ref, key, case, lmax, Ql_ref, half):
    """the restatement of the global variable in FRAME with the oracle's Q_lm; nl: the list the oracle reads"""
    def run():
        kw = dict(case, lmax=lmax, Ql_ref=Ql_ref, half=half)
        return gvir_ref.compute(**kw, Qlm=gvir_ref.oracle_cv(ref, **kw)[1], bias=BIAS, frame=FRAME)
    return reference(("global",) + key, run)


GLOBAL_DEGREES = {4: [0.2, 0, 1.0, 0.5, 1.0], 6: QL_46, 12: [0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0.5, 0.3, 0.25]}   # 4 and 12: odd and even degrees


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("snap", SNAPS)
@pytest.mark.parametrize("lmax", sorted(GLOBAL_DEGREES))
def test_global_forces_and_virial_full_list(abi, ref, dtype, snap, lmax):
    """mtd_ql_forces and mtd_ql_forces_virial, half_nlist 0"""
    case, n_on = snapshot(snap, dtype)
    label = "%s %s global lmax %d full list" % (snap, np.dtype(dtype).name, lmax)
    pos, types, L, nl, r_cut, r_on = geometry(case)
    g = run_global(abi, pos, types, L, nl, lmax, GLOBAL_DEGREES[lmax], dtype, mode=0, rcut=r_cut, ron=r_on, bias=BIAS)
    r = global_reference(ref, (snap, np.dtype(dtype).name, lmax, False), case, lmax, GLOBAL_DEGREES[lmax], False)
    check_forces(label, n_on, g["F_plain"], r["F"])
    check_virial(label, g["raw"], r["virial"], r["W"], dtype)
    assert np.array_equal(g["F"], g["F_plain"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("snap", SNAPS)
@pytest.mark.parametrize("mode", [2, 1], ids=["symmetrised", "third-law"])
def test_global_forces_half_list(abi, ref, dtype, snap, mode):
    """a half list through mtd_ql_symmetrize_half_list (mode 2, with the virial) and through the third-law pass (half_nlist 1, which
    takes no virial array)"""
    case, n_on = snapshot(snap, dtype)
    label = "%s %s global %s" % (snap, np.dtype(dtype).name, "mode 2" if mode == 2 else "half list")
    pos, types, L, nl, r_cut, r_on = geometry(case)
    half = util.build_nlist(pos, L, util.COLUMNS_R_LIST, half=True)
    lst = symmetrize(abi, len(pos), half) if mode == 2 else half
    g = run_global(abi, pos, types, L, lst, 6, QL_46, dtype, mode=mode, rcut=r_cut, ron=r_on, bias=BIAS, pass_virial=mode == 2)
    r = global_reference(ref, (snap, np.dtype(dtype).name, 6, True), dict(case, nl=half), 6, QL_46, True)
    on, _ = util.axis_entries(pos, L, half, r_cut)
    assert 2 * int(on.sum()) == n_on                                      # every on-axis pair once in the half list
    check_forces(label, n_on if mode == 2 else n_on // 2, g["F_plain"], r["F"])
    assert np.array_equal(g["F"], g["F_plain"])
    if mode == 2:
        check_virial(label, g["raw"], r["virial"], r["W"], dtype)


# ---- 4. next to the axis: the same bounds over the whole range of offsets ------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("snap", SNAPS)
@pytest.mark.parametrize("variable", ["local", "local-average", "global"])
def test_near_the_axis(abi, ref, dtype, snap, variable):
    """bonds from exactly on the axis (a quarter of the columns) through 1e-14 (fp32: one ulp of the coordinate) to 1e-2 off it: a form
    that changes at some small rho has to be right on both sides of the change"""
    case, n_on = snapshot(snap, dtype, near=True)
    label = "near_axis(%s) %s %s" % (snap, np.dtype(dtype).name, variable)
    pos, types, L, nl, r_cut, r_on = geometry(case)
    key = (snap, np.dtype(dtype).name, variable, "near")
    if variable == "global":
        g = run_global(abi, pos, types, L, nl, 6, QL_46, dtype, mode=0, rcut=r_cut, ron=r_on, bias=BIAS)
        r = global_reference(ref, key, case, 6, QL_46, False)
        check_forces(label, n_on, g["F_plain"], r["F"])
        check_virial(label, g["raw"], r["virial"], r["W"], dtype)
        return
    opt = dict(average=True) if variable == "local-average" else dict()
    g = run_opt(abi, *geometry(case), 6, 0, QL_46, dtype, opt=opt, bias=BIAS)
    r = reference(key, lambda: avg_ref.compute(**case, lmax=6, Ql_ref=QL_46, frame=FRAME, **opt))
    check_values(label, g, r, ("c", "n", "v"))
    check_forces(label, n_on, g["F"], -BIAS * r["grad"])


# ---- 5. through the host classes -----------------------------------------------------------------------------------------------------------

@pytest.fixture()
def api():
    from metadynamics import context, cv, integrate
    yield context, cv, integrate
    context.current = None


KAPPA = 35.0


def perfect_bcc():
    """the crystal bcc_columns is built from, without its noise: every particle an inversion centre, 256 entries on the axis"""
    n, basis, _ = util.COLUMNS["bcc_columns"]
    cells = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    pos = (cells[:, None, :] + np.asarray(basis)[None, :, :]).reshape(-1, 3) - n / 2 + 0.25
    return dict(pos=pos, types=np.zeros(len(pos), dtype=np.int32), L=float(n), nl=util.build_nlist(pos, float(n), util.COLUMNS_R_LIST),
                r_cut=util.COLUMNS_R_CUT, r_on=util.COLUMNS_R_ON, type_id=0)


def _host_run(api, case, which, val):
    """2 steps with cv.nlist_cell(device=True) under a harmonic umbrella (a bias factor of order kappa val, whatever the grid holds);
    returns (force array, the total bias factor: the integrator's own plus the umbrella's at the value it reports)"""
    context, cv, integrate = api
    context.initialize(case["pos"], case["types"], ["A"], case["L"], dtype=np.float64)
    meta = integrate.mode_metadynamics(dt=0.005, stride=1, mode="well_tempered", W=1.0, deltaT=7.0, T=1.0)
    nl = cv.nlist_cell(r_cut=util.COLUMNS_R_LIST, r_buff=0.4, device=True)      # r_list 1.75 < L / 2; entries beyond r_cut are skipped
    make = cv.steinhardt_local if which == "local" else cv.steinhardt
    st = make(r_cut=case["r_cut"], r_on=case["r_on"], lmax=6, Ql_ref=QL_46, nlist=nl, type="A", sigma=0.02 * val)
    st.set_grid(0.55 * val, 1.3 * val, 512)
    cv0 = 0.8 * val
    st.set_params(umbrella="harmonic", kappa=KAPPA, cv0=cv0)
    context.run(2)
    s = meta.cpp_integrator.getCurrentValues()[0]
    assert s == pytest.approx(val, rel=1e-10)
    total = meta.cpp_integrator.getBiasFactors()[0] + KAPPA * (s - cv0)
    assert abs(KAPPA * (s - cv0)) > 0.1 * abs(total)
    F = np.array(st.cpp_force.getForceArray())
    context.current = None
    return F, total


@pytest.mark.parametrize("which", ["local", "global"])
def test_host_classes_start_from_a_crystal(api, ref, which):
    """cv.steinhardt_local and cv.steinhardt: a perfect bcc crystal (forces finite and zero), then bcc_columns (forces equal to the
    restatement at the bias factor the integrator reports)"""
    noisy, n_on = snapshot("bcc_columns", np.float64)

    def answer(case, bias):
        kw = dict(case, lmax=6, Ql_ref=QL_46)
        if which == "local":
            r = loc_ref.compute(**kw, frame=FRAME)
            return r["s"], -bias * r["grad"]
        s, Qlm = gvir_ref.oracle_cv(ref, **kw)
        return s, gvir_ref.compute(**kw, Qlm=Qlm, bias=bias, frame=FRAME)["F"]

    perfect = perfect_bcc()
    on, _ = util.axis_entries(perfect["pos"], perfect["L"], perfect["nl"], perfect["r_cut"])
    assert int(on.sum()) == 256
    val, _ = answer(perfect, 1.0)
    F, total = _host_run(api, perfect, which, val)
    scale = abs(total) * np.abs(answer(noisy, 1.0)[1]).max()                 # max|F| of the noisy crystal at this bias factor
    assert np.isfinite(F).all(), "perfect bcc: %d force entries are not finite" % (~np.isfinite(F)).sum()
    print("cv.steinhardt%s, perfect bcc: max|F| %.3e against %.4g of the noisy crystal" % ("_local" if which == "local" else "", np.abs(F).max(), scale))
    assert scale > 0 and np.abs(F).max() <= 1e-5 * scale

    val, _ = answer(noisy, 1.0)
    F, total = _host_run(api, noisy, which, val)
    check_forces("cv.steinhardt%s, bcc_columns" % ("_local" if which == "local" else ""), n_on, F, answer(noisy, total)[1])
