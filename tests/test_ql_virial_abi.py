"""CPU: mtd_ql_forces_virial (the force pass of cv.steinhardt with the virial of the bias force beside it) is exported, declared and
registered, refuses what mtd_ql_forces refuses with the same codes plus a virial pitch below the particle count and the third-law pass of
a half list, all before it touches a device, and is reachable from the Python API.  Nothing here needs a GPU."""
import ctypes as C

import util

INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0


def test_symbol_exported_declared_and_registered(abi):
    lib = abi.load()
    assert "mtd_ql_forces_virial" in abi.declared_symbols()
    assert hasattr(lib, "mtd_ql_forces_virial")
    # the arguments of mtd_ql_forces, then void *d_virial, unsigned int virial_pitch
    res, args = abi._SIGNATURES["mtd_ql_forces_virial"]
    res_f, args_f = abi._SIGNATURES["mtd_ql_forces"]
    assert res is res_f and args[:len(args_f)] == args_f and args[len(args_f):] == [C.c_void_p, C.c_uint]


def _call(lib, abi, box, entry="virial", n=4, pos=1, force=1, head=1, nn=1, dtype=1, mode=0, rcut=1.4, ron=1.2, lmax=6, ql=True, n_global=4,
          scratch=4096, virial=1, pitch=4):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    ql_ref = util.dbl_array([0, 0, 0, 0, 1, 0, 1] + [0] * 6) if ql else None
    args = (n, pos * 4096 or None, force * 4096 or None, dtype, C.byref(box) if box is not None else None, head * 4096 or None, nn * 4096 or None,
            4096, mode, rcut, ron, lmax, 0, ql_ref, n_global, scratch or None, None, 0.5, None)
    if entry == "forces":
        return lib.mtd_ql_forces(*args)
    return lib.mtd_ql_forces_virial(*args, virial * 4096 or None, pitch)


REFUSED = [dict(pos=0), dict(force=0), dict(head=0), dict(nn=0), dict(ql=False), dict(scratch=0), dict(rcut=1.0, ron=1.2), dict(rcut=0.0, ron=0.0),
           dict(rcut=-1.0, ron=0.0), dict(rcut=float("nan")), dict(ron=-0.1), dict(dtype=7), dict(n_global=0), dict(lmax=13)]


def test_refuses_what_the_force_entry_point_refuses(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _call(lib, abi, None) == INVALID and _call(lib, abi, None, entry="forces") == INVALID
    refused = 0
    for mode in (0, 1, 2):
        for kw in REFUSED:
            want = _call(lib, abi, box, entry="forces", mode=mode, **kw)
            assert want in (INVALID, UNSUPPORTED), (mode, kw)
            assert _call(lib, abi, box, mode=mode, virial=0, pitch=0, **kw) == want, (mode, kw)      # without a virial array
            assert _call(lib, abi, box, mode=mode, **kw) == want, (mode, kw)                         # and with one (mode 1: the argument's code comes first)
            refused += 1
    assert refused == 3 * len(REFUSED)
    assert _call(lib, abi, box, lmax=13) == UNSUPPORTED and _call(lib, abi, box, entry="forces", lmax=13) == UNSUPPORTED


def test_pitch_below_the_particle_count_is_refused(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _call(lib, abi, box, n=4, pitch=3) == INVALID
    assert _call(lib, abi, box, n=4, pitch=0) == INVALID
    assert _call(lib, abi, box, n=1000, pitch=999, n_global=1000) == INVALID
    assert _call(lib, abi, box, n=4, pitch=3, mode=2) == INVALID
    assert _call(lib, abi, box, n=4, pitch=3, dtype=0) == INVALID


def test_third_law_pass_with_a_virial_array_is_unsupported(abi):
    """half_nlist == 1 with a virial array: MTD_ERR_UNSUPPORTED before the device is touched (every pointer here is a dummy); without one
    the call is mtd_ql_forces and passes the same validation — seen on the device-free path, n = 0"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _call(lib, abi, box, mode=1) == UNSUPPORTED
    assert _call(lib, abi, box, mode=1, pitch=100) == UNSUPPORTED
    assert _call(lib, abi, box, mode=1, dtype=0) == UNSUPPORTED
    assert _call(lib, abi, box, mode=1, n=0, virial=0, pitch=0) == SUCCESS
    assert _call(lib, abi, box, mode=1, n=0, entry="forces") == SUCCESS


def test_no_particles_is_success(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    for mode in (0, 2):
        assert _call(lib, abi, box, n=0, pitch=0, mode=mode) == SUCCESS
        assert _call(lib, abi, box, n=0, pitch=0, virial=0, mode=mode) == SUCCESS
        assert _call(lib, abi, box, n=0, pitch=0, pos=0, force=0, head=0, nn=0, mode=mode) == SUCCESS
        assert _call(lib, abi, box, n=0, entry="forces", mode=mode) == SUCCESS


def test_python_surface():
    from metadynamics import cv
    assert hasattr(cv.steinhardt, "get_virial")
