"""CPU: mtd_ql_local_forces_virial (the force pass of cv.steinhardt_local with the virial of the bias force beside it) is exported and
declared, refuses what mtd_ql_local_forces_opt refuses plus a virial pitch below the particle count, all before it touches a device,
and is reachable from the Python API.  Nothing here needs a GPU."""
import ctypes as C

import util

INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0


def test_symbol_exported_declared_and_registered(abi):
    lib = abi.load()
    assert "mtd_ql_local_forces_virial" in abi.declared_symbols()
    assert hasattr(lib, "mtd_ql_local_forces_virial")
    # the arguments of mtd_ql_local_forces_opt, then void *d_virial, unsigned int virial_pitch
    res, args = abi._SIGNATURES["mtd_ql_local_forces_virial"]
    res_opt, args_opt = abi._SIGNATURES["mtd_ql_local_forces_opt"]
    assert res is res_opt and args[:len(args_opt)] == args_opt and args[len(args_opt):] == [C.c_void_p, C.c_uint]


def _call(lib, abi, box, entry="virial", n=4, pos=1, force=1, head=1, nn=1, dtype=1, rcut=1.4, ron=1.2, lmax=6, ql=True, n_global=4, scratch=4096,
          opt=None, virial=1, pitch=4):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    ql_ref = util.dbl_array([0, 0, 0, 0, 1, 0, 1] + [0] * 6) if ql else None
    o = abi.QlLocalOptions.make(**opt) if isinstance(opt, dict) else opt
    args = (n, pos * 4096 or None, force * 4096 or None, dtype, C.byref(box) if box is not None else None, head * 4096 or None, nn * 4096 or None,
            4096, rcut, ron, lmax, 0, ql_ref, n_global, scratch or None, None, 0.5, None, C.byref(o) if o is not None else None)
    if entry == "opt":
        return lib.mtd_ql_local_forces_opt(*args)
    return lib.mtd_ql_local_forces_virial(*args, virial * 4096 or None, pitch)


REFUSED = [dict(pos=0), dict(force=0), dict(head=0), dict(nn=0), dict(ql=False), dict(scratch=0), dict(scratch=4096 + 8), dict(rcut=1.0, ron=1.2),
           dict(rcut=0.0, ron=0.0), dict(rcut=-1.0, ron=0.0), dict(rcut=float("nan")), dict(ron=-0.1), dict(dtype=7), dict(n_global=0),
           dict(lmax=13), dict(opt=dict(switch=(0.0, 3))), dict(opt=dict(switch=(0.1, 0))), dict(opt=dict(gate=(3.0, 3.0))),
           dict(opt=dict(gate=(-1.0, 3.0))), dict(opt=dict(gate=(float("nan"), 3.0)))]


def test_refuses_what_the_opt_entry_point_refuses(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _call(lib, abi, None) == INVALID and _call(lib, abi, None, entry="opt") == INVALID
    for kw in REFUSED:
        want = _call(lib, abi, box, entry="opt", **kw)
        assert want in (INVALID, UNSUPPORTED), kw
        assert _call(lib, abi, box, **kw) == want, kw                    # with a virial array
        assert _call(lib, abi, box, virial=0, pitch=0, **kw) == want, kw  # and without
    assert _call(lib, abi, box, lmax=13) == UNSUPPORTED


def test_pitch_below_the_particle_count_is_refused(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _call(lib, abi, box, n=4, pitch=3) == INVALID
    assert _call(lib, abi, box, n=4, pitch=0) == INVALID
    assert _call(lib, abi, box, n=1000, pitch=999, n_global=1000) == INVALID
    assert _call(lib, abi, box, n=4, pitch=3, opt=dict(average=True)) == INVALID
    assert _call(lib, abi, box, n=4, pitch=3, dtype=0) == INVALID


def test_no_particles_is_success(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _call(lib, abi, box, n=0, pitch=0) == SUCCESS
    assert _call(lib, abi, box, n=0, pitch=0, virial=0) == SUCCESS
    assert _call(lib, abi, box, n=0, pitch=0, pos=0, force=0, head=0, nn=0) == SUCCESS
    assert _call(lib, abi, box, n=0, entry="opt") == SUCCESS


def test_python_surface():
    from metadynamics import cv
    assert hasattr(cv.steinhardt_local, "get_virial")
