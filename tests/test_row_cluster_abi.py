"""CPU: the largest-cluster entry points of the coordination number and the tetrahedral order (mtd_coord_accumulate_cluster,
mtd_tetrahedral_accumulate_cluster) are exported, declared and registered, take no bare stream, refuse what they do not take before they
touch a device, and are reachable from the host classes and the Python API.  Nothing here needs a GPU: every pointer is a small non-null
value that is never dereferenced when the arguments are refused."""
import ctypes as C
import os
import re

import pytest

INVALID, UNSUPPORTED = -1, -2
NAN, INF = float("nan"), float("inf")
SYMBOLS = ("mtd_coord_accumulate_cluster", "mtd_tetrahedral_accumulate_cluster")


def _header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mtd_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    text = _header()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
        args = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % s, text, flags=re.S).group(1)
        assert "mtd_stream_t" not in args                               # the stream stays inside the call block
        assert len(args.split(",")) == 9 == len(abi._SIGNATURES[s][1])
        assert "mtd_cluster_params" in args.split(",")[2]
    # the existing entry points and structures keep their shape
    assert len(abi._SIGNATURES["mtd_coord_accumulate"][1]) == 4 and len(abi._SIGNATURES["mtd_tet_accumulate"][1]) == 4
    assert C.sizeof(abi.CoordParams) == 64 and C.sizeof(abi.RowCall) == 72 and abi.RowCall.stream.offset == 64


def _call(abi, box, n_particles=4, n_ghost=0, nl=1, scratch=4096, dtype=1, **_):
    return abi.RowCall(n_particles, n_ghost, 4096 if n_particles else None, dtype, C.pointer(box), 4096 if n_particles else None,
                       4096 if n_particles else None, nl * 4096 or None, scratch or None, None)


def _cluster(abi, cluster=(0.3, 1.2), on=None, no_cluster=False, **_):
    if no_cluster:
        return None
    p = abi.ClusterParams.make(cluster)
    if on is not None:
        p.on = on
    return p


def _coord(lib, abi, box, switch=(6.0, 8), cscratch=8192, plain=False, **kw):
    par = abi.CoordParams.make(0, 1, kw.get("r_0", 1.2), 1.5, n=kw.get("n", 6), m=kw.get("m", 12), switch=switch)
    call, cl = _call(abi, box, **kw), _cluster(abi, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    if plain:
        return lib.mtd_coord_accumulate(C.byref(par), C.byref(call), C.byref(sums), C.byref(n_sums))
    outs = [C.c_void_p() for _ in range(3)]
    return lib.mtd_coord_accumulate_cluster(C.byref(par), C.byref(call), C.byref(cl) if cl is not None else None, cscratch or None, C.byref(sums),
                                            C.byref(n_sums), *[C.byref(o) for o in outs])


def _tet(lib, abi, box, normalise=True, switch=None, gate=None, cscratch=8192, plain=False, **kw):
    par = abi.TetParams.make(0, kw.get("r_cut", 1.4), 1.2, normalise=normalise, switch=switch, gate=gate)
    call, cl = _call(abi, box, **kw), _cluster(abi, **kw)
    sums, n_sums = C.c_void_p(), C.c_uint()
    if plain:
        return lib.mtd_tet_accumulate(C.byref(par), C.byref(call), C.byref(sums), C.byref(n_sums))
    outs = [C.c_void_p() for _ in range(3)]
    return lib.mtd_tetrahedral_accumulate_cluster(C.byref(par), C.byref(call), C.byref(cl) if cl is not None else None, cscratch or None,
                                                  C.byref(sums), C.byref(n_sums), *[C.byref(o) for o in outs])


CLUSTER_INVALID = [dict(cluster=(0.3, 0.0)), dict(cluster=(0.3, -1.0)), dict(cluster=(0.3, NAN)), dict(cluster=(0.3, INF)),
                   dict(cluster=(NAN, 1.2)), dict(cluster=(INF, 1.2)), dict(cluster=(-INF, 1.2)),
                   dict(cscratch=0), dict(cscratch=8192 + 8), dict(nl=0)]


@pytest.mark.parametrize("call", [_coord, _tet], ids=["coordination", "tetrahedral"])
def test_refusals_without_gpu(abi, call):
    """everything cluster_refuse refuses, a NULL or misaligned cluster scratch, no list with particles: MTD_ERR_INVALID_ARGUMENT; ghosts:
    MTD_ERR_UNSUPPORTED; the variable's own refusals as they were, with the option on or off; an invalid argument beside an unsupported one
    is invalid — all before a device is touched"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    for kw in CLUSTER_INVALID:
        assert call(lib, abi, box, **kw) == INVALID, kw
        assert call(lib, abi, box, n_ghost=2, **kw) == INVALID, kw      # ahead of what is merely not built
    assert call(lib, abi, box, n_ghost=1) == UNSUPPORTED
    # the plain accumulate's refusals stay: a misaligned or missing scratch, an unknown dtype, with the option on and off
    for kw in (dict(scratch=0), dict(scratch=4096 + 8), dict(dtype=7)):
        for off in (dict(), dict(on=0), dict(no_cluster=True)):
            assert call(lib, abi, box, **kw, **off) == INVALID, (kw, off)
            assert call(lib, abi, box, plain=True, **kw) == INVALID
    # off is not looked at: a bad r_link, no cluster scratch and no list are the plain call's business, which does not read them
    for off in (dict(on=0), dict(no_cluster=True)):
        plain = call(lib, abi, box, n_particles=0, plain=True)
        assert call(lib, abi, box, n_particles=0, cluster=(NAN, -1.0), cscratch=0, nl=0, **off) == plain
        assert call(lib, abi, box, n_particles=0, n_ghost=0, **off) == plain


def test_coordination_refusals_of_its_own(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _coord(lib, abi, box, switch=None) == UNSUPPORTED            # the plain route stores summed gradients: nothing to mask
    assert _coord(lib, abi, box, switch=None, n_ghost=2) == UNSUPPORTED
    assert _coord(lib, abi, box, switch=None, cluster=(0.3, NAN)) == INVALID
    assert _coord(lib, abi, box, switch=None, cscratch=0) == INVALID
    assert _coord(lib, abi, box, m=33) == UNSUPPORTED and _coord(lib, abi, box, m=33, cscratch=8) == INVALID
    assert _coord(lib, abi, box, r_0=NAN) == INVALID and _coord(lib, abi, box, switch=(NAN, 8)) == INVALID
    # accepted at n_particles == 0 with the option off: the call gets past every refusal (what it returns then is the device's answer)
    for off in (dict(on=0), dict(no_cluster=True)):
        for switch in (None, (6.0, 8)):
            rc = _coord(lib, abi, box, n_particles=0, switch=switch, cscratch=0, **off)
            assert rc not in (INVALID, UNSUPPORTED) and rc == _coord(lib, abi, box, n_particles=0, switch=switch, plain=True)


def test_tetrahedral_refusals_of_its_own(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    assert _tet(lib, abi, box, normalise=False) == INVALID              # A_i is a penalty, not an order
    assert _tet(lib, abi, box, normalise=False, n_ghost=2) == INVALID
    assert _tet(lib, abi, box, normalise=False, on=0, n_ghost=2) == UNSUPPORTED      # off: the plain call's answer
    assert _tet(lib, abi, box, normalise=False, switch=(0.5, 6)) == INVALID
    assert _tet(lib, abi, box, r_cut=NAN) == INVALID and _tet(lib, abi, box, gate=(0.5, 3.0)) == INVALID
    for kw in (dict(switch=(0.7, 8)), dict(switch=(0.7, 8), gate=(1.5, 3.0))):
        assert _tet(lib, abi, box, n_ghost=1, **kw) == UNSUPPORTED
        assert _tet(lib, abi, box, cscratch=8192 + 4, **kw) == INVALID


class _Recorder(object):
    """stands in for the host object: records what set_cluster hands on"""

    def __init__(self, refuse=False):
        self.calls, self.refuse = [], refuse

    def setCluster(self, v_min, r_link):
        if self.refuse:
            raise RuntimeError("cv.x: the neighbour list must reach r_link")
        self.calls.append(("set", v_min, r_link))

    def clearCluster(self):
        self.calls.append(("clear",))


@pytest.mark.parametrize("name", ["coordination", "tetrahedral"])
def test_python_surface(name):
    from metadynamics import cv
    cls = getattr(cv, name)
    for meth in ("set_cluster", "get_cluster_mask", "get_cluster_labels", "get_largest_cluster"):
        assert hasattr(cls, meth), meth
        assert getattr(cls, meth).__doc__
    assert cls.get_cluster_mask.__doc__ == cv.steinhardt_local.get_cluster_mask.__doc__
    assert cls.get_cluster_labels.__doc__ == cv.steinhardt_local.get_cluster_labels.__doc__
    assert cls.get_largest_cluster.__doc__ == cv.steinhardt_local.get_largest_cluster.__doc__
    assert type(cls) is type                                            # no metaclass: the option is a method, not a keyword of the call
    for word in ("set_cluster", "JUMPS", "Single-domain", "unmasked"):
        assert word in cls.__doc__, word
    if name == "coordination":
        assert "Needs a switch" in cls.__doc__
    obj = object.__new__(cls)
    obj.cpp_force = _Recorder()
    obj.set_cluster(dict(v_min=0.25, r_link=1.2))
    obj.set_cluster(dict(v_min=-1, r_link=2))
    obj.set_cluster(None)
    assert obj.cpp_force.calls == [("set", 0.25, 1.2), ("set", -1.0, 2.0), ("clear",)]
    obj.cpp_force.calls.clear()
    bad = [dict(v_min=0.25), dict(r_link=1.2), dict(v_min=0.25, r_link=1.2, extra=1), dict(v_min=NAN, r_link=1.2), dict(v_min=INF, r_link=1.2),
           dict(v_min=0.25, r_link=0.0), dict(v_min=0.25, r_link=-1.0), dict(v_min=0.25, r_link=INF), dict(v_min=0.25, r_link=NAN),
           dict(v_min="a", r_link=1.2), (0.25, 1.2), 0.25, True]
    for cluster in bad:
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            obj.set_cluster(cluster)
    assert obj.cpp_force.calls == []                                    # a refused call leaves the option as it was
    obj.cpp_force = _Recorder(refuse=True)
    with pytest.raises(RuntimeError, match="Error creating collective variable."):
        obj.set_cluster(dict(v_min=0.25, r_link=1.2))


def test_pybind_surface():
    from metadynamics import _metadynamics as mod
    for cls in (mod.CoordinationNumber, mod.TetrahedralOrder):
        for meth in ("setCluster", "clearCluster", "getClusterLabels", "getClusterMask", "getLargestCluster"):
            assert hasattr(cls, meth), (cls.__name__, meth)
