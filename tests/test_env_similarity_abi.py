"""CPU: the environment similarity (mtd_es_*, csrc/env_similarity.hip) is exported, declared and registered, refuses bad arguments before
it touches a device, and is reachable from the host classes and the Python API.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import re
import types

import numpy as np
import pytest

ES_SYMBOLS = ("mtd_es_scratch_doubles", "mtd_es_accumulate", "mtd_es_forces")
INVALID, UNSUPPORTED, SUCCESS = -1, -2, 0
FCC = [[0.5 * x for x in t] for t in ((1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (1, 0, 1), (1, 0, -1), (-1, 0, 1), (-1, 0, -1),
                                      (0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1))]       # length 1 / sqrt(2)


def test_symbols_exported_declared_and_registered(abi):
    lib = abi.load()
    declared = abi.declared_symbols()
    for s in ES_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in abi._SIGNATURES, s
    assert abi._SIGNATURES["mtd_es_forces"][1][-2:] == [C.c_void_p, C.c_uint]      # void *d_virial, unsigned int virial_pitch
    assert len(abi._SIGNATURES["mtd_es_accumulate"][1]) == 18 and len(abi._SIGNATURES["mtd_es_forces"][1]) == 18


def test_params_struct_matches_the_header(abi):
    """the field list of mtd_es_params in include/mtd_abi.h, in order, against the ctypes structure; capacities 4 and 64"""
    text = open(abi.HEADER_PATH).read()
    assert re.search(r"#define MTD_ES_MAX_ENV 4\b", text) and re.search(r"#define MTD_ES_MAX_VEC 64\b", text)
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*mtd_es_params;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\w+\])*\s*[,;]", body)            # every declarator: the word in front of its dimensions and , or ;
    assert names == ["n_env", "n_vec", "vec", "sigma_env", "r_on", "r_cut", "lambda", "switch_on", "c0", "p"]
    assert [f[0] for f in abi.EsParams._fields_] == [n if n != "lambda" else "lam" for n in names]
    # unsigned n_env + unsigned n_vec[4] (20 bytes, padded to 24) | double vec[64][3] | 4 doubles | int (padded) | double | unsigned (padded)
    assert C.sizeof(abi.EsParams) == 24 + 64 * 3 * 8 + 4 * 8 + 8 + 8 + 8
    assert abi.MTD_ES_MAX_ENV == 4 and abi.MTD_ES_MAX_VEC == 64


def test_scratch_size(abi):
    lib = abi.load()
    for n in (0, 1, 500, 256000):
        d = lib.mtd_es_scratch_doubles(n)
        assert d >= 10 * n + 1 and d % 2 == 0          # k^e [4], beta^e [4], k, v per particle, and block sums


def _params(abi, templates=None, sigma_env=0.12, r_on=1.3, r_cut=1.5, lam=100.0, switch=None, n_env=None, n_vec=None):
    p = abi.EsParams.make([FCC] if templates is None else templates, sigma_env, r_on, r_cut, lam, switch)
    if n_env is not None:
        p.n_env = n_env
    for e, m in (n_vec or {}).items():
        p.n_vec[e] = m
    return p


def _acc(lib, abi, box, par, n=4, ghost=0, pos=1, head=1, nn=1, dtype=1, scratch=4096, n_global=4, out=True):
    """every pointer is a small non-null value that is never dereferenced when the arguments are refused"""
    partials, n_partials = C.c_void_p(), C.c_uint()
    return lib.mtd_es_accumulate(n, ghost, pos * 4096 or None, dtype, C.byref(box) if box is not None else None, head * 4096 or None,
                                 nn * 4096 or None, 4096, 0, C.byref(par) if par is not None else None, n_global, scratch or None,
                                 C.byref(partials) if out else None, C.byref(n_partials) if out else None, None, None, None, None)


def _frc(lib, abi, box, par, n=4, ghost=0, pos=1, force=1, head=1, nn=1, dtype=1, scratch=4096, n_global=4, virial=0, pitch=0):
    return lib.mtd_es_forces(n, ghost, pos * 4096 or None, force * 4096 or None, dtype, C.byref(box) if box is not None else None,
                             head * 4096 or None, nn * 4096 or None, 4096, 0, C.byref(par) if par is not None else None, n_global,
                             scratch or None, None, 0.5, None, virial * 4096 or None, pitch)


NAN, INF = float("nan"), float("inf")
CALL_KW = [dict(scratch=0), dict(scratch=4096 + 8), dict(pos=0), dict(head=0), dict(nn=0), dict(dtype=7), dict(n_global=0)]
BAD_PARAMS = [dict(sigma_env=0.0), dict(sigma_env=-0.1), dict(sigma_env=NAN), dict(sigma_env=INF), dict(r_on=-0.1), dict(r_on=1.5), dict(r_on=1.6),
              dict(r_on=NAN), dict(r_cut=NAN), dict(r_cut=INF), dict(r_cut=0.0, r_on=0.0),
              dict(n_env=0), dict(n_vec={0: 0}),
              dict(templates=[FCC[:11] + [[0.0, 0.0, 0.0]]]),            # a zero vector
              dict(templates=[FCC[:11] + [[NAN, 0.0, 0.0]]]), dict(templates=[FCC[:11] + [[0.0, INF, 0.0]]]),
              dict(templates=[FCC[:11] + [[1.5, 0.0, 0.0]]]),            # |T| = r_cut: not shorter
              dict(templates=[FCC[:11] + [[1.2, 1.2, 0.0]]]),
              dict(templates=[FCC, FCC[:6]], lam=0.0), dict(templates=[FCC, FCC[:6]], lam=-1.0), dict(templates=[FCC, FCC[:6]], lam=NAN),
              dict(templates=[FCC, FCC[:6]], lam=INF),
              dict(switch=(0.0, 6)), dict(switch=(-0.5, 6)), dict(switch=(NAN, 6)), dict(switch=(0.5, 0))]
TOO_MANY = [dict(n_env=5), dict(n_env=100000), dict(n_vec={0: 33}),
            dict(templates=[FCC * 2, FCC * 2, FCC * 2], n_vec={2: 17}),                                 # 24 + 24 + 17 = 65 vectors
            dict(templates=[FCC * 2 + FCC[:8]] * 2, n_vec={2: 1}, n_env=3)]                            # 32 + 32 + 1


def test_argument_validation_without_gpu(abi):
    """every refusal of include/mtd_abi.h "Environment similarity", before any device call (this test runs on a machine without a GPU)"""
    lib = abi.load()
    box = abi.Box.make(10.0)
    good = _params(abi)
    for call in (_acc, _frc):
        assert call(lib, abi, None, good) == INVALID
        assert call(lib, abi, box, None) == INVALID
        for kw in CALL_KW:
            assert call(lib, abi, box, good, **kw) == INVALID, (call.__name__, kw)
        for kw in BAD_PARAMS:
            assert call(lib, abi, box, _params(abi, **kw)) == INVALID, (call.__name__, kw)
        for kw in TOO_MANY:
            assert call(lib, abi, box, _params(abi, **kw)) == UNSUPPORTED, (call.__name__, kw)
        # ghosts: only the plain variable (one environment, no switch) takes them
        assert call(lib, abi, box, _params(abi, switch=(0.5, 6)), ghost=3) == UNSUPPORTED
        assert call(lib, abi, box, _params(abi, templates=[FCC, FCC[:6]]), ghost=3) == UNSUPPORTED
    assert _acc(lib, abi, box, good, out=False) == INVALID
    assert _frc(lib, abi, box, good, force=0) == INVALID
    assert _frc(lib, abi, box, good, virial=1, pitch=3) == INVALID          # a virial pitch below the particle count


def test_no_particles_is_success_in_the_force_pass(abi):
    lib = abi.load()
    box = abi.Box.make(10.0)
    good = _params(abi)
    assert _frc(lib, abi, box, good, n=0) == SUCCESS
    assert _frc(lib, abi, box, good, n=0, pos=0, force=0, head=0, nn=0) == SUCCESS
    assert _frc(lib, abi, box, good, n=0, virial=1, pitch=0) == SUCCESS
    assert _frc(lib, abi, box, _params(abi, templates=[FCC, FCC[:6]], switch=(0.5, 6), lam=20.0), n=0) == SUCCESS
    assert _frc(lib, abi, box, _params(abi, lam=NAN), n=0) == SUCCESS        # lambda is not read with one environment


def test_python_and_pybind_surface():
    from metadynamics import _metadynamics as mod
    from metadynamics import cv
    E = inspect.Parameter.empty
    params = [(n, p.default) for n, p in inspect.signature(cv.environment_similarity.__init__).parameters.items() if n != "self"]
    assert params == [("templates", E), ("sigma_env", E), ("r_cut", E), ("r_on", E), ("nlist", E), ("type", E), ("lam", 100.0), ("switch", None),
                      ("name", None), ("sigma", 1.0)]
    assert issubclass(cv.environment_similarity, cv._collective_variable)
    for meth in ("get_rcut", "get_local", "get_environments", "get_switched", "get_virial", "set_switch", "set_grid", "set_params"):
        assert hasattr(cv.environment_similarity, meth), meth
    assert list(inspect.signature(cv.environment_similarity.get_virial).parameters.items())[1][1].default is False
    assert issubclass(mod.EnvironmentSimilarity, mod.CollectiveVariable)
    for meth in ("getLocalValues", "getEnvironmentValues", "getSwitchedValues", "setSwitch", "clearSwitch", "getVirial", "getCurrentValue",
                 "getForceArray", "getLogValue", "getProvidedLogQuantities", "getRCut"):
        assert hasattr(mod.EnvironmentSimilarity, meth), meth


def _closed(env):
    have = {tuple(float(x) + 0.0 for x in t) for t in env}
    return all(tuple(-x + 0.0 for x in t) in have for t in have)


def test_environment_templates():
    from metadynamics import cv
    import env_similarity_ref as es
    a = 1.7
    want = dict(fcc=(12, [a / np.sqrt(2)] * 12), bcc=(14, [a * np.sqrt(3) / 2] * 8 + [a] * 6), sc=(6, [a] * 6))
    for name, (count, lengths) in want.items():
        t = np.array(cv.environment_templates(name, a))
        assert t.shape == (count, 3), name
        assert np.allclose(sorted(np.linalg.norm(t, axis=1)), sorted(lengths), rtol=1e-15), name
        assert len({tuple(v) for v in t}) == count and _closed(t), name
        assert {tuple(v) for v in t} == {tuple(v) for v in es.templates(name, a)}, name
    d = cv.environment_templates("diamond", a)
    assert len(d) == 2 and all(np.array(e).shape == (4, 3) for e in d)
    assert np.allclose(np.linalg.norm(np.array(d[0]), axis=1), a * np.sqrt(3) / 4, rtol=1e-15)
    assert not _closed(d[0]) and not _closed(d[1]) and _closed(d[0] + d[1])
    assert {tuple(v) for v in d[1]} == {tuple(-x + 0.0 for x in v) for v in d[0]}
    assert np.allclose(np.array(d[0]).sum(axis=0), 0.0, atol=1e-15)          # a tetrahedron
    for bad in (("hcp", 1.0), ("fcc", 0.0), ("fcc", -1.0)):
        with pytest.raises(RuntimeError):
            cv.environment_templates(*bad)


def test_python_class_refusals_leave_no_half_made_variable(monkeypatch):
    """unknown type, empty template, a vector longer than r_cut, a list that is too short, a bad switch: refused in Python, before any
    host object exists, and removed from the context's forces"""
    from metadynamics import context, cv
    fake = types.SimpleNamespace(type_names=["A", "B"], forces=[], system_definition=None, system=None, integrator=None)
    monkeypatch.setattr(context, "current", fake)
    nl = types.SimpleNamespace(r_cut=1.5, device=False, cpp_nlist=None)
    good = dict(templates=FCC, sigma_env=0.12, r_cut=1.5, r_on=1.3, nlist=nl, type="A")
    bad = [dict(type="Z"), dict(templates=[]), dict(templates=[[]]), dict(templates=[FCC, []]), dict(templates=FCC[:11] + [[2.0, 0.0, 0.0]]),
           dict(templates=FCC[:11] + [[0.0, 0.0, 0.0]]), dict(templates=FCC[:11] + [[1.0, 0.0]]), dict(templates=[FCC] * 5),
           dict(templates=[FCC * 3]), dict(nlist=types.SimpleNamespace(r_cut=1.4, device=False, cpp_nlist=None)), dict(sigma_env=0.0),
           dict(r_on=1.5), dict(lam=0.0), dict(switch=dict(c0=0.0, p=6)), dict(switch=dict(c0=0.5, p=0)), dict(switch=dict(c0=0.5, p=2.5)),
           dict(switch=dict(c0=0.5)), dict(switch=dict(c0=0.5, p=6, q=1)), dict(switch=(0.5, 6))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="Error creating collective variable."):
            cv.environment_similarity(**{**good, **kw})
        assert fake.forces == [], kw
