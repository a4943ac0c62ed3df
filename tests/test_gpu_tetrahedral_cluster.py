"""GPU: the tetrahedral order restricted to the largest cluster (mtd_tetrahedral_accumulate_cluster, csrc/tetrahedral.hip with csrc/row_mask.hpp
and csrc/cluster.hip) through the C ABI against the fp64 restatement (tests/row_cluster_ref.py, itself checked on the CPU in
tests/test_row_cluster_ref.py), with fp32 and fp64 arrays and both scratches pre-filled with garbage.  Runner, tolerances and
comparisons: tests/row_cluster_gpu.py.  Every figure is printed before it is asserted.

Condition on the inputs, asserted on the restatement before any GPU call (condition()): every pair weight W_i is 0 or >= 1e-5 and no
distance lies within 1e-9 of r_on or r_cut.  tests/test_gpu_tetrahedral.py asks W_i >= 1e-3 of its lattices; the gas of two_diamonds() holds
one particle with W_i = 1.6e-5.  The bound follows from the arithmetic: the moment form of W_i cancels terms of size n_i^2 <= 4 there, an
absolute error of a few 1e-16, which is 1e-10 of W_i at 1e-5 — a tenth of the tolerance on t_i."""
import numpy as np
import pytest

import ql_local_cluster_ref as cl
import row_cluster_gpu as rg
import row_cluster_ref as rc
import tetrahedral_ref as tr
import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KIND = "tetrahedral"
DTYPES = [np.float64, np.float32]
INVALID = -1


def condition(pos, types, L, nl, par):
    r = tr.compute(pos, types, L, nl, par)
    W = r["W"]
    assert np.all((W == 0.0) | (W >= 1e-5)), W[(W != 0.0) & (W < 1e-5)]
    if len(r["r"]):
        assert np.abs(r["r"] - par["r_on"]).min() > 1e-9 and np.abs(r["r"] - par["r_cut"]).min() > 1e-9
    return r


def _run(abi, c, dtype, **kw):
    return rg.run(abi, KIND, c["pos"], c["types"], c["L"], c["nl"], c["par"], dtype, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(rc.TET_COMBOS))
def test_parity_on_the_fixture(abi, dtype, name):
    c = rc.tetrahedral_case(name, dtype)
    assert min(c["margins"]) > 1e-6
    condition(c["pos"], c["types"], c["L"], c["nl"], c["par"])
    g = _run(abi, c, dtype, cluster=c["cluster"])
    r = rc.tetrahedral(c["pos"], c["types"], c["L"], c["nl"], c["par"], cluster=c["cluster"], bias=0.9)
    rg.compare(KIND, g, r, 0.9, dtype, c["types"], 0)
    assert g["summary"][1] == g["w"].sum() > 1 and g["summary"][2] > 1                # several clusters, one picked
    far = rc.far_from_members(c["pos"], c["L"], r["w"], 2.0 * c["par"]["r_cut"])
    assert far.sum() > 10
    assert np.all(g["F"][far] == 0.0) and np.all(g["virial"][far] == 0.0)            # exactly: their adjoint rows and their neighbours' are 0
    plain = _run(abi, c, dtype, entry="plain")
    for k in ("switched", "local", "coordination"):
        assert np.array_equal(plain[k], g[k]), k                                     # v_i stays unmasked
    assert g["s"] < plain["s"] and not np.array_equal(plain["F"], g["F"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_off_is_off(abi, dtype):
    """cluster == NULL and an all-zero struct: the scratch and the forces of mtd_tet_accumulate, bit for bit — the order and the penalty"""
    c = rc.tetrahedral_case("switch+gate", dtype)
    penalty = tr.params(0, rc.TET_ARGS["r_cut"], rc.TET_ARGS["r_on"], normalise=False)
    for par in (c["par"], penalty):
        k = dict(c, par=par)
        plain = _run(abi, k, dtype, entry="plain")
        for off in ("null", "zero"):
            g = _run(abi, k, dtype, off=off)
            assert g["null"]
            rg.same_bits(g, plain, ("scratch", "F", "virial", "s", "sums"))
    assert _run(abi, dict(c, par=penalty), dtype, cluster=c["cluster"], expect=INVALID) is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["plain", "switch+gate"])
def test_all_members(abi, dtype, name):
    """a periodic diamond lattice, v_min below every v_i of the type: w = 1 on the type, forces and virial are the plain call's bit for
    bit, the value is the plain call's (only the order of the sum may differ)"""
    pos, L = tr.diamond_lattice(2)
    pos = (pos + np.random.default_rng(3).normal(0, 0.03, pos.shape)).astype(dtype).astype(np.float64)
    types = (np.arange(len(pos)) % 9 == 4).astype(np.int32)
    nl = util.build_nlist(pos, L, rc.TET_LIST)
    par = tr.params(0, rc.TET_ARGS["r_cut"], rc.TET_ARGS["r_on"], **rc.TET_COMBOS[name][0])
    condition(pos, types, L, nl, par)
    k = dict(pos=pos, types=types, L=L, nl=nl, par=par)
    r = rc.tetrahedral(pos, types, L, nl, par, cluster=(-0.5, 1.2), bias=0.9)
    assert np.array_equal(r["w"], (types == 0).astype(np.float64))                   # one cluster holds the whole type
    g = _run(abi, k, dtype, cluster=(-0.5, 1.2))
    plain = _run(abi, k, dtype, entry="plain")
    rg.compare(KIND, g, r, 0.9, dtype, types, 0)
    rg.same_bits(g, plain, ("F", "virial", "local", "switched", "coordination"))
    print("s %.17g, plain %.17g" % (g["s"], plain["s"]))
    assert abs(g["s"] - plain["s"]) <= 1e-12 * abs(plain["s"]) and np.abs(plain["F"]).max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_solid(abi, dtype):
    c = rc.tetrahedral_case("switch", dtype)
    g = _run(abi, c, dtype, cluster=(2.0, c["cluster"][1]))                           # v_i <= 1
    assert g["s"] == 0.0 and g["sums"][0] == 0.0 and g["sums"][1] == (c["types"] == 0).sum()
    assert g["summary"].tolist() == [cl.NONE, 0, 0, 0] and np.all(g["label"] == cl.NONE) and np.all(g["w"] == 0.0)
    assert np.all(g["F"] == 0.0) and np.all(g["virial"] == 0.0)
    assert np.abs(g["switched"]).max() > 0.5                                          # unmasked


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_shapes_of_the_mask_step(abi, dtype, n):
    """one particle, one short of a chunk of 32, a whole chunk, one more than the chunk (a second block): cut from the big crystallite"""
    k = rc.cut(rc.tetrahedral_case("switch", dtype), n, rc.TET_LIST)
    v = condition(k["pos"], k["types"], k["L"], k["nl"], k["par"])["switched"]
    cluster = (-0.5 if n == 1 else 0.3, 1.2)                                          # (alone, v_i = 0: a node all the same, a cluster of one)
    assert min(cl.margins(k["pos"], k["types"], k["L"], k["nl"], 0, v, *cluster)) > 1e-6
    r = rc.tetrahedral(k["pos"], k["types"], k["L"], k["nl"], k["par"], cluster=cluster, bias=0.9)
    g = _run(abi, k, dtype, cluster=cluster)
    rg.compare(KIND, g, r, 0.9, dtype, k["types"], 0, forces=n > 1)
    assert 0 < r["w"].sum() < max(n, 2)                                               # n > 1: the mask takes something away
    again = _run(abi, k, dtype, cluster=cluster)
    rg.same_bits(g, again, rg.OUTPUTS + ("coordination", "scratch"))                  # two identical calls: identical bits
