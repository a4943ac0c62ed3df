"""CPU: the yardstick of the cluster option (tests/ql_local_cluster_ref.py) is checked before anything is held against it.  Its labels
on hand-made graphs; with the mask all ones it is ql_local_bonds_ref; its analytic gradient of s = sum_i w_i v_i / N against central
differences of s WITH the clusters found again at every displaced position — only particles whose move leaves every label unchanged are
displaced, and that is asserted; its summed virial against the strain derivative with the mask kept.  Nothing here needs a GPU.

Bounds are those of the restatements this one is built from: 1e-7 of max |ds/dr| for central differences with a step of 1e-6
(tests/test_ql_local_bonds_ref.py), 1e-8 of max |W| for strain differences with eps = 1e-6 (tests/test_ql_local_virial_ref.py)."""
import numpy as np
import pytest

import ql_local_bonds_ref as bonds_ref
import ql_local_cluster_ref as cr
import util

BIAS = 0.9
_state = {}


def system():
    """two_crystallites() with its list at 1.55, built once"""
    if not _state:
        case = cr.two_crystallites()
        _state.update(case, nl=util.build_nlist(case["pos"], case["L"], 1.55))
    return _state


_results = {}


def result(combo):
    if combo not in _results:
        s = system()
        opt, window = cr.COMBOS[combo]
        cluster, margin = cr.choose(s["pos"], s["types"], s["L"], s["nl"], opt, window)
        out = cr.compute(s["pos"], s["types"], s["L"], s["nl"], cluster=cluster, bias=BIAS, **cr.ARGS, **opt)
        _results[combo] = (opt, cluster, margin, out)
    return _results[combo]


def test_labels_on_hand_made_graphs():
    """a chain, a pair, a lone node, a particle below v_min, one of another type, a ghost entry, a self entry and a one-directional list"""
    pos = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [0, 4, 0], [1, 4, 0], [0, -4, 0], [5, 0, 0], [4, 0, 0]], dtype=np.float64)
    types = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1])
    v = np.array([1, 1, 1, 1, 1, 1, 1, 0.2, 1.0])
    rows = [[1, 0, 99], [], [1, 3], [7, 8], [5], [], [], [3], [3]]      # 0 -> 1 only one way; 3 - 7 and 3 - 8 never link
    nn = np.array([len(r) for r in rows])
    head = np.concatenate([[0], np.cumsum(nn)[:-1]])
    nl = (head, nn, np.array([j for r in rows for j in r]))
    out = cr.clusters(pos, types, 20.0, nl, 0, v, 0.5, 1.1)
    N = cr.NONE
    assert out["label"].tolist() == [0, 0, 0, 0, 4, 4, 6, N, N]
    assert out["size"].tolist() == [4, 0, 0, 0, 2, 0, 1, 0, 0]
    assert out["summary"].tolist() == [0, 4, 3, 7]
    assert out["w"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    # a tie goes to the smaller root; NaN is not a node; v == v_min is one
    v2 = np.array([1, 1, np.nan, 0.5, 1, 1, 1, 0.2, 1.0])
    out = cr.clusters(pos, types, 20.0, nl, 0, v2, 0.5, 1.1)
    assert out["label"].tolist() == [0, 0, N, 3, 4, 4, 6, N, N]
    assert out["summary"].tolist() == [0, 2, 4, 6]
    # nothing solid
    out = cr.clusters(pos, types, 20.0, nl, 0, v, 2.0, 1.1)
    assert out["summary"].tolist() == [N, 0, 0, 0] and not out["w"].any() and (out["label"] == N).all()


@pytest.mark.parametrize("combo", ["plain", "switch+gate", "bonds+switch"])
def test_mask_of_ones_is_the_restatement_without_clusters(combo):
    s = system()
    opt, _ = cr.COMBOS[combo]
    a = cr.compute(s["pos"], s["types"], s["L"], s["nl"], cluster=None, bias=BIAS, **cr.ARGS, **opt)
    b = bonds_ref.compute(s["pos"], s["types"], s["L"], s["nl"], bias=BIAS, **cr.ARGS, **opt)
    assert a["s"] == b["s"]
    for key in ("c", "v", "n", "grad", "virial", "W"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("combo", sorted(cr.COMBOS))
def test_the_parity_configuration_is_what_it_is_meant_to_be(combo):
    """the inputs of the GPU parity test: v_min and r_link sit in gaps far wider than any rounding, the largest cluster is the big
    crystallite, the small one is a cluster of its own, and most particles are outside both"""
    s = system()
    opt, cluster, margin, out = result(combo)
    root, members, n_clusters, n_nodes = (int(x) for x in out["summary"])
    inside = np.isin(np.nonzero(out["w"])[0], s["big"]).sum()
    print("%s: v_min %.6g (margin %.2e), r_link %.6f (margin %.2e relative); largest cluster: root %d, %d members, %d of them of the big "
          "crystallite; %d clusters, %d nodes of %d particles" % (combo, *np.ravel([cluster[0], margin[0], cluster[1], margin[1]]), root,
                                                                   members, inside, n_clusters, n_nodes, len(s["pos"])))
    assert margin[0] > 1e-6 and margin[1] > 1e-6
    assert inside >= 150 and members >= inside and n_clusters >= 2
    small_labels = out["label"][s["small"]]
    small_labels = small_labels[small_labels != cr.NONE]
    assert len(small_labels) >= 10 and not np.isin(small_labels, out["label"][out["w"] == 1.0]).any()
    assert out["s"] == pytest.approx((out["w"] * out["v"]).sum() / len(s["pos"]), rel=1e-15)
    assert 0 < out["s"] < out["v"].sum() / len(s["pos"])                # the mask removes something


@pytest.mark.parametrize("combo", sorted(cr.COMBOS))
def test_analytic_gradient_against_central_differences_with_the_clusters_found_again(combo):
    s = system()
    pos, types, L, nl = s["pos"], s["types"], s["L"], s["nl"]
    opt, cluster, margin, out = result(combo)
    g = out["grad"]
    assert np.isfinite(g).all()
    scale = np.abs(g).max()
    assert scale > 0
    members = np.nonzero(out["w"])[0]
    rng = np.random.default_rng(4)
    # members, their non-member neighbours (the largest gradients belong to both kinds) and far particles
    strong = np.argsort(-np.abs(g).max(axis=1))[:40]
    picks = list(rng.choice(members, 4, replace=False)) + list(rng.choice(strong, 4, replace=False)) + list(rng.choice(len(pos), 2, replace=False))
    step, worst, used = 1e-6, 0.0, 0
    for k in picks:
        a = int(rng.integers(3))
        sp, same = [], True
        for sign in (1.0, -1.0):
            p = pos.copy()
            p[k, a] += sign * step
            r = cr.compute(p, types, L, nl, cluster=cluster, gradient=False, **cr.ARGS, **opt)
            same = same and np.array_equal(r["label"], out["label"])
            sp.append(r["s"])
        assert same, "particle %d: a label changed at +-h (margins %s)" % (k, margin)      # the margins make this impossible at h = 1e-6
        worst = max(worst, abs((sp[0] - sp[1]) / (2 * step) - g[k, a]))
        used += 1
    print("%s: max |ds/dr| %.4g, largest difference on %d coordinates %.3e (%.3e of it)" % (combo, scale, used, worst, worst / scale))
    assert worst <= 1e-7 * scale
    assert np.abs(g.sum(axis=0)).max() <= 1e-14 * scale * len(pos) ** 0.5            # translation invariance
    assert np.all(g[types == 1] == 0.0)


@pytest.mark.parametrize("combo", sorted(cr.COMBOS))
def test_summed_virial_against_strain_differences(combo):
    s = system()
    opt, cluster, margin, out = result(combo)
    W, T = out["W"], out["tensor"]
    top = np.abs(W).max()
    fd = -BIAS * cr.strain_derivative(s["pos"], s["types"], s["L"], s["nl"], eps=1e-6, w=out["w"], **cr.ARGS, **opt)
    err = np.abs(fd - W).max()
    print("%s: W = %s\n  -bias ds/d eps = %s\n  largest difference %.3e (%.3e of max|W| = %.4g)" % (combo, W, fd, err, err / top, top))
    assert top > 0
    assert err <= 1e-8 * top
    assert np.abs(T - T.T).max() / 2 <= 1e-12 * top
    assert np.abs(np.array([T[a, b] for a, b in cr.COMPONENTS]) - W).max() <= 1e-13 * top


def test_forces_vanish_two_shells_away_from_the_cluster():
    """a non-member with no member within 2 r_cut has no gradient at all, with the bond count (which reaches second neighbours) too"""
    s = system()
    for combo in ("switch", "bonds+switch"):
        opt, cluster, margin, out = result(combo)
        far = cr.far_from_members(s["pos"], s["L"], out["w"], 2 * cr.ARGS["r_cut"])
        assert far.sum() > 100
        assert np.all(out["grad"][far] == 0.0) and np.all(out["virial"][far] == 0.0)
