"""CPU: the yardstick of cv.steinhardt_local (tests/ql_local_ref.py) is checked before anything is held against it —
values against the committed oracle (the reference's own harmonics, one populated row at a time), known answers, and the analytic
gradient against central differences of the restatement's own s.  Nothing here needs a GPU."""
import numpy as np
import pytest

import ql_local_ref
import util


def oracle_rows(ref, pos, types, L, nl, r_cut, r_on, lmax, type_id, Ql_ref, n_global):
    """c_i, n_i and s from mtd_ref.ql_compute_cv with a list in which only row i is populated, Ql_ref = 1, n_global = 1:
    it returns Ql[l] = 4 pi/(2l+1) sum_m |A_lm(i)|^2 and Ql[0] = n_i^2, so q_l^2(i) = Ql[l] / Ql[0] and n_i = sqrt(Ql[0])"""
    N = len(pos)
    box = ref.Box.make(L)
    pt = util.oracle_postype(pos, types)
    head, nn, lst = nl
    c, n = np.zeros(N), np.zeros(N)
    ones = [1.0] * (lmax + 1)
    for i in range(N):
        if types[i] != type_id:
            continue
        only = np.zeros_like(nn)
        only[i] = nn[i]
        _, _, Ql = ref.ql_compute_cv(pt, box, head, only, lst, r_cut, r_on, lmax, type_id, ones, n_global=1)
        if Ql[0] > 0:
            n[i] = np.sqrt(Ql[0])
            c[i] = sum(Ql_ref[l] * Ql[l] / Ql[0] for l in range(lmax + 1))
    return c, n, c.sum() / n_global


def test_restatement_matches_oracle_rows(ref):
    case = ql_local_ref.issue_case()
    out = ql_local_ref.compute(gradient=False, **case)
    c, n, s = oracle_rows(ref, **case)
    sel = case["types"] == 0
    print("max |dc| %.3e, max |dn| %.3e, s %.15g vs %.15g" % (np.abs(out["c"] - c).max(), np.abs(out["n"] - n).max(), out["s"], s))
    assert np.abs(out["c"] - c).max() <= 1e-12 * np.abs(c).max()
    assert np.abs(out["n"] - n).max() <= 1e-12 * np.abs(n).max()
    assert out["s"] == pytest.approx(s, rel=1e-12)
    assert np.all(out["c"][~sel] == 0.0) and np.all(out["n"][~sel] == 0.0)
    assert n[sel].min() == pytest.approx(6.65, abs=0.01) and c[sel].mean() == pytest.approx(0.318, abs=0.001)


def test_known_answers():
    # perfect fcc: 12 neighbours, q_4^2 = 7/192, q_6^2 = 169/512 for every particle
    pos, L = util.fcc_lattice(3)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, 1.4)
    for ql_ref, want in (([0, 0, 0, 0, 1, 0, 0], 7.0 / 192.0), ([0, 0, 0, 0, 0, 0, 1], 169.0 / 512.0)):
        out = ql_local_ref.compute(pos, types, L, nl, 1.4, 1.2, 6, 0, ql_ref, gradient=False)
        assert np.abs(out["n"] - 12.0).max() <= 1e-13 * 12
        assert np.abs(out["c"] - want).max() <= 1e-13
        assert out["s"] == pytest.approx(want, abs=1e-13)
    # the noisy two-type case
    out = ql_local_ref.compute(gradient=False, **ql_local_ref.issue_case())
    assert out["s"] == pytest.approx(0.253169653157423, rel=1e-12)


def test_analytic_gradient_against_central_differences():
    case = ql_local_ref.issue_case()
    out = ql_local_ref.compute(**case)
    g = out["grad"]
    h = 1e-5
    num = np.zeros_like(g)
    pos = case["pos"]
    for k in range(len(pos)):
        for a in range(3):
            sp = []
            for sign in (1.0, -1.0):
                p = pos.copy()
                p[k, a] += sign * h
                sp.append(ql_local_ref.compute(**{**case, "pos": p}, gradient=False)["s"])
            num[k, a] = (sp[0] - sp[1]) / (2 * h)
    scale = np.abs(num).max()
    err = np.abs(g - num).max()
    print("max |ds/dr| %.4g, largest difference %.3e" % (scale, err))
    assert scale == pytest.approx(0.026, abs=0.002)
    assert err <= 1e-6 * scale
    assert np.all(g[case["types"] == 1] == 0.0)                       # particles of the other type: exactly 0
