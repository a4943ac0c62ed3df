"""CPU: the numpy restatement of the coordination number (tests/coordination_ref.py) that the GPU tests compare against is itself checked
here: its analytic gradient against central differences of its value, its virial against differences of the value under strained
positions and box (tilted), the limit of the switching function at x = 1 and its agreement with the quotient form away from it, a
perfect fcc crystal against the closed sum over its shells, the pair-sum identity N_A s_AB = N_B s_BA, the sum rule of the gradient, a
rocksalt lattice against its shuffled copy, and that one dropped or one stale list entry moves the result."""
import math

import numpy as np
import pytest

import coordination_ref as cn
import util

R0, R_CUT = 1.15, 2.0
PAIRS = [(6, 12), (5, 9), (1, 2), (31, 32)]


def snapshot(noise=0.05, n=5, seed=777):
    pos, L = util.fcc_lattice(n)
    return pos + np.random.default_rng(seed).normal(0, noise, pos.shape), L


@pytest.fixture(scope="module")
def crystal():
    """the noisy fcc 5 with interleaved types and the parameters of the difference tests: (5, 9), d_0 = 0.1, switch (5.0, 8)"""
    pos, L = snapshot()
    types = (np.arange(len(pos)) % 2).astype(np.int32)
    nl = util.build_nlist(pos, L, R_CUT)
    par = cn.params(0, 1, R0, R_CUT, d_0=0.1, n=5, m=9, switch=(5.0, 8))
    return dict(pos=pos, types=types, L=L, nl=nl, par=par, r=cn.compute(pos, types, L, nl, par))


def test_gather_form_is_the_gradient_on_a_symmetric_list_and_sums_to_zero(crystal):
    pos, types, L, nl = (crystal[k] for k in ("pos", "types", "L", "nl"))
    for a, b in ((0, 1), (1, 0), (0, 0)):
        for switch in (None, (5.0, 8), (5.0, 8, True)):
            r = cn.compute(pos, types, L, nl, cn.params(a, b, R0, R_CUT, switch=switch))
            top = np.abs(r["grad"]).max()
            assert top > 1e-5
            assert np.abs(r["gather"] - r["grad"]).max() <= 1e-13 * top
            assert np.abs(r["grad"].sum(axis=0)).max() <= 1e-13 * top * len(pos)     # the sum rule: no net force
            assert r["switched"].sum() / r["n_a"] == pytest.approx(r["s"], rel=1e-14)
            assert np.all(r["local"][types != a] == 0.0)


def test_gradient_against_central_differences(crystal):
    pos, types, L, nl, par, r = (crystal[k] for k in ("pos", "types", "L", "nl", "par", "r"))
    top = np.abs(r["grad"]).max()
    h, worst = 1e-5, 0.0
    for k in (0, 7, 123, 256, 499):
        for a in range(3):
            p, m = pos.copy(), pos.copy()
            p[k, a] += h
            m[k, a] -= h
            fd = (cn.value(p, types, L, nl, par) - cn.value(m, types, L, nl, par)) / (2 * h)
            worst = max(worst, abs(fd - r["grad"][k, a]))
    print("gradient vs central differences: %.3e of max |ds/dr| %.3e" % (worst / top, top))
    assert top > 0
    assert worst <= 1e-7 * top          # rounding of a value of order 1 over 2 h


def test_strain_derivatives_tilted_box():
    """the six derivatives of s under x -> (1 + eps) x of positions and box, against -virial_sum / bias, in a sheared box"""
    pos, L = snapshot(n=4, seed=11)
    tilt = dict(xy=0.15, xz=-0.1, yz=0.2)
    h = np.array([[L, tilt["xy"] * L, tilt["xz"] * L], [0, L, tilt["yz"] * L], [0, 0, L]])
    pos = (pos / L) @ h.T
    types = (np.arange(len(pos)) % 2).astype(np.int32)
    nl = cn.brute_nlist(pos, h, R_CUT + 0.05)
    for par in (cn.params(0, 1, R0, R_CUT, d_0=0.1, n=5, m=9, switch=(5.0, 8)), cn.params(0, 0, R0, R_CUT)):
        r = cn.compute(pos, types, L, nl, par, tilt=tilt, bias=1.0)
        e, worst = 1e-6, 0.0
        top = np.abs(r["virial_sum"]).max()
        for c6, (a, b) in enumerate(cn.PAIRS6):
            vals = []
            for sgn in (1.0, -1.0):
                # an upper-triangular strain keeps the cell in HOOMD's form: eps_ab with a <= b moves x_a by eps x_b
                F = np.eye(3)
                F[a, b] += sgn * e
                h2 = F @ h
                L2 = np.array([h2[0, 0], h2[1, 1], h2[2, 2]])
                t2 = dict(xy=h2[0, 1] / L2[1], xz=h2[0, 2] / L2[2], yz=h2[1, 2] / L2[2])
                vals.append(cn.value(pos @ F.T, types, L2, nl, par, tilt=t2))
            fd = (vals[0] - vals[1]) / (2 * e)
            worst = max(worst, abs(fd + r["virial_sum"][c6]))
            print("eps_%d%d: difference %.10g, -virial sum %.10g" % (a, b, fd, -r["virial_sum"][c6]))
        assert top > 0.01
        assert worst <= 1e-6 * top
        gtop = np.abs(r["grad"]).max()
        assert np.abs(r["gather"] - r["grad"]).max() <= 1e-13 * gtop


@pytest.mark.parametrize("n,m", PAIRS)
def test_limit_at_x_equal_one(n, m):
    s, ds = cn.rational(np.array([1.0]), n, m)
    assert s[0] == pytest.approx(n / m, rel=1e-15)
    assert ds[0] == pytest.approx(n * (n - m) / (2.0 * m), rel=1e-14)


@pytest.mark.parametrize("n,m", PAIRS)
def test_agreement_with_the_quotient_form_away_from_one(n, m):
    x = np.concatenate([np.linspace(0.0, 0.9, 91), np.linspace(1.1, 2.0, 91)])
    assert np.all(np.abs(x - 1.0) > 0.1 - 1e-15)
    s, ds = cn.rational(x, n, m)
    q, dq = cn.quotient(x, n, m)
    assert np.abs(s - q).max() <= 1e-13 * np.abs(s).max()
    assert np.abs(ds - dq).max() <= 1e-13 * max(np.abs(ds).max(), 1.0)


def test_restatement_beats_the_quotient_form():
    """The Horner form is well conditioned at every offset from x = 1; the quotient form breaks AT x = 1 (0 / 0) and at
    |x - 1| = 1e-12.  No claim at 1e-9: rounding analysis puts the error of the quotient's value near 2e-8 there, float64 runs showed
    1.3e-10 and 3e-9.  At 1e-12 what breaks is the quotient's DERIVATIVE (two terms of order delta cancel to order delta^2: relative
    error 1.0 in a float64 run); its value erred by 3e-12 (6, 12) and 2e-12 (5, 9) in that run, by 1.1e-5 and 0 in another: x^n - 1 is
    a whole number of ulps there, and the error depends on which.  The assertion takes the worse of the two."""
    for n, m in ((6, 12), (5, 9)):
        s1, d1 = n / m, n * (n - m) / (2.0 * m)
        for off in (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6):
            s, ds = cn.rational(np.array([1.0 + off]), n, m)
            # against the first-order expansion about 1, whose own remainder is O(m^2 off^2) <= 2e-9 at 1e-6
            assert abs(s[0] - (s1 + d1 * off)) <= 1e-14 + 1e4 * off * off, (n, m, off)
            assert abs(ds[0] - d1) <= 1e-13 + 1e3 * abs(off), (n, m, off)
        q, dq = cn.quotient(np.array([1.0]), n, m)
        assert not np.isfinite(q[0]) and not np.isfinite(dq[0])
    worst = 0.0
    for off in (1e-12, -1e-12):
        for n, m in ((6, 12), (5, 9)):
            s, ds = cn.rational(np.array([1.0 + off]), n, m)
            q, dq = cn.quotient(np.array([1.0 + off]), n, m)
            err_s, err_d = abs(q[0] - s[0]) / s[0], abs(dq[0] - ds[0]) / abs(ds[0])
            print("quotient form at x - 1 = %g, (%d, %d): relative error of s %.3e, of ds/dx %.3e" % (off, n, m, err_s, err_d))
            worst = max(worst, err_s, err_d)
    assert worst > 1e-7


def test_perfect_fcc_against_the_closed_shell_sum():
    """12 at 1, 6 at sqrt 2, 24 at sqrt 3 and 12 at 2 = r_cut, where s~ = 0: whether rounding puts that shell inside or outside does not
    show"""
    pos, L = util.fcc_lattice(5)
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, R_CUT + 0.01)
    par = cn.params(0, 0, R0, R_CUT)
    r = cn.compute(pos, types, L, nl, par)
    shells = [(12, 1.0), (6, math.sqrt(2.0)), (24, math.sqrt(3.0)), (12, 2.0)]
    want = sum(k * float(cn.switching(np.array([d]), par)[0][0]) for k, d in shells)
    print("perfect fcc: %.12f (closed sum %.12f)" % (r["s"], want))
    assert float(cn.switching(np.array([2.0]), par)[0][0]) == 0.0
    assert r["s"] == pytest.approx(want, abs=1e-12)
    assert want == pytest.approx(10.519420723844, abs=1e-11)
    assert np.allclose(r["local"], r["s"], rtol=1e-12)
    # every site is a centre of inversion: no gradient — with no shell AT the cut-off, where the slope has its step and rounding decides
    # entry by entry
    r = cn.compute(pos, types, L, nl, cn.params(0, 0, R0, 1.9))
    assert r["s"] > 10.0 and np.abs(r["grad"]).max() <= 1e-12


def test_pair_sum_identity_with_unequal_counts():
    pos, L = snapshot()
    types = (np.random.default_rng(2).random(len(pos)) < 0.3).astype(np.int32)
    assert (types == 0).sum() == 340 and (types == 1).sum() == 160
    nl = util.build_nlist(pos, L, R_CUT)
    ab = cn.compute(pos, types, L, nl, cn.params(0, 1, R0, R_CUT))
    ba = cn.compute(pos, types, L, nl, cn.params(1, 0, R0, R_CUT))
    print("N_A s_AB = %.10f, N_B s_BA = %.10f" % (340 * ab["s"], 160 * ba["s"]))
    assert ab["n_a"] == 340 and ba["n_a"] == 160
    assert 340 * ab["s"] == pytest.approx(160 * ba["s"], rel=1e-13)
    assert 340 * ab["s"] == pytest.approx(1151.7367242932, abs=1e-9)
    # the two variables differ by their normalisation only: so do their gradients
    assert np.abs(340 * ab["grad"] - 160 * ba["grad"]).max() <= 1e-12 * np.abs(340 * ab["grad"]).max()


def test_known_values_of_the_common_snapshot(crystal):
    pos, types, L, nl = (crystal[k] for k in ("pos", "types", "L", "nl"))
    for (a, b), mean_n, switched in (((0, 1), 6.165718608, 0.839369040), ((0, 0), 4.322091307, 0.241907792)):
        assert cn.compute(pos, types, L, nl, cn.params(a, b, R0, R_CUT))["s"] == pytest.approx(mean_n, abs=1e-8)
        assert cn.compute(pos, types, L, nl, cn.params(a, b, R0, R_CUT, switch=(5.0, 8)))["s"] == pytest.approx(switched, abs=1e-8)


def test_one_dropped_or_one_stale_entry_moves_the_result(crystal):
    pos, L, nl = (crystal[k] for k in ("pos", "L", "nl"))
    types = np.zeros(len(pos), dtype=np.int32)
    par = cn.params(0, 0, R0, R_CUT)
    r = cn.compute(pos, types, L, nl, par)
    head, nn, lst = (np.array(x).copy() for x in nl)
    top = np.abs(r["gather"]).max()
    # the entry of row 17 that lies nearest to r_0 (the steepest part of the switching function) changes places with the last and is lost
    row = lst[head[17]:head[17] + nn[17]].astype(np.int64)
    dist = np.sqrt((cn.min_image(pos[17] - pos[row], L) ** 2).sum(axis=1))
    k = int(np.argmin(np.abs(dist - R0)))
    lst1 = lst.copy()
    lst1[head[17] + k], lst1[head[17] + nn[17] - 1] = lst[head[17] + nn[17] - 1], lst[head[17] + k]
    nn2 = nn.copy()
    nn2[17] -= 1
    a = cn.compute(pos, types, L, (head, nn2, lst1), par)
    assert abs(a["s"] - r["s"]) > 1e-6 * abs(r["s"]) and np.abs(a["gather"][17] - r["gather"][17]).max() > 1e-4 * top
    lst2 = lst.copy()
    members = set(row.tolist())
    near = int(row[int(np.argmin(dist))])
    other = next(int(j) for j in lst[head[near]:head[near] + nn[near]] if int(j) not in members and int(j) != 17)
    lst2[head[17] + int(np.argmin(dist))] = other                        # a stale entry: a particle that is no neighbour any more
    b = cn.compute(pos, types, L, (head, nn, lst2), par)
    assert np.abs(b["gather"][17] - r["gather"][17]).max() > 1e-4 * top and b["local"][17] != r["local"][17]


def test_rocksalt_orders_above_its_shuffled_copy():
    """8^3 simple-cubic sites with checkerboard types: every A has six B at distance 1 and twelve A at sqrt 2; shuffled types lose both"""
    g = np.arange(8)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    types = (sites.sum(axis=1).astype(np.int64) % 2).astype(np.int32)
    L = 8.0
    pos = sites - 3.5 + np.random.default_rng(3).normal(0, 0.05, sites.shape)
    nl = util.build_nlist(pos, L, 1.8)
    val = lambda t, a, b: cn.compute(pos, t, L, nl, cn.params(a, b, 1.2, 1.8))["s"]
    ab, aa = val(types, 0, 1), val(types, 0, 0)
    shuffled = types[np.random.default_rng(4).permutation(len(types))]
    ab_s, aa_s = val(shuffled, 0, 1), val(shuffled, 0, 0)
    print("rocksalt A-B %.3f A-A %.3f; shuffled %.3f %.3f" % (ab, aa, ab_s, aa_s))
    assert ab > ab_s > aa and ab > aa_s > aa


def test_nothing_to_sum_inner_region_and_a_coincident_pair():
    pos, L = snapshot()
    types = np.zeros(len(pos), dtype=np.int32)
    nl = util.build_nlist(pos, L, R_CUT)
    r = cn.compute(pos, types, L, nl, cn.params(1, 0, R0, R_CUT))
    assert r["s"] == 0.0 and r["n_a"] == 0 and np.all(r["grad"] == 0.0) and np.all(r["local"] == 0.0)
    r = cn.compute(pos, types, L, nl, cn.params(0, 1, R0, R_CUT, switch=(5.0, 8, True)))
    assert r["s"] == 1.0 and np.all(r["local"] == 0.0) and np.all(r["grad"] == 0.0)
    three = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.05, 1.0, 1.0]])
    nl = (np.array([0, 2, 4]), np.array([2, 2, 2]), np.array([1, 2, 0, 2, 0, 1]))
    for d_0 in (0.0, 0.1):
        r = cn.compute(three, np.zeros(3, dtype=np.int32), 20.0, nl, cn.params(0, 0, 1.0, R_CUT, d_0=d_0))
        assert np.isfinite(r["grad"]).all() and np.isfinite(r["s"])
        if d_0 == 0.1:                                                   # all three pairs lie inside d_0: each counts 1, no force
            assert np.all(r["local"] == 2.0) and np.all(r["grad"] == 0.0)
        else:
            assert r["local"][0] == r["local"][1] and 1.9 < r["local"][0] < 2.0 and np.all(r["grad"][:2, 1:] == 0.0)
