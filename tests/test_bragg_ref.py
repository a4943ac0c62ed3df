"""CPU: the restatement of the Bragg intensity (tests/bragg_ref.py) against known answers, central differences and the invariances that
set the variable apart from cv.lamellar.  The GPU tests compare the kernels with this restatement; nothing here needs a GPU."""
import numpy as np
import pytest

import bragg_ref as br

HKL = [(0, 0, 2), (1, -1, 0), (2, 1, -3)]
COEFF = [1.0, -0.7, 0.0]                                                  # three types, one without an amplitude
BOX = (6.0, 7.0, 8.0)


def _snapshot(n=150, seed=11):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) - 0.5) * np.array(BOX)
    pos[:, 2] += 0.8 * np.sin(2 * np.pi * 2 * pos[:, 2] / BOX[2])         # some order along (0, 0, 2)
    return pos, rng.integers(0, 3, n)


def test_known_answers():
    pos, iz, L = br.cubic_lattice(4)
    one = np.zeros(len(pos), dtype=int)
    for modulus in (False, True):
        assert br.value(pos, one, [1.0], [(0, 0, 4)], L, [1.0], modulus) == pytest.approx(1.0, abs=1e-13)
        assert abs(br.value(pos, one, [1.0], [(0, 0, 1)], L, [1.0], modulus)) <= (1e-15 if modulus else 1e-30)
    layers = (iz % 4 >= 2).astype(int)                                    # A A B B along z: period 4
    assert br.value(pos, layers, [1.0, -1.0], [(0, 0, 1)], L, [1.0]) == pytest.approx(0.5, abs=1e-13)
    assert br.value(pos, layers, [1.0, -1.0], [(0, 0, 1)], L, [1.0], modulus=True) == pytest.approx(np.sqrt(0.5), abs=1e-13)
    n = 4096
    rnd = (np.random.default_rng(5).random((n, 3)) - 0.5) * 16.0
    s = br.value(rnd, np.zeros(n, dtype=int), [1.0], [(0, 0, 4)], 16.0, [1.0])
    print("random positions: s = %.3e, N s = %.3f" % (s, n * s))
    assert 0.0 < s <= 10.0 / n                                            # N s is exponentially distributed with mean 1


def test_value_bounds_and_defaults():
    pos, types = _snapshot()
    for modulus in (False, True):
        r = br.compute(pos, types, COEFF, HKL, BOX, modulus=modulus)
        assert np.allclose(r["w"], 1.0 / 3.0) and 0.0 <= r["s"] <= 1.0
        assert r["A1"] == pytest.approx(np.abs(np.array(COEFF)[types]).sum()) and r["A2"] == pytest.approx((np.array(COEFF)[types] ** 2).sum())
        assert np.allclose(r["S"], (r["rho"] ** 2).sum(axis=1) / r["A2"])


@pytest.mark.parametrize("modulus", [False, True])
@pytest.mark.parametrize("tilt", [None, dict(xy=0.3, xz=-0.2, yz=0.15)])
def test_gradient_against_central_differences(modulus, tilt):
    pos, types = _snapshot()
    w = [0.5, 1.5, -0.25]
    r = br.compute(pos, types, COEFF, HKL, BOX, w, modulus, tilt)
    top = np.abs(r["dsdr"]).max()
    assert top > 0
    h = 1e-5
    worst = 0.0
    for j in range(len(pos)):
        for d in range(3):
            p, m = pos.copy(), pos.copy()
            p[j, d] += h
            m[j, d] -= h
            fd = (br.value(p, types, COEFF, HKL, BOX, w, modulus, tilt) - br.value(m, types, COEFF, HKL, BOX, w, modulus, tilt)) / (2 * h)
            worst = max(worst, abs(fd - r["dsdr"][j, d]))
    print("max |fd - grad| = %.3e of max |grad| = %.3e (%.3e rel)" % (worst, top, worst / top))
    assert worst <= 1e-7 * top
    assert np.all(r["dsdr"][types == 2] == 0.0)                           # no amplitude, no force


@pytest.mark.parametrize("modulus", [False, True])
def test_invariances_and_the_difference_to_lamellar(modulus):
    pos, types = _snapshot()
    tilt = dict(xy=0.3, xz=-0.2, yz=0.15)
    r = br.compute(pos, types, COEFF, HKL, BOX, None, modulus, tilt, bias=1.7)
    # a rigid shift of all particles
    shift = np.array([0.37, -1.21, 0.5])
    s_shift = br.value(pos + shift, types, COEFF, HKL, BOX, None, modulus, tilt)
    assert abs(s_shift - r["s"]) <= 1e-14
    # an affine strain of box and positions: fractional coordinates, and with them every phase, stay
    A0 = br.lattice(BOX, **tilt)
    L1, tilt1 = (6.6, 6.3, 8.8), dict(xy=0.1, xz=0.25, yz=-0.3)
    A1 = br.lattice(L1, **tilt1)
    strained = pos @ np.linalg.inv(A0) @ A1
    assert abs(br.value(strained, types, COEFF, HKL, L1, None, modulus, tilt1) - r["s"]) <= 1e-13
    # the net force vanishes
    assert np.abs(r["F"].sum(axis=0)).max() <= 1e-14
    # cv.lamellar on the same snapshot does depend on the shift: a quarter period along the ordered direction
    quarter = np.array([0.0, 0.0, BOX[2] / 8.0])
    lam0 = br.lamellar_value(pos, types, COEFF, [(0, 0, 2)], BOX)
    lam1 = br.lamellar_value(pos + quarter, types, COEFF, [(0, 0, 2)], BOX)
    b0 = br.value(pos, types, COEFF, [(0, 0, 2)], BOX, None, modulus)
    b1 = br.value(pos + quarter, types, COEFF, [(0, 0, 2)], BOX, None, modulus)
    print("lamellar %.6f -> %.6f, bragg %.6f -> %.6f" % (lam0, lam1, b0, b1))
    assert abs(lam1 - lam0) > 0.01 and abs(b1 - b0) <= 1e-14


def test_split_over_ranks_and_empty_amplitudes():
    pos, types = _snapshot()
    one = br.compute(pos, types, COEFF, HKL, BOX)
    idx = np.arange(len(pos))
    two = br.compute(pos, types, COEFF, HKL, BOX, ranks=[idx[:50], idx[50:]])
    assert two["s"] == pytest.approx(one["s"], rel=1e-13) and np.allclose(two["dsdr"], one["dsdr"], rtol=0, atol=1e-15)
    for modulus in (False, True):
        z = br.compute(pos, np.full(len(pos), 2), COEFF, HKL, BOX, modulus=modulus)
        assert z["s"] == 0.0 and not z["S"].any() and not z["grad"].any() and not z["F"].any()
    # modulus form where a peak vanishes exactly: coefficients 0, everything finite
    pair = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0]])                   # half a period of (0, 0, 2) in a box of 8 apart
    z = br.compute(pair, [0, 0], [1.0], [(0, 0, 2)], (8.0, 8.0, 8.0), [1.0], modulus=True)
    assert z["s"] <= 1e-16 and np.isfinite(z["F"]).all()
