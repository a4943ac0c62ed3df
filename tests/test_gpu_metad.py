"""GPU parity: device-resident bias grid (C-ABI) vs the CPU oracle restatement of
IntegratorMetaDynamics.cc — every grid array, the bias factors, V(s) and w(s), step by step.

Integer arrays (histograms) must match bit for bit; floating arrays to 1e-12 relative (both sides
are IEEE double; only summation order and FMA contraction differ), far inside the 1e-6 / 1e-5
tolerances BASELINE.json states for CV values / bias forces.
"""
import ctypes as C

import numpy as np
import pytest

import util

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

RTOL = 1e-11


class GpuMetad:
    """stream: the HIP stream every call of the engine is handed (None: the NULL stream); may be set between calls"""

    def __init__(self, abi, sigma, cv_min, cv_max, num_points, W=1.0, T_shift=1.0, T=1.0, stride=1,
                 mode="standard", add_bias=True, stream=None):
        self.abi = abi
        self.stream = stream
        self.lib = abi.load()
        self.n_cv = len(sigma)
        h = C.c_void_p()
        rc = self.lib.mtd_metad_create(C.byref(h), self.n_cv, util.dbl_array(sigma), util.dbl_array(cv_min),
                                       util.dbl_array(cv_max), util.uint_array(num_points), W, T_shift, T, stride,
                                       {"standard": 0, "well_tempered": 1}[mode], int(add_bias))
        abi.check(rc)
        self.h = h
        self.len = self.lib.mtd_metad_num_elements(h)

    def close(self):
        if self.h:
            self.abi.check(self.lib.mtd_metad_destroy(self.h))
            self.h = None

    def step(self, t, vals):
        for c, v in enumerate(vals):
            self.abi.check(self.lib.mtd_metad_set_cv_value(self.h, c, float(v)))
        self.abi.check(self.lib.mtd_metad_update_bias(self.h, t, self.stream))

    def state(self):
        cv = (C.c_double * self.n_cv)()
        bias = (C.c_double * self.n_cv)()
        V, w = C.c_double(), C.c_double()
        ng, oob = C.c_uint(), C.c_uint()
        self.abi.check(self.lib.mtd_metad_get_state(self.h, cv, bias, C.byref(V), C.byref(w), C.byref(ng),
                                                    C.byref(oob), self.stream))
        return dict(cv=np.array(cv[:]), bias=np.array(bias[:]), V=V.value, w=w.value, num_gaussians=ng.value,
                    oob=oob.value)

    def array(self, name):
        which = self.abi.ARRAY_NAMES.index(name)
        out = np.zeros(self.len, dtype=np.float64 if which < 6 else np.uint32)
        self.abi.check(self.lib.mtd_metad_get_array(self.h, which, out.ctypes.data, self.stream))
        return out


def compare(g, r, bias_ref, label=""):
    st = g.state()
    for name in ("hist", "hist_delta", "hist_gauss", "hist_gauss_delta"):
        assert np.array_equal(g.array(name), r.array(name)), (label, name)
    for name in ("grid", "grid_delta", "reweighted", "weight", "sigma_grid", "sigma_grid_delta"):
        a, b = g.array(name), r.array(name)
        if np.isnan(b).any():
            assert np.array_equal(np.isnan(a), np.isnan(b)), (label, name)
            continue
        scale = np.abs(b).max()
        assert np.abs(a - b).max() <= RTOL * max(scale, 1e-300), (label, name, np.abs(a - b).max(), scale)
    if not np.isnan(bias_ref).any():
        assert np.allclose(st["bias"], bias_ref, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(r.array("grid")).max())), \
            (label, st["bias"], bias_ref)
        assert st["V"] == pytest.approx(r.curr_bias, rel=1e-11, abs=1e-300, nan_ok=True), label
        assert st["w"] == pytest.approx(r.curr_weight, rel=1e-11, abs=1e-300, nan_ok=True), label
    assert st["num_gaussians"] == r.num_gaussians, label


def run_pair(abi, ref, kw, trajectory, t0=0):
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        for i, vals in enumerate(trajectory):
            t = t0 + i
            g.step(t, vals)
            b = r.update_bias(t, vals)
            compare(g, r, b, label="step %d" % t)
    finally:
        g.close()
    return r


def test_1d_well_tempered_config0b_grid(abi, ref):
    """config 0b grid: [-1,1] x 128, sigma .05, W=1, dT=7, T=1, stride 1, 10 steps"""
    kw = dict(sigma=[0.05], cv_min=[-1.0], cv_max=[1.0], num_points=[128], W=1.0, T_shift=7.0, T=1.0, stride=1,
              mode="well_tempered")
    traj = [[0.62 + 0.013 * np.sin(0.9 * t)] for t in range(10)]
    run_pair(abi, ref, kw, traj)


@pytest.mark.parametrize("mode", ["standard", "well_tempered"])
def test_2d_headline_grid(abi, ref, mode):
    """256 x 256 over [-0.02, 0.02]^2, sigma 1e-3 (config 2), stride 1, a wandering 2-d trajectory"""
    kw = dict(sigma=[1e-3, 1e-3], cv_min=[-0.02, -0.02], cv_max=[0.02, 0.02], num_points=[256, 256], W=1.0,
              T_shift=7.0, T=1.0, stride=1, mode=mode)
    rng = np.random.default_rng(7)
    pts = np.cumsum(rng.normal(0, 4e-4, size=(12, 2)), axis=0)
    run_pair(abi, ref, kw, pts.tolist())


def test_stride_and_no_hills(abi, ref):
    """stride 3 starting at t=1 (deposits at t=3,6,...; histogram accumulates in between, Q13) and
    add_hills=False (only histogram + evaluation)"""
    kw = dict(sigma=[0.2, 0.1], cv_min=[0.0, 0.0], cv_max=[1.0, 2.0], num_points=[20, 30], W=0.5, T_shift=2.0,
              T=0.7, stride=3, mode="well_tempered")
    traj = [[0.3 + 0.05 * np.cos(t), 1.0 + 0.2 * np.sin(1.3 * t)] for t in range(11)]
    run_pair(abi, ref, kw, traj, t0=1)
    kw2 = dict(kw, add_bias=False)
    run_pair(abi, ref, kw2, traj[:4])


def test_edges_and_out_of_bounds(abi, ref):
    """values on / beyond the grid edges: forward / backward differences (:746-764), the upper >= L clamp
    (:689-693), out-of-range => V = 0 and off-grid histogram (Q13, Q14); never-on-grid deposit => NaN (Q15)"""
    kw = dict(sigma=[0.05], cv_min=[0.0], cv_max=[1.0], num_points=[11], W=1.0, T_shift=3.0, T=1.0, stride=1,
              mode="well_tempered")
    traj = [[0.5], [0.04], [0.97], [0.0], [1.0 - 1e-12], [0.999999], [0.55]]
    run_pair(abi, ref, kw, traj)
    # start off-grid: norm = 0 -> NaN weights in the reference
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        for t, v in enumerate([[1.5], [-0.3], [0.5]]):
            g.step(t, v)
            b = r.update_bias(t, v)
            compare(g, r, b, label="oob %d" % t)
        assert np.isnan(r.array("weight")).all() and np.isnan(g.array("weight")).all()
    finally:
        g.close()


def test_3d_and_sigma_matrix(abi, ref):
    """3 CVs, full (non-diagonal) inverse-sigma matrix: element-wise square in the exponent (Q12)"""
    kw = dict(sigma=[0.3, 0.2, 0.25], cv_min=[-1.0, 0.0, 2.0], cv_max=[1.0, 1.0, 4.0], num_points=[9, 7, 8], W=1.2,
              T_shift=5.0, T=1.5, stride=2, mode="well_tempered")
    sinv = np.array([[3.0, 0.4, -0.2], [0.4, 5.0, 0.7], [-0.2, 0.7, 4.0]])
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        abi.check(g.lib.mtd_metad_set_sigma_inv(g.h, util.dbl_array(sinv.reshape(-1))))
        r.set_sigma_inv(sinv)
        assert g.lib.mtd_metad_sigma_determinant(g.h) == pytest.approx(r.sigma_determinant, rel=1e-14)
        rng = np.random.default_rng(11)
        for t in range(8):
            v = [rng.uniform(-0.9, 0.9), rng.uniform(0.05, 0.95), rng.uniform(2.1, 3.9)]
            g.step(t, v)
            b = r.update_bias(t, v)
            compare(g, r, b, label="3d %d" % t)
    finally:
        g.close()


def test_walker_phases(abi, ref):
    """multiple walkers (.cc:393-409): two engines deposit, their four delta arrays are summed (what the
    RCCL all-reduce does), then both reweight/accumulate — compared with two oracle engines"""
    kw = dict(sigma=[0.1, 0.1], cv_min=[0.0, 0.0], cv_max=[1.0, 1.0], num_points=[24, 16], W=1.0, T_shift=4.0, T=1.0,
              stride=1, mode="well_tempered")
    lib = abi.load()
    gs = [GpuMetad(abi, **kw) for _ in range(2)]
    rs = [ref.Metad(**kw) for _ in range(2)]
    try:
        G = gs[0].len
        views = []
        for g in gs:
            p_real, p_cnt, n = C.c_void_p(), C.c_void_p(), C.c_uint()
            abi.check(lib.mtd_metad_delta_buffers(g.h, C.byref(p_real), C.byref(p_cnt), C.byref(n)))
            assert n.value == G
            assert p_real.value == lib.mtd_metad_device_array(g.h, 1)   # grid_delta leads the real pack
            assert p_cnt.value == lib.mtd_metad_device_array(g.h, 7)    # hist_delta leads the count pack
            views.append((p_real.value, p_cnt.value))
        for t in range(5):
            vals = [[0.3 + 0.05 * t, 0.6 - 0.03 * t], [0.7 - 0.04 * t, 0.2 + 0.06 * t]]
            dep = []
            for g, v in zip(gs, vals):
                for c, x in enumerate(v):
                    abi.check(lib.mtd_metad_set_cv_value(g.h, c, x))
                d = C.c_int()
                abi.check(lib.mtd_metad_update_phase_a(g.h, t, C.byref(d), None))
                dep.append(d.value)
            rdep = [r.phase_a(t, v) for r, v in zip(rs, vals)]
            assert dep == rdep
            # "all-reduce": sum the packed delta buffers over the walkers, on the host here
            real = [np.concatenate([g.array("grid_delta"), g.array("sigma_grid_delta")]) for g in gs]
            cnt = [np.concatenate([g.array("hist_delta"), g.array("hist_gauss_delta")]) for g in gs]
            real_sum, cnt_sum = real[0] + real[1], cnt[0] + cnt[1]
            for g in gs:
                abi.check(lib.mtd_metad_set_array(g.h, 1, real_sum[:G].ctypes.data, None))
                abi.check(lib.mtd_metad_set_array(g.h, 5, real_sum[G:].ctypes.data, None))
                abi.check(lib.mtd_metad_set_array(g.h, 7, cnt_sum[:G].ctypes.data, None))
                abi.check(lib.mtd_metad_set_array(g.h, 9, cnt_sum[G:].ctypes.data, None))
            for name in ("grid_delta", "sigma_grid_delta", "hist_delta", "hist_gauss_delta"):
                tot = rs[0].array(name) + rs[1].array(name)
                for r in rs:
                    r.array(name)[:] = tot
            for g, r, v in zip(gs, rs, vals):
                abi.check(lib.mtd_metad_update_phase_b(g.h, dep[0], None))
                b = r.phase_b(rdep[0], v)
                compare(g, r, b, label="walker %d" % t)
    finally:
        for g in gs:
            g.close()


def test_cv_from_device_partials(abi, ref):
    """CV values taken from device partial sums (mtd_metad_set_cv_source): s = shift + scale * sum"""
    kw = dict(sigma=[0.05, 0.05], cv_min=[-1.0, -1.0], cv_max=[1.0, 1.0], num_points=[32, 32], W=1.0, T_shift=7.0,
              T=1.0, stride=1, mode="well_tempered")
    g = GpuMetad(abi, **kw)
    r = ref.Metad(**kw)
    try:
        rng = np.random.default_rng(3)
        parts = rng.normal(size=(300, 3))
        d_parts = torch.from_numpy(parts).cuda()
        abi.check(g.lib.mtd_metad_set_cv_source(g.h, 0, abi.ptr(d_parts), 300, 3, 0, 1.0 / 500.0, 0.1))
        abi.check(g.lib.mtd_metad_set_cv_source(g.h, 1, abi.ptr(d_parts), 300, 3, 2, -1.0 / 400.0, 0.0))
        vals = [0.1 + parts[:, 0].sum() / 500.0, -parts[:, 2].sum() / 400.0]
        abi.check(g.lib.mtd_metad_update_bias(g.h, 0, None))
        st = g.state()
        assert np.allclose(st["cv"], vals, rtol=1e-13, atol=1e-15)
        b = r.update_bias(0, st["cv"])
        compare(g, r, b)
        # the bias factors are readable in place by device code: copy them out with a kernel
        d_bias = g.lib.mtd_metad_bias_device(g.h)
        out = torch.zeros(2, dtype=torch.float64, device="cuda")
        abi.check(g.lib.mtd_reduce_partials(d_bias, 1, 2, 2, 1.0, 0.0, abi.ptr(out), None))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), st["bias"])
    finally:
        g.close()


def test_dropin_update_grid(abi, ref):
    """gpu_update_grid replacement: grid_delta += W * scal * gauss (accumulates, Q11)"""
    lib = abi.load()
    lengths, cv_min, cv_max = [20, 30], [0.0, 0.0], [1.0, 2.0]
    sinv = [4.0, 0.0, 0.0, 10.0]
    cur = [0.37, 1.21]
    d_cur = torch.tensor(cur, dtype=torch.float64, device="cuda")
    d_delta = torch.full((600,), 0.25, dtype=torch.float64, device="cuda")
    abi.check(lib.mtd_update_grid(600, util.uint_array(lengths), 2, abi.ptr(d_cur), abi.ptr(d_delta),
                                  util.dbl_array(cv_min), util.dbl_array(cv_max), util.dbl_array(sinv), 0.8, 1.5, None))
    torch.cuda.synchronize()
    expect = 0.25 + ref.update_grid(lengths, cv_min, cv_max, sinv, cur, 0.8, 1.5)
    assert np.allclose(d_delta.cpu().numpy(), expect, rtol=1e-13, atol=0)


def test_create_errors(abi):
    """setGrid(true) input checks (.cc:798-812): cv_min >= cv_max, num_points < 2"""
    lib = abi.load()
    h = C.c_void_p()
    args = lambda lo, hi, n: (C.byref(h), 1, util.dbl_array([0.1]), util.dbl_array([lo]), util.dbl_array([hi]),
                              util.uint_array([n]), 1.0, 1.0, 1.0, 1, 0, 1)
    assert lib.mtd_metad_create(*args(1.0, 1.0, 10)) == -1
    assert lib.mtd_metad_create(*args(0.0, 1.0, 1)) == -1
    assert lib.mtd_metad_create(*args(0.0, 1.0, 2)) == 0
    abi.check(lib.mtd_metad_destroy(h))
