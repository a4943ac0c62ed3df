"""CPU: bench.py --dump-outputs writes float32 / float64 .npy files, 64 MB at most: per-particle arrays that do not fit keep the
same fixed, seeded sample of rows, whose indices go beside them.  Runs bench.dump_outputs in a child process (importing bench.py
sets the process environment the benchmark needs)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
n = int(sys.argv[3])
rng = np.random.default_rng(5)
small = {"cv": [0.25, -0.5], "bias_grid": np.linspace(0.0, 1.0, 256 * 256), "num_gaussians": [7]}
per = {"forces_cv0": rng.standard_normal((n, 4)), "forces_cv1": rng.standard_normal((n, 4)).astype(np.float32)}
np.save(sys.argv[2] + "_in0.npy", per["forces_cv0"])
bench.dump_outputs(sys.argv[2], small, per)
"""


def _dump(tmp_path, tag, n):
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out, str(n)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    files = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    size = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
    return files, size, np.load(out + "_in0.npy")


def test_small_dump_is_whole(tmp_path):
    files, size, f0 = _dump(tmp_path, "a", 1000)
    assert set(files) == {"cv", "bias_grid", "num_gaussians", "forces_cv0", "forces_cv1"}
    assert files["cv"].dtype == np.float64 and files["forces_cv1"].dtype == np.float32 and files["num_gaussians"][0] == 7.0
    assert np.array_equal(files["forces_cv0"], f0)


def test_large_dump_is_a_fixed_sample_within_64_mb(tmp_path):
    n = 1_500_000                                   # 48 MB + 24 MB of per-particle arrays
    a, size_a, f0 = _dump(tmp_path, "a", n)
    b, _, _ = _dump(tmp_path, "b", n)
    assert size_a <= 64 * 1024 * 1024
    rows = a["sample_rows"]
    assert rows.dtype == np.float64 and np.array_equal(rows, b["sample_rows"])
    assert np.all(np.diff(rows) > 0) and rows[-1] < n and len(rows) > n // 2
    idx = rows.astype(np.int64)
    assert a["forces_cv0"].shape == (len(idx), 4) and np.array_equal(a["forces_cv0"], f0[idx])
    assert a["forces_cv1"].dtype == np.float32 and a["forces_cv1"].shape == (len(idx), 4)
