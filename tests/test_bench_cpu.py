"""`bench.py`'s command line on CPU (the test-only numpy stand-in for the kernels, `tiny` size): what a plain run
reports, that `--steps` sets the timed steps, and that `--dump-outputs` writes the fit's arrays, identical for two
runs with the same arguments."""
import glob
import os

import numpy as np

from tests.cpu_backend import NumpyBackend


def _run(argv):
    import bench
    return bench.main(["--gpus", "1", "--size", "tiny"] + argv, backend=NumpyBackend(), device="cpu")


def _dumped(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_plain_run_reports_the_headline_only():
    out = _run(["--steps", "3", "--warmup", "1"])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 3 and len(out["train_rmse"]) == 4
    assert out["ms_per_step"] > 0 and out["value"] > 0
    assert "cpu_baseline" not in out and "secondary" not in out and "dumped_outputs" not in out


def test_full_run_adds_the_cpu_baseline():
    out = _run(["--steps", "2", "--warmup", "1", "--full"])
    assert out["steps"] == 2 and out["cpu_baseline"]["value"] > 0 and out["speedup_vs_cpu_baseline"] > 0


def test_dump_outputs_are_the_fit_and_reproducible(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = _run(["--steps", "2", "--warmup", "1", "--dump-outputs", a])
    _run(["--steps", "2", "--warmup", "1", "--dump-outputs", b])
    da, db = _dumped(a), _dumped(b)
    import bench
    m, n, _, k = bench.SIZES["tiny"]
    assert set(da) == {"U", "V", "b_u", "b_i", "mu", "history"}
    assert da["U"].shape == (m, k) and da["V"].shape == (n, k) and da["b_u"].shape == (m,) and da["b_i"].shape == (n,)
    assert da["history"].shape == (3, 5)
    np.testing.assert_array_equal(da["history"][:, 0], out["train_rmse"])
    assert sum(x.nbytes for x in da.values()) <= 64_000_000
    for name, x in da.items():
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x)), name
        np.testing.assert_array_equal(x, db[name], err_msg=name)


def test_dump_samples_large_sides_with_a_fixed_seed(monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_FACTOR_BYTES", 64 * 4 * 100)
    a = bench._row_sample(4000, 64 * 4, 5001)
    assert a.size == 100 and np.all(np.diff(a) > 0) and a[-1] < 4000
    np.testing.assert_array_equal(a, bench._row_sample(4000, 64 * 4, 5001))
    assert bench._row_sample(100, 64 * 4, 5001) is None
