"""bench.py command line: the plain run's result line, --dump-outputs and
--full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--series", "3000", "--samples", "60", *extra],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load_matrix(d, name):
    """Rebuild a dumped matrix from its finite values and its mask."""
    a = np.load(os.path.join(d, name + ".npy"))
    kind = np.load(os.path.join(d, name + "_nonfinite.npy"))
    assert a.dtype == np.float64 and kind.dtype == np.float32
    assert np.isfinite(a).all() and (a[kind != 0] == 0).all()
    a = a.copy()
    for k, v in ((1, np.nan), (2, np.inf), (3, -np.inf)):
        a[kind == k] = v
    return a


def test_dump_outputs_samples_large_matrices(tmp_path):
    """Arrays over the per-matrix budget are cut to the same seeded rows on
    every call; every file is finite float32/float64, non-finite points are
    carried by the mask, and the whole dump stays under 64 MB."""
    import bench
    rng = np.random.default_rng(1)
    rows = bench.DUMP_MAX_BYTES // (16 * 8) + 1000
    out = rng.random((rows, 16))
    out[rng.random(out.shape) < 0.01] = np.nan
    out[5, 3], out[6, 4] = np.inf, -np.inf
    big_counts = rng.integers(0, 5, (rows, 16)).astype(np.float64)
    last = {"out": out, "counts": big_counts, "scanned": 12345}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), None, last, 16, grouped=True)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["aggr_counts.npy", "aggr_counts_nonfinite.npy",
                     "aggr_values.npy", "aggr_values_nonfinite.npy",
                     "samples_scanned.npy"]
    total = 0
    for n in names:
        a = np.load(tmp_path / "a" / n)
        assert a.dtype in (np.float32, np.float64)
        assert np.isfinite(a).all()
        assert np.array_equal(a, np.load(tmp_path / "b" / n))
        total += a.nbytes
    assert total <= 64_000_000
    keep = bench.DUMP_MAX_BYTES // (16 * 8)
    picked = np.sort(np.random.default_rng(8428).choice(rows, size=keep,
                                                        replace=False))
    vals = _load_matrix(tmp_path / "a", "aggr_values")
    assert np.array_equal(vals, out[picked], equal_nan=True)
    assert np.array_equal(_load_matrix(tmp_path / "a", "aggr_counts"),
                          big_counts[picked])
    # a matrix within the budget is written whole
    small = {"out": out[:7], "counts": big_counts[:7], "scanned": 1}
    bench.dump_outputs(str(tmp_path / "c"), None, small, 16, grouped=True)
    assert np.array_equal(_load_matrix(tmp_path / "c", "aggr_values"),
                          out[:7], equal_nan=True)
    assert np.load(tmp_path / "a" / "samples_scanned.npy")[0] == 12345


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain run times exactly --steps steps, leaves the secondary
    measurements out, and dumps the rollup matrix the last step computed —
    the same one the engine returns to a direct caller."""
    res = _bench("--steps", "3", "--warmup", "1",
                 "--dump-outputs", str(tmp_path / "d"))
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["metric"] == "rollup samples/sec"
    assert res["unit"] == "samples/s" and res["dtype"] == "f64"
    assert res["higher_is_better"] is True
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(
        3000 * 60 / (res["ms_per_step"] / 1e3), rel=1e-9)
    assert res["cpu_baseline"] is None and res["cold_query"] is None \
        and res["grouped"] is None

    from victoriametrics_amd import engine, synth
    import bench
    ts, vals, offsets = synth.counter_batch(3000, 60, bench.START_TS,
                                            step=bench.STEP_MS, seed=8428)
    plan = engine.RollupPlan("rate", bench.START_TS,
                             bench.START_TS + 59 * bench.STEP_MS,
                             bench.STEP_MS, window=bench.WINDOW_MS)
    want, _, scanned = engine.rollup_eval(plan, ts, vals, offsets)
    assert np.isnan(want).any()  # the shape has grid points without a value
    got = _load_matrix(tmp_path / "d", "rollup_values")
    assert np.array_equal(got, want, equal_nan=True)
    assert np.load(tmp_path / "d" / "samples_scanned.npy")[0] == scanned


@pytest.mark.gpu
def test_full_run_adds_secondary_measurements():
    res = _bench("--steps", "2", "--warmup", "1", "--full", "--groups", "10",
                 "--cpu-baseline-target-s", "0.05", "--cold-queries", "1",
                 "--grouped-steps", "1")
    assert res["steps"] == 2
    assert res["cpu_baseline"]["value"] > 0
    assert res["cold_query"]["queries"] == 1
    assert res["grouped"]["steps"] == 1
