"""Ad-hoc measurement: histogram_over_time(m[5m]) on the device over a
resident batch (csrc/hot.hip), next to avg_over_time on the same batch and
grid (it reads the same columns) and to the host function on a subsample.
Run on a GPU box:
    python tests/bench_histogram_over_time.py [n_series] [--reps N]
                                              [--skip-host]
Numbers land in profiles/histogram_over_time.md."""
import argparse
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from victoriametrics_amd import engine, rollup_multi  # noqa: E402
from victoriametrics_amd.engine import RollupPlan, SeriesBatch  # noqa: E402
from victoriametrics_amd.metric_name import MetricName  # noqa: E402

START = 1_000_000_000_000
ROWS = 240
SCRAPE = 15_000
STEP = 60_000
WINDOW = 300_000
HOST_SUBSAMPLE = 200


def make_columns(n_series, seed=8428):
    """Log-normal gauges: per-series median log-uniform over [1e-2, 1e4],
    sigma 0.5 (a latency- or queue-depth-like spread)."""
    rng = np.random.default_rng(seed)
    ts = (START + np.arange(ROWS, dtype=np.int64)[None, :] * SCRAPE +
          rng.integers(-500, 500, (n_series, ROWS))).astype(np.int64)
    med = 10.0 ** rng.uniform(-2.0, 4.0, (n_series, 1))
    vals = med * np.exp(rng.normal(0.0, 0.5, (n_series, ROWS)))
    offsets = np.arange(n_series + 1, dtype=np.uint64) * ROWS
    return ts.reshape(-1), vals.reshape(-1), offsets


def exec_only(batch, start, end, step, window):
    """vmgpu_histogram_over_time_exec without the fetch: the result stays
    resident, as a caller chaining device stages would leave it."""
    lib = engine._load_lib()
    engine._upload_vmrange_thresholds(lib)
    n_rows = ctypes.c_uint64(0)
    scanned = ctypes.c_uint64(0)
    errbuf = ctypes.create_string_buffer(256)
    rc = lib.vmgpu_histogram_over_time_exec(
        ctypes.c_uint64(batch.handle), ctypes.c_int64(start),
        ctypes.c_int64(end), ctypes.c_int64(step), ctypes.c_int64(window),
        ctypes.c_int32(1), ctypes.byref(n_rows), ctypes.byref(scanned),
        errbuf, ctypes.c_size_t(len(errbuf)))
    if rc != 0:
        raise engine.VmGpuError(errbuf.value.decode())
    return n_rows.value, scanned.value, engine.last_kernel_ms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_series", nargs="?", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()

    n_series = args.n_series
    ts, vals, offsets = make_columns(n_series)
    start = START + WINDOW
    end = START + (ROWS - 1) * SCRAPE
    n_grid = 1 + (end - start) // STEP
    n_samples = n_series * ROWS
    engine.init()
    res = {"n_series": n_series, "rows": ROWS, "n_grid": int(n_grid),
           "step_ms": STEP, "window_ms": WINDOW,
           "device": engine.device_info()}

    with SeriesBatch(ts, vals, offsets) as batch:
        plan = RollupPlan("avg_over_time", start, end, STEP, window=WINDOW)
        hot_ms, avg_ms, wall_ms = [], [], []
        # alternate the two so they see the same machine state
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            n_rows, scanned, ms = exec_only(batch, start, end, STEP, WINDOW)
            wall = (time.perf_counter() - t0) * 1e3
            batch.exec(plan, download=False)
            if i >= args.warmup:
                hot_ms.append(ms)
                wall_ms.append(wall)
                avg_ms.append(engine.last_kernel_ms())
        hot = float(np.median(hot_ms))
        avg = float(np.median(avg_ms))
        res.update({
            "hot_kernel_ms_median": hot, "hot_kernel_ms_min": min(hot_ms),
            "hot_kernel_ms_max": max(hot_ms),
            "hot_wall_ms_median": float(np.median(wall_ms)),
            "gsamples_per_s": n_samples / hot / 1e6,
            "samples_scanned": scanned, "n_rows": n_rows,
            "rows_per_series": n_rows / n_series,
            "output_bytes": n_rows * int(n_grid) * 8,
            "avg_over_time_kernel_ms_median": avg,
            "avg_over_time_kernel_ms_min": min(avg_ms),
            "ratio_to_avg_over_time": hot / avg,
        })

    if not args.skip_host:
        # host function on a subsample, scaled; the same subsample as its
        # own small batch doubles as a results check at this shape
        sub = np.linspace(0, n_series - 1, HOST_SUBSAMPLE).astype(np.int64)
        mn = MetricName(b"m", [])
        cols = [(ts[s * ROWS:(s + 1) * ROWS], vals[s * ROWS:(s + 1) * ROWS])
                for s in sub]
        t0 = time.perf_counter()
        ref = [rollup_multi.histogram_over_time(t, v, mn, start, end, STEP,
                                                WINDOW) for t, v in cols]
        host_s = time.perf_counter() - t0
        res["host_subsample_s"] = host_s
        res["host_scaled_s"] = host_s * n_series / HOST_SUBSAMPLE
        res["host_scaled_over_device"] = res["host_scaled_s"] * 1e3 / hot
        with SeriesBatch(np.concatenate([t for t, _ in cols]),
                         np.concatenate([v for _, v in cols]),
                         np.arange(HOST_SUBSAMPLE + 1, dtype=np.uint64) * ROWS
                         ) as small:
            rs, rb, values, sc = small.histogram_over_time(start, end, STEP,
                                                           WINDOW)
        ok = sc == sum(x for _, x in ref)
        for s, (series, _) in enumerate(ref):
            idx = np.flatnonzero(rs == s)
            got = {rollup_multi.vmrange_label(int(rb[i])).encode():
                   values[i].view(np.uint64) for i in idx}
            want = {r.mn.get_tag_value(b"vmrange"): r.values.view(np.uint64)
                    for r in series}
            ok = ok and set(got) == set(want) and all(
                np.array_equal(got[k], want[k]) for k in want)
        res["subsample_matches_host"] = bool(ok)

    print(json.dumps(res))


if __name__ == "__main__":
    main()
