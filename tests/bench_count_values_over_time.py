"""Ad-hoc measurement: count_values_over_time(m[5m]) on the device over a
resident batch (csrc/cvot.hip), next to avg_over_time on the same batch and
grid (it reads the same columns) and to the host function on a subsample.
Two workloads on the 240-sample, step 60 s, window 300 s shape:
  enum      100 000 series of 2-8 state / HTTP codes held for geometric run
            lengths — what the function is used for
  distinct  2 000 all-distinct gauges — the worst case, one row per covered
            sample, about as many output rows as the enum workload
Run on a GPU box:
    python tests/bench_count_values_over_time.py [--workload enum|distinct|both]
                                                 [--reps N] [--skip-host]
Prints one JSON line per workload.  Numbers land in
profiles/count_values_over_time.md."""
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
CODE_POOL = np.asarray([0.0, 1.0, 2.0, 3.0, 4.0, 200.0, 204.0, 301.0, 400.0,
                        404.0, 500.0, 503.0])
WORKLOADS = {"enum": 100_000, "distinct": 2_000}


def _timestamps(rng, n_series):
    return (START + np.arange(ROWS, dtype=np.int64)[None, :] * SCRAPE +
            rng.integers(-500, 500, (n_series, ROWS))).astype(np.int64)


def make_enum_columns(n_series, seed=1490):
    """Every series draws 2-8 codes from CODE_POOL and holds each for a
    geometric run length (mean 12 scrapes)."""
    rng = np.random.default_rng(seed)
    ts = _timestamps(rng, n_series)
    k = rng.integers(2, 9, n_series)
    # a per-series choice of codes: the first k[s] entries of a permutation
    perm = np.argsort(rng.random((n_series, len(CODE_POOL))), axis=1)
    change = rng.random((n_series, ROWS)) < 1.0 / 12.0
    draw = rng.integers(0, 1 << 30, (n_series, ROWS))
    draw[~change] = 0
    # state index = the last draw at or before the sample
    last = np.maximum.accumulate(
        np.where(change, np.arange(ROWS)[None, :], 0), axis=1)
    state = np.take_along_axis(draw, last, axis=1) % k[:, None]
    vals = CODE_POOL[np.take_along_axis(perm, state, axis=1)]
    offsets = np.arange(n_series + 1, dtype=np.uint64) * ROWS
    return ts.reshape(-1), vals.reshape(-1), offsets


def make_distinct_columns(n_series, seed=1491):
    """Log-normal gauges: every sample of a series is its own value."""
    rng = np.random.default_rng(seed)
    ts = _timestamps(rng, n_series)
    med = 10.0 ** rng.uniform(-2.0, 4.0, (n_series, 1))
    vals = med * np.exp(rng.normal(0.0, 0.5, (n_series, ROWS)))
    offsets = np.arange(n_series + 1, dtype=np.uint64) * ROWS
    return ts.reshape(-1), vals.reshape(-1), offsets


def exec_only(batch, start, end, step, window):
    """vmgpu_count_values_over_time_exec without the fetch: the result
    stays resident, as a caller chaining device stages would leave it."""
    lib = engine._load_lib()
    n_rows = ctypes.c_uint64(0)
    scanned = ctypes.c_uint64(0)
    errbuf = ctypes.create_string_buffer(256)
    rc = lib.vmgpu_count_values_over_time_exec(
        ctypes.c_uint64(batch.handle), ctypes.c_int64(start),
        ctypes.c_int64(end), ctypes.c_int64(step), ctypes.c_int64(window),
        ctypes.c_int32(1), ctypes.c_uint64(0), ctypes.byref(n_rows),
        ctypes.byref(scanned), errbuf, ctypes.c_size_t(len(errbuf)))
    if rc != 0:
        raise engine.VmGpuError(errbuf.value.decode())
    return n_rows.value, scanned.value, engine.last_kernel_ms()


def run(workload, n_series, reps, warmup, skip_host):
    make = make_enum_columns if workload == "enum" else make_distinct_columns
    ts, vals, offsets = make(n_series)
    start = START + WINDOW
    end = START + (ROWS - 1) * SCRAPE
    n_grid = 1 + (end - start) // STEP
    n_samples = n_series * ROWS
    res = {"workload": workload, "n_series": n_series, "rows": ROWS,
           "n_grid": int(n_grid), "step_ms": STEP, "window_ms": WINDOW,
           "device": engine.device_info()}

    with SeriesBatch(ts, vals, offsets) as batch:
        plan = RollupPlan("avg_over_time", start, end, STEP, window=WINDOW)
        cv_ms, avg_ms, wall_ms = [], [], []
        # alternate the two so they see the same machine state
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            n_rows, scanned, ms = exec_only(batch, start, end, STEP, WINDOW)
            wall = (time.perf_counter() - t0) * 1e3
            batch.exec(plan, download=False)
            if i >= warmup:
                cv_ms.append(ms)
                wall_ms.append(wall)
                avg_ms.append(engine.last_kernel_ms())
        cv = float(np.median(cv_ms))
        avg = float(np.median(avg_ms))
        res.update({
            "cvot_kernel_ms_median": cv, "cvot_kernel_ms_min": min(cv_ms),
            "cvot_kernel_ms_max": max(cv_ms),
            "cvot_wall_ms_median": float(np.median(wall_ms)),
            "gsamples_per_s": n_samples / cv / 1e6,
            "samples_scanned": scanned, "n_rows": n_rows,
            "rows_per_series": n_rows / n_series,
            "output_bytes": n_rows * int(n_grid) * 8,
            "avg_over_time_kernel_ms_median": avg,
            "avg_over_time_kernel_ms_min": min(avg_ms),
            "avg_over_time_kernel_ms_max": max(avg_ms),
            "ratio_to_avg_over_time": cv / avg,
        })

    if not skip_host:
        # host function on a subsample, scaled; the same subsample as its
        # own small batch doubles as a results check at this shape
        sub = np.linspace(0, n_series - 1, HOST_SUBSAMPLE).astype(np.int64)
        mn = MetricName(b"m", [])
        cols = [(ts[s * ROWS:(s + 1) * ROWS], vals[s * ROWS:(s + 1) * ROWS])
                for s in sub]
        t0 = time.perf_counter()
        ref = [rollup_multi.count_values_over_time(
            "v", t, v, mn, start, end, STEP, WINDOW) for t, v in cols]
        host_s = time.perf_counter() - t0
        res["host_subsample_s"] = host_s
        res["host_scaled_s"] = host_s * n_series / HOST_SUBSAMPLE
        res["host_scaled_over_device"] = res["host_scaled_s"] * 1e3 / cv
        with SeriesBatch(np.concatenate([t for t, _ in cols]),
                         np.concatenate([v for _, v in cols]),
                         np.arange(HOST_SUBSAMPLE + 1, dtype=np.uint64) * ROWS
                         ) as small:
            rs, rv, values, sc = small.count_values_over_time(
                start, end, STEP, WINDOW)
        ok = sc == sum(x for _, x in ref)
        for s, (series, _) in enumerate(ref):
            idx = np.flatnonzero(rs == s)
            got = {rollup_multi.format_go_float_g(float(rv[i])).encode():
                   values[i].view(np.uint64) for i in idx}
            want = {r.mn.get_tag_value(b"v"): r.values.view(np.uint64)
                    for r in series}
            ok = ok and set(got) == set(want) and all(
                np.array_equal(got[k], want[k]) for k in want)
        res["subsample_matches_host"] = bool(ok)

    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["enum", "distinct", "both"],
                    default="both")
    ap.add_argument("--n-series", type=int, default=0,
                    help="override the workload's series count")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    engine.init()
    names = ["enum", "distinct"] if args.workload == "both" else [args.workload]
    for w in names:
        run(w, args.n_series or WORKLOADS[w], args.reps, args.warmup,
            args.skip_host)


if __name__ == "__main__":
    main()
