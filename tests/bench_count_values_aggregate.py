"""Ad-hoc measurement: the count_values() aggregate on the device
(csrc/aggrcv.hip) over the resident rollup output of a batch, for the three
groupings of a 100 000 x 55 matrix that bench_histogram_aggregate.py uses
and two value sets: an enum of 8 states, and about 900 distinct values a
group (as many as the group's cells allow), near the default limit of 1000.
Beside it, on the same matrix and groups: the histogram() aggregate's batch
form (two passes over the same bytes), vmgpu_colagg SUM (one pass) and the
host function on a subsample.
Run on a GPU box:
    python tests/bench_count_values_aggregate.py [n_series] [--reps N]
                                                 [--skip-host]
Numbers land in profiles/count_values_aggregate.md.

vmgpu_colagg takes a host matrix and reports no kernel time, so SUM is
timed on the wall, upload included; the host-matrix form of count_values
(vmgpu_aggr_count_values_exec, same upload, fetch included) is timed the
same way beside it.  The batch forms are timed by their own hipEvents: no
PCIe inside the bracket."""
import argparse
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from victoriametrics_amd import aggregate, engine  # noqa: E402
from victoriametrics_amd.binary_op import Series  # noqa: E402
from victoriametrics_amd.engine import RollupPlan, SeriesBatch  # noqa: E402
from victoriametrics_amd.metric_name import MetricName  # noqa: E402

START = 1_000_000_000_000
STEP = 60_000
N_GRID = 55
LIMIT = 1000
HOST_SUBSAMPLE = 2000


def make_matrix(n_series, n_distinct, seed=8428):
    """Uniform draws from n_distinct values: small integers for the enum,
    rounded log-normals for the wide set (non-negative, so the histogram
    yardstick classifies every one of them)."""
    rng = np.random.default_rng(seed)
    if n_distinct <= 16:
        pool = np.arange(n_distinct, dtype=np.float64)
    else:
        pool = np.unique(np.round(np.exp(rng.normal(3.0, 2.0, 2 * n_distinct)), 4))
        pool = rng.permutation(pool)[:n_distinct]
    assert len(pool) == n_distinct
    return pool[rng.integers(0, n_distinct, (n_series, N_GRID))]


def csr(group_of, n_groups):
    order = np.argsort(group_of, kind="stable")
    offsets = np.zeros(n_groups + 1, dtype=np.uint64)
    np.cumsum(np.bincount(group_of, minlength=n_groups), out=offsets[1:])
    return np.ascontiguousarray(order, dtype=np.uint32), offsets


def _batch_exec(symbol, batch, group_rows, group_offsets, *extra):
    lib = engine._load_lib()
    n_rows = ctypes.c_uint64(0)
    errbuf = ctypes.create_string_buffer(256)
    rc = getattr(lib, symbol)(
        ctypes.c_uint64(batch.handle),
        group_rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
        group_offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        ctypes.c_uint32(len(group_offsets) - 1), *extra, ctypes.byref(n_rows),
        errbuf, ctypes.c_size_t(len(errbuf)))
    if rc != 0:
        raise engine.VmGpuError(errbuf.value.decode())
    return n_rows.value, engine.last_kernel_ms()


def cv_exec_only(batch, group_rows, group_offsets):
    """vmgpu_batch_aggr_count_values_exec without the fetch."""
    return _batch_exec("vmgpu_batch_aggr_count_values_exec", batch, group_rows,
                       group_offsets, ctypes.c_uint32(LIMIT))


def hist_exec_only(batch, group_rows, group_offsets):
    engine._upload_vmrange_thresholds(engine._load_lib())
    return _batch_exec("vmgpu_batch_aggr_histogram_exec", batch, group_rows,
                       group_offsets)


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)),
            "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_series", nargs="?", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--sets", default="enum8,wide900",
                    help="value sets to run (a profiler run takes one)")
    ap.add_argument("--skip-yardsticks", action="store_true",
                    help="time only the count_values batch form")
    args = ap.parse_args()

    n = args.n_series
    engine.init()
    res = {"n_series": n, "n_grid": N_GRID, "limit": LIMIT,
           "device": engine.device_info(), "cases": {}}

    # a batch whose last_over_time output IS the matrix: one sample on every
    # grid point, window = step
    ts = np.tile(START + np.arange(N_GRID, dtype=np.int64) * STEP, n)
    offsets = np.arange(n + 1, dtype=np.uint64) * N_GRID
    end = START + (N_GRID - 1) * STEP
    ids = np.arange(n, dtype=np.int32)
    groupings = {
        "one_group": (np.zeros(n, np.int32), 1),
        "1000_groups": (ids % 1000, 1000),
        "groups_of_2": (ids // 2, (n + 1) // 2),
    }
    enum_values = None
    for set_name, n_distinct in (("enum8", 8), ("wide900", 900)):
        if set_name not in args.sets.split(","):
            continue
        values = make_matrix(n, n_distinct)
        with SeriesBatch(ts, values.reshape(-1), offsets) as batch:
            plan = RollupPlan("last_over_time", START, end, STEP, window=STEP)
            batch.exec(plan, download=False)
            resident, _ = batch.fetch_out(n, N_GRID)
            assert np.array_equal(resident.view(np.uint64), values.view(np.uint64))
            values = resident  # every form below sees the very same matrix
            if enum_values is None:
                enum_values = values
            for name, (group_of, n_groups) in groupings.items():
                gr, go = csr(group_of, n_groups)
                cv_ms, hist_ms, cv_wall, sum_wall = [], [], [], []
                hist_rows = None
                # alternate the forms so they see the same machine state
                for i in range(args.warmup + args.reps):
                    n_rows, ms = cv_exec_only(batch, gr, go)
                    if not args.skip_yardsticks:
                        hist_rows, hms = hist_exec_only(batch, gr, go)
                    if i >= args.warmup:
                        cv_ms.append(ms)
                        if not args.skip_yardsticks:
                            hist_ms.append(hms)
                    # the wall-clock forms move the matrix and the whole
                    # result over PCIe: a few repetitions each, one warm-up
                    if not args.skip_yardsticks and i <= args.wall_reps:
                        t0 = time.perf_counter()
                        engine.aggr_count_values(values, gr, go, LIMIT)
                        t1 = time.perf_counter()
                        engine.colagg("sum", values, gr, go)
                        t2 = time.perf_counter()
                        if i >= 1:
                            cv_wall.append((t1 - t0) * 1e3)
                            sum_wall.append((t2 - t1) * 1e3)
                case = {
                    "n_groups": n_groups, "n_rows": n_rows,
                    "batch_kernel_ms": stats(cv_ms),
                    "gvalues_per_s": n * N_GRID / np.median(cv_ms) / 1e6,
                }
                if not args.skip_yardsticks:
                    case.update({
                        "histogram_rows": hist_rows,
                        "histogram_batch_kernel_ms": stats(hist_ms),
                        "kernel_ratio_to_histogram": float(
                            np.median(cv_ms) / np.median(hist_ms)),
                        "host_matrix_wall_ms": stats(cv_wall),
                        "colagg_sum_wall_ms": stats(sum_wall),
                        "wall_ratio_to_sum": float(np.median(cv_wall) /
                                                   np.median(sum_wall)),
                    })
                res["cases"][f"{set_name}/{name}"] = case

    if not args.skip_host and enum_values is not None:
        # the parent's only way to this result, on HOST_SUBSAMPLE series of
        # the enum matrix as one group, scaled linearly to n
        sub = np.linspace(0, n - 1, HOST_SUBSAMPLE).astype(np.int64)
        named = [(MetricName(b"m", [(b"s", b"%d" % s)]), enum_values[s])
                 for s in sub]

        def fresh():
            return [Series(mn.copy(), v.copy()) for mn, v in named]

        t0 = time.perf_counter()
        want = aggregate.count_values("v", fresh())
        host_s = time.perf_counter() - t0
        got = aggregate.count_values_device("v", fresh())

        def as_map(ss):
            return {s.mn.marshal_sorted(): s.values.view(np.uint64).tobytes()
                    for s in ss}

        res["host_subsample_series"] = HOST_SUBSAMPLE
        res["host_subsample_s"] = host_s
        res["host_scaled_s"] = host_s * n / HOST_SUBSAMPLE
        res["host_scaled_over_device_one_group"] = (
            res["host_scaled_s"] * 1e3 /
            res["cases"]["enum8/one_group"]["batch_kernel_ms"]["median"])
        res["subsample_matches_host"] = bool(
            len(got) == len(want) and as_map(got) == as_map(want))

    print(json.dumps(res))


if __name__ == "__main__":
    main()
