"""Ad-hoc measurement: the histogram() aggregate on the device
(csrc/aggrhist.hip) over the resident rollup output of a batch, for three
groupings of the same 100 000 x 55 matrix, next to vmgpu_colagg SUM over
the same matrix and groups and to the host function on a subsample.
Run on a GPU box:
    python tests/bench_histogram_aggregate.py [n_series] [--reps N]
                                              [--skip-host]
Numbers land in profiles/histogram_aggregate.md.

vmgpu_colagg takes a host matrix and reports no kernel time, so SUM is
timed on the wall, upload included; the host-matrix form of the histogram
(vmgpu_aggr_histogram_exec, same upload) is timed the same way beside it.
The batch form is timed by its own hipEvents: no PCIe inside the bracket."""
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
HOST_SUBSAMPLE = 2000


def make_matrix(n_series, seed=8428):
    """Log-normal values: per-series median log-uniform over [1e-2, 1e4],
    sigma 0.5, as the histogram_over_time measurement uses."""
    rng = np.random.default_rng(seed)
    med = 10.0 ** rng.uniform(-2.0, 4.0, (n_series, 1))
    return med * np.exp(rng.normal(0.0, 0.5, (n_series, N_GRID)))


def csr(group_of, n_groups):
    order = np.argsort(group_of, kind="stable")
    offsets = np.zeros(n_groups + 1, dtype=np.uint64)
    np.cumsum(np.bincount(group_of, minlength=n_groups), out=offsets[1:])
    return np.ascontiguousarray(order, dtype=np.uint32), offsets


def batch_exec_only(batch, group_rows, group_offsets):
    """vmgpu_batch_aggr_histogram_exec without the fetch."""
    lib = engine._load_lib()
    engine._upload_vmrange_thresholds(lib)
    n_rows = ctypes.c_uint64(0)
    errbuf = ctypes.create_string_buffer(256)
    rc = lib.vmgpu_batch_aggr_histogram_exec(
        ctypes.c_uint64(batch.handle),
        group_rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
        group_offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        ctypes.c_uint32(len(group_offsets) - 1), ctypes.byref(n_rows), errbuf,
        ctypes.c_size_t(len(errbuf)))
    if rc != 0:
        raise engine.VmGpuError(errbuf.value.decode())
    return n_rows.value, engine.last_kernel_ms()


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)),
            "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_series", nargs="?", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()

    n = args.n_series
    values = make_matrix(n)
    engine.init()
    res = {"n_series": n, "n_grid": N_GRID, "device": engine.device_info(),
           "cases": {}}

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
    with SeriesBatch(ts, values.reshape(-1), offsets) as batch:
        plan = RollupPlan("last_over_time", START, end, STEP, window=STEP)
        batch.exec(plan, download=False)
        resident, _ = batch.fetch_out(n, N_GRID)
        res["resident_equals_input"] = bool(
            np.array_equal(resident.view(np.uint64), values.view(np.uint64)))
        values = resident  # every form below sees the very same matrix
        for name, (group_of, n_groups) in groupings.items():
            gr, go = csr(group_of, n_groups)
            k_ms, hist_wall, sum_wall = [], [], []
            # alternate the three so they see the same machine state
            for i in range(args.warmup + args.reps):
                n_rows, ms = batch_exec_only(batch, gr, go)
                t0 = time.perf_counter()
                engine.aggr_histogram(values, gr, go)
                t1 = time.perf_counter()
                engine.colagg("sum", values, gr, go)
                t2 = time.perf_counter()
                if i >= args.warmup:
                    k_ms.append(ms)
                    hist_wall.append((t1 - t0) * 1e3)
                    sum_wall.append((t2 - t1) * 1e3)
            res["cases"][name] = {
                "n_groups": n_groups, "n_rows": n_rows,
                "batch_kernel_ms": stats(k_ms),
                "gvalues_per_s": n * N_GRID / np.median(k_ms) / 1e6,
                "host_matrix_wall_ms": stats(hist_wall),
                "colagg_sum_wall_ms": stats(sum_wall),
                "wall_ratio_to_sum": float(np.median(hist_wall) /
                                           np.median(sum_wall)),
            }

    if not args.skip_host:
        sub = np.linspace(0, n - 1, HOST_SUBSAMPLE).astype(np.int64)
        named = [(MetricName(b"m", [(b"s", b"%d" % s)]), values[s]) for s in sub]

        def fresh():
            return [Series(mn.copy(), v.copy()) for mn, v in named]

        t0 = time.perf_counter()
        want = aggregate.histogram_aggregate(fresh())
        host_s = time.perf_counter() - t0
        got = aggregate.histogram_aggregate_device(fresh())

        def as_map(ss):
            return {s.mn.marshal_sorted(): s.values.view(np.uint64).tobytes()
                    for s in ss}

        res["host_subsample_s"] = host_s
        res["host_scaled_s"] = host_s * n / HOST_SUBSAMPLE
        res["host_scaled_over_device_one_group"] = (
            res["host_scaled_s"] * 1e3 /
            res["cases"]["one_group"]["batch_kernel_ms"]["median"])
        res["subsample_matches_host"] = bool(
            len(got) == len(want) and as_map(got) == as_map(want))

    print(json.dumps(res))


if __name__ == "__main__":
    main()
