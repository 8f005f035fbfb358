"""Ad-hoc measurement: the grouped pointwise topk on the device
(csrc/aggrtopk.hip) over the resident rollup output of a batch, on the shape
of profiles/topk_pointwise.md: synth.gauge_batch(100_000, 240, seed=77),
avg_over_time with a 45 s window on a 240-point grid, 100000 x 240 f64
resident.  Three groupings (1 group, 100 groups, 10 000 groups of 10) and two
values of k (10: list class, 100: sort class), not reversed.
Run on a GPU box:
    python tests/bench_topk_grouped.py [n_series] [--reps N] [--skip-host]
Numbers land in profiles/topk_grouped.md.

One process.  The batch form is timed by its own hipEvents (no PCIe inside
the bracket, the fetch of the kept rows is timed apart on the wall).  Beside
it, alternated call by call: vmgpu_topk_pointwise, device only (out = NULL,
host clock around the call, which ends in a stream synchronise; it NaN-fills
the resident output in place, so the output is restored by an untimed exec
before every call of either kind), and the download of the full matrix that
a caller pays today before it can group on the host.  The host
aggregate("topk") runs once on a 2000-series subsample."""
import argparse
import ctypes
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from victoriametrics_amd import aggregate, engine, synth  # noqa: E402
from victoriametrics_amd.binary_op import Series  # noqa: E402
from victoriametrics_amd.engine import RollupPlan, SeriesBatch  # noqa: E402
from victoriametrics_amd.metric_name import MetricName  # noqa: E402

START = 1_000_000_000_000
STEP = 15_000
N_GRID = 240
HOST_SUBSAMPLE = 2000


def csr(group_of, n_groups):
    order = np.argsort(group_of, kind="stable")
    offsets = np.zeros(n_groups + 1, dtype=np.uint64)
    np.cumsum(np.bincount(group_of, minlength=n_groups), out=offsets[1:])
    return np.ascontiguousarray(order, dtype=np.uint32), offsets


def grouped_exec_only(batch, group_rows, group_offsets, ks):
    """vmgpu_batch_aggr_topk_exec without the fetch."""
    lib = engine._load_lib()
    n_rows = ctypes.c_uint64(0)
    errbuf = ctypes.create_string_buffer(256)
    rc = lib.vmgpu_batch_aggr_topk_exec(
        ctypes.c_uint64(batch.handle),
        group_rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
        group_offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        ctypes.c_uint32(len(group_offsets) - 1),
        ks.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        ctypes.c_uint32(len(ks)), ctypes.c_int32(0), ctypes.byref(n_rows),
        errbuf, ctypes.c_size_t(len(errbuf)))
    if rc != 0:
        raise engine.VmGpuError(errbuf.value.decode())
    return n_rows.value, engine.last_kernel_ms()


def pointwise_device_only(batch, k):
    """vmgpu_topk_pointwise with out = NULL, on the wall."""
    lib = engine._load_lib()
    errbuf = ctypes.create_string_buffer(256)
    t0 = time.perf_counter()
    rc = lib.vmgpu_topk_pointwise(ctypes.c_uint64(batch.handle),
                                  ctypes.c_double(k), ctypes.c_int32(0), None,
                                  errbuf, ctypes.c_size_t(len(errbuf)))
    ms = (time.perf_counter() - t0) * 1e3
    if rc != 0:
        raise engine.VmGpuError(errbuf.value.decode())
    return ms


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)),
            "max": float(max(xs)), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_series", nargs="?", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sort-reps", type=int, default=30,
                    help="timed calls of the k = 100 cases")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--only", default="",
                    help="one case, such as k10/1_group (a profiler run)")
    args = ap.parse_args()

    n = args.n_series
    engine.init()
    res = {"n_series": n, "n_grid": N_GRID, "device": engine.device_info(),
           "cases": {}}
    ts, vals, offsets = synth.gauge_batch(n, N_GRID, START, STEP, seed=77)
    plan = RollupPlan("avg_over_time", START, START + (N_GRID - 1) * STEP, STEP,
                      window=45_000)
    ids = np.arange(n, dtype=np.int32)
    groupings = {
        "1_group": (np.zeros(n, np.int32), 1),
        "100_groups": (ids % 100, 100),
        "groups_of_10": (ids // 10, (n + 9) // 10),
    }
    with SeriesBatch(ts, vals, offsets) as batch:
        batch.exec(plan, download=False)
        matrix = np.empty((n, N_GRID))
        download_ms = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            batch.fetch_out_into(matrix, N_GRID)
            if i >= args.warmup:
                download_ms.append((time.perf_counter() - t0) * 1e3)
        res["full_matrix_download_ms"] = stats(download_ms)
        res["full_matrix_mb"] = matrix.nbytes / 1e6

        for k in (10, 100):
            ks = np.full(N_GRID, float(k))
            reps = args.reps if k == 10 else args.sort_reps
            for name, (group_of, n_groups) in groupings.items():
                if args.only and args.only != f"k{k}/{name}":
                    continue
                gr, go = csr(group_of, n_groups)
                grouped_ms, pointwise_ms = [], []
                n_rows = 0
                for i in range(args.warmup + reps):
                    n_rows, ms = grouped_exec_only(batch, gr, go, ks)
                    if i >= args.warmup:
                        grouped_ms.append(ms)
                    if name == "1_group" and not args.only:
                        # the yardstick masks the output in place: time it,
                        # then put the output back for the next grouped call
                        pms = pointwise_device_only(batch, k)
                        batch.exec(plan, download=False)
                        if i >= args.warmup:
                            pointwise_ms.append(pms)
                t0 = time.perf_counter()
                engine._aggr_topk_fetch(engine._load_lib(), n_rows, N_GRID)
                fetch_ms = (time.perf_counter() - t0) * 1e3
                case = {"n_groups": n_groups, "k": k, "n_rows": n_rows,
                        "batch_kernel_ms": stats(grouped_ms),
                        "fetch_kept_rows_ms": fetch_ms,
                        "gvalues_per_s": n * N_GRID / np.median(grouped_ms) / 1e6}
                if pointwise_ms:
                    case["topk_pointwise_device_only_ms"] = stats(pointwise_ms)
                res["cases"][f"k{k}/{name}"] = case

        # the grouped result of one group is the pointwise result
        kept = batch.aggr_topk(np.zeros(n, np.int32), 1, 10)[3]
        res["one_group_kept_cells"] = int((~np.isnan(kept)).sum())
        res["one_group_kept_sum"] = float(np.nansum(kept))

    if not args.skip_host:
        # today's only grouped path, on HOST_SUBSAMPLE series as 100 groups
        sub = np.linspace(0, n - 1, HOST_SUBSAMPLE).astype(np.int64)
        named = [(MetricName(b"m", [(b"g", b"%d" % (s % 100)), (b"s", b"%d" % s)]),
                  matrix[s]) for s in sub]

        def fresh():
            return [Series(mn.copy(), v.copy()) for mn, v in named]

        t0 = time.perf_counter()
        want = aggregate.aggregate("topk", fresh(), "by", (b"g",), arg=10)
        host_s = time.perf_counter() - t0
        got = aggregate.topk_device(fresh(), 10, "by", (b"g",))

        def as_map(ss):
            return {s.mn.marshal_sorted(): s.values.view(np.uint64).tobytes()
                    for s in ss}

        res["host_subsample_series"] = HOST_SUBSAMPLE
        res["host_subsample_s"] = host_s
        res["host_scaled_s"] = host_s * n / HOST_SUBSAMPLE
        # continuous values: no ties, so the two paths keep the same cells
        res["subsample_matches_host"] = bool(
            len(got) == len(want) and as_map(got) == as_map(want))

    print(json.dumps(res))


if __name__ == "__main__":
    main()
