#!/usr/bin/env python3
"""bench.py — flagship benchmark: vmselect rollup hot path on MI355X.

Workload (BASELINE.json configs[1]): rate(metric[5m])[1h:15s] over 1M
synthetic counter series x 240 samples, f64, per GPU.  A "step" is one pass
of the hot path over one resident batch: removeCounterResets + rollup grid
evaluation over all series (the RunParallel seam, eval.go:1927/1968).

  python bench.py --gpus N --steps K --warmup W [--series S] [--aggr sum]
                  [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line.
--dump-outputs DIR then writes what the last timed step computed as
DIR/<name>.npy (a fixed seeded sample of rows where the output is large;
NaN points are zeroed and marked in <name>_nonfinite.npy), so two builds
can be compared output for output: the inputs depend on the arguments
alone.  --full adds the secondary measurements, which take
runs of their own: cpu_baseline, cold_query and grouped (each null in the
line of a plain run).

N>1 runs under torchrun (one rank per GPU over RCCL); series are sharded by
seriesID with a full-size shard per rank (weak scaling); the
ungrouped headline path has no data-path collective.  --aggr sum switches to
configs[2] (sum by(pod), 10k groups) whose only exchange is one all-reduce of
the [groups x grid] partial matrices.

Prints ONE JSON line from rank 0 (driver contract), including:
  roofline: achieved = algorithmic bytes/launch / HIP-event kernel time
            of the timed steps (16 B/sample read + 8 B/grid-point write,
            SURVEY.md §8d)
  cpu_baseline (--full): the CPU oracle (kind "port") on the host cores
            over a bounded subsample of the same workload
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEP_MS = 15_000
WINDOW_MS = 300_000
START_TS = 1_600_000_000_000
HBM_PEAK_GBS = 8000.0  # gfx950 spec peak (MI355X_MICROARCH.md)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=240)
    ap.add_argument("--func", type=str, default="rate")
    ap.add_argument("--aggr", type=str, default="none",
                    choices=["none", "sum", "min", "max", "avg", "count"])
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR/*.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (CPU baseline, "
                         "cold query, grouped config 3)")
    ap.add_argument("--cpu-baseline-target-s", type=float, default=15.0)
    ap.add_argument("--skip-cpu-baseline", action="store_true")
    ap.add_argument("--skip-cold", action="store_true",
                    help="skip the end-to-end cold-query measurement")
    ap.add_argument("--cold-queries", type=int, default=5)
    ap.add_argument("--skip-grouped", action="store_true",
                    help="skip the secondary grouped (config 3) measurement")
    ap.add_argument("--grouped-steps", type=int, default=4)
    return ap.parse_args()


def cpu_baseline(args, plan_c, ts, vals, offsets, n_grid):
    """Time the CPU oracle (the reference algorithm restated in C, OpenMP)
    on a bounded subsample; reported, not the target."""
    import oracle
    cores = os.cpu_count() or 1
    n_series = len(offsets) - 1
    # calibrate on 4k series, then size the sample for the target seconds
    probe = min(4096, n_series)
    rc = oracle.RollupConfigC(
        func=plan_c.func, may_adjust_window=plan_c.may_adjust_window,
        start=plan_c.start, end=plan_c.end, step=plan_c.step,
        window=plan_c.window, lookback_delta=plan_c.lookback_delta,
        min_staleness_interval=plan_c.min_staleness_interval,
        is_default_rollup=plan_c.is_default_rollup,
        samples_scanned_per_call=plan_c.samples_scanned_per_call,
        arg=plan_c.arg)

    def run(n):
        off = offsets[:n + 1]
        t0 = time.perf_counter()
        oracle.rollup_eval_batch(
            rc, ts[:int(off[-1])], vals[:int(off[-1])], off,
            remove_counter_resets=bool(plan_c.remove_counter_resets),
            drop_stale_nans=bool(plan_c.drop_stale_nans),
            n_threads=cores)
        return time.perf_counter() - t0

    run(probe)  # warm (OpenMP spawn + page faults)
    t_probe = run(probe)
    per_series = t_probe / probe
    n_target = int(min(n_series, max(probe, args.cpu_baseline_target_s / per_series)))
    t = run(n_target)
    sps = (n_target * args.samples) / t
    return {
        "value": sps,
        "unit": "samples/s",
        "cores": cores,
        "kind": "port",
        "sample": f"{n_target} of {n_series} series x {args.samples} samples, "
                  f"{t:.2f}s wall",
        "basis": f"rate measured on that subsample with {cores} OpenMP "
                 "threads and reported as-is (per-series work is uniform; "
                 "no further extrapolation applied)",
    }


def cold_query(args, engine, plan, ts, vals, offsets):
    """End-to-end cold query at the same shape: synthetic COMPRESSED block
    payload (packed stream) -> native C descriptor parse
    (vmgpu_batch_create_packed) -> PCIe -> device decode+merge -> resident
    batch -> rollup -> full result matrix back on the host.  The payload
    generation (oracle.pack_blocks — the encode side the product does not
    ship) happens outside the timed region, like synth data generation."""
    import oracle
    vals_int = vals.astype(np.int64)  # synthetic counters are whole numbers
    packed, n_blocks, sbs = oracle.pack_blocks(ts, vals_int, offsets)
    samples = len(ts)
    n_series = len(offsets) - 1
    # payload and result live in PINNED buffers (vmgpu_host_alloc) so the
    # PCIe legs run at link rate; the fetch layer writes the stream into the
    # pinned buffer as it assembles it, so the staging copy is untimed.
    pay_buf, pay_ptr = engine.host_alloc(len(packed))
    pay_buf[:] = np.frombuffer(packed, np.uint8)
    out_raw, out_ptr = engine.host_alloc(n_series * plan.n_grid * 8)
    out_view = out_raw.view(np.float64).reshape(n_series, plan.n_grid)
    walls, create_ms, exec_ms = [], [], []
    try:
        for _ in range(args.cold_queries):
            t0 = time.perf_counter()
            b = engine.SeriesBatch.from_packed(pay_buf, n_blocks, sbs)
            t1 = time.perf_counter()
            b.exec(plan, download=True, out_buf=out_view)
            t2 = time.perf_counter()
            b.close()
            walls.append(time.perf_counter() - t0)
            create_ms.append((t1 - t0) * 1e3)
            exec_ms.append((t2 - t1) * 1e3)
    finally:
        engine.host_free(pay_ptr)
        engine.host_free(out_ptr)
    p50 = float(np.median(walls))
    return {
        "p50_ms": p50 * 1e3,
        "p50_create_ms": float(np.median(create_ms)),
        "p50_exec_download_ms": float(np.median(exec_ms)),
        "walls_ms": [round(w * 1e3, 1) for w in walls],
        "create_walls_ms": [round(w, 1) for w in create_ms],
        "samples_per_s": samples / p50,
        "queries": args.cold_queries,
        "payload_bytes": len(packed),
        "pipeline": "packed compressed blocks (pinned) -> native C "
                    "descriptor parse -> PCIe -> device decode+merge -> "
                    "rollup -> result matrix in pinned host memory",
    }


def grouped_probe(args, engine, ts, vals, offsets, end):
    """Secondary measurement in the same driver-run line: BASELINE
    configs[2] (sum by(pod)(rate(m[5m])), 10k label groups) on its own
    group-relayouted batch; kernel-resident like the headline."""
    gids = (np.arange(args.series) % args.groups).astype(np.int32)
    plan = engine.RollupPlan(args.func, START_TS, end, STEP_MS,
                             window=WINDOW_MS, aggr="sum")
    b = engine.SeriesBatch(ts, vals, offsets, group_ids=gids,
                           n_groups=args.groups)
    try:
        for _ in range(2):
            b.exec(plan, download=False)
        t0 = time.perf_counter()
        kms = 0.0
        for _ in range(args.grouped_steps):
            b.exec(plan, download=False)
            kms += engine.last_kernel_ms()
        wall = time.perf_counter() - t0
    finally:
        b.close()
    kernel_s = kms / args.grouped_steps / 1e3
    algo = args.series * args.samples * 16 + args.groups * args.samples * 16
    achieved = algo / kernel_s / 1e9 if kernel_s > 0 else 0.0
    return {
        "workload": "sum by(pod)(rate(metric[5m])) over 1M series / "
                    f"{args.groups} groups",
        "steps": args.grouped_steps,
        "kernel_ms": kernel_s * 1e3,
        "ms_per_step": wall / args.grouped_steps * 1e3,
        "samples_per_s": args.series * args.samples / (wall / args.grouped_steps),
        "roofline": {"bound": "hbm", "achieved": achieved,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS,
                     "algorithmic_bytes": algo},
    }


DUMP_MAX_BYTES = 16 << 20  # per matrix; its float32 mask adds half of it


def dump_outputs(dirname, batch, last, n_grid, grouped):
    """Write what the last timed step returned to its caller as
    DIR/<name>.npy.  The ungrouped step leaves its [series x grid] matrix
    on the device, where a caller reads it with fetch_out; it is far larger
    than the budget, so a fixed seeded sample of its rows is kept (the same
    rows on every run, in ascending order).  Grouped steps return the
    [groups x grid] values and counts.

    A rollup has NaN wherever a grid point has no value (too few samples in
    its window), so every matrix is written as two finite arrays:
    <name>.npy (float64, 0.0 at the points without a finite value) and
    <name>_nonfinite.npy (float32: 0 finite, 1 NaN, 2 +Inf, 3 -Inf)."""
    os.makedirs(dirname, exist_ok=True)

    def save(name, a):
        np.save(os.path.join(dirname, name + ".npy"), a)

    def save_matrix(name, a):
        keep = DUMP_MAX_BYTES // (a.shape[1] * 8)
        if a.shape[0] > keep:
            rows = np.random.default_rng(8428).choice(a.shape[0], size=keep,
                                                      replace=False)
            a = a[np.sort(rows)]
        a = np.ascontiguousarray(a, dtype=np.float64)
        kind = np.zeros(a.shape, dtype=np.float32)
        kind[np.isnan(a)] = 1
        kind[a == np.inf] = 2
        kind[a == -np.inf] = 3
        save(name, np.where(kind == 0, a, 0.0))
        save(name + "_nonfinite", kind)

    if grouped:
        save_matrix("aggr_values", last["out"])
        save_matrix("aggr_counts", last["counts"])
    else:
        out, _ = batch.fetch_out(batch.n_series, n_grid)
        save_matrix("rollup_values", out)
    # exact in float64: far below 2**53
    save("samples_scanned", np.array([last["scanned"]], dtype=np.float64))


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    # VMGPU_FORCE_DIST=1 exercises the RCCL init/exchange path even at
    # world size 1 (single-GPU de-risking of the multi-GPU code)
    distributed = world > 1 or (os.environ.get("VMGPU_FORCE_DIST") == "1"
                                and "RANK" in os.environ)

    import torch
    if distributed:
        import torch.distributed as dist
        dist.init_process_group("nccl")
        torch.cuda.set_device(local_rank)

    from victoriametrics_amd import engine, synth
    engine.init(local_rank)

    n_grid = args.samples  # grid has one point per scrape slot (1h @ 15s)
    end = START_TS + (n_grid - 1) * STEP_MS
    grouped = args.aggr != "none"

    ts, vals, offsets = synth.counter_batch(
        args.series, args.samples, START_TS, step=STEP_MS,
        seed=8428 + rank)
    gids = None
    if grouped:
        gids = (np.arange(args.series) % args.groups).astype(np.int32)

    plan = engine.RollupPlan(args.func, START_TS, end, STEP_MS, window=WINDOW_MS,
                             aggr=args.aggr,
                             skip_finalize=grouped and distributed)
    batch = engine.SeriesBatch(ts, vals, offsets, group_ids=gids,
                               n_groups=args.groups if grouped else 0)

    last = {}  # what the latest step handed its caller (--dump-outputs)

    def one_step():
        out, counts, scanned = batch.exec(plan, download=grouped)
        if grouped and distributed:
            import torch.distributed as dist
            tv = torch.from_numpy(out).cuda(local_rank)
            tc = torch.from_numpy(counts).cuda(local_rank)
            dist.all_reduce(tv)  # SUM (sum/avg/count); one 19 MB exchange
            dist.all_reduce(tc)
            counts = tc.cpu().numpy()
            out = engine.aggr_finalize(args.aggr, tv.cpu().numpy(), counts)
        last.update(out=out, counts=counts, scanned=scanned)
        return engine.last_kernel_ms()

    # warmup
    for _ in range(args.warmup):
        one_step()

    if distributed:
        import torch.distributed as dist
        dist.barrier()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    step_walls = []
    kernel_ms_acc = 0.0
    for _ in range(args.steps):
        s0 = time.perf_counter()
        kernel_ms_acc += one_step()
        step_walls.append(time.perf_counter() - s0)
    if distributed:
        import torch.distributed as dist
        torch.cuda.synchronize()
        dist.barrier()
    elapsed = time.perf_counter() - t0

    if distributed:
        import torch.distributed as dist
        t = torch.tensor([elapsed], dtype=torch.float64).cuda(local_rank)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.cpu().item())

    samples_per_step = args.series * args.samples
    total_samples = world * samples_per_step * args.steps
    value = total_samples / elapsed
    ms_per_step = elapsed / args.steps * 1e3
    p50_ms = float(np.median(step_walls) * 1e3)

    # roofline: dominant kernel = rollup_wave_kernel (HIP-event time per exec)
    avg_kernel_s = kernel_ms_acc / args.steps / 1e3
    # algorithmic traffic per launch: 16 B/sample read +
    # 8 B/grid-point write for the ungrouped rollup; grouped output is
    # negligible (groups x grid).
    read_bytes = samples_per_step * 16
    write_bytes = (args.series * n_grid * 8) if not grouped else (args.groups * n_grid * 16)
    algo_bytes = read_bytes + write_bytes
    achieved_gbs = algo_bytes / avg_kernel_s / 1e9 if avg_kernel_s > 0 else 0.0
    traffic = None
    if os.environ.get("VMGPU_TRAFFIC_BYTES"):
        traffic = float(os.environ["VMGPU_TRAFFIC_BYTES"])

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, batch, last, n_grid, grouped)

    result = None
    if rank == 0:
        cb = None
        if args.full and not args.skip_cpu_baseline and world == 1:
            cb = cpu_baseline(args, plan._c, ts, vals, offsets, n_grid)
        cold = None
        if args.full and not args.skip_cold and world == 1 and not grouped:
            cold = cold_query(args, engine, plan, ts, vals, offsets)
        grouped_info = None
        if args.full and not args.skip_grouped and world == 1 and not grouped:
            grouped_info = grouped_probe(args, engine, ts, vals, offsets, end)
        workload = (f"{args.func}(metric[5m])[1h:15s] over 1M series x 240 samples"
                    if not grouped else
                    "sum by(pod)(rate(metric[5m])) over 1M series / 10k groups")
        result = {
            "metric": "rollup samples/sec",
            "value": value,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "p50_query_latency_ms": p50_ms,
            "p90_query_latency_ms": float(np.percentile(step_walls, 90) * 1e3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (seed 8428: counters, rate~Poisson(10/s), "
                    "15s scrape +/-500ms jitter, reset p=0.01/sample)",
            "config": {
                "workload": workload,
                "series_per_gpu": args.series,
                "samples_per_series": args.samples,
                "grid_points": n_grid,
                "window_ms": WINDOW_MS,
                "step_ms": STEP_MS,
                "aggr": args.aggr,
                "parallelism": f"series-sharded dp{world}",
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved_gbs,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved_gbs / HBM_PEAK_GBS,
                "traffic": traffic,
                "kernel_ms": avg_kernel_s * 1e3,
                "algorithmic_bytes": algo_bytes,
            },
            "cpu_baseline": cb,
            "cold_query": cold,
            "grouped": grouped_info,
        }
        print(json.dumps(result), flush=True)

    batch.close()
    if distributed:
        import torch.distributed as dist
        dist.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
