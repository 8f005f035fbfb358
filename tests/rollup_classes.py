"""Batches, plans and oracle references shared by test_rollup_class_inputs.py
(CPU: the inputs are not trivial) and test_gpu_rollup_classes.py (GPU: every
rollup function on every kernel).  Test infrastructure.

The engine picks its kernel by series length: the wave kernel up to 512
samples, the block kernel up to 4064, the huge kernel beyond.  A class batch
holds one series of every kind of seriesgen.tie_batch at each of the class's
lengths, which straddle the class boundaries, the 64-lane tile and odd sizes.
"""
import functools

import numpy as np

import oracle
from seriesgen import INF_KIND, TIE_KINDS, tie_batch

START = 1_000_000_000_000
STEP = 15_000
N_GRID = 300      # more than 256 points: two trips of the block/huge grid loop
END = START + (N_GRID - 1) * STEP
LBD = 5 * STEP    # the lookback_delta of the plan-shape tests

CLASSES = {
    "wave": (1, 2, 63, 64, 65, 257, 512),
    "block": (513, 600, 4064),
    "huge": (4065, 4300),
}
# the length whose cadence sizes the window of its class
REF_LEN = {"wave": 257, "block": 600, "huge": 4300}
WINDOW_SAMPLES = {"w12": 12, "w64": 64}
KINDSETS = {"ties": TIE_KINDS, "inf": (INF_KIND,)}

POW_FUNCS = {"geomean_over_time", "hoeffding_bound_lower",
             "hoeffding_bound_upper"}
ALL_FUNCS = sorted(set(oracle.FUNC_IDS) - {"increase_prometheus", "timestamp",
                                           "timestamp_with_name"})
# arguments from the alphabet 0..5, so the comparisons hit equal samples
ARGS = {
    "quantile_over_time": (0.9, 0.0), "count_le_over_time": (2.0, 0.0),
    "count_gt_over_time": (2.0, 0.0), "count_eq_over_time": (2.0, 0.0),
    "count_ne_over_time": (2.0, 0.0), "share_le_over_time": (2.0, 0.0),
    "share_gt_over_time": (2.0, 0.0), "share_eq_over_time": (2.0, 0.0),
    "sum_le_over_time": (2.0, 0.0), "sum_gt_over_time": (2.0, 0.0),
    "sum_eq_over_time": (2.0, 0.0), "predict_linear": (120.0, 0.0),
    "duration_over_time": (60.0, 0.0), "hoeffding_bound_lower": (0.9, 0.0),
    "hoeffding_bound_upper": (0.9, 0.0), "holt_winters": (0.3, 0.4),
}


def class_window(cls, wid):
    """Window in ms holding about WINDOW_SAMPLES[wid] samples of the class's
    reference length.  With cadence = (grid + window) / (n - 1), a window of
    W cadences solves to W * grid / (n - 1 - W).  w12 is rounded to a step
    multiple where it exceeds a step (the rate kernels' shared-boundary
    cache needs that) and to a second otherwise; w64 is pushed 7 s off the
    step multiple, so both rate paths run."""
    w_samples = WINDOW_SAMPLES[wid]
    grid = (N_GRID - 1) * STEP
    w = w_samples * grid / (REF_LEN[cls] - 1 - w_samples)
    if w >= STEP:
        w = int(round(w / STEP)) * STEP
        if wid == "w64":
            w += 7_000
    else:
        w = max(1_000, int(round(w / 1_000)) * 1_000)
    return w


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def class_batch(cls, wid, kindset):
    """Flat ts, vals, offsets of one class batch (read-only, built once)."""
    window = class_window(cls, wid)
    seed = 1000 + 10 * sorted(CLASSES).index(cls) + sorted(KINDSETS).index(kindset)
    return _frozen(*tie_batch(CLASSES[cls], START, N_GRID, window, step=STEP,
                              kinds=KINDSETS[kindset], gap=window + LBD + 2 * STEP,
                              seed=seed))


def series_labels(cls, kindset):
    """(length, kind) of every series of class_batch, in batch order."""
    return [(n, k) for n in CLASSES[cls] for k in KINDSETS[kindset]]


def make_plan(func, start=START, end=END, window=0, **kwargs):
    from victoriametrics_amd.engine import RollupPlan
    arg, arg2 = ARGS.get(func, (0.0, 0.0))
    kwargs.setdefault("arg", arg)
    kwargs.setdefault("arg2", arg2)
    return RollupPlan(func, start, end, STEP, window=window, **kwargs)


def oracle_batch(plan, ts, vals, offsets, group_ids=None, n_groups=0,
                 aggr="none", n_threads=4):
    """The oracle under exactly the flags the engine plan carries."""
    c = plan._c
    rc = oracle.RollupConfigC(
        func=c.func, may_adjust_window=c.may_adjust_window, start=c.start,
        end=c.end, step=c.step, window=c.window,
        lookback_delta=c.lookback_delta,
        min_staleness_interval=c.min_staleness_interval,
        is_default_rollup=c.is_default_rollup,
        samples_scanned_per_call=c.samples_scanned_per_call,
        arg=c.arg, arg2=c.arg2)
    return oracle.rollup_eval_batch(
        rc, ts, vals, offsets, group_ids=group_ids, n_groups=n_groups,
        aggr=aggr, remove_counter_resets=bool(c.remove_counter_resets),
        max_staleness_interval=c.max_staleness_interval,
        drop_stale_nans=bool(c.drop_stale_nans), n_threads=n_threads,
        pre_func=c.pre_func)


@functools.lru_cache(maxsize=None)
def class_reference(func, cls, wid, kindset):
    """Oracle output and samplesScanned of func over a class batch with the
    class window set explicitly (read-only, computed once)."""
    plan = make_plan(func, window=class_window(cls, wid))
    ref, _, scanned = oracle_batch(plan, *class_batch(cls, wid, kindset))
    ref.setflags(write=False)
    return ref, scanned
