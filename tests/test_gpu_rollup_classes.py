"""Every rollup function against the oracle on every rollup kernel.

The wave, block and huge kernels stage, compact, scan and seek differently
and share only the device function set of csrc/rollup_device.h.  This suite
runs all of that set through each of them on the tie-heavy class batches of
rollup_classes.py (test_rollup_class_inputs.py shows on the oracle alone that
no function is trivial there), then the argument edges, the plan shapes
(window auto-adjust, instant query, lookback_delta, the rollup_* expansions
with their pre-functions) on the block and huge kernels, more series than
either kernel launches blocks, and one grouped aggregate fed by all three
kernels.

Bar: bit-exact outside POW_FUNCS, rtol 1e-12 inside, NaN
placement equal, samplesScanned equal; 1e-9 for cross-series float sums.
"""
import math

import numpy as np
import pytest

from rollup_classes import (ALL_FUNCS, CLASSES, KINDSETS, LBD, N_GRID,
                            POW_FUNCS, START, STEP, WINDOW_SAMPLES,
                            class_batch, class_reference, class_window,
                            make_plan, oracle_batch)
from seriesgen import TIE_KINDS, assert_parity, tie_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


@pytest.fixture(scope="module")
def resident(engine):
    """Class batches uploaded once and kept resident for the module."""
    cache = {}

    def get(cls, wid, kindset="ties"):
        key = (cls, wid, kindset)
        if key not in cache:
            cache[key] = engine.SeriesBatch(*class_batch(*key))
        return cache[key]

    yield get
    for b in cache.values():
        b.close()


def _check(batch, plan, columns, context, exact=True):
    out, _, scanned = batch.exec(plan)
    ref, _, ref_scanned = oracle_batch(plan, *columns)
    assert scanned == ref_scanned, f"{context}: samplesScanned"
    assert_parity(out, ref, exact=exact, context=context)
    return ref


# ---- every function x length class x window -------------------------------

@pytest.mark.parametrize("kindset", list(KINDSETS))
@pytest.mark.parametrize("wid", list(WINDOW_SAMPLES))
@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("func", ALL_FUNCS)
def test_func_on_class(resident, func, cls, wid, kindset):
    """The "inf" batches found one disagreement: where the window's median
    is infinite, mad_over_time's deviations of the infinite samples are NaN
    and the reference drops them; the device kept them in the rank and
    answered NaN where the reference answers +Inf (fixed in
    vm_dev_quantile_absdev)."""
    plan = make_plan(func, window=class_window(cls, wid))
    out, _, scanned = resident(cls, wid, kindset).exec(plan)
    ref, ref_scanned = class_reference(func, cls, wid, kindset)
    context = f"{func} {cls} {wid} {kindset}"
    assert scanned == ref_scanned, f"{context}: samplesScanned"
    assert_parity(out, ref, exact=func not in POW_FUNCS, context=context)


# ---- argument edges --------------------------------------------------------

_FILTERS = ["count_le", "count_gt", "count_eq", "count_ne", "share_le",
            "share_gt", "share_eq", "sum_le", "sum_gt", "sum_eq"]
ARG_EDGES = (
    [("quantile_over_time", phi, 0.0)
     for phi in (-0.5, 0.0, 0.5, 1.0, 1.5, math.nan)] +
    [("holt_winters", sf, tf)
     for sf, tf in ((0.0, 0.0), (1.0, 1.0), (-0.1, 0.5), (0.5, 1.1),
                    (0.3, 0.4))] +
    [(f, phi, 0.0)
     for f in ("hoeffding_bound_lower", "hoeffding_bound_upper")
     for phi in (-1.0, 0.0, 0.5, 1.0, 2.0)] +
    [("predict_linear", secs, 0.0) for secs in (-3600.0, 0.0, 120.0)] +
    [("duration_over_time", d, 0.0) for d in (0.0, 0.001, 1e9)] +
    [(f + "_over_time", a, 0.0)
     for f in _FILTERS for a in (3.0, -0.0, math.inf, -math.inf, math.nan)])


@pytest.mark.parametrize("func,arg,arg2", ARG_EDGES,
                         ids=[f"{f}-{a!r}-{b!r}" for f, a, b in ARG_EDGES])
def test_argument_edges(resident, func, arg, arg2):
    """The argument is a runtime value every kernel reads the same way: the
    wave class and one block batch."""
    for cls in ("wave", "block"):
        plan = make_plan(func, window=class_window(cls, "w12"), arg=arg,
                         arg2=arg2)
        _check(resident(cls, "w12"), plan, class_batch(cls, "w12", "ties"),
               f"{func}({arg!r}, {arg2!r}) {cls}",
               exact=func not in POW_FUNCS)


# ---- plan shapes on the block and huge kernels -----------------------------

LONG = ("block", "huge")


@pytest.mark.parametrize("cls", LONG)
@pytest.mark.parametrize("func", ["rate", "delta", "avg_over_time",
                                  "default_rollup", "deriv_fast"])
def test_window_autoadjust_long(resident, func, cls):
    """window=0: the per-series scrape interval sizes the window
    (rollup.go:719-756), with and without a lookback_delta."""
    for lbd in (0, 40_000):
        plan = make_plan(func, window=0, lookback_delta=lbd)
        _check(resident(cls, "w12"), plan, class_batch(cls, "w12", "ties"),
               f"{func} {cls} window=0 lbd={lbd}")


@pytest.mark.parametrize("cls", LONG)
@pytest.mark.parametrize("func", ["rate", "increase", "changes",
                                  "default_rollup", "median_over_time"])
def test_instant_query_long(resident, func, cls):
    """start == end at mid-series: maxPrevInterval is the step itself."""
    at = START + (N_GRID // 2) * STEP
    for wid in WINDOW_SAMPLES:
        plan = make_plan(func, start=at, end=at,
                         window=class_window(cls, wid))
        ref = _check(resident(cls, wid), plan, class_batch(cls, wid, "ties"),
                     f"instant {func} {cls} {wid}")
        assert np.isfinite(ref).any()


@pytest.mark.parametrize("cls", LONG)
@pytest.mark.parametrize("func", ["rate", "increase", "increase_pure",
                                  "delta", "changes", "irate", "integrate",
                                  "default_rollup", "avg_over_time",
                                  "tlast_change_over_time"])
def test_lookback_delta_long(resident, func, cls):
    """lookback_delta != 0: removeCounterResets forgets its correction
    across the gap series' hole (staleness = lookback_delta + window), and
    realPrevValue is cut where the previous sample is that far back."""
    for wid in WINDOW_SAMPLES:
        plan = make_plan(func, window=class_window(cls, wid),
                         lookback_delta=LBD)
        _check(resident(cls, wid), plan, class_batch(cls, wid, "ties"),
               f"{func} {cls} {wid} lbd={LBD}")


@pytest.mark.parametrize("cls", LONG)
@pytest.mark.parametrize("parent", ["rollup", "rollup_rate", "rollup_deriv",
                                    "rollup_increase", "rollup_delta",
                                    "rollup_scrape_interval",
                                    "rollup_candlestick"])
def test_rollup_fake_expansions_long(engine, resident, parent, cls):
    """The rollup_* expansions (rollup.go:436-516): the delta, deriv and
    scrape_interval pre-functions rewrite an LDS column in the block kernel
    and a global scratch column in the huge kernel."""
    plans = engine.rollup_fake_plans(parent, START, START + (N_GRID - 1) * STEP,
                                     STEP, window=class_window(cls, "w12"))
    assert len(plans) == (4 if parent == "rollup_candlestick" else 3)
    for tag, plan in plans:
        _check(resident(cls, "w12"), plan, class_batch(cls, "w12", "ties"),
               f"{parent}/{tag} {cls}")


# ---- more series than the block and huge kernels launch blocks -------------

STRIDE_CASES = {
    # name: (series lengths, grid points, window)
    "block": (513 + np.arange(2100) % 8, 40, 4 * STEP),
    "huge": (4065 + np.arange(2049) % 36, 16, 2 * STEP),
}


@pytest.mark.parametrize("name", list(STRIDE_CASES))
def test_series_stride_loop(engine, name):
    """Both kernels launch at most 2048 blocks and walk the series list with
    a grid-wide stride: with more series than that a block reuses its LDS
    column (block kernel) and reads scratch slots past the block count (huge
    kernel).  Every series is its own plateau counter, so a column or slot
    taken from the wrong series shows.  rate takes the compile-time path,
    changes the generic one."""
    lengths, n_grid, window = STRIDE_CASES[name]
    columns = tie_batch(list(lengths), START, n_grid, window, step=STEP,
                        kinds=("counter",), seed=77)
    end = START + (n_grid - 1) * STEP
    with engine.SeriesBatch(*columns) as batch:
        for func in ("rate", "changes"):
            plan = make_plan(func, end=end, window=window)
            ref = _check(batch, plan, columns, f"{name} stride {func}")
            # rows differ, so a misrouted series cannot go unnoticed
            assert len({row.tobytes() for row in ref}) > 0.99 * len(ref)


# ---- one grouped aggregate fed by all three kernels ------------------------

GROUP_LENGTHS = (40, 300, 700, 4100)
N_GROUPS = 5


@pytest.fixture(scope="module")
def mixed_grouped(engine):
    window = 20 * STEP
    columns = tie_batch(GROUP_LENGTHS, START, N_GRID, window, step=STEP,
                        kinds=TIE_KINDS, seed=55)
    lens = np.diff(columns[2].astype(np.int64))
    gids = (np.arange(len(lens)) % N_GROUPS).astype(np.int32)
    gids[0] = -1                        # "not grouped": skipped
    cls_of = np.where(lens <= 512, 0, np.where(lens <= 4064, 1, 2))
    for g in range(N_GROUPS):
        assert set(cls_of[gids == g]) == {0, 1, 2}, g
    batch = engine.SeriesBatch(*columns, group_ids=gids, n_groups=N_GROUPS)
    yield batch, columns, gids, window
    batch.close()


@pytest.mark.parametrize("aggr", ["sum", "min", "max", "avg", "count",
                                  "sum2", "geomean"])
@pytest.mark.parametrize("func", ["rate", "avg_over_time"])
def test_grouped_across_classes(mixed_grouped, func, aggr):
    """Every group has members in the wave, block and huge class, so three
    launches accumulate into one matrix.  min/max/count bit-exact; the float
    sums at 1e-9 (atomic order), as test_grouped_aggregation."""
    batch, columns, gids, window = mixed_grouped
    plan = make_plan(func, window=window, aggr=aggr)
    out, _, scanned = batch.exec(plan)
    ref, _, ref_scanned = oracle_batch(plan, *columns, group_ids=gids,
                                       n_groups=N_GROUPS, aggr=aggr)
    assert scanned == ref_scanned
    assert np.isfinite(ref).mean() > 0.9
    exact = aggr in ("min", "max", "count")
    assert_parity(out, ref, exact=exact, rtol=1e-9,
                  context=f"{aggr}({func}) across classes")
