"""The pipelined rate kernel's boundary probe and the time held in its series
slab (rollup_pipe_kernel, csrc/pipe_probe.h): every answer class of the
probe, grids far from the series, series spans on both sides of 2^31 ms,
timestamps below zero and near 2^62, the slab's other producers (compaction, LDS scan, slab-derived scrape
interval), the scan's staleness-gap test and the loops besides the fused one.

Every input meets the host's pipe gating (rate / deriv_fast, series of at most
256 samples, window > 0 and a multiple of step, n_grid > 1), so these cases
run through the pipe kernel; results are compared bit for bit with the oracle.
At most 64 series, 256 samples and 300 grid points per case.
"""
import numpy as np
import pytest

import oracle
from seriesgen import assert_parity

pytestmark = pytest.mark.gpu

START = 1_000_000_000_000
STEP = 15_000
DAY = 86_400_000
LIMIT = (1 << 31) - 2          # a span just inside the 31-bit dt path (< 2^31)


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


def _oracle_batch(plan, ts, vals, offsets, group_ids=None, n_groups=0,
                  aggr="none"):
    c = plan._c
    rc = oracle.RollupConfigC(
        func=c.func, may_adjust_window=c.may_adjust_window,
        start=c.start, end=c.end, step=c.step, window=c.window,
        lookback_delta=c.lookback_delta,
        min_staleness_interval=c.min_staleness_interval,
        is_default_rollup=c.is_default_rollup,
        samples_scanned_per_call=c.samples_scanned_per_call,
        arg=c.arg, arg2=c.arg2)
    return oracle.rollup_eval_batch(
        rc, ts, vals, offsets, group_ids=group_ids, n_groups=n_groups,
        aggr=aggr, remove_counter_resets=bool(c.remove_counter_resets),
        max_staleness_interval=c.max_staleness_interval,
        drop_stale_nans=bool(c.drop_stale_nans), n_threads=4,
        pre_func=c.pre_func)


def _batch(series):
    """series: list of (ts, vals) arrays -> flat columns + offsets."""
    assert 0 < len(series) <= 64
    assert all(len(t) <= 256 and len(t) == len(v) for t, v in series)
    offsets = np.zeros(len(series) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(t) for t, _ in series])
    ts = np.concatenate([np.asarray(t, np.int64) for t, _ in series])
    vals = np.concatenate([np.asarray(v, np.float64) for _, v in series])
    return ts.astype(np.int64), vals.astype(np.float64), offsets


def _check(engine, series, start, n_grid, step, window, func="rate",
           lookback_delta=0, min_staleness=0, context=""):
    assert window > 0 and window % step == 0 and 1 < n_grid <= 300
    ts, vals, offsets = _batch(series)
    end = start + (n_grid - 1) * step
    plan = engine.RollupPlan(func, start, end, step, window=window,
                             lookback_delta=lookback_delta,
                             min_staleness_interval=min_staleness)
    out, _, scanned = engine.rollup_eval(plan, ts, vals, offsets)
    ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets)
    assert scanned == ref_scanned, context
    assert_parity(out, ref, exact=True, context=context)
    return out


def _values(rng, n, reset_p=0.02):
    """Whole-number counter values with full resets."""
    v = np.cumsum(rng.poisson(150.0, n).astype(np.float64)) + 3.0
    for k in np.flatnonzero(rng.random(n) < reset_p):
        v[k:] -= v[k] - 1.0
    return v


def _counter(rng, n, t0, step=STEP, jitter=500, reset_p=0.02):
    t = t0 + np.arange(n, dtype=np.int64) * step
    if n and jitter:
        t = np.sort(t + rng.integers(-jitter, jitter + 1, n))
    return t, _values(rng, n, reset_p)


def _probe_tier_series(rng):
    """Series that force every answer class of the probe.  The hint is
    1 + (t_end - first) * (count - 1) / span, which on a regular cadence is
    the index of the sample at t_end plus one."""
    n = 200
    k = np.arange(n, dtype=np.int64)
    grid_t = START - 30 * STEP + k * STEP           # samples ON grid points
    series = [
        (grid_t, _values(rng, n)),                  # hit everywhere
        (grid_t + 1, _values(rng, n)),              # sample just after: g - 1
        (grid_t - 1, _values(rng, n)),              # sample just before
        # the three classes inside one 64-point round
        (grid_t + (k % 3 - 1), _values(rng, n)),
        (grid_t + np.where(k % 2 == 0, 1, -1), _values(rng, n)),
    ]
    # jittered as the benchmark data: a coin toss per point
    series += [_counter(rng, 240, START - 20 * STEP) for _ in range(6)]
    # a burst of 40 samples inside one step, then a gap of 40 steps: the hint
    # is off by far more than one, so the binary search runs
    for s in range(4):
        t, pos = [], START - 45 * STEP + s * 1777
        for _ in range(5):
            t.append(pos + np.sort(rng.choice(STEP, 40, replace=False)))
            pos += 41 * STEP
        t = np.concatenate(t).astype(np.int64)
        series.append((t, _values(rng, len(t))))
    # repeated timestamps, off and on the grid
    for s in range(3):
        t, v = _counter(rng, 200, START - 30 * STEP)
        dup = rng.random(len(t)) < 0.2
        t[dup] = np.roll(t, 1)[dup]
        series.append((np.sort(t), v))
    t = np.repeat(START + np.arange(-10, 90, dtype=np.int64) * STEP, 2)
    series.append((t, _values(rng, len(t))))
    # counts at which the four probed records reach the sentinels
    for n_s in (0, 1, 2, 3, 255, 256):
        series.append(_counter(rng, n_s, START + 10 * STEP))
        series.append(_counter(rng, n_s, START - (n_s // 2) * STEP, jitter=0))
    return series


@pytest.fixture(scope="module")
def tier_series():
    return _probe_tier_series(np.random.default_rng(20240))


@pytest.mark.parametrize("func", ["rate", "deriv_fast"])
def test_probe_tiers(engine, tier_series, func):
    """Hit, g+1, g-1, a mix within one round, the binary search, repeated
    timestamps and counts 0, 1, 2, 3, 255, 256 in one batch."""
    _check(engine, tier_series, START, 130, STEP, 20 * STEP, func=func,
           context=f"probe tiers {func}")


@pytest.mark.parametrize("ratio,n_grid", [(64, 130), (100, 130), (64, 64),
                                          (20, 2), (1, 2), (100, 2), (20, 257)])
def test_other_loops(engine, tier_series, ratio, n_grid):
    """The same batch through the j-cache loops (window / step >= 64), with
    n_grid no multiple of 64, a whole number of rounds, and n_grid = 2."""
    _check(engine, tier_series, START, n_grid, STEP, ratio * STEP,
           context=f"loops w/s={ratio} n_grid={n_grid}")


def test_other_loops_deriv_fast(engine, tier_series):
    _check(engine, tier_series, START, 130, STEP, 64 * STEP, func="deriv_fast",
           context="loops deriv_fast")


def _far_series(rng, n_grid, step):
    """Series far before, far after and far wider than the grid
    [START, START + (n_grid - 1) * step], each next to a plain one."""
    end = START + (n_grid - 1) * step
    n = 200
    span = (n - 1) * STEP
    plain = lambda: _counter(rng, 240, START - 20 * STEP)
    wide_t = START - 40 * step + (np.arange(256, dtype=np.int64) * LIMIT) // 255
    assert wide_t[-1] - wide_t[0] == LIMIT
    assert wide_t[0] < START and wide_t[-1] > end
    return [
        plain(),
        _counter(rng, n, START - 30 * DAY - span),     # ends 30 d before start
        plain(),
        _counter(rng, n, end + 30 * DAY),              # begins 30 d after end
        plain(),
        (wide_t, _values(rng, 256)),                   # the grid lies inside it
        _counter(rng, n, START - 30 * DAY - span, jitter=0),
        (wide_t[:2], _values(rng, 2)),
        _counter(rng, 3, end + 30 * DAY),
        plain(),
    ]


@pytest.mark.parametrize("lookback,min_staleness",
                         [(0, 0), (40 * DAY, 0), (40 * DAY, 40 * DAY)],
                         ids=["lbd0", "lbd40d", "lbd40d_minstale40d"])
def test_grid_far_from_series(engine, lookback, min_staleness):
    """Seeks and prev-interval bounds more than 2^31 ms away from the series.
    A 40-day lookback_delta puts the scan's staleness interval past
    2^31 ms; with a 40-day minimum staleness the prev-sample interval is
    that large too."""
    rng = np.random.default_rng(77)
    for func in ("rate", "deriv_fast"):
        _check(engine, _far_series(rng, 130, STEP), START, 130, STEP, 20 * STEP,
               func=func, lookback_delta=lookback, min_staleness=min_staleness,
               context=f"far {func} lbd={lookback}")
        if lookback:
            break  # deriv_fast once


def test_grid_straddles_wide_series(engine):
    """A grid that runs from 20 steps before a series of span 2^31 - 2 ms to
    20 steps behind it: seeks from before its first sample to past its last."""
    rng = np.random.default_rng(78)
    step = 8_640_000
    n_grid = 290
    t = START + 20 * step + (np.arange(256, dtype=np.int64) * LIMIT) // 255
    assert t[-1] - t[0] == LIMIT
    assert START + (n_grid - 1) * step > t[-1] + 20 * step
    series = [(t, _values(rng, 256)), _counter(rng, 240, START, step=step),
              (t[::5], _values(rng, len(t[::5])))]
    for lookback in (0, 40 * DAY):
        for ratio in (2, 70):
            _check(engine, series, START, n_grid, step, ratio * step,
                   lookback_delta=lookback,
                   context=f"straddle lbd={lookback} w/s={ratio}")


def _span_series(rng, base):
    """Two-sample and 256-sample series of span 2^31 - 3, 2^31 - 2, 2^31 - 1
    (the widest on the 31-bit dt path) and 2^31 + 5 ms (too wide for it),
    interleaved so that one wave hands over in both directions."""
    series = []
    for span in (LIMIT - 1, LIMIT + 1, LIMIT, LIMIT + 7, LIMIT + 1, LIMIT - 1):
        t = base + (np.arange(256, dtype=np.int64) * span) // 255
        assert t[-1] - t[0] == span and np.all(np.diff(t) > 0)
        series.append((t, _values(rng, 256)))
        series.append((t[[0, -1]], _values(rng, 2, reset_p=0)))
    assert sorted({int(t[-1] - t[0]) for t, _ in series}) == \
        [(1 << 31) - 3, (1 << 31) - 2, (1 << 31) - 1, (1 << 31) + 5]
    return series


@pytest.mark.parametrize("base", [START, -(1 << 31) - 12_345,
                                  (1 << 62) - (1 << 30)],
                         ids=["epoch", "negative", "near_2e62"])
def test_span_at_the_limit(engine, base):
    """Spans on both sides of the 32-bit limit in one batch, at ordinary,
    negative and very large timestamps.  The grid covers the whole span; the
    window reaches the previous sample, so slopes use the large dt."""
    rng = np.random.default_rng(79)
    step = 8_640_000
    series = _span_series(rng, base)
    start = base - 10 * step
    for func in ("rate", "deriv_fast"):
        _check(engine, series, start, 280, step, 2 * step, func=func,
               context=f"span limit {func} base={base}")
        if base != START:
            break  # deriv_fast once
    # the two-sample series' slope spans the whole series
    _check(engine, series, start + 240 * step, 40, step, 70 * step,
           context=f"span limit jcache base={base}")


def test_other_slab_producers(engine):
    """Series that do not reach the slab through the pair staging: odd sample
    offsets (compacted from global memory), stale NaNs (compacted, scanned in
    LDS, scrape interval taken from the slab because samples were dropped),
    and an ordinary NaN value; each between plain series."""
    rng = np.random.default_rng(80)
    stale = oracle.stale_nan()
    series = []

    def add(item, odd=False):
        """append at an even (odd) sample offset, behind a one-sample filler
        where the offset has the other parity"""
        if (sum(len(t) for t, _ in series) & 1) != int(odd):
            series.append(_counter(rng, 1, START + 5 * STEP))
        series.append(item)

    def plain():
        add(_counter(rng, 240, START - 20 * STEP))

    plain()
    for n in (240, 255, 129):
        add(_counter(rng, n, START - 20 * STEP), odd=True)
        plain()
    for n, p, cadence in ((256, 0.05, STEP), (200, 0.5, STEP),
                          (240, 0.1, 4 * STEP), (64, 0.3, 60_000)):
        t, v = _counter(rng, n, START - 20 * STEP, step=cadence)
        v = np.where(rng.random(n) < p, stale, v)
        add((t, v))
        plain()
    t, v = _counter(rng, 8, START, step=20 * STEP)
    v[:] = stale                                            # nothing is left
    add((t, v))
    plain()
    for at in ((100,), (0, 127, 128, 239)):
        t, v = _counter(rng, 240, START - 20 * STEP)
        v[list(at)] = np.nan                                # ordinary NaN
        add((t, v))
        plain()
    # a stale series too wide for the 31-bit dt path, and one just inside it
    for span in (LIMIT + 1, LIMIT):
        t = START - 20 * STEP + (np.arange(200, dtype=np.int64) * span) // 199
        v = _values(rng, 200)
        v[5::9] = stale
        v[0] = v[-1] = 1.0                                  # ends are kept
        add((t, v))
        plain()
    offs = np.cumsum([0] + [len(t) for t, _ in series])
    assert (offs[:-1] & 1).any() and not (offs[:-1] & 1).all()
    for func in ("rate", "deriv_fast"):
        _check(engine, series, START, 130, STEP, 20 * STEP, func=func,
               context=f"producers {func}")
    _check(engine, series, START, 130, STEP, 64 * STEP, lookback_delta=5 * STEP,
           context="producers jcache")


@pytest.mark.parametrize("rel", [-1, 0, 1, None],
                         ids=["below_gap", "equal_gap", "above_gap", "over_2e31"])
def test_scan_gap(engine, rel):
    """removeCounterResets' staleness test `t[k] - t[k-1] > interval` with the
    interval (lookback_delta + window) one below, equal to and one above a gap
    in the series, and past 2^31 ms."""
    rng = np.random.default_rng(81)
    window = 20 * STEP
    gap = 30 * STEP
    lookback = 40 * DAY if rel is None else gap - window + rel
    series = []
    for at in (1, 63, 64, 100, 127, 128, 129, 200, 255):
        for n in (256, 201):
            if at >= n:
                continue
            t = START - 60 * STEP + np.arange(n, dtype=np.int64) * STEP
            t[at:] += gap - STEP                 # t[at] - t[at-1] == gap
            assert t[at] - t[at - 1] == gap
            v = _values(rng, n, reset_p=0.03)
            v[at - 1:] -= v[at - 1] - 2.0        # a reset right before the gap
            v[at:] += 50.0
            series.append((t, v))
    series.append(_counter(rng, 240, START - 20 * STEP))
    _check(engine, series, START, 130, STEP, window, lookback_delta=lookback,
           context=f"scan gap rel={rel}")


def test_grouped_sum(engine, tier_series):
    """The grouped instantiation over the probe-tier batch, 3 groups: the
    presence mask and the contribution counts (aggr count) exactly, the sums
    at the float-sum bar of the other grouped tests (atomic order varies)."""
    ts, vals, offsets = _batch(tier_series)
    n_groups = 3
    gids = (np.arange(len(tier_series)) % n_groups).astype(np.int32)
    end = START + 129 * STEP
    for aggr, exact in (("sum", False), ("count", True)):
        plan = engine.RollupPlan("rate", START, end, STEP, window=20 * STEP,
                                 aggr=aggr)
        out, _, scanned = engine.rollup_eval(plan, ts, vals, offsets,
                                             group_ids=gids, n_groups=n_groups)
        ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets,
                                            group_ids=gids, n_groups=n_groups,
                                            aggr=aggr)
        assert scanned == ref_scanned
        assert_parity(out, ref, exact=exact, rtol=1e-9,
                      context=f"grouped {aggr}")
