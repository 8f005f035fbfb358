"""Edge cases of the pipelined rate kernel (rollup_pipe_kernel): the
sentinel-padded series slab and its probe, the strength-reduced hint, the two
dt / 1e3 paths and the removeCounterResets clamp shortcut.

Every input meets the host's pipe gating (rate / deriv_fast, series of at most
256 samples, window > 0 and a multiple of step, n_grid > 1), so these cases
run through the pipe kernel; results are compared bit for bit with the oracle.
"""
import numpy as np
import pytest

import oracle
from seriesgen import assert_parity

pytestmark = pytest.mark.gpu

START = 1_000_000_000_000
STEP = 15_000


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
    offsets = np.zeros(len(series) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(t) for t, _ in series])
    ts = (np.concatenate([np.asarray(t, np.int64) for t, _ in series])
          if series else np.empty(0, np.int64))
    vals = (np.concatenate([np.asarray(v, np.float64) for _, v in series])
            if series else np.empty(0, np.float64))
    assert all(len(t) <= 256 for t, _ in series)
    return ts.astype(np.int64), vals.astype(np.float64), offsets


def _check(engine, series, start, n_grid, step, window, func="rate",
           lookback_delta=0, context=""):
    assert window > 0 and window % step == 0 and n_grid > 1
    ts, vals, offsets = _batch(series)
    end = start + (n_grid - 1) * step
    plan = engine.RollupPlan(func, start, end, step, window=window,
                             lookback_delta=lookback_delta)
    out, _, scanned = engine.rollup_eval(plan, ts, vals, offsets)
    ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets)
    assert scanned == ref_scanned, context
    assert_parity(out, ref, exact=True, context=context)
    return out


def _counter(rng, n, t0, step=STEP, jitter=500, reset_p=0.02):
    """Whole-number counter on a jittered cadence with full resets."""
    t = t0 + np.arange(n, dtype=np.int64) * step
    if n:
        t = np.sort(t + rng.integers(-jitter, jitter + 1, n))
    v = np.cumsum(rng.poisson(150.0, n).astype(np.float64))
    for k in np.flatnonzero(rng.random(n) < reset_p):
        v[k:] -= v[k] - 1.0
    return t, v


COUNTS = [0, 1, 2, 3, 127, 128, 129, 255, 256]


@pytest.mark.parametrize("odd_offset", [False, True],
                         ids=["pair_aligned", "odd_offset"])
def test_counts(engine, odd_offset):
    """Every sample count around the 128-sample chunk edges.  With
    odd_offset each series starts at an odd sample offset, so it cannot be
    staged by 16-byte pair loads and takes the compacting fallback."""
    rng = np.random.default_rng(101)
    series, pos = [], 0
    for rep in range(3):
        for n in COUNTS:
            if (pos & 1) != int(odd_offset):
                series.append(_counter(rng, 1, START + 30 * STEP))  # filler
                pos += 1
            t0 = START - 20 * STEP + int(rng.integers(0, 40)) * STEP
            series.append(_counter(rng, n, t0))
            pos += n
    assert len(series) <= 64
    for func in ("rate", "deriv_fast"):
        _check(engine, series, START, 130, STEP, 20 * STEP, func=func,
               context=f"counts {func} odd={odd_offset}")
        if odd_offset:
            break  # deriv_fast once


def _positions(rng, n_grid, window):
    """Series placed against the grid [START, START + (n_grid-1)*STEP]."""
    end = START + (n_grid - 1) * STEP
    mid = START + (n_grid // 2) * STEP
    n = 200
    span = (n - 1) * STEP
    return [
        _counter(rng, n, end + 3 * STEP),                  # grid before: j = 0
        _counter(rng, n, end + 1),
        _counter(rng, n, START - window - 5 * STEP - span),  # i = j = count
        _counter(rng, n, START - 2 * STEP - span),         # ends inside 1st window
        _counter(rng, n, mid),                             # starts mid-grid
        _counter(rng, n, mid - span),                      # ends mid-grid
        _counter(rng, 256, START - 60 * STEP),             # covers the grid
        _counter(rng, 7, mid - 3 * STEP),                  # inside the grid
    ]


@pytest.mark.parametrize("ratio", [1, 20, 63, 64, 100])
@pytest.mark.parametrize("n_grid", [2, 63, 64, 65, 130])
def test_grid_position(engine, n_grid, ratio):
    """Grid before / after / across the series, for grid lengths around the
    64-point round and window/step on both sides of the fused-loop limit
    (1, 20, 63: fused seek+eval; 64, 100: j-cache)."""
    rng = np.random.default_rng(1000 * n_grid + ratio)
    window = ratio * STEP
    _check(engine, _positions(rng, n_grid, window), START, n_grid, STEP,
           window, context=f"grid n={n_grid} w/s={ratio}")


@pytest.mark.parametrize("ratio", [20, 64])
def test_probe_irregular(engine, ratio):
    """Cadences the density hint cannot follow: bursts of 30 samples inside
    one step followed by gaps of 30 steps (hint off by far more than 1, so
    the binary-search fallback runs), duplicate timestamps, and samples
    exactly on grid timestamps."""
    rng = np.random.default_rng(7 + ratio)
    series = []
    for s in range(12):
        t, k = [], START - 40 * STEP + s * 1234
        for _ in range(8):
            t.append(k + np.sort(rng.integers(0, STEP, 30)))
            k += 31 * STEP
        t = np.concatenate(t).astype(np.int64)
        v = np.cumsum(rng.poisson(50.0, len(t)).astype(np.float64))
        series.append((t, v))
    for s in range(8):   # duplicate timestamps
        t, v = _counter(rng, 200, START - 30 * STEP)
        dup = rng.random(len(t)) < 0.15
        t[dup] = np.roll(t, 1)[dup]
        series.append((np.sort(t), v))
    for s in range(8):   # samples exactly on grid timestamps (some doubled)
        k = np.sort(rng.choice(np.arange(-30, 160), 180, replace=False))
        t = START + k.astype(np.int64) * STEP
        if s & 1:
            t[1::7] = t[0::7][:len(t[1::7])]
            t = np.sort(t)
        v = np.cumsum(rng.poisson(20.0, len(t)).astype(np.float64))
        series.append((t, v))
    _check(engine, series, START, 130, STEP, ratio * STEP,
           context=f"probe w/s={ratio}")


def _two_clusters(e_end, span, n):
    """n samples at the scrape cadence from e_end - span, and n more ending
    at e_end."""
    cl = (n - 1) * STEP
    t = np.concatenate([e_end - span + np.arange(n) * STEP,
                        e_end - cl + np.arange(n) * STEP]).astype(np.int64)
    assert t[-1] - t[0] == span and np.all(np.diff(t) > 0)
    v = np.cumsum(np.full(2 * n, 37.0)) + (np.arange(2 * n) % 5)
    return t, v


def _used_dt(t, n, te, window):
    """dt of the slope at grid point te when the previous sample lies in the
    first cluster: last sample <= te minus last sample <= te - window."""
    t_start = te - window
    assert t[0] + 2 * STEP < t_start < t[n - 1] - 2 * STEP   # in cluster 1
    assert t[n] <= te <= t[-1]                               # in cluster 2
    return int(t[t <= te][-1] - t[t <= t_start][-1])


def test_dt_paths(engine):
    """Series spanning just under, exactly and over 2^31 ms: two clusters of
    samples far apart, the grid over the second cluster and a window that
    reaches back into the first, so the slope's dt is the large cross-gap
    difference (previous sample in the first cluster, has_prev true).

    Run 1: window just under 2^31 ms, so all three spans use a dt just under
    2^31 — the narrow series through the 31-bit path at the top of its
    range, the wide ones through the i64 path.  Run 2: window just over
    2^31 ms on a wider series, whose used dt is itself >= 2^31: a 31-bit
    path taken for it (a wrong span threshold) would give a wrong slope."""
    step = 60_000
    n = 120
    e_end = START + (1 << 32)              # common end of the second cluster
    g0 = e_end - 323_648
    n_grid = 4
    grid = [g0 + m * step for m in range(n_grid)]

    window = 35_776 * step                 # 2_146_560_000 ms, under 2^31
    series = [_two_clusters(e_end, span, n)
              for span in ((1 << 31) - 1, 1 << 31, (1 << 31) + 100_000)]
    for (t, _) in series:                  # the case must be what it says
        for te in grid:
            assert (1 << 31) - 2_000_000 < _used_dt(t, n, te, window) < 1 << 31
    for func in ("rate", "deriv_fast"):
        out = _check(engine, series, g0, n_grid, step, window, func=func,
                     context=f"dt paths {func}")
        assert np.isfinite(out).all() and (out > 0).all()

    window = 35_800 * step                 # 2_148_000_000 ms, over 2^31
    wide = _two_clusters(e_end, (1 << 31) + 1_500_000, n)
    for te in grid:
        assert _used_dt(wide[0], n, te, window) >= 1 << 31
    out = _check(engine, series + [wide], g0, n_grid, step, window,
                 context="dt paths, dt >= 2^31")
    assert np.isfinite(out).all() and (out > 0).all()


def _rcr_model_clamps(v, t, msi):
    """removeCounterResets without its monotonic clamp: True when some
    corrected value falls below its predecessor, i.e. when the reference's
    clamp changes the series."""
    corr, prev, last = 0.0, v[0], None
    for i, x in enumerate(v):
        d = x - prev
        if d < 0:
            corr += (prev - x) if (-d * 8) < prev else prev
        if i > 0 and msi > 0 and t[i] - t[i - 1] > msi:
            corr, prev, last = 0.0, x, x
            continue
        prev = x
        f = x + corr
        if i > 0 and f < last:
            return True
        last = f
    return False


def _fractional_counter(rng, n, p_reset):
    inc = rng.random(n) * 3.0 + 0.001
    v = np.empty(n)
    cur = rng.random() * 100 + inc[0]
    for k in range(n):
        if k and rng.random() < p_reset:
            cur *= 0.9 + 0.1 * rng.random()   # partial reset: a small drop
        elif k:
            cur += inc[k]
        v[k] = cur
    return v


def test_scan_clamp_engaged(engine):
    """Fractional counters with frequent partial resets: rounding in the
    running correction makes the reference's monotonic clamp fire, so the
    full prefix-max path runs next to the shortcut."""
    rng = np.random.default_rng(77)
    n = 200
    series, clamped = [], 0
    for s in range(64):
        t = START - 20 * STEP + np.arange(n, dtype=np.int64) * STEP
        v = _fractional_counter(rng, n, 0.2)
        clamped += _rcr_model_clamps(v, t, 0)
        series.append((t, v))
    assert clamped >= 1, "no series engages the monotonic clamp"
    assert clamped < len(series), "no series takes the clamp shortcut"
    _check(engine, series, START, 130, STEP, 20 * STEP, context="clamp")


def test_scan_cases(engine):
    """removeCounterResets shapes: none / full / partial resets, staleness
    gaps inside a chunk and exactly at the 128-sample chunk boundary, a
    non-stale NaN and -0.0 values."""
    rng = np.random.default_rng(5)
    n = 256
    window = 20 * STEP
    lbd = 5 * STEP                          # staleness = lbd + window
    gap = lbd + window + STEP
    base_t = START - 60 * STEP + np.arange(n, dtype=np.int64) * STEP
    mono = np.cumsum(rng.poisson(150.0, n).astype(np.float64)) + 1000.0

    def with_gap(at):
        t = base_t.copy()
        t[at:] += gap
        return t

    full = mono.copy()
    full[90:] -= full[90] - 1.0
    full[200:] -= full[200]
    part = mono.copy()
    part[70:] -= 0.05 * part[69]            # -d*8 < prev: partial reset
    part[130:] -= 0.01 * part[129]
    assert (part[69] - part[70]) * 8 < part[69]
    nan_v = mono.copy()
    nan_v[100] = np.nan                     # ordinary NaN, not the stale one
    nan_v[128] = np.nan
    negz = np.zeros(n)
    negz[::3] = -0.0
    negz[150:] = np.cumsum(np.ones(n - 150))
    negz2 = mono.copy()
    negz2[40] = -0.0                        # full reset down to -0.0
    negz2[41:] -= negz2[41] - 5.0
    series = [
        (base_t, mono), (base_t, full), (base_t, part),
        (with_gap(50), full), (with_gap(128), full), (with_gap(128), part),
        (with_gap(127), mono), (with_gap(129), part),
        (base_t, nan_v), (base_t, negz), (base_t, negz2),
        (with_gap(128), nan_v),
    ]
    # the same shapes cut to lengths around the chunk edge
    series += [(t[:k], v[:k]) for (t, v) in series[:8] for k in (129, 255)]
    assert len(series) <= 64
    _check(engine, series, START, 130, STEP, window, lookback_delta=lbd,
           context="scan lbd")
    _check(engine, series, START, 130, STEP, window, context="scan")


def test_scan_stale_nans_dropped(engine):
    """Prometheus stale NaNs with drop_stale (rate's default): the series is
    compacted from global memory and the final count is below the raw one."""
    rng = np.random.default_rng(12)
    series = []
    for s, n in enumerate([256, 255, 200, 129, 128, 64, 3, 2] * 3):
        t, v = _counter(rng, n, START - 30 * STEP)
        sm = rng.random(n) < (0.05 if s % 3 else 0.5)
        if s == 5:
            sm[:] = True                    # everything dropped: count 0
        v = np.where(sm, oracle.stale_nan(), v)
        series.append((t, v))
    _check(engine, series, START, 130, STEP, 20 * STEP, context="stale")
    _check(engine, series, START, 65, STEP, 64 * STEP, context="stale jcache")


def test_grouped_sum(engine):
    """The grouped instantiation of the pipe kernel over the same kinds of
    series (sum by group: float-sum bar, atomic order varies)."""
    rng = np.random.default_rng(31)
    series = _positions(rng, 130, 20 * STEP)
    series += [_counter(rng, n, START - 20 * STEP) for n in COUNTS]
    series += [(START - 20 * STEP + np.arange(200, dtype=np.int64) * STEP,
                _fractional_counter(rng, 200, 0.2)) for _ in range(16)]
    ts, vals, offsets = _batch(series)
    n_groups = 5
    gids = (np.arange(len(series)) % n_groups).astype(np.int32)
    end = START + 129 * STEP
    plan = engine.RollupPlan("rate", START, end, STEP, window=20 * STEP,
                             aggr="sum")
    out, _, scanned = engine.rollup_eval(plan, ts, vals, offsets,
                                         group_ids=gids, n_groups=n_groups)
    ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets,
                                        group_ids=gids, n_groups=n_groups,
                                        aggr="sum")
    assert scanned == ref_scanned
    assert_parity(out, ref, exact=False, rtol=1e-9, context="grouped sum")


@pytest.mark.parametrize("func", ["rate", "deriv_fast"])
def test_nan_values_longer_series(engine, func):
    """Ordinary (non-stale) NaN samples in series too long for the pipe
    kernel: 300 and 500 samples (wave kernel), 700 and 2000 (block kernel)
    and 4200 (huge kernel) share the rate evaluator and the
    removeCounterResets scans with it.  A NaN previous sample means "no
    previous value", and the monotonic clamp leaves a NaN and its successor
    alone, as in the reference."""
    rng = np.random.default_rng(404)
    series = []
    for n in (300, 500, 700, 2000, 4200):
        for reset_p in (0.0, 0.03):
            t = START - 20 * STEP + np.arange(n, dtype=np.int64) * STEP
            v = np.cumsum(rng.poisson(150.0, n).astype(np.float64)) + 7.0
            for k in np.flatnonzero(rng.random(n) < reset_p):
                v[k:] -= v[k] - 1.0
            # NaNs alone, doubled, next to a reset and on the 64 / 128 edges
            for k in (5, 63, 64, 127, 128, 129, 200, 201, n - 2):
                v[k] = np.nan
            v[rng.integers(0, n, 6)] = np.nan
            series.append((t, v))
    ts = np.concatenate([t for t, _ in series])
    vals = np.concatenate([v for _, v in series])
    offsets = np.zeros(len(series) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(t) for t, _ in series])
    for n_grid, ratio in ((260, 20), (130, 70)):
        end = START + (n_grid - 1) * STEP
        plan = engine.RollupPlan(func, START, end, STEP, window=ratio * STEP)
        out, _, scanned = engine.rollup_eval(plan, ts, vals, offsets)
        ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets)
        assert scanned == ref_scanned
        assert np.isnan(ref).any() and np.isfinite(ref).any()
        assert_parity(out, ref, exact=True,
                      context=f"NaN values {func} n_grid={n_grid}")
