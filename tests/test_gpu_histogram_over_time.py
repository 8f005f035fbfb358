"""Device histogram_over_time (csrc/hot.hip) against the host reference
rollup_multi.histogram_over_time, series by series on the same columns.

Counts are integers, so everything is compared exactly: the set of vmrange
labels per series, every value bit for bit (NaN where the count is zero),
and samples_scanned summed over the series.  Each reference is computed once
per (batch, grid) and shared; every case stays within a few 10^5 inner
iterations of the Python reference.
"""
import functools
from collections import Counter

import numpy as np
import pytest

import oracle
from seriesgen import assert_parity
from victoriametrics_amd import rollup_multi, transform
from victoriametrics_amd.decimal import STALE_NAN_BITS
from victoriametrics_amd.metric_name import MetricName

pytestmark = pytest.mark.gpu

SEC = 1000
START = 1_600_000_000_000
G0 = START + 300 * SEC  # first grid point: 300 s of samples lie before it
STALE = np.array([STALE_NAN_BITS], dtype=np.uint64).view(np.float64)[0]

# name -> (start, end, step, window); n_grid = 1 + (end - start) // step
CASES = {
    "grid1_window_eq_step": (G0, G0, 60 * SEC, 60 * SEC),
    "grid2_window_gt_range": (G0, G0 + 3600 * SEC, 3600 * SEC, 10_000_000),
    "grid65_window_lt_step": (G0, G0 + 64 * 60 * SEC, 60 * SEC, 7 * SEC),
    # odd start, end off the grid
    "grid65_window_eq_step": (G0 + 7, G0 + 7 + 64 * 60 * SEC + 59, 60 * SEC,
                              60 * SEC),
    "grid130_window_20_steps": (G0, G0 + 129 * 30 * SEC, 30 * SEC, 600 * SEC),
}
N_GRID = {"grid1_window_eq_step": 1, "grid2_window_gt_range": 2,
          "grid65_window_lt_step": 65, "grid65_window_eq_step": 65,
          "grid130_window_20_steps": 130}

I_EMPTY, I_NOTHING, I_LOGUNIFORM = 0, 9, 8


def _jittered_ts(rng, n, t0=START):
    return (t0 + np.arange(n, dtype=np.int64) * SEC +
            rng.integers(-400, 400, n)).astype(np.int64)


def _special_values():
    thr = rollup_multi.vmrange_bucket_thresholds()
    vals = []
    # k = 162: the first double above the exact-integer run over 1.0;
    # 17/18, 35/36, 179/180: both sides of the decade edges 1e-8, 1e-7, 10
    for k in (0, 1, 17, 18, 35, 36, 161, 162, 163, 179, 180, 485, 486):
        vals += [np.nextafter(thr[k], 0.0), thr[k], np.nextafter(thr[k], np.inf)]
    vals += [0.0, -0.0, -3.0, np.nan, STALE, np.inf, -np.inf, 5e-324, 1e19,
             1e-9, 1.0, 1e18, STALE, 2.5]
    return np.asarray(vals, dtype=np.float64)


def _boundary_ts():
    t = []
    for start, end, step, window in CASES.values():
        n_grid = 1 + (end - start) // step
        for g in {0, min(1, n_grid - 1), n_grid - 1}:
            t_end = start + g * step
            t += [t_end - window, t_end - window + 1, t_end, t_end + 1]
        t += [start - window - 5, end + 5, end + 5]  # outside every window
    return np.sort(np.asarray(t + t[::3], dtype=np.int64))  # with duplicates


def _flatten(series):
    offsets = np.zeros(len(series) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(t) for t, _ in series])
    ts = np.concatenate([np.asarray(t, np.int64) for t, _ in series])
    vals = np.concatenate([np.asarray(v, np.float64) for _, v in series])
    return ts, vals, offsets


def _mns(n):
    # every third name already carries a vmrange tag, which must be replaced
    return [MetricName(b"m", [(b"s", b"%d" % s)] +
                       ([(b"vmrange", b"old")] if s % 3 == 0 else []))
            for s in range(n)]


@functools.lru_cache(maxsize=None)
def _batch_a():
    """Lengths 0, 1, 63, 64, 65, 129, 300, 700, 4200 (series 1 makes every
    later sample offset odd until series 2 ends), then the value and
    timestamp edge cases."""
    rng = np.random.default_rng(486)
    series = [(np.empty(0, np.int64), np.empty(0))]
    series.append((np.asarray([G0], np.int64), np.asarray([3.0])))
    for n in (63, 64, 65, 129, 300, 700):
        series.append((_jittered_ts(rng, n), np.exp(rng.normal(0.0, 3.0, n))))
    series.append((_jittered_ts(rng, 4200),                     # I_LOGUNIFORM
                   10.0 ** rng.uniform(-10.0, 19.0, 4200)))
    nothing = np.tile(np.asarray([np.nan, -1.0, -np.inf, -5e-324]), 10)
    series.append((_jittered_ts(rng, 40, G0 - 20 * SEC), nothing))  # I_NOTHING
    sv = _special_values()
    series.append((_jittered_ts(rng, len(sv), G0 - 10 * SEC), sv))
    dup = np.repeat(_jittered_ts(rng, 50, G0 - 25 * SEC), 3)[:-1]
    series.append((dup, np.exp(rng.normal(0.0, 3.0, len(dup)))))
    bt = _boundary_ts()
    series.append((bt, np.exp(rng.normal(0.0, 3.0, len(bt)))))
    v = np.exp(rng.normal(0.0, 3.0, 200))
    v[rng.random(200) < 0.15] = STALE
    v[rng.random(200) < 0.05] = np.nan
    series.append((_jittered_ts(rng, 200, G0 - 100 * SEC), v))
    # few buckets over the whole range: on the 130-point grid its rows are
    # longer than a wavefront and its whole [rows x n_grid] block still fits
    # one LDS tile of the count pass
    t = (START + np.arange(500, dtype=np.int64) * 8 * SEC +
         rng.integers(-400, 400, 500)).astype(np.int64)
    series.append((t, 5.0 * np.exp(rng.normal(0.0, 0.3, 500))))
    return series


@functools.lru_cache(maxsize=None)
def _batch_b():
    """Small batch for the drop_stale, grouped, re-exec and batch-level
    cases."""
    rng = np.random.default_rng(487)
    series = [(np.empty(0, np.int64), np.empty(0))]
    for n in (5, 70, 130, 300):
        series.append((_jittered_ts(rng, n, G0 - 60 * SEC),
                       np.exp(rng.normal(0.0, 3.0, n))))
    sv = _special_values()
    series.append((_jittered_ts(rng, len(sv), G0 - 10 * SEC), sv))
    v = np.exp(rng.normal(0.0, 3.0, 150))
    v[rng.random(150) < 0.2] = STALE
    series.append((_jittered_ts(rng, 150, G0 - 30 * SEC), v))
    return series


B_GRID = (G0, G0 + 64 * 60 * SEC, 60 * SEC, 300 * SEC)   # n_grid 65
B_GRID2 = (G0 + 11, G0 + 11 + 9 * 45 * SEC, 45 * SEC, 45 * SEC)  # n_grid 10


@functools.lru_cache(maxsize=None)
def _reference(which, grid, drop_stale=True, keep_metric_names=False):
    """[(list[Series], samples_scanned)] per series from the host function."""
    series = _batch_a() if which == "a" else _batch_b()
    mns = _mns(len(series))
    start, end, step, window = grid
    return [rollup_multi.histogram_over_time(
        t, v, mns[s], start, end, step, window,
        keep_metric_names=keep_metric_names, drop_stale=drop_stale)
        for s, (t, v) in enumerate(series)]


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


@pytest.fixture(scope="module")
def batch_a(engine):
    with engine.SeriesBatch(*_flatten(_batch_a())) as b:
        yield b


@pytest.fixture(scope="module")
def batch_b(engine):
    with engine.SeriesBatch(*_flatten(_batch_b())) as b:
        yield b


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_matches(got, ref, n_grid, context):
    row_series, row_bucket, values, scanned = got
    assert row_series.dtype == np.uint32 and row_bucket.dtype == np.uint16
    assert values.shape == (len(row_series), n_grid), context
    assert len(row_bucket) == len(row_series)
    assert np.all(row_bucket < 488), context
    want_scanned = 0
    seen_rows = 0
    for s, (ref_series, ref_scanned) in enumerate(ref):
        want_scanned += ref_scanned
        idx = np.flatnonzero(row_series == s)
        seen_rows += len(idx)
        if len(idx):
            # the API's order: a series' rows are adjacent, codes ascending
            assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))), \
                f"{context}: rows of series {s} not adjacent"
            assert np.all(np.diff(row_bucket[idx].astype(np.int64)) > 0), \
                f"{context}: codes of series {s} not ascending"
        got_map = {rollup_multi.vmrange_label(int(row_bucket[i])).encode():
                   values[i] for i in idx}
        ref_map = {r.mn.get_tag_value(b"vmrange"): r.values for r in ref_series}
        assert set(got_map) == set(ref_map), f"{context}: series {s} labels"
        for label, want in ref_map.items():
            assert np.array_equal(_bits(got_map[label]), _bits(want)), \
                f"{context}: series {s} {label!r}: {got_map[label]} != {want}"
    assert seen_rows == len(row_series), f"{context}: rows of unknown series"
    assert scanned == want_scanned, f"{context}: samples_scanned"


@pytest.mark.parametrize("case", sorted(CASES))
def test_matches_host_reference(batch_a, case):
    grid = CASES[case]
    assert 1 + (grid[1] - grid[0]) // grid[2] == N_GRID[case]
    got = batch_a.histogram_over_time(*grid)
    _assert_matches(got, _reference("a", grid), N_GRID[case], case)
    # identity layout: rows globally ordered by (series, code)
    key = got[0].astype(np.int64) * 1000 + got[1]
    assert np.all(np.diff(key) > 0)


def test_window_lt_step_leaves_samples_out():
    """The 7 s window on a 60 s step must really skip samples, or the case
    checks nothing."""
    grid = CASES["grid65_window_lt_step"]
    ref = _reference("a", grid)
    n_in_grid_span = sum(
        int(((t > grid[0] - grid[3]) & (t <= grid[1])).sum())
        for t, _ in _batch_a())
    assert 0 < sum(sc for _, sc in ref) < n_in_grid_span // 4


def test_row_structure(batch_a):
    grid = CASES["grid130_window_20_steps"]
    ref = _reference("a", grid)
    # the reference itself: the log-uniform series touches > 400 codes, the
    # NaN/negative series none, the empty series none
    assert len(ref[I_LOGUNIFORM][0]) > 400
    assert ref[I_NOTHING][0] == [] and ref[I_NOTHING][1] > 0
    assert ref[I_EMPTY] == ([], 0)
    row_series, row_bucket, values, _ = batch_a.histogram_over_time(*grid)
    assert not np.any(row_series == I_NOTHING)
    assert not np.any(row_series == I_EMPTY)
    codes = row_bucket[row_series == I_LOGUNIFORM]
    assert len(codes) == len(ref[I_LOGUNIFORM][0])
    assert set((codes >> 5).tolist()) == set(range(16))  # all 16 mask words
    assert codes[0] == 0 and codes[-1] == 487              # lower and upper
    # a row exists only if it is non-zero somewhere
    assert np.all(np.any(~np.isnan(values), axis=1))


def test_drop_stale_false(batch_b):
    keep = _reference("b", B_GRID, drop_stale=False)
    drop = _reference("b", B_GRID, drop_stale=True)
    # on the reference: stale NaNs are scanned but never bucketed
    assert sum(sc for _, sc in keep) > sum(sc for _, sc in drop)
    for (ks, _), (ds, _) in zip(keep, drop):
        assert ({r.mn.get_tag_value(b"vmrange") for r in ks} ==
                {r.mn.get_tag_value(b"vmrange") for r in ds})
    got_keep = batch_b.histogram_over_time(*B_GRID, drop_stale=False)
    _assert_matches(got_keep, keep, 65, "drop_stale=False")
    got_drop = batch_b.histogram_over_time(*B_GRID, drop_stale=True)
    _assert_matches(got_drop, drop, 65, "drop_stale=True")
    assert got_keep[3] > got_drop[3]
    assert np.array_equal(got_keep[0], got_drop[0])
    assert np.array_equal(got_keep[1], got_drop[1])
    assert np.array_equal(_bits(got_keep[2]), _bits(got_drop[2]))


def test_grouped_batch_names_original_series(engine):
    series = _batch_b()
    group_ids = np.asarray([2, 0, 1, 0, 2, 1, 0], dtype=np.int32)
    assert len(group_ids) == len(series)
    with engine.SeriesBatch(*_flatten(series), group_ids=group_ids,
                            n_groups=3) as b:
        assert b._perm is not None  # physically relayouted
        got = b.histogram_over_time(*B_GRID)
        _assert_matches(got, _reference("b", B_GRID), 65, "grouped")
        # rows follow the physical (group-contiguous) order
        order = [int(s) for i, s in enumerate(got[0])
                 if i == 0 or got[0][i - 1] != s]
        assert order == [int(s) for s in b._perm if np.any(got[0] == s)]


def test_reexec_then_ordinary_rollup(engine):
    rng = np.random.default_rng(488)
    series = [(_jittered_ts(rng, n, G0 - 60 * SEC),
               np.exp(rng.normal(0.0, 3.0, n))) for n in (5, 70, 130, 300)]
    ts, vals, offsets = _flatten(series)
    mn = MetricName(b"m", [])

    def ref(grid):
        return [rollup_multi.histogram_over_time(t, v, mn, *grid)
                for t, v in series]

    with engine.SeriesBatch(ts, vals, offsets) as b:
        _assert_matches(b.histogram_over_time(*B_GRID), ref(B_GRID), 65,
                        "first exec")
        _assert_matches(b.histogram_over_time(*B_GRID2), ref(B_GRID2), 10,
                        "second exec")
        start, end, step, window = B_GRID
        plan = engine.RollupPlan("avg_over_time", start, end, step,
                                 window=window)
        out, _, scanned = b.exec(plan)
        rc = oracle.make_config("avg_over_time", start, end, step,
                                window=window)
        want, _, want_scanned = oracle.rollup_eval_batch(
            rc, ts, vals, offsets, remove_counter_resets=False,
            drop_stale_nans=True)
        assert scanned == want_scanned
        assert_parity(out, want, exact=True, context="avg after histogram")
        # and the ordinary exec disturbed nothing the histogram path uses
        _assert_matches(b.histogram_over_time(*B_GRID), ref(B_GRID), 65,
                        "third exec")


def _multiset(series_list):
    return Counter((s.mn.marshal_sorted(), _bits(s.values).tobytes())
                   for s in series_list)


@pytest.mark.parametrize("keep_metric_names", [False, True])
def test_batch_level_and_quantile(batch_b, keep_metric_names):
    mns = _mns(len(_batch_b()))
    got, scanned = rollup_multi.histogram_over_time_batch(
        batch_b, mns, *B_GRID, keep_metric_names=keep_metric_names)
    ref = _reference("b", B_GRID, True, keep_metric_names)
    want = [s.copy_shallow() for ss, _ in ref for s in ss]
    assert scanned == sum(sc for _, sc in ref)
    assert len(want) > 50
    assert _multiset(got) == _multiset(want)
    for s in got:
        assert s.mn.metric_group == (b"m" if keep_metric_names else b"")
        assert s.mn.get_tag_value(b"vmrange") != b"old"
    # end to end: vmrange -> le buckets -> histogram_quantile(0.5, ...)
    le_got = transform.vmrange_buckets_to_le([s.copy_shallow() for s in got])
    le_want = transform.vmrange_buckets_to_le([s.copy_shallow() for s in want])
    assert _multiset(le_got) == _multiset(le_want)
    q_got = transform.histogram_transform("histogram_quantile", got, arg=0.5)
    q_want = transform.histogram_transform("histogram_quantile", want, arg=0.5)
    assert len(q_want) == 6  # every non-empty series of the batch
    assert _multiset(q_got) == _multiset(q_want)


def test_rejects_bad_arguments(engine, batch_b):
    for grid in ((G0, G0 + 60 * SEC, 60 * SEC, 0),
                 (G0, G0 + 60 * SEC, 60 * SEC, -5),
                 (G0, G0 + 60 * SEC, 0, 60 * SEC),
                 (G0 + 1, G0, 60 * SEC, 60 * SEC)):
        with pytest.raises(engine.VmGpuError):
            batch_b.histogram_over_time(*grid)
