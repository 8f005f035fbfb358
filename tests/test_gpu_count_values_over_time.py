"""Device count_values_over_time (csrc/cvot.hip) against the host reference
rollup_multi.count_values_over_time, series by series on the same columns.

Counts are integers, so everything is compared exactly: the set of labels
per series (format_go_float_g of the device's row value against the
reference's tag), every value bit for bit (NaN where the count is zero),
samples_scanned summed over the series, and the API's row order (a series'
rows adjacent, count_values_order_key strictly ascending).  Each reference
is computed once per (batch, grid) and shared; every case stays within a few
10^5 inner iterations of the Python reference.
"""
import ctypes
import functools
from collections import Counter

import numpy as np
import pytest

import oracle
from seriesgen import assert_parity
from victoriametrics_amd import limits, rollup_multi
from victoriametrics_amd.decimal import STALE_NAN_BITS
from victoriametrics_amd.metric_name import MetricName

pytestmark = pytest.mark.gpu

SEC = 1000
START = 1_600_000_000_000
G0 = START + 300 * SEC  # first grid point: 300 s of samples lie before it
LABEL = b"v"


def _from_bits(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


STALE = _from_bits(STALE_NAN_BITS)

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
# outside every window of every grid above
FAR_BEFORE = G0 - 10_000_000 - 5
FAR_AFTER = G0 + 4000 * SEC
ONLY_OUTSIDE = 777.0

# Series lengths of batch A.  The class caps of csrc/cvot.hip:
#   CVOT_WAVE_CAP  = 256   one wavefront sorts in its LDS slab up to here
#   CVOT_BLOCK_CAP = 2048  one workgroup sorts in LDS up to here, in the
#                          batch's global scratch above
# so 255/256/257 and 2047/2048/2049 sit on both sides of each, and 4200 is
# well inside the global class.
LENGTHS = (63, 64, 65, 129, 300, 255, 256, 257, 2047, 2048, 2049)
ALL_DISTINCT_AT = {64, 129, 256, 257, 2048, 2049}
I_EMPTY, I_ONE = 0, 1
I_DISTINCT_4200 = 2 + len(LENGTHS)
I_ENUM_4200 = I_DISTINCT_4200 + 1
I_SPECIALS = I_ENUM_4200 + 1
I_TRIPLE = I_SPECIALS + 1
I_BOUNDARY = I_TRIPLE + 1
I_ALL_STALE = I_BOUNDARY + 1


def _jittered_ts(rng, n, t0=START):
    return (t0 + np.arange(n, dtype=np.int64) * SEC +
            rng.integers(-400, 400, n)).astype(np.int64)


def _signed_distinct(rng, n):
    v = rng.normal(0.0, 1.0, n) * np.exp(rng.normal(0.0, 3.0, n))
    assert len(np.unique(v)) == n
    return v


def _from_pool(rng, n):
    """About n / 3 distinct values of both signs, so most are repeated."""
    pool = _signed_distinct(rng, n // 3 + 1)
    return rng.choice(pool, n)


def _special_values():
    one, mil = 1.0, 1e6
    vals = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324,
            1.7976931348623157e308,
            _from_bits(0x7FF8000000000000), _from_bits(0xFFF8000000000000),
            _from_bits(0x7FF8000000000123), STALE,
            np.nextafter(one, 0.0), one, np.nextafter(one, 2.0),
            np.nextafter(mil, 0.0), mil, np.nextafter(mil, np.inf)]
    return np.asarray(vals + vals[::-1], dtype=np.float64)  # each twice


def _boundary_ts():
    t = [FAR_BEFORE, FAR_BEFORE, FAR_AFTER]
    for start, end, step, window in CASES.values():
        n_grid = 1 + (end - start) // step
        for g in {0, n_grid - 1}:
            t_end = start + g * step
            t += [t_end - window, t_end - window + 1, t_end, t_end + 1]
        t += [start - window - 5, end + 5, end + 5]
    return np.sort(np.asarray(t + t[3::3], dtype=np.int64))  # with duplicates


def _flatten(series):
    offsets = np.zeros(len(series) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(t) for t, _ in series])
    ts = np.concatenate([np.asarray(t, np.int64) for t, _ in series])
    vals = np.concatenate([np.asarray(v, np.float64) for _, v in series])
    return ts, vals, offsets


def _mns(n):
    # every third name already carries the label, which must be replaced
    return [MetricName(b"m", [(b"s", b"%d" % s)] +
                       ([(LABEL, b"old")] if s % 3 == 0 else []))
            for s in range(n)]


@functools.lru_cache(maxsize=None)
def _batch_a():
    rng = np.random.default_rng(1490)
    series = [(np.empty(0, np.int64), np.empty(0))]              # I_EMPTY
    series.append((np.asarray([G0], np.int64), np.asarray([3.0])))  # I_ONE
    for n in LENGTHS:
        v = _signed_distinct(rng, n) if n in ALL_DISTINCT_AT \
            else _from_pool(rng, n)
        series.append((_jittered_ts(rng, n), v))
    v = np.exp(rng.normal(0.0, 3.0, 4200))                  # I_DISTINCT_4200
    assert len(np.unique(v)) == 4200
    series.append((_jittered_ts(rng, 4200), v))
    codes = rng.choice(np.asarray([0.0, 1.0, 200.0, 404.0, 503.0]), 3,
                       replace=False)                            # I_ENUM_4200
    series.append((_jittered_ts(rng, 4200), codes[rng.integers(0, 3, 4200)]))
    sv = _special_values()                                       # I_SPECIALS
    series.append((_jittered_ts(rng, len(sv), G0 - 10 * SEC), sv))
    dup = np.repeat(_jittered_ts(rng, 50, G0 - 25 * SEC), 3)[:-1]  # I_TRIPLE
    series.append((dup, _from_pool(rng, len(dup))))
    bt = _boundary_ts()                                          # I_BOUNDARY
    bv = rng.choice(np.asarray([-2.5, 0.0, 7.0, 1e-5]), len(bt))
    bv[(bt == FAR_BEFORE) | (bt == FAR_AFTER)] = ONLY_OUTSIDE
    series.append((bt, bv))
    series.append((_jittered_ts(rng, 20, G0 - 10 * SEC),         # I_ALL_STALE
                   np.full(20, STALE)))
    assert len(series) == I_ALL_STALE + 1
    return series


@functools.lru_cache(maxsize=None)
def _batch_b():
    """Small batch for the drop_stale, grouped, re-exec, max_rows and
    batch-level cases."""
    rng = np.random.default_rng(1491)
    series = [(np.empty(0, np.int64), np.empty(0))]
    for n in (5, 70, 130):
        series.append((_jittered_ts(rng, n, G0 - 60 * SEC), _from_pool(rng, n)))
    series.append((_jittered_ts(rng, 300, G0 - 60 * SEC),
                   _signed_distinct(rng, 300)))
    sv = _special_values()
    series.append((_jittered_ts(rng, len(sv), G0 - 10 * SEC), sv))
    v = rng.choice(np.asarray([1.0, 2.0, 200.0]), 150)           # I_B_STALE
    v[rng.random(150) < 0.2] = STALE
    v[rng.random(150) < 0.1] = np.nan
    series.append((_jittered_ts(rng, 150, G0 - 30 * SEC), v))
    series.append((_jittered_ts(rng, 20, G0 - 10 * SEC),     # I_B_ALL_STALE
                   np.full(20, STALE)))
    return series


I_B_STALE, I_B_ALL_STALE = 6, 7
B_GRID = (G0, G0 + 64 * 60 * SEC, 60 * SEC, 300 * SEC)   # n_grid 65
B_GRID2 = (G0 + 11, G0 + 11 + 9 * 45 * SEC, 45 * SEC, 45 * SEC)  # n_grid 10


@functools.lru_cache(maxsize=None)
def _reference(which, grid, drop_stale=True, keep_metric_names=False):
    """[(list[Series], samples_scanned)] per series from the host function."""
    series = _batch_a() if which == "a" else _batch_b()
    mns = _mns(len(series))
    start, end, step, window = grid
    return [rollup_multi.count_values_over_time(
        LABEL, t, v, mns[s], start, end, step, window,
        keep_metric_names=keep_metric_names, drop_stale=drop_stale)
        for s, (t, v) in enumerate(series)]


def _n_covered(ts, grid):
    """Samples that lie in one or more windows, from the window definition."""
    start, end, step, window = grid
    n_grid = 1 + (end - start) // step
    ts = np.asarray(ts, dtype=np.int64)
    g_lo = np.maximum(-((start - ts) // step), 0)            # ceil
    g_hi = np.minimum((ts + window - 1 - start) // step, n_grid - 1)
    return int((g_lo <= g_hi).sum())


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


def _label(v):
    return rollup_multi.format_go_float_g(float(v)).encode()


def _assert_matches(got, ref, n_grid, context):
    row_series, row_value, values, scanned = got
    assert row_series.dtype == np.uint32 and row_value.dtype == np.float64
    assert values.shape == (len(row_series), n_grid), context
    assert len(row_value) == len(row_series)
    want_scanned = 0
    seen_rows = 0
    for s, (ref_series, ref_scanned) in enumerate(ref):
        want_scanned += ref_scanned
        idx = np.flatnonzero(row_series == s)
        seen_rows += len(idx)
        if len(idx):
            # the API's order: a series' rows are adjacent, values ascending
            assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))), \
                f"{context}: rows of series {s} not adjacent"
            keys = [rollup_multi.count_values_order_key(row_value[i])
                    for i in idx]
            assert all(a < b for a, b in zip(keys, keys[1:])), \
                f"{context}: values of series {s} not ascending"
        got_map = {_label(row_value[i]): values[i] for i in idx}
        assert len(got_map) == len(idx), f"{context}: series {s} label clash"
        ref_map = {r.mn.get_tag_value(LABEL): r.values for r in ref_series}
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
    got = batch_a.count_values_over_time(*grid)
    _assert_matches(got, _reference("a", grid), N_GRID[case], case)
    # identity layout: series ascending over the whole result
    assert np.all(np.diff(got[0].astype(np.int64)) >= 0)
    # a row exists only if it is non-zero somewhere
    assert np.all(np.any(~np.isnan(got[2]), axis=1))


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_row_structure(case):
    """What the cases are there for, asserted on the reference itself."""
    grid = CASES[case]
    ref = _reference("a", grid)
    series = _batch_a()
    # all-distinct: one row per covered sample
    for i in (I_DISTINCT_4200, 2 + LENGTHS.index(2048), 2 + LENGTHS.index(256)):
        assert len(ref[i][0]) == _n_covered(series[i][0], grid)
    # a value that occurs only outside every window has no row
    assert np.any(series[I_BOUNDARY][1] == ONLY_OUTSIDE)
    labels = {r.mn.get_tag_value(LABEL) for r in ref[I_BOUNDARY][0]}
    assert labels and _label(ONLY_OUTSIDE) not in labels
    assert ref[I_EMPTY] == ([], 0)
    assert ref[I_ALL_STALE] == ([], 0)
    if case == "grid130_window_20_steps":
        # the row-tiling case and the rows longer than a wavefront
        assert len(ref[I_DISTINCT_4200][0]) > 3800
        assert len(ref[I_ENUM_4200][0]) == 3
        spec = {r.mn.get_tag_value(LABEL) for r in ref[I_SPECIALS][0]}
        assert {b"0", b"-0", b"+Inf", b"-Inf", b"NaN", b"5e-324", b"-5e-324",
                b"1.7976931348623157e+308", b"1", b"1e+06"} <= spec
        assert len(spec) == 14  # 17 values, four of them NaNs, one dropped


def test_drop_stale_false(batch_b):
    keep = _reference("b", B_GRID, drop_stale=False)
    drop = _reference("b", B_GRID, drop_stale=True)
    assert sum(sc for _, sc in keep) > sum(sc for _, sc in drop)
    # on the reference: the all-stale series has no row, or the one NaN row
    assert drop[I_B_ALL_STALE] == ([], 0)
    assert [r.mn.get_tag_value(LABEL) for r in keep[I_B_ALL_STALE][0]] == [b"NaN"]
    got_keep = batch_b.count_values_over_time(*B_GRID, drop_stale=False)
    _assert_matches(got_keep, keep, 65, "drop_stale=False")
    got_drop = batch_b.count_values_over_time(*B_GRID, drop_stale=True)
    _assert_matches(got_drop, drop, 65, "drop_stale=True")
    assert got_keep[3] > got_drop[3]
    assert not np.any(got_drop[0] == I_B_ALL_STALE)
    assert int((got_keep[0] == I_B_ALL_STALE).sum()) == 1

    def nan_row(got):
        i = np.flatnonzero((got[0] == I_B_STALE) & np.isnan(got[1]))
        assert len(i) == 1
        assert _bits(got[1][i])[0] == 0x7FF8000000000000
        return got[2][i[0]]

    # stale NaNs are counted under NaN only when they are kept
    assert not np.array_equal(_bits(nan_row(got_keep)), _bits(nan_row(got_drop)))
    assert np.nansum(nan_row(got_keep)) > np.nansum(nan_row(got_drop))


def test_grouped_batch_names_original_series(engine):
    series = _batch_b()
    group_ids = np.asarray([2, 0, 1, 0, 2, 1, 0, 1], dtype=np.int32)
    assert len(group_ids) == len(series)
    with engine.SeriesBatch(*_flatten(series), group_ids=group_ids,
                            n_groups=3) as b:
        assert b._perm is not None  # physically relayouted
        got = b.count_values_over_time(*B_GRID)
        _assert_matches(got, _reference("b", B_GRID), 65, "grouped")
        # rows follow the physical (group-contiguous) order
        order = [int(s) for i, s in enumerate(got[0])
                 if i == 0 or got[0][i - 1] != s]
        assert order == [int(s) for s in b._perm if np.any(got[0] == s)]
        assert order != sorted(order)


def _fetch_histogram(engine, batch, n_rows, n_grid):
    lib = engine._load_lib()
    rs = np.empty(n_rows, dtype=np.uint32)
    rb = np.empty(n_rows, dtype=np.uint16)
    out = np.empty((n_rows, n_grid), dtype=np.float64)
    errbuf = ctypes.create_string_buffer(256)
    rc = lib.vmgpu_histogram_over_time_fetch(
        ctypes.c_uint64(batch.handle),
        rs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
        rb.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        errbuf, ctypes.c_size_t(len(errbuf)))
    assert rc == 0, errbuf.value
    return rs, rb, out


def test_reexec_next_to_histogram_and_ordinary_rollup(engine):
    rng = np.random.default_rng(1492)
    series = [(_jittered_ts(rng, n, G0 - 60 * SEC),
               np.round(np.exp(rng.normal(0.0, 3.0, n)), 1))
              for n in (5, 70, 130, 300)]
    ts, vals, offsets = _flatten(series)
    mn = MetricName(b"m", [])

    def ref(grid):
        return [rollup_multi.count_values_over_time(LABEL, t, v, mn, *grid)
                for t, v in series]

    ref_a = ref(B_GRID)
    with engine.SeriesBatch(ts, vals, offsets) as b:
        _assert_matches(b.count_values_over_time(*B_GRID), ref_a, 65,
                        "first exec")
        _assert_matches(b.count_values_over_time(*B_GRID2), ref(B_GRID2), 10,
                        "second exec, smaller grid")
        hist = b.histogram_over_time(*B_GRID)
        assert len(hist[0]) > 0
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
        assert_parity(out, want, exact=True, context="avg after count_values")
        _assert_matches(b.count_values_over_time(*B_GRID), ref_a, 65,
                        "third exec")
        # the two sparse results coexist: the histogram is still there,
        # unchanged by the count_values exec after it
        rs, rb, hout = _fetch_histogram(engine, b, len(hist[0]), 65)
        assert np.array_equal(rs, hist[0]) and np.array_equal(rb, hist[1])
        assert np.array_equal(_bits(hout), _bits(hist[2]))


def test_max_rows(engine, batch_b):
    ref = _reference("b", B_GRID)
    n = sum(len(ss) for ss, _ in ref)
    assert n > 300
    got = batch_b.count_values_over_time(*B_GRID, max_rows=n)
    _assert_matches(got, ref, 65, "max_rows = n_rows")
    with pytest.raises(engine.VmGpuError) as exc:
        batch_b.count_values_over_time(*B_GRID, max_rows=n - 1)
    assert str(n) in str(exc.value) and str(n - 1) in str(exc.value)
    # the refused exec left no result behind
    lib = engine._load_lib()
    errbuf = ctypes.create_string_buffer(256)
    rc = lib.vmgpu_count_values_over_time_fetch(
        ctypes.c_uint64(batch_b.handle), None, None, None, errbuf,
        ctypes.c_size_t(len(errbuf)))
    assert rc != 0 and b"no count_values_over_time result" in errbuf.value
    _assert_matches(batch_b.count_values_over_time(*B_GRID), ref, 65,
                    "unlimited exec after a refused one")


def test_rejects_bad_arguments(engine, batch_b):
    for grid in ((G0, G0 + 60 * SEC, 60 * SEC, 0),
                 (G0, G0 + 60 * SEC, 60 * SEC, -5),
                 (G0, G0 + 60 * SEC, 0, 60 * SEC),
                 (G0 + 1, G0, 60 * SEC, 60 * SEC)):
        with pytest.raises(engine.VmGpuError):
            batch_b.count_values_over_time(*grid)


def _multiset(series_list):
    return Counter((s.mn.marshal_sorted(), _bits(s.values).tobytes())
                   for s in series_list)


@pytest.mark.parametrize("keep_metric_names", [False, True])
def test_batch_level(batch_b, keep_metric_names):
    mns = _mns(len(_batch_b()))
    got, scanned = rollup_multi.count_values_over_time_batch(
        LABEL, batch_b, mns, *B_GRID, keep_metric_names=keep_metric_names)
    ref = _reference("b", B_GRID, True, keep_metric_names)
    want = [s for ss, _ in ref for s in ss]
    assert scanned == sum(sc for _, sc in ref)
    assert len(want) > 300
    assert _multiset(got) == _multiset(want)
    for s in got:
        assert s.mn.metric_group == (b"m" if keep_metric_names else b"")
        assert s.mn.get_tag_value(LABEL) != b"old"


def test_batch_level_default_limit_is_the_aggr_func_limit(engine, batch_b,
                                                         monkeypatch):
    mns = _mns(len(_batch_b()))
    n = sum(len(ss) for ss, _ in _reference("b", B_GRID))
    monkeypatch.setattr(limits, "max_series_per_aggr_func", n - 1)
    with pytest.raises(engine.VmGpuError):
        rollup_multi.count_values_over_time_batch(LABEL, batch_b, mns, *B_GRID)
    monkeypatch.setattr(limits, "max_series_per_aggr_func", n)
    got, _ = rollup_multi.count_values_over_time_batch(LABEL, batch_b, mns,
                                                       *B_GRID)
    assert len(got) == n
