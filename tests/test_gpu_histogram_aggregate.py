"""Device histogram() aggregate (csrc/aggrhist.hip) against the host
reference.

Counts are integers, so everything is compared exactly.  The raw sparse
result (row_group, row_code, every value's bits) is held to a reference
built here from rollup_multi._vmrange_code, which wraps
aggregate._histogram_update; the final series of
histogram_aggregate_device / histogram_aggregate_batch are held to
aggregate.histogram_aggregate on the same input, as a map from marshaled
metric name to value row plus the series count.

One seeded matrix of 130 columns serves every grid width (a prefix of its
columns), so the per-value reference runs once: about 2.7e5 values.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from conftest import REPO_ROOT
from victoriametrics_amd import aggregate, rollup_multi
from victoriametrics_amd.binary_op import Series
from victoriametrics_amd.decimal import STALE_NAN_BITS
from victoriametrics_amd.metric_name import MetricName

pytestmark = pytest.mark.gpu

STALE = np.array([STALE_NAN_BITS], dtype=np.uint64).view(np.float64)[0]
WIDTHS = (1, 2, 63, 64, 65, 130)
N_COLS = max(WIDTHS)


def _chunk_members():
    """M: the compile-time chunk size of the work list."""
    src = open(os.path.join(REPO_ROOT, "victoriametrics_amd", "csrc",
                            "aggrhist.hip")).read()
    return int(re.search(r"^#define AH_CHUNK_MEMBERS (\d+)", src, re.M).group(1))


M = _chunk_members()
# one chunk, exactly one, just over one, three chunks with a ragged last one
GROUP_SIZES = tuple(sorted({1, 2, 63, 64, 65, M - 1, M, M + 1, 2 * M + 3}))
# the special groups sit between the sized ones, G_NOTHING early so that
# every later group's row offset depends on it contributing no rows
G_NOTHING, G_ALL_CODES, G_SPECIAL, G_MOVING = 2, 5, 7, 9
N_UNUSED_ROWS = 17  # matrix rows that belong to no group


def _special_values():
    thr = rollup_multi.vmrange_bucket_thresholds()
    vals = []
    for k in (0, 1, 17, 18, 35, 36, 161, 162, 163, 179, 180, 485, 486):
        vals += [np.nextafter(thr[k], 0.0), thr[k], np.nextafter(thr[k], np.inf)]
    vals += [0.0, -0.0, -3.0, np.nan, STALE, np.inf, -np.inf, 5e-324, 1e19,
             1e-9, 1.0, 1e18, 2.5]
    return np.asarray(vals, dtype=np.float64)


def _group_blocks():
    """[(name, values[members x N_COLS])] in group order."""
    rng = np.random.default_rng(316)
    thr = rollup_multi.vmrange_bucket_thresholds()
    blocks = []
    for i, n in enumerate(GROUP_SIZES):
        if i % 2 == 0:
            v = np.exp(rng.normal(0.0, 3.0, (n, N_COLS)))
        else:
            v = 10.0 ** rng.uniform(-10.0, 19.0, (n, N_COLS))
        if n > 2:
            v[rng.random(v.shape) < 0.03] = np.nan
            v[rng.random(v.shape) < 0.02] *= -1.0
        blocks.append(("size%d" % n, v))
    nothing = np.tile(np.asarray([np.nan, -1.0, -np.inf, -5e-324, STALE]),
                      (5, N_COLS // 5 + 1))[:, :N_COLS]
    # one member per code: 0.0 and all 487 thresholds, every column
    all_codes = np.repeat(np.concatenate([[0.0], thr])[:, None], N_COLS, axis=1)
    sv = _special_values()
    idx = (np.arange(len(sv))[:, None] + np.arange(N_COLS)[None, :]) % len(sv)
    special = sv[idx]
    # a single code per column, a different one in most columns; the other
    # member contributes nothing
    moving = np.full((2, N_COLS), np.nan)
    moving[0] = thr[(5 * np.arange(N_COLS) + 3) % len(thr)]
    moving[0, 1] = moving[0, 0]  # one row with two non-zero columns
    for pos, blk in sorted([(G_NOTHING, ("nothing", nothing)),
                            (G_ALL_CODES, ("allcodes", all_codes)),
                            (G_SPECIAL, ("special", special)),
                            (G_MOVING, ("moving", moving))]):
        blocks.insert(pos, blk)
    return blocks


@functools.lru_cache(maxsize=None)
def _matrix130():
    """(values[n_in_rows x 130], group_rows, group_offsets, names): the
    members of every group scattered over the matrix by a seeded shuffle,
    so they are non-contiguous and the groups interleave."""
    blocks = _group_blocks()
    assert [b[0] for b in blocks][G_NOTHING] == "nothing"
    assert [b[0] for b in blocks][G_ALL_CODES] == "allcodes"
    assert [b[0] for b in blocks][G_MOVING] == "moving"
    n_members = sum(len(v) for _, v in blocks)
    rng = np.random.default_rng(317)
    n_in_rows = n_members + N_UNUSED_ROWS
    values = np.exp(rng.normal(5.0, 3.0, (n_in_rows, N_COLS)))  # unused rows
    where = rng.permutation(n_in_rows)[:n_members]
    group_rows = where.astype(np.uint32)
    group_offsets = np.zeros(len(blocks) + 1, dtype=np.uint64)
    lo = 0
    for g, (_, v) in enumerate(blocks):
        values[where[lo:lo + len(v)]] = v
        lo += len(v)
        group_offsets[g + 1] = lo
    values.setflags(write=False)
    return values, group_rows, group_offsets, [b[0] for b in blocks]


@functools.lru_cache(maxsize=None)
def _counts130():
    """Per group: {code: counts[130]} from rollup_multi._vmrange_code."""
    values, group_rows, group_offsets, _ = _matrix130()
    out = []
    for g in range(len(group_offsets) - 1):
        d = {}
        for r in group_rows[int(group_offsets[g]):int(group_offsets[g + 1])]:
            for j, v in enumerate(values[r].tolist()):
                c = rollup_multi._vmrange_code(v)
                if c is None:
                    continue
                row = d.get(c)
                if row is None:
                    row = d[c] = np.zeros(N_COLS)
                row[j] += 1.0
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def _case(n_grid):
    values, group_rows, group_offsets, _ = _matrix130()
    return np.ascontiguousarray(values[:, :n_grid]), group_rows, group_offsets


@functools.lru_cache(maxsize=None)
def _raw_reference(n_grid):
    rg, rc, rows = [], [], []
    for g, d in enumerate(_counts130()):
        for c in sorted(d):
            if np.any(d[c][:n_grid] != 0):
                rg.append(g)
                rc.append(c)
                rows.append(d[c][:n_grid])
    return (np.asarray(rg, np.uint32), np.asarray(rc, np.uint16),
            np.asarray(rows, np.float64).reshape(len(rows), n_grid))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_raw(got, want, context):
    row_group, row_code, values = got
    assert row_group.dtype == np.uint32 and row_code.dtype == np.uint16
    assert values.dtype == np.float64
    assert np.array_equal(row_group, want[0]), f"{context}: row_group"
    assert np.array_equal(row_code, want[1]), f"{context}: row_code"
    assert values.shape == want[2].shape, context
    assert np.array_equal(_bits(values), _bits(want[2])), f"{context}: values"


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


@pytest.mark.parametrize("n_grid", WIDTHS)
def test_raw_matches_reference(engine, n_grid):
    want = _raw_reference(n_grid)
    got = engine.aggr_histogram(*_case(n_grid))
    _assert_raw(got, want, f"n_grid={n_grid}")
    # ordered by group, then ascending code
    key = got[0].astype(np.int64) * 1000 + got[1]
    assert np.all(np.diff(key) > 0)


def test_row_structure(engine):
    """What the special groups are there for, checked on the reference and
    on the device result."""
    n_grid = 65
    want = _raw_reference(n_grid)
    row_group, row_code, values = engine.aggr_histogram(*_case(n_grid))
    _assert_raw((row_group, row_code, values), want, "structure")
    # NaN / negative / -Inf / stale members: no rows, later groups unmoved
    assert not np.any(row_group == G_NOTHING)
    assert np.any(row_group == G_NOTHING - 1) and np.any(row_group == G_NOTHING + 1)
    # one member per code: 488 rows of ones, more than one count band
    sel = row_group == G_ALL_CODES
    assert np.array_equal(row_code[sel], np.arange(488))
    assert np.all(values[sel] == 1.0)
    # the single moving code: a zero count is 0.0, never NaN
    sel = row_group == G_MOVING
    assert sel.sum() == n_grid - 1
    assert np.all(values[sel].sum(axis=0) == 1.0)
    assert np.all((values[sel] != 0).sum(axis=1) <= 2)
    assert not np.any(np.isnan(values))
    assert np.all(_bits(values[values == 0]) == 0)  # +0.0
    # a row exists only if it is non-zero somewhere
    assert np.all(np.any(values != 0, axis=1))
    # +Inf lands in the upper bucket, -0.0 and 5e-324 in the lower one
    codes = row_code[row_group == G_SPECIAL]
    assert codes[0] == 0 and codes[-1] == 487


def test_empty_inputs(engine):
    values = _case(2)[0]
    for rows, offsets in ((np.empty(0, np.uint32), np.zeros(1, np.uint64)),
                          (np.empty(0, np.uint32), np.zeros(4, np.uint64))):
        rg, rc, out = engine.aggr_histogram(values, rows, offsets)
        assert len(rg) == 0 and len(rc) == 0 and out.shape == (0, 2)


def _small_case():
    values = np.asarray([[1.0, np.nan], [1.0, 250.0], [7e-3, -1.0]])
    return (values, np.asarray([2, 0, 1], np.uint32),
            np.asarray([0, 1, 3], np.uint64))


def _small_reference():
    values, group_rows, group_offsets = _small_case()
    rows = {}
    for g in range(2):
        for r in group_rows[int(group_offsets[g]):int(group_offsets[g + 1])]:
            for j, v in enumerate(values[r]):
                c = rollup_multi._vmrange_code(v)
                if c is not None:
                    rows.setdefault((g, c), np.zeros(2))[j] += 1.0
    keys = sorted(rows)
    return (np.asarray([k[0] for k in keys], np.uint32),
            np.asarray([k[1] for k in keys], np.uint16),
            np.asarray([rows[k] for k in keys]))


def test_large_small_large(engine):
    """Grow-only buffers reused by a smaller call, and no mask or counter
    left over from the call before."""
    _assert_raw(engine.aggr_histogram(*_case(130)), _raw_reference(130), "large")
    want = _small_reference()
    assert len(want[0]) == 3
    _assert_raw(engine.aggr_histogram(*_small_case()), want, "small")
    _assert_raw(engine.aggr_histogram(*_case(130)), _raw_reference(130),
                "large again")
    _assert_raw(engine.aggr_histogram(*_small_case()), want, "small again")


# --- final series ----------------------------------------------------------

def _series_map(series_list):
    m = {s.mn.marshal_sorted(): _bits(s.values).tobytes() for s in series_list}
    assert len(m) == len(series_list), "duplicate metric names"
    return m


def _assert_same_series(got, want, context):
    assert len(got) == len(want), f"{context}: {len(got)} != {len(want)} series"
    assert _series_map(got) == _series_map(want), context


@functools.lru_cache(maxsize=None)
def _big_series():
    """The 65-column case as named series: g=<group> is the `by` label."""
    values, group_rows, group_offsets = _case(65)
    names = _matrix130()[3]
    out = []
    for g, name in enumerate(names):
        for i, r in enumerate(
                group_rows[int(group_offsets[g]):int(group_offsets[g + 1])]):
            mn = MetricName(b"m", [(b"g", name.encode()), (b"i", b"%d" % i)])
            out.append((mn, values[r]))
    return out


def _fresh(named):
    return [Series(mn.copy(), v.copy()) for mn, v in named]


@functools.lru_cache(maxsize=None)
def _host_big():
    return aggregate.histogram_aggregate(_fresh(_big_series()), "by", ["g"])


def test_device_matches_host_by_label(engine):
    want = _host_big()
    got = aggregate.histogram_aggregate_device(_fresh(_big_series()), "by", ["g"])
    _assert_same_series(got, want, "by (g)")
    # the one-member-per-code group comes out as 488 le series
    n = sum(1 for s in got if s.mn.get_tag_value(b"g") == b"allcodes")
    assert n == 488
    assert all(s.mn.get_tag_value(b"vmrange") is None for s in got)


@functools.lru_cache(maxsize=None)
def _named_small():
    """48 series x 33 points with job / inst labels; some names already
    carry vmrange and le tags."""
    rng = np.random.default_rng(318)
    out = []
    for s in range(48):
        tags = [(b"job", b"j%d" % (s % 6)), (b"inst", b"i%d" % s)]
        if s % 4 == 0:
            tags.append((b"vmrange", b"1.000e+00...1.136e+00"))
        if s % 5 == 0:
            tags.append((b"le", b"0.5"))
        v = np.exp(rng.normal(float(s % 6), 2.0, 33))
        v[rng.random(33) < 0.1] = np.nan
        if s == 7:
            v[:] = np.nan  # dropped by remove_empty_series
        out.append((MetricName(b"lat", tags), v))
    return out


@pytest.mark.parametrize("op,args,limit", [
    ("by", ("job",), 0),
    ("without", ("inst",), 0),
    ("without", ("inst", "vmrange", "le"), 0),
    ("", (), 0),
    ("by", ("job",), 4),       # limit below the 6 groups
    ("by", ("job", "le"), 0),  # groups that differ only in le merge in to_le
])
def test_device_matches_host_names(engine, op, args, limit):
    want = aggregate.histogram_aggregate(_fresh(_named_small()), op,
                                         list(args), limit)
    got = aggregate.histogram_aggregate_device(_fresh(_named_small()), op,
                                               list(args), limit)
    assert len(want) > 0
    _assert_same_series(got, want, f"{op} {args} limit={limit}")
    if limit:
        jobs = {s.mn.get_tag_value(b"job") for s in got}
        assert len(jobs) == limit


# --- batch form ------------------------------------------------------------

SEC = 1000
T0 = 1_600_000_000_000
B_START, B_STEP, B_WINDOW = T0 + 300 * SEC, 20 * SEC, 60 * SEC
B_END = B_START + 64 * B_STEP  # 65 points


@functools.lru_cache(maxsize=None)
def _batch_columns():
    rng = np.random.default_rng(319)
    ts, vals, offsets = [], [], [0]
    for i, n in enumerate((0, 1, 64, 300, 300, 64, 1, 0, 300)):
        t = T0 + 290 * SEC + np.arange(n, dtype=np.int64) * 5 * SEC + \
            rng.integers(-400, 400, n)
        ts.append(t.astype(np.int64))
        vals.append(np.exp(rng.normal(float(i % 3), 3.0, n)))
        offsets.append(offsets[-1] + n)
    mns = [MetricName(b"m", [(b"job", b"j%d" % (s % 2)), (b"s", b"%d" % s)])
           for s in range(len(ts))]
    return (np.concatenate(ts), np.concatenate(vals),
            np.asarray(offsets, np.uint64), mns)


def _check_batch(engine, batch):
    ts, vals, offsets, mns = _batch_columns()
    plan = engine.RollupPlan("avg_over_time", B_START, B_END, B_STEP,
                             window=B_WINDOW)
    out, _, _ = batch.exec(plan)  # rows in original series order
    assert out.shape == (len(mns), 65)
    assert np.all(np.isnan(out[0])) and not np.all(np.isnan(out[3]))
    before, _ = batch.fetch_out(len(mns), 65)
    for op, args in (("by", ["job"]), ("", [])):
        want = aggregate.histogram_aggregate(
            [Series(mn.copy(), row.copy()) for mn, row in zip(mns, out)],
            op, args)
        got = aggregate.histogram_aggregate_batch(batch, mns, op, args)
        assert len(want) > 0
        _assert_same_series(got, want, f"batch {op}")
    after, _ = batch.fetch_out(len(mns), 65)
    assert np.array_equal(_bits(before), _bits(after))  # only read


def test_batch_matches_host(engine):
    ts, vals, offsets, _ = _batch_columns()
    with engine.SeriesBatch(ts, vals, offsets) as b:
        _check_batch(engine, b)


def test_batch_relayouted_and_grouped_exec(engine):
    ts, vals, offsets, mns = _batch_columns()
    group_ids = np.asarray([2, 0, 1, 0, 2, 1, 0, 1, 2], dtype=np.int32)
    with engine.SeriesBatch(ts, vals, offsets, group_ids=group_ids,
                            n_groups=3) as b:
        assert b._perm is not None  # physically relayouted
        _check_batch(engine, b)
        plan = engine.RollupPlan("avg_over_time", B_START, B_END, B_STEP,
                                 window=B_WINDOW, aggr="sum")
        b.exec(plan)
        with pytest.raises(engine.VmGpuError):
            aggregate.histogram_aggregate_batch(b, mns, "by", ["job"])
        _check_batch(engine, b)  # an ungrouped exec makes it valid again


# --- errors ----------------------------------------------------------------

def test_errors_then_clean_call(engine):
    values, group_rows, group_offsets = _small_case()
    lib = engine._load_lib()
    E = engine.VmGpuError

    def fetch_fails():
        with pytest.raises(E):
            engine._aggr_histogram_fetch(lib, 0, 2)

    with pytest.raises(E):  # offsets do not start at 0
        engine.aggr_histogram(values, group_rows, np.asarray([1, 1, 3], np.uint64))
    fetch_fails()
    with pytest.raises(E):  # offsets decrease
        engine.aggr_histogram(values, group_rows, np.asarray([0, 3, 2], np.uint64))
    with pytest.raises(E):  # row out of range
        engine.aggr_histogram(values, np.asarray([2, 0, 3], np.uint32), group_offsets)
    with pytest.raises(E):  # n_grid == 0
        engine.aggr_histogram(np.empty((3, 0)), group_rows, group_offsets)
    fetch_fails()

    # through the C ABI, where no matrix of that size has to exist: the
    # checks run before the values are touched
    def raw(n_grid, rows, offsets):
        n_rows = ctypes.c_uint64(0)
        errbuf = ctypes.create_string_buffer(256)
        rc = lib.vmgpu_aggr_histogram_exec(
            values.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            ctypes.c_uint32(1), ctypes.c_int32(n_grid),
            rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            ctypes.c_uint32(len(offsets) - 1), ctypes.byref(n_rows), errbuf,
            ctypes.c_size_t(len(errbuf)))
        return rc, errbuf.value.decode()

    one = np.zeros(1, np.uint32)
    rc, msg = raw((1 << 30) + 1, one, np.asarray([0, 1], np.uint64))
    assert rc != 0 and "grid" in msg
    rc, msg = raw(-1, one, np.asarray([0, 1], np.uint64))
    assert rc != 0 and "grid" in msg
    # 2.3e6 one-member groups x 488 codes x 2^30 points x 8 B > 2^63
    n = 2_300_000
    rc, msg = raw(1 << 30, np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
    assert rc != 0 and "overflow" in msg
    fetch_fails()

    ts, vals, offsets, mns = _batch_columns()
    with engine.SeriesBatch(ts, vals, offsets) as b:
        with pytest.raises(E):  # no exec yet: no last output
            b.aggr_histogram(np.zeros(len(mns), np.int32), 1)
    fetch_fails()

    _assert_raw(engine.aggr_histogram(values, group_rows, group_offsets),
                _small_reference(), "clean call after the errors")
