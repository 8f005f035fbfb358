"""Device count_values() aggregate (csrc/aggrcv.hip) against the host
reference.

Counts are integers, so everything is compared exactly, bit for bit.  The
raw sparse result (row_group, row_value, every count's bits) is held to a
numpy restatement built here: per group the distinct non-NaN values with -0
and 0 merged, ordered by rollup_multi.count_values_order_key, and
(vals == u).sum(axis=0) with 0 -> NaN; the zero row's value carries the sign
of the first zero in (member position, grid index) order.  The final series
of count_values_device / count_values_batch are held to
aggregate.count_values on the same input, as a map from marshaled metric
name to value bits plus the series count.

One seeded matrix of 130 columns serves every grid width (a prefix of its
columns): about 1.3e5 values.
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
LIMIT = 1000  # tables of 2048 slots for the large groups: sorted in LDS


def _define(name):
    src = open(os.path.join(REPO_ROOT, "victoriametrics_amd", "csrc",
                            "aggrcv.hip")).read()
    return int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1))


M = _define("CV_CHUNK_MEMBERS")   # members per work item
BAND = _define("CV_BAND_ROWS")    # rows of the count tile
# one chunk, exactly one, just over one, three chunks with a ragged last one
GROUP_SIZES = tuple(sorted({1, 2, 63, 64, 65, M - 1, M, M + 1, 2 * M + 3}))
# distinct values per sized group at full width: one row, three, around the
# band height, two bands and one row, past the banded path, past the keys
# kept in LDS, just under the limit
POOL_SIZES = (3, 1, BAND - 1, BAND, BAND + 1, 2 * BAND + 1, 4 * BAND + 1,
              600, LIMIT - 10)
G_NOTHING, G_CONST, G_SPECIAL, G_MOVING = 2, 5, 7, 9
N_UNUSED_ROWS = 17  # matrix rows that belong to no group


def _special_values():
    one = np.float64(1.0)
    tenth = np.float64(0.1)
    vals = [np.inf, -np.inf, 5e-324, -5e-324, 1e21, -1e21, -3.5, -1.0,
            np.nextafter(one, 2.0), np.nextafter(one, 0.0), tenth,
            np.nextafter(tenth, 1.0), np.nan, STALE, 0.0, -0.0]
    # small integers as doubles share all their low mantissa bits
    vals += [float(i) for i in range(64)]
    return np.asarray(vals, dtype=np.float64)


def _zero_groups():
    """+-0 in both first-seen orders, across members and across columns."""
    nan = np.nan
    a = np.full((2, N_COLS), 1.5)
    a[0, :2] = [-0.0, 0.0]
    a[1, :2] = [0.0, -0.0]          # -0 first: member 0, column 0
    b = np.full((2, N_COLS), 2.5)
    b[0, :2] = [0.0, -0.0]
    b[1, :2] = [-0.0, 0.0]          # 0 first
    c = np.full((2, N_COLS), nan)
    c[0, 1] = -0.0                  # member order beats grid order:
    c[1, 0] = 0.0                   # -0 first for n_grid > 1, 0 for n_grid 1
    d = np.full((2, N_COLS), nan)
    d[0, 5] = 0.0
    d[0, 7] = -0.0
    d[1, 0:3] = 4.0                 # 0 first once column 5 is in the grid
    return [("zeroA", a), ("zeroB", b), ("zeroC", c), ("zeroD", d)]


def _group_blocks():
    """[(name, values[members x N_COLS])] in group order."""
    rng = np.random.default_rng(566)
    blocks = []
    for n, p in zip(GROUP_SIZES, POOL_SIZES):
        pool = np.round(rng.normal(0.0, 50.0, p), 3)
        if p > 3:
            pool[: p // 4] = np.arange(p // 4)  # enum-like part
            pool[-1] = -0.0
        pool = np.unique(pool)
        while len(pool) < p:  # rounding or the integers collided
            pool = np.unique(np.concatenate([pool, rng.normal(0, 50.0, p - len(pool))]))
        cells = n * N_COLS
        idx = rng.integers(0, p, cells)
        if cells >= p:
            idx[rng.permutation(cells)[:p]] = np.arange(p)  # every value once
        v = pool[idx].reshape(n, N_COLS)
        if n > 2:
            v[rng.random(v.shape) < 0.03] = np.nan
        blocks.append(("size%d" % n, v))
    nothing = np.tile(np.asarray([np.nan, STALE]), (5, N_COLS // 2 + 1))[:, :N_COLS]
    const = np.full((5, N_COLS), 7.25)
    sv = _special_values()
    idx = (np.arange(len(sv))[:, None] + np.arange(N_COLS)[None, :]) % len(sv)
    special = sv[idx]
    # a value of its own in every column; the other member holds nothing
    moving = np.full((2, N_COLS), np.nan)
    moving[0] = np.arange(N_COLS) + 0.5
    for pos, blk in sorted([(G_NOTHING, ("nothing", nothing)),
                            (G_CONST, ("const", const)),
                            (G_SPECIAL, ("special", special)),
                            (G_MOVING, ("moving", moving))]):
        blocks.insert(pos, blk)
    return blocks + _zero_groups()


def _scatter(blocks, seed, n_unused):
    """(values, group_rows, group_offsets): the members of every group
    scattered over the matrix by a seeded shuffle, so they are
    non-contiguous and the groups interleave."""
    n_cols = blocks[0][1].shape[1]
    n_members = sum(len(v) for _, v in blocks)
    rng = np.random.default_rng(seed)
    n_in_rows = n_members + n_unused
    values = np.round(rng.normal(5.0, 3.0, (n_in_rows, n_cols)), 2)  # unused
    where = rng.permutation(n_in_rows)[:n_members]
    group_rows = where.astype(np.uint32)
    group_offsets = np.zeros(len(blocks) + 1, dtype=np.uint64)
    lo = 0
    for g, (_, v) in enumerate(blocks):
        values[where[lo:lo + len(v)]] = v
        lo += len(v)
        group_offsets[g + 1] = lo
    values.setflags(write=False)
    return values, group_rows, group_offsets


@functools.lru_cache(maxsize=None)
def _matrix130():
    blocks = _group_blocks()
    names = [b[0] for b in blocks]
    assert names[G_NOTHING] == "nothing" and names[G_CONST] == "const"
    assert names[G_SPECIAL] == "special" and names[G_MOVING] == "moving"
    return _scatter(blocks, 567, N_UNUSED_ROWS) + (names,)


@functools.lru_cache(maxsize=None)
def _case(n_grid):
    values, group_rows, group_offsets, _ = _matrix130()
    return np.ascontiguousarray(values[:, :n_grid]), group_rows, group_offsets


def _reference(values, group_rows, group_offsets):
    """The numpy restatement: (row_group, row_value, counts, rows per group)."""
    n_grid = values.shape[1]
    rg, rv, rows, per_group = [], [], [], []
    for g in range(len(group_offsets) - 1):
        blk = values[group_rows[int(group_offsets[g]):int(group_offsets[g + 1])]]
        present = blk[~np.isnan(blk)]
        distinct = sorted({0.0 if v == 0 else v for v in present.tolist()},
                          key=rollup_multi.count_values_order_key)
        per_group.append(len(distinct))
        for u in distinct:
            cnt = (blk == u).sum(axis=0).astype(np.float64)
            cnt[cnt == 0] = np.nan
            if u == 0:
                # the first zero in (member position, grid index) order
                pos = np.flatnonzero(blk.ravel() == 0)[0]
                u = blk.ravel()[pos]
            rg.append(g)
            rv.append(u)
            rows.append(cnt)
    return (np.asarray(rg, np.uint32), np.asarray(rv, np.float64),
            np.asarray(rows, np.float64).reshape(len(rows), n_grid), per_group)


@functools.lru_cache(maxsize=None)
def _raw_reference(n_grid):
    return _reference(*_case(n_grid))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_raw(got, want, context):
    row_group, row_value, values = got
    assert row_group.dtype == np.uint32 and row_value.dtype == np.float64
    assert values.dtype == np.float64
    assert np.array_equal(row_group, want[0]), f"{context}: row_group"
    assert np.array_equal(_bits(row_value), _bits(want[1])), f"{context}: row_value"
    assert values.shape == want[2].shape, context
    assert np.array_equal(_bits(values), _bits(want[2])), f"{context}: values"


def _run(engine, case, limit, context):
    """Reference first (its rows per group must respect the limit), then the
    device, compared exactly."""
    want = _reference(*case) if not isinstance(case, int) else _raw_reference(case)
    args = _case(case) if isinstance(case, int) else case
    assert max(want[3], default=0) <= limit, context
    got = engine.aggr_count_values(*args, limit)
    _assert_raw(got, want, context)
    return got, want


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


def test_reference_covers_the_paths():
    """What the pools are there for, asserted on the reference alone."""
    per_group = _raw_reference(N_COLS)[3]
    names = _matrix130()[3]
    sized = [r for r, n in zip(per_group, names) if n.startswith("size")]
    assert tuple(sized) == POOL_SIZES
    assert max(per_group) == LIMIT - 10
    assert per_group[G_NOTHING] == 0 and per_group[G_CONST] == 1
    assert per_group[G_MOVING] == N_COLS


@pytest.mark.parametrize("n_grid", WIDTHS)
def test_raw_matches_reference(engine, n_grid):
    got, _ = _run(engine, n_grid, LIMIT, f"n_grid={n_grid}")
    # ordered by group, then ascending value, no value twice in a group
    keys = [(int(g), rollup_multi.count_values_order_key(0.0 if v == 0 else v))
            for g, v in zip(got[0], got[1])]
    assert keys == sorted(set(keys))


def test_row_structure(engine):
    n_grid = 65
    (row_group, row_value, values), _ = _run(engine, n_grid, LIMIT, "structure")
    names = _matrix130()[3]
    # all-NaN / stale members: no rows, later groups unmoved
    assert not np.any(row_group == G_NOTHING)
    assert np.any(row_group == G_NOTHING - 1) and np.any(row_group == G_NOTHING + 1)
    # one value held everywhere: one row, the member count in every column
    sel = row_group == G_CONST
    assert sel.sum() == 1 and row_value[sel][0] == 7.25
    assert np.all(values[sel] == 5.0)
    # a value of its own per column: n_grid rows of one non-NaN cell each
    sel = row_group == G_MOVING
    assert sel.sum() == n_grid
    assert np.all((~np.isnan(values[sel])).sum(axis=1) == 1)
    assert np.all(values[sel][~np.isnan(values[sel])] == 1.0)
    # an absent count is NaN, never 0.0; every row counts somewhere
    assert not np.any(values == 0)
    assert np.all(np.any(~np.isnan(values), axis=1))
    # the specials: -Inf first, +Inf last, neighbours one ulp apart apart
    sv = row_value[row_group == G_SPECIAL]
    assert sv[0] == -np.inf and sv[-1] == np.inf
    assert not np.any(np.isnan(sv))
    for x in (5e-324, -5e-324, 1e21, np.nextafter(np.float64(1.0), 2.0), 1.0,
              np.nextafter(np.float64(1.0), 0.0)):
        assert (sv == x).sum() == 1
    assert (sv == 0).sum() == 1  # +-0 is one row
    assert set(range(64)) <= set(sv.tolist())
    # the zero row's sign is the first-seen zero's
    for name, negative in (("zeroA", True), ("zeroB", False), ("zeroC", True),
                           ("zeroD", False)):
        zv = row_value[(row_group == names.index(name)) & (row_value == 0)]
        assert len(zv) == 1 and bool(np.signbit(zv[0])) == negative, name
    # ... and at one column zeroC meets member 1's +0 first
    rg1, rv1, _ = engine.aggr_count_values(*_case(1), LIMIT)
    zv = rv1[(rg1 == names.index("zeroC")) & (rv1 == 0)]
    assert len(zv) == 1 and not np.signbit(zv[0])


def test_tiny_groups_wave_sort(engine):
    """members x n_grid <= 32: tables of 64 slots, sorted one wave each."""
    rng = np.random.default_rng(568)
    blocks = []
    for g in range(37):
        n = 1 + g % 4
        v = rng.integers(-3, 4, (n, 8)).astype(np.float64)
        v[rng.random(v.shape) < 0.2] = np.nan
        if g % 5 == 0:
            v[0, 0] = -0.0
        blocks.append(("t%d" % g, v))
    _run(engine, _scatter(blocks, 569, 3), LIMIT, "tiny groups")


def _many_distinct(rng, n_distinct, members):
    pool = np.unique(np.round(rng.normal(0.0, 1e3, 2 * n_distinct), 4))
    pool = rng.permutation(pool)[:n_distinct]
    assert len(pool) == n_distinct
    idx = np.concatenate([np.arange(n_distinct),
                          rng.integers(0, n_distinct, members * N_COLS - n_distinct)])
    return pool[rng.permutation(idx)].reshape(members, N_COLS)


@pytest.mark.parametrize("limit,n_distinct,members", [
    # tables of 4096 slots, more than a workgroup holds in LDS; the 1100
    # occupied ones still fit and are gathered there
    (1500, 1100, 30),
    # more rows than LDS holds: the slice is sorted in place
    (3000, 2500, 20),
])
def test_large_table_sort_classes(engine, limit, n_distinct, members):
    rng = np.random.default_rng(570)
    big = _many_distinct(rng, n_distinct, members)
    small = rng.integers(0, 9, (40, N_COLS)).astype(np.float64)
    case = _scatter([("small", small), ("big", big), ("small2", small + 0.5)], 571, 5)
    _, want = _run(engine, case, limit, "large tables")
    assert want[3] == [9, n_distinct, 9]


def _distinct_group(n_distinct, base):
    """3 members x 40 columns holding exactly n_distinct values."""
    idx = np.arange(120) % n_distinct
    return (base + idx.astype(np.float64)).reshape(3, 40)


def test_limit(engine):
    L = 70
    lib = engine._load_lib()
    exact = _scatter([("a", _distinct_group(L, 0.0))], 572, 2)
    _, want = _run(engine, exact, L, "exactly the limit")
    assert want[3] == [L]
    two = _scatter([("a", _distinct_group(L, 0.0)),
                    ("b", _distinct_group(L, 1000.0))], 573, 2)
    _run(engine, two, L, "two groups at the limit")
    over = _scatter([("a", _distinct_group(L, 0.0)),
                     ("b", _distinct_group(L + 1, 0.0))], 574, 2)
    with pytest.raises(engine.CountValuesLimitError) as ei:
        engine.aggr_count_values(*over, L)
    assert "group 1" in str(ei.value) and "70" in str(ei.value)
    with pytest.raises(engine.VmGpuError):  # a failed exec leaves no result
        engine._aggr_count_values_fetch(lib, 0, 40)
    # the wrappers speak the host function's words
    series = [Series(MetricName(b"m", [(b"i", b"%d" % i)]), row.copy())
              for i, row in enumerate(_distinct_group(L + 1, 0.0))]
    with pytest.raises(ValueError) as host:
        aggregate.count_values("v", [Series(s.mn.copy(), s.values.copy())
                                     for s in series], max_series_per_aggr=L)
    with pytest.raises(ValueError) as dev:
        aggregate.count_values_device("v", series, max_series_per_aggr=L)
    assert str(dev.value) == str(host.value)
    assert str(dev.value) == "more than 70 series generated by count_values()"
    _run(engine, exact, L, "clean call after the failure")


def test_two_runs_same_bits(engine):
    a = engine.aggr_count_values(*_case(130), LIMIT)
    b = engine.aggr_count_values(*_case(130), LIMIT)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_shuffled_matrix_rows(engine):
    """The same members at other matrix rows behind the same CSR order."""
    values, group_rows, group_offsets = _case(65)
    want = engine.aggr_count_values(values, group_rows, group_offsets, LIMIT)
    p = np.random.default_rng(575).permutation(len(values))
    moved = np.empty_like(values)
    moved[p] = values
    got = engine.aggr_count_values(moved, p[group_rows].astype(np.uint32),
                                   group_offsets, LIMIT)
    _assert_raw(got, _raw_reference(65)[:3], "shuffled")
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()


def _small_case():
    values = np.asarray([[1.0, np.nan], [1.0, 250.0], [-0.0, 1.0]])
    return (values, np.asarray([2, 0, 1], np.uint32),
            np.asarray([0, 1, 3], np.uint64))


def test_large_small_large(engine):
    """Grow-only buffers reused by a smaller call, and no table, counter or
    zero word left over from the call before."""
    small = _reference(*_small_case())
    assert len(small[0]) == 4
    _run(engine, 130, LIMIT, "large")
    _assert_raw(engine.aggr_count_values(*_small_case(), 5), small, "small")
    _run(engine, 130, LIMIT, "large again")
    _assert_raw(engine.aggr_count_values(*_small_case(), 5), small, "small again")


def test_empty_inputs(engine):
    values = _case(2)[0]
    for rows, offsets in ((np.empty(0, np.uint32), np.zeros(1, np.uint64)),
                          (np.empty(0, np.uint32), np.zeros(4, np.uint64))):
        rg, rv, out = engine.aggr_count_values(values, rows, offsets, LIMIT)
        assert len(rg) == 0 and len(rv) == 0 and out.shape == (0, 2)
    # empty groups between groups with members
    v, gr, _ = _small_case()
    _run(engine, (v, gr, np.asarray([0, 0, 1, 1, 3, 3], np.uint64)), 5,
         "empty groups")


# --- final series ----------------------------------------------------------

def _series_map(series_list):
    m = {s.mn.marshal_sorted(): _bits(s.values).tobytes() for s in series_list}
    assert len(m) == len(series_list), "duplicate metric names"
    return m


def _assert_same_series(got, want, context):
    assert len(got) == len(want), f"{context}: {len(got)} != {len(want)} series"
    assert _series_map(got) == _series_map(want), context


def _fresh(named):
    return [Series(mn.copy(), v.copy()) for mn, v in named]


@functools.lru_cache(maxsize=None)
def _named_small():
    """48 series x 33 points with job / inst labels; some names already
    carry the destination label."""
    rng = np.random.default_rng(576)
    out = []
    for s in range(48):
        tags = [(b"job", b"j%d" % (s % 6)), (b"inst", b"i%d" % s)]
        if s % 4 == 0:
            tags.append((b"state", b"old%d" % (s % 3)))
        v = rng.integers(-2, 6, 33).astype(np.float64) * 0.5
        v[rng.random(33) < 0.1] = np.nan
        v[rng.random(33) < 0.05] = -0.0
        if s == 7:
            v[:] = np.nan  # dropped by remove_empty_series
        if s == 8:
            v[:] = [np.inf, -np.inf, 1e21] * 11
        out.append((MetricName(b"up", tags), v))
    return out


@pytest.mark.parametrize("op,args,limit", [
    ("by", ("job",), 0),
    ("by", ("job", "state"), 0),   # dst_label inside the by list
    ("without", ("inst",), 0),
    ("without", ("inst", "state"), 0),
    ("", (), 0),
    ("by", ("job",), 4),           # limit below the 6 groups
])
def test_device_matches_host_names(engine, op, args, limit):
    want = aggregate.count_values("state", _fresh(_named_small()), op,
                                  list(args), limit)
    got = aggregate.count_values_device("state", _fresh(_named_small()), op,
                                        list(args), limit)
    assert len(want) > 0
    _assert_same_series(got, want, f"{op} {args} limit={limit}")
    labels = {s.mn.get_tag_value(b"state") for s in got}
    assert b"-0" in labels or b"0" in labels
    assert not any(lab.startswith(b"old") for lab in labels)
    if limit:
        assert len({s.mn.get_tag_value(b"job") for s in got}) == limit


# --- batch form ------------------------------------------------------------

SEC = 1000
T0 = 1_600_000_000_000
B_START, B_STEP, B_WINDOW = T0 + 300 * SEC, 20 * SEC, 60 * SEC
B_END = B_START + 64 * B_STEP  # 65 points


@functools.lru_cache(maxsize=None)
def _batch_columns():
    rng = np.random.default_rng(577)
    ts, vals, offsets = [], [], [0]
    for i, n in enumerate((0, 1, 64, 300, 300, 64, 1, 0, 300)):
        t = T0 + 290 * SEC + np.arange(n, dtype=np.int64) * 5 * SEC + \
            rng.integers(-400, 400, n)
        ts.append(t.astype(np.int64))
        v = rng.integers(0, 3, n).astype(np.float64)
        if i == 3:
            v[:] = -0.0
        if i == 4:
            v[:] = 0.0
        vals.append(v)
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
        want = aggregate.count_values(
            "v", [Series(mn.copy(), row.copy()) for mn, row in zip(mns, out)],
            op, args)
        got = aggregate.count_values_batch("v", batch, mns, op, args)
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
            aggregate.count_values_batch("v", b, mns, "by", ["job"])
        _check_batch(engine, b)  # an ungrouped exec makes it valid again


# --- errors ----------------------------------------------------------------

def test_errors_then_clean_call(engine):
    values, group_rows, group_offsets = _small_case()
    lib = engine._load_lib()
    E = engine.VmGpuError

    def fetch_fails():
        with pytest.raises(E):
            engine._aggr_count_values_fetch(lib, 0, 2)

    with pytest.raises(E):  # offsets do not start at 0
        engine.aggr_count_values(values, group_rows,
                                 np.asarray([1, 1, 3], np.uint64), 5)
    fetch_fails()
    with pytest.raises(E):  # offsets decrease
        engine.aggr_count_values(values, group_rows,
                                 np.asarray([0, 3, 2], np.uint64), 5)
    with pytest.raises(E):  # row out of range
        engine.aggr_count_values(values, np.asarray([2, 0, 3], np.uint32),
                                 group_offsets, 5)
    with pytest.raises(E):  # n_grid == 0
        engine.aggr_count_values(np.empty((3, 0)), group_rows, group_offsets, 5)
    fetch_fails()

    # through the C ABI, where no matrix of that size has to exist: the
    # checks run before the values are touched
    def raw(n_grid, rows, offsets, limit=1000):
        n_rows = ctypes.c_uint64(0)
        errbuf = ctypes.create_string_buffer(256)
        rc = lib.vmgpu_aggr_count_values_exec(
            values.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            ctypes.c_uint32(1), ctypes.c_int32(n_grid),
            rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            ctypes.c_uint32(len(offsets) - 1), ctypes.c_uint32(limit),
            ctypes.byref(n_rows), errbuf, ctypes.c_size_t(len(errbuf)))
        return rc, errbuf.value.decode()

    one = np.zeros(1, np.uint32)
    rc, msg = raw((1 << 30) + 1, one, np.asarray([0, 1], np.uint64))
    assert rc != 0 and "grid" in msg
    rc, msg = raw(-1, one, np.asarray([0, 1], np.uint64))
    assert rc != 0 and "grid" in msg
    for bad in (0, (1 << 24) + 1):
        rc, msg = raw(2, one, np.asarray([0, 1], np.uint64), bad)
        assert rc != 0 and "max_rows_per_group" in msg
    # 2.3e6 one-member groups x 1000 rows x 2^30 points x 8 B > 2^63
    n = 2_300_000
    rc, msg = raw(1 << 30, np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
    assert rc != 0 and "overflow" in msg
    fetch_fails()

    ts, vals, offsets, mns = _batch_columns()
    with engine.SeriesBatch(ts, vals, offsets) as b:
        with pytest.raises(E):  # no exec yet: no last output
            b.aggr_count_values(np.zeros(len(mns), np.int32), 1, 5)
    fetch_fails()

    _assert_raw(engine.aggr_count_values(values, group_rows, group_offsets, 5),
                _reference(values, group_rows, group_offsets),
                "clean call after the errors")
