"""Grouped device topk / bottomk (csrc/aggrtopk.hip) against the oracle.

Reference: oracle.topk_pointwise applied to each group's rows in member
order (for a per-point k once per distinct k, taking that k's columns).  The
device keeps, of equal values, the later member, as the oracle does, so the
bar is equality of bits: of values after mapping every NaN payload to one,
and of row_group, row_src and row_last.

One seeded matrix of 130 columns serves every grid width (a prefix of its
columns): about 2e5 values.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import oracle
import topk_check
from conftest import REPO_ROOT
from test_topk_grouped_plumbing import (_by_group, _full_matrix, _series,
                                        canon)
from victoriametrics_amd import aggregate
from victoriametrics_amd.binary_op import Series
from victoriametrics_amd.decimal import STALE_NAN_BITS
from victoriametrics_amd.metric_name import MetricName

pytestmark = pytest.mark.gpu

STALE = np.array([STALE_NAN_BITS], dtype=np.uint64).view(np.float64)[0]
CSRC = os.path.join(REPO_ROOT, "victoriametrics_amd", "csrc")


def _define(name, header="aggrtopk.hip"):
    src = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1))


M = _define("AT_CHUNK_MEMBERS")     # members per work item
C = _define("AT_LIST_CAP")          # largest k of the list class
WAVE_CAP = _define("CVOT_WAVE_CAP", "value_key.h")
BLOCK_CAP = _define("CVOT_BLOCK_CAP", "value_key.h")
WIDTHS = (1, 63, 64, 65, 130)
N_COLS = max(WIDTHS)
# around k = 3 and k = C, C + 1; one chunk, exactly one, just over one, three
# chunks with a ragged last one; group 6 is empty
GROUP_SIZES = (1, 2, 3, 4, C - 1, C, 0, C + 1, C + 2, 64, 65, M - 1, M, M + 1,
               2 * M + 3)
KS = (0, 1, 3, C, C + 1, 2.9, np.inf, np.nan, -1)


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


@functools.lru_cache(maxsize=None)
def _matrix130():
    """(values, group_rows, group_offsets): members at shuffled matrix rows,
    some rows in no group, the first member of group 0 also the last member
    of the last group.  Even columns hold normals, odd ones half-integers in
    [-3, 3] (ties everywhere); 5 % NaN."""
    rng = np.random.default_rng(646)
    n_members = sum(GROUP_SIZES)
    n_rows = n_members + 17
    values = rng.normal(size=(n_rows, N_COLS))
    values[:, 1::2] = np.clip(np.round(values[:, 1::2] * 2) / 2, -3, 3)
    values[rng.random(values.shape) < 0.05] = np.nan
    rows = rng.permutation(n_rows)[:n_members].astype(np.uint32)
    group_rows = np.concatenate([rows, rows[:1]])
    offsets = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.uint64)
    offsets[-1] += 1
    return values, group_rows, offsets


def _case(n_grid):
    values, group_rows, offsets = _matrix130()
    return np.ascontiguousarray(values[:, :n_grid]), group_rows, offsets


def _reference(values, group_rows, group_offsets, k, reverse):
    """The raw result the device must return, from the oracle."""
    n_grid = values.shape[1]
    ks = np.broadcast_to(np.asarray(k, np.float64), (n_grid,))
    distinct = {}
    for c, kc in enumerate(ks):
        distinct.setdefault(float(kc) if kc == kc else "nan", []).append(c)
    rg, rs, rl, out = [], [], [], []
    for g in range(len(group_offsets) - 1):
        mem = group_rows[int(group_offsets[g]):int(group_offsets[g + 1])]
        if len(mem) == 0:
            continue
        X = np.ascontiguousarray(values[mem])
        kept = np.empty_like(X)
        for kc, cols in distinct.items():
            kept[:, cols] = oracle.topk_pointwise(
                X, np.nan if kc == "nan" else kc, reverse)[:, cols]
        for p in np.flatnonzero(~np.isnan(kept).all(axis=1)):
            rg.append(g)
            rs.append(mem[p])
            rl.append(X[p, -1])
            out.append(kept[p])
    return (np.asarray(rg, np.uint32), np.asarray(rs, np.uint32),
            np.asarray(rl, np.float64),
            np.asarray(out, np.float64).reshape(len(rg), n_grid))


def _assert_raw(got, want, context):
    assert got[3].shape == want[3].shape, \
        f"{context}: {got[3].shape} rows x cols, want {want[3].shape}"
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]), f"{context}: row_group"
    assert np.array_equal(got[1], want[1]), f"{context}: row_src"
    assert np.array_equal(canon(got[2]), canon(want[2])), f"{context}: row_last"
    differ = canon(got[3]) != canon(want[3])
    assert not differ.any(), \
        f"{context}: values differ at {np.argwhere(differ)[:5].tolist()}"
    # what is not kept is the canonical NaN itself
    assert (got[3].view(np.uint64)[np.isnan(got[3])]
            == 0x7FF8000000000000).all(), f"{context}: NaN payload"


def _check(engine, values, group_rows, group_offsets, k, reverse, context):
    before = values.copy()
    got = engine.aggr_topk(values, group_rows, group_offsets, k, reverse)
    assert np.array_equal(canon(values), canon(before)), f"{context}: input"
    _assert_raw(got, _reference(values, group_rows, group_offsets, k, reverse),
                context)
    return got


# --- geometry ----------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n_grid", WIDTHS)
def test_geometry(engine, n_grid, reverse):
    """Every k of KS over the same data; C and C + 1 put it through both
    classes."""
    for k in KS:
        _check(engine, *_case(n_grid), k, reverse,
               f"n_grid={n_grid} k={k} reverse={reverse}")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("k", [C + 1, "per-point"])
def test_sort_class_sizes(engine, k, reverse):
    """Groups at both edges of the three sort size classes, 3 columns."""
    rng = np.random.default_rng(669)
    sizes = (WAVE_CAP, WAVE_CAP + 1, BLOCK_CAP, BLOCK_CAP + 1)
    n = sum(sizes)
    values = rng.normal(size=(n, 3))
    values[:, 1] = rng.integers(0, 40, n)          # ties at every threshold
    values[rng.random(values.shape) < 0.05] = np.nan
    group_rows = rng.permutation(n).astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    if k == "per-point":
        k = np.asarray([C + 1, WAVE_CAP + 44, BLOCK_CAP - 1], np.float64)
    _check(engine, values, group_rows, offsets, k, reverse, f"sort k={k}")


@pytest.mark.parametrize("reverse", [False, True])
def test_per_point_k(engine, reverse):
    """The class follows the largest k, the threshold its own column's."""
    pattern = [0, 1, C, C + 1, 64, np.inf, np.nan]
    for n_grid, pat in ((65, pattern), (65, pattern[:3]), (7, pattern)):
        ks = np.resize(np.asarray(pat, np.float64), n_grid)
        _check(engine, *_case(n_grid), ks, reverse, f"per-point {pat}")


# --- values ------------------------------------------------------------------

def _value_case():
    rng = np.random.default_rng(793)
    n_a = 2 * M + 3
    a = rng.choice(np.asarray([-2.0, -0.0, 3.0]), size=(n_a, 6))
    a[:, 0] = 7.0                       # all equal: the position decides
    a[:, 1] = np.nan                    # nothing to keep
    a[:, 2] = rng.choice(np.asarray([0.0, -0.0]), n_a)
    nothing = np.tile(np.asarray([np.nan, STALE]), (5, 3))
    sv = np.asarray([0.0, -0.0, np.inf, -np.inf, STALE, np.nan, 5e-324, -5e-324])
    special = sv[rng.integers(0, len(sv), size=(40, 6))]
    minus_zero = np.full((4, 6), -0.0)
    blocks = [a, nothing, special, minus_zero]
    values = np.concatenate(blocks)
    sizes = [len(b) for b in blocks]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return values, np.arange(len(values), dtype=np.uint32), offsets


@pytest.mark.parametrize("reverse", [False, True])
def test_ties_nans_and_zeros(engine, reverse):
    values, group_rows, offsets = _value_case()
    for k in (1, 3, C, C + 1, M + 1, 2 * M + 3):
        got = _check(engine, values, group_rows, offsets, k, reverse,
                     f"values k={k} reverse={reverse}")
        row_group, row_src, _, out = got
        assert 1 not in row_group            # the all-NaN group has no row
        assert np.isnan(out[row_group == 0, 1]).all()
        # the last k members of the all-equal column, nobody else
        kept0 = row_src[(row_group == 0) & ~np.isnan(out[:, 0])]
        n_a = int(offsets[1])
        assert kept0.tolist() == list(range(n_a - min(k, n_a), n_a))
        # a kept -0.0 is still -0.0
        mz = out[row_group == 3]
        assert len(mz) == min(k, 4)
        assert np.signbit(mz).all() and (mz == 0).all()


def test_two_runs_same_bytes(engine):
    for k in (3, C + 1):
        a = engine.aggr_topk(*_case(130), k)
        b = engine.aggr_topk(*_case(130), k)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


# --- batch forms ---------------------------------------------------------------

START = 1_000_000_000_000
STEP = 15_000


class _Resident:
    """A matrix made resident as a batch's evaluated output."""

    def __init__(self, engine, X, group_ids=None, n_groups=0):
        n_grid = X.shape[1]
        present = ~np.isnan(X)
        grid = START + np.arange(n_grid, dtype=np.int64) * STEP
        ts = np.broadcast_to(grid, X.shape)[present]
        offsets = np.concatenate(
            [[0], np.cumsum(present.sum(axis=1))]).astype(np.uint64)
        self.engine = engine
        self.args = (START, START + (n_grid - 1) * STEP, STEP)
        self.batch = engine.SeriesBatch(ts, X[present], offsets, group_ids,
                                        n_groups)
        self.host_out = self.exec()

    def exec(self, aggr="none"):
        plan = self.engine.RollupPlan("last_over_time", *self.args,
                                      window=STEP, aggr=aggr)
        return self.batch.exec(plan)[0]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.batch.close()


def _batch_matrix():
    rng = np.random.default_rng(704)
    X = rng.normal(size=(300, 65))
    X[:, 1::2] = np.round(X[:, 1::2])
    X[rng.random(X.shape) < 0.1] = np.nan
    X[11] = np.nan                      # a series with no output at all
    group_of = rng.integers(-1, 5, len(X)).astype(np.int32)
    mns = [MetricName(b"m", [(b"dc", b"dc%d" % (i % 4)), (b"host", b"h%d" % i)])
           for i in range(len(X))]
    return X, group_of, mns


def _csr(group_of, n_groups):
    rows = np.flatnonzero(group_of >= 0)
    order = np.argsort(group_of[rows], kind="stable")
    offsets = np.zeros(n_groups + 1, np.uint64)
    np.cumsum(np.bincount(group_of[rows], minlength=n_groups), out=offsets[1:])
    return rows[order].astype(np.uint32), offsets


def _names_and_bits(series):
    return [(s.mn.marshal_sorted(), canon(s.values).tobytes()) for s in series]


def _check_batch(engine, res, X, group_of, mns):
    out = res.exec()
    assert np.array_equal(canon(out), canon(X))
    before, _ = res.batch.fetch_out(len(X), X.shape[1])
    group_rows, offsets = _csr(group_of, 5)
    for k, reverse in ((3, False), (C + 1, True)):
        got = res.batch.aggr_topk(group_of, 5, k, reverse)
        # row_src names ORIGINAL series, also on a relayouted batch
        _assert_raw(got, _reference(X, group_rows, offsets, k, reverse),
                    f"batch k={k}")
        via_batch = aggregate.topk_batch(res.batch, mns, k, "by", (b"dc",),
                                         reverse=reverse)
        via_host_matrix = aggregate.topk_device(
            _series_named(mns, out), k, "by", (b"dc",), reverse=reverse)
        assert len(via_batch) > 0
        assert _names_and_bits(via_batch) == _names_and_bits(via_host_matrix)
    after, _ = res.batch.fetch_out(len(X), X.shape[1])
    assert np.array_equal(canon(before), canon(after))   # only read
    # the in-place device topk still finds the matrix it expects
    got = engine.topk_pointwise(res.batch, 5)
    topk_check.assert_topk_pointwise(X, got, oracle.topk_pointwise(X, 5))


def _series_named(mns, values):
    return [Series(mn.copy(), row.copy()) for mn, row in zip(mns, values)]


def test_batch_reads_resident_output(engine):
    X, group_of, mns = _batch_matrix()
    with _Resident(engine, X) as res:
        _check_batch(engine, res, X, group_of, mns)


def test_batch_relayouted_and_grouped_exec(engine):
    X, group_of, mns = _batch_matrix()
    group_ids = (np.arange(len(X)) % 3).astype(np.int32)
    with _Resident(engine, X, group_ids, 3) as res:
        assert res.batch._perm is not None  # physically relayouted
        _check_batch(engine, res, X, group_of, mns)
        res.exec(aggr="sum")
        with pytest.raises(engine.VmGpuError):
            res.batch.aggr_topk(group_of, 5, 3)
        with pytest.raises(engine.VmGpuError):
            aggregate.topk_batch(res.batch, mns, 3, "by", (b"dc",))
        _check_batch(engine, res, X, group_of, mns)  # valid again


# --- host parity ---------------------------------------------------------------

@pytest.mark.parametrize("op,args", [("", ()), ("by", (b"dc",)),
                                     ("without", (b"host",))])
@pytest.mark.parametrize("name,k,limit", [
    ("topk", 2, 0), ("bottomk", 2, 0), ("topk", C + 1, 0), ("bottomk", 3, 2),
    ("topk", "per-point", 2)])
def test_device_matches_host(engine, op, args, name, k, limit):
    rng = np.random.default_rng(751)
    n, n_grid = 90, 9
    values = rng.normal(size=(n, n_grid))
    values[:, 1::2] = np.round(values[:, 1::2])   # ties: kept values only
    values[rng.random(values.shape) < 0.15] = np.nan
    values[5] = np.nan
    if k == "per-point":
        k = np.resize(np.asarray([0, 1, C + 1, np.nan, np.inf, 2.9]), n_grid)
    reverse = name == "bottomk"
    inputs = _series(values)
    got = aggregate.topk_device(inputs, k, op, args, limit, reverse)
    for s, row in zip(inputs, values):
        assert np.array_equal(canon(s.values), canon(row))
    host = aggregate.aggregate(name, _series(values), op, args, limit, arg=k)
    members = _by_group(aggregate.remove_empty_series(_series(values)), op, args)
    got_g, host_g = _by_group(got, op, args), _by_group(host, op, args)
    assert len(host_g) > 0 and list(got_g) == list(host_g)
    for key in host_g:
        X = np.stack([s.values for s in members[key]])
        topk_check.assert_topk_pointwise(
            X, _full_matrix(members[key], got_g[key]),
            _full_matrix(members[key], host_g[key]), context=f"{name} {op}")
        # best-first by the last input value, whoever was kept at a tie
        last = {s.mn.marshal_sorted(): s.values[-1] for s in members[key]}
        seq = [last[s.mn.marshal_sorted()] for s in got_g[key]]
        want = sorted(seq, key=(
            aggregate._greater_with_nans_key if reverse
            else aggregate._less_with_nans_key))[::-1]
        assert np.array_equal(seq, want, equal_nan=True)


# --- errors --------------------------------------------------------------------

def _small_case():
    values, group_rows, offsets = _value_case()
    return values[-44:], np.arange(44, dtype=np.uint32), \
        np.asarray([0, 40, 44], np.uint64)


def test_errors_then_clean_call(engine):
    values, group_rows, offsets = _small_case()
    lib = engine._load_lib()
    E = engine.VmGpuError

    def fetch_fails():
        with pytest.raises(E, match="no aggr topk result"):
            engine._aggr_topk_fetch(lib, 0, 6)

    with pytest.raises(E, match="start at 0"):
        engine.aggr_topk(values, group_rows, np.asarray([1, 40, 44], np.uint64), 2)
    fetch_fails()
    with pytest.raises(E, match="decrease"):
        engine.aggr_topk(values, group_rows, np.asarray([0, 44, 40], np.uint64), 2)
    with pytest.raises(E, match="out of range"):
        bad = group_rows.copy()
        bad[7] = 44
        engine.aggr_topk(values, bad, offsets, 2)
    with pytest.raises(E, match="grid"):
        engine.aggr_topk(np.empty((44, 0)), group_rows, offsets, 2)
    fetch_fails()

    def raw(ks, n_ks):
        n_rows = ctypes.c_uint64(0)
        errbuf = ctypes.create_string_buffer(256)
        rc = lib.vmgpu_aggr_topk_exec(
            values.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            ctypes.c_uint32(44), ctypes.c_int32(6),
            group_rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            ctypes.c_uint32(2),
            ks.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            if ks is not None else None,
            ctypes.c_uint32(n_ks), ctypes.c_int32(0), ctypes.byref(n_rows),
            errbuf, ctypes.c_size_t(len(errbuf)))
        return rc, errbuf.value.decode()

    rc, msg = raw(None, 6)
    assert rc != 0 and "ks" in msg
    fetch_fails()
    for n_ks in (5, 7):
        rc, msg = raw(np.ones(7), n_ks)
        assert rc != 0 and "n_ks" in msg
    fetch_fails()

    with engine.SeriesBatch(np.zeros(1, np.int64), np.ones(1),
                            np.asarray([0, 1], np.uint64)) as b:
        with pytest.raises(E, match="no rollup output"):
            b.aggr_topk(np.zeros(1, np.int32), 1, 2)
    fetch_fails()

    _check(engine, values, group_rows, offsets, 2, False,
           "clean call after the errors")


def test_large_small_large_small(engine):
    """Grow-only result buffers reused by a smaller call, and no flag or
    threshold left over from the call before."""
    for turn in range(2):
        _check(engine, *_case(130), C + 1, False, f"large {turn}")
        _check(engine, *_small_case(), 2, True, f"small {turn}")


def test_empty(engine):
    values = _case(5)[0]

    def assert_empty(got):
        assert [x.shape for x in got] == [(0,), (0,), (0,), (0, 5)]
        assert [x.dtype for x in got] == [np.uint32, np.uint32, np.float64,
                                          np.float64]

    for rows, offsets in ((np.empty(0, np.uint32), np.zeros(1, np.uint64)),
                          (np.empty(0, np.uint32), np.zeros(4, np.uint64))):
        assert_empty(engine.aggr_topk(values, rows, offsets, 3))
    _, group_rows, offsets = _case(5)
    for k in (0, -2.0, np.nan, np.zeros(5)):
        assert_empty(engine.aggr_topk(values, group_rows, offsets, k))
    _check(engine, *_case(5), 1, False, "after the empty calls")
