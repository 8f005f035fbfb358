"""Host side of the grouped device topk, without a device: a numpy model of
the selection rule of csrc/aggrtopk.hip (held to the oracle bit for bit), and
aggregate._topk_rows_to_series driven by the rows that model produces,
against the host aggregate("topk" / "bottomk")."""
import numpy as np
import pytest

import oracle
import topk_check
from victoriametrics_amd import aggregate
from victoriametrics_amd.binary_op import Series
from victoriametrics_amd.decimal import STALE_NAN_BITS
from victoriametrics_amd.metric_name import MetricName

NAN_BITS = np.uint64(0x7FF8000000000000)


def canon(a):
    """int64 view with every NaN payload mapped to the canonical one."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    bits = a.view(np.uint64).copy()
    bits[np.isnan(a)] = NAN_BITS
    return bits.view(np.int64)


def model_keys(X, reverse):
    """The value key: order-preserving u64, -0.0 folded onto +0.0 first,
    inverted for bottomk, 0 for every NaN."""
    v = np.where(X == 0, 0.0, X)
    b = np.ascontiguousarray(v).view(np.uint64)
    sign = (b >> np.uint64(63)).astype(bool)
    key = np.where(sign, ~b, b | np.uint64(1 << 63))
    if reverse:
        key = ~key
    return np.where(np.isnan(X), np.uint64(0), key)


def model_group(X, ks, reverse):
    """One group: X[n, n_grid] in member order -> the matrix with every cell
    that is not kept set to the canonical NaN."""
    n, n_grid = X.shape
    keys = model_keys(X, reverse)
    out = np.full(X.shape, np.nan)
    pos = np.arange(n)
    for c in range(n_grid):
        kn = aggregate._get_int_k(float(ks[c]), n)
        if kn == 0:
            continue
        order = np.lexsort((pos, keys[:, c]))  # by key, then by position
        keep = order[n - kn:]
        keep = keep[keys[keep, c] != 0]        # a NaN is never kept
        out[keep, c] = X[keep, c]
    return out


def model_rows(values, group_rows, group_offsets, k, reverse=False):
    """What engine.aggr_topk returns, from the model."""
    n_grid = values.shape[1]
    ks = np.broadcast_to(np.asarray(k, np.float64), (n_grid,))
    rg, rs, rl, out = [], [], [], []
    for g in range(len(group_offsets) - 1):
        mem = group_rows[int(group_offsets[g]):int(group_offsets[g + 1])]
        if len(mem) == 0:
            continue
        X = values[mem]
        kept = model_group(X, ks, reverse)
        for p in np.flatnonzero(~np.isnan(kept).all(axis=1)):
            rg.append(g)
            rs.append(mem[p])
            rl.append(X[p, -1])
            out.append(kept[p])
    return (np.asarray(rg, np.uint32), np.asarray(rs, np.uint32),
            np.asarray(rl, np.float64),
            np.asarray(out, np.float64).reshape(len(rg), n_grid))


def _bits(x):
    return np.array([x], dtype=np.uint64).view(np.float64)[0]


SPECIALS = np.array([0.0, -0.0, np.nan, _bits(STALE_NAN_BITS), np.inf, -np.inf,
                     1.0, -1.0, 5e-324])
KS = [0, 1, 2, "n-1", "n", "n+3", 2.9, np.inf, np.nan, -1]


def _datasets(rng, n, n_grid):
    yield rng.normal(size=(n, n_grid))
    yield rng.integers(0, 3, size=(n, n_grid)).astype(np.float64)
    yield SPECIALS[rng.integers(0, len(SPECIALS), size=(n, n_grid))]
    x = rng.integers(0, 2, size=(n, n_grid)).astype(np.float64)
    x[rng.random((n, n_grid)) < 0.3] = np.nan
    yield x


@pytest.mark.parametrize("reverse", [False, True])
def test_model_equals_oracle_bit_for_bit(reverse):
    rng = np.random.default_rng(646)
    for n in (1, 2, 5, 17):
        for X in _datasets(rng, n, 6):
            for k in KS:
                if isinstance(k, str):
                    k = {"n-1": n - 1, "n": n, "n+3": n + 3}[k]
                want = oracle.topk_pointwise(X, float(k), reverse)
                got = model_group(X, np.full(X.shape[1], float(k)), reverse)
                assert np.array_equal(canon(got), canon(want)), (n, k, reverse)
                kept = ~np.isnan(got)
                assert np.array_equal(got.view(np.int64)[kept],
                                      X.view(np.int64)[kept])


def _series(values):
    """Series i carries tags dc = i % 3 and host = i, so `by (dc)` gives
    three groups and `without (host)` the same three under other names."""
    return [Series(MetricName(b"m", [(b"dc", b"dc%d" % (i % 3)),
                                     (b"host", b"h%d" % i)]), row.copy())
            for i, row in enumerate(values)]


def _group_key(mn, op, args):
    mn = mn.copy()
    aggregate.remove_group_tags(mn, op, args)
    return mn.marshal_sorted()


def _by_group(series, op, args):
    out = {}
    for s in series:
        out.setdefault(_group_key(s.mn, op, args), []).append(s)
    return out


def _device_like(series, k, op, args, limit, reverse):
    """aggregate.topk_device with the model in the engine's place."""
    groups = aggregate.prepare_series(series, op, args, limit,
                                      keep_original=True)
    if not groups:
        return []
    v, gr, go = aggregate._matrix(groups)
    raw = model_rows(v, gr, go, k, reverse)
    mns = [s.mn for _, members in groups for s in members]
    return aggregate._topk_rows_to_series(mns, *raw, reverse=reverse)


def _full_matrix(members, result):
    """Rows of result scattered to their member's position; NaN elsewhere."""
    by_name = {s.mn.marshal_sorted(): s.values for s in result}
    nan_row = np.full(len(members[0].values), np.nan)
    return np.stack([by_name.get(s.mn.marshal_sorted(), nan_row)
                     for s in members])


MODIFIERS = [("", ()), ("by", (b"dc",)), ("without", (b"host",))]


@pytest.mark.parametrize("op,args", MODIFIERS)
@pytest.mark.parametrize("name", ["topk", "bottomk"])
@pytest.mark.parametrize("k", [1, 3, 2.9, "per-point"])
@pytest.mark.parametrize("limit", [0, 2])
def test_rows_to_series_matches_host(op, args, name, k, limit):
    """Distinct values: the reference defines every kept cell, so names,
    order and values must agree with the host path."""
    rng = np.random.default_rng(669)
    n, n_grid = 14, 7
    values = rng.normal(size=(n, n_grid))
    values[rng.random((n, n_grid)) < 0.2] = np.nan
    values[4] = np.nan                      # an empty series: dropped first
    values[7, -1] = values[10, -1] = np.nan  # NaN in the column that orders
    if k == "per-point":
        k = np.array([0, 1, 2, 3, np.nan, np.inf, 2.9])
    reverse = name == "bottomk"
    inputs = _series(values)
    got = _device_like(inputs, k, op, args, limit, reverse)
    for s, row in zip(inputs, values):      # the inputs are left alone
        assert np.array_equal(canon(s.values), canon(row))
        assert not any(np.shares_memory(s.values, r.values) for r in got)
    host = aggregate.aggregate(name, _series(values), op, args, limit, arg=k)
    members = _by_group(aggregate.remove_empty_series(_series(values)), op, args)
    got_g, host_g = _by_group(got, op, args), _by_group(host, op, args)
    assert list(got_g) == list(host_g)       # groups in grouping order
    last = {s.mn.marshal_sorted(): s.values[-1] for s in _series(values)}
    for key in host_g:
        names_g = [s.mn.marshal_sorted() for s in got_g[key]]
        names_h = [s.mn.marshal_sorted() for s in host_g[key]]
        assert set(names_g) == set(names_h)
        assert np.array_equal(canon([last[x] for x in names_g]),
                              canon([last[x] for x in names_h]))
        X = np.stack([s.values for s in members[key]])
        topk_check.assert_topk_pointwise(
            X, _full_matrix(members[key], got_g[key]),
            _full_matrix(members[key], host_g[key]), context=f"{name} {op}")


@pytest.mark.parametrize("name", ["topk", "bottomk"])
def test_rows_to_series_matches_host_at_ties(name):
    """Few distinct values: which of the tied members is kept is open in the
    reference, the kept values are not."""
    rng = np.random.default_rng(793)
    values = rng.integers(0, 3, size=(12, 5)).astype(np.float64)
    values[values == 0] = -0.0
    reverse = name == "bottomk"
    got = _device_like(_series(values), 2, "by", (b"dc",), 0, reverse)
    host = aggregate.aggregate(name, _series(values), "by", (b"dc",), arg=2)
    members = _by_group(_series(values), "by", (b"dc",))
    got_g, host_g = (_by_group(x, "by", (b"dc",)) for x in (got, host))
    assert list(got_g) == list(host_g)
    for key in host_g:
        X = np.stack([s.values for s in members[key]])
        topk_check.assert_topk_pointwise(
            X, _full_matrix(members[key], got_g[key]),
            _full_matrix(members[key], host_g[key]), context=name)


def test_rows_order_inside_a_group():
    """Best-first by the last input value, NaN last, ties by descending
    member position; groups in the order given."""
    mns = [MetricName(b"m", [(b"i", b"%d" % i)]) for i in range(6)]
    row_group = np.asarray([0, 0, 0, 0, 1, 1], np.uint32)
    row_member = np.arange(6, dtype=np.uint32)
    row_last = np.asarray([2.0, np.nan, 5.0, 2.0, -1.0, 7.0])
    values = np.arange(12, dtype=np.float64).reshape(6, 2)
    top = aggregate._topk_rows_to_series(mns, row_group, row_member, row_last,
                                         values)
    assert [s.mn.marshal_sorted() for s in top] == \
        [mns[i].marshal_sorted() for i in (2, 3, 0, 1, 5, 4)]
    bottom = aggregate._topk_rows_to_series(mns, row_group, row_member,
                                            row_last, values, reverse=True)
    assert [s.mn.marshal_sorted() for s in bottom] == \
        [mns[i].marshal_sorted() for i in (3, 0, 2, 1, 4, 5)]
    assert np.array_equal(top[0].values, values[2])
    assert aggregate._topk_rows_to_series(
        mns, row_group[:0], row_member[:0], row_last[:0], values[:0]) == []
