"""colagg_kernel and colagg_filter_kernel (csrc/aggrcol.hip) on the class
batches of matrix_classes.py, and at the launch shapes no other test reaches.

The device is held to the C oracle (same statement order: equal bits, NaN
payloads aside) and to the plain reference of matrix_reference.py, which
shares no code with either (equal values, -0.0 == 0.0).  geomean ends in
pow() and keeps rtol 1e-12; sum, avg, sum2 and share are also held to
math.fsum within the derived summation bound.
test_matrix_class_inputs.py shows on the CPU that none of these inputs is
trivial.

The "inf" batch found one disagreement with the reference: where a column's
median is infinite the deviations of the infinite samples are NaN; the
reference's quantile() drops them, the kernel (and the oracle) sorted them
along and answered NaN.  [+Inf, 1, +Inf, 2] gave NaN and now gives +Inf.
"""
import math

import numpy as np
import pytest

import oracle
import matrix_classes as mc
import matrix_reference as mr

pytestmark = pytest.mark.gpu

NAN = mc.NAN


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


def _bits(a):
    """Bit patterns with every NaN made the same one."""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = NAN
    return a.view(np.int64)


def _assert_bits(got, exp, context):
    bad = _bits(got) != _bits(exp)
    assert not bad.any(), (f"{context}: {int(bad.sum())} differ from the "
                           f"oracle, first at {np.argwhere(bad)[0]}: "
                           f"{got[bad][0]!r} != {exp[bad][0]!r}")


def _assert_same(got, exp, context):
    bad = mr.same_arrays(got, exp)
    assert not bad.any(), (f"{context}: {int(bad.sum())} differ from the "
                           f"plain reference, first at {np.argwhere(bad)[0]}: "
                           f"{got[bad][0]!r} != {exp[bad][0]!r}")


def _assert_pow_close(got, exp, context):
    assert np.array_equal(np.isnan(got), np.isnan(exp)), context
    inf = np.isinf(exp)
    assert np.array_equal(got[inf], exp[inf]), context
    fin = np.isfinite(exp)
    np.testing.assert_allclose(got[fin], exp[fin], rtol=1e-12, atol=0,
                               err_msg=context)


def _case_id(case):
    return "-".join(str(c) for c in case)


def _as_tuple(x):
    return x if isinstance(x, tuple) else (x,)


# ---- every op on both class batches ----------------------------------------

@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("case", mc.COLAGG_CASES, ids=_case_id)
def test_colagg_on_class(engine, case, kind):
    op, phi = case
    v, rows, offsets = mc.colagg_batch(kind)
    got = _as_tuple(engine.colagg(op, v, rows, offsets, phi=phi))
    ref = _as_tuple(mc.oracle_colagg(op, phi, kind))
    plain = _as_tuple(mc.plain_colagg(op, phi, kind))
    context = f"{op} phi={phi} {kind}"
    for g, r, p in zip(got, ref, plain):
        if op in mc.PER_SERIES_OPS:
            # rows of no group: undefined today, see colagg_member_mask
            m = mc.colagg_member_mask(kind)
            g, r, p = g[m], r[m], p[m]
        if op == "geomean":
            _assert_pow_close(g, r, context)
            _assert_pow_close(g, p, context)
        else:
            _assert_bits(g, r, context)
            _assert_same(g, p, context)
    if op in mc.SUM_OPS:
        bad = mr.colagg_fsum_check(op, v, rows, offsets, got[0])
        assert not bad, f"{context}: beyond the summation bound: {bad[:3]}"


def test_mad_of_an_infinite_median(engine):
    v = np.asarray([[math.inf], [1.0], [math.inf], [2.0]])
    rows, offsets = np.arange(4, dtype=np.uint32), np.asarray([0, 4], np.uint64)
    assert engine.colagg("median", v, rows, offsets)[0, 0] == math.inf
    assert engine.colagg("mad", v, rows, offsets)[0, 0] == math.inf


# ---- the outlier filters ----------------------------------------------------

# A series is flagged when any of its points lies outside, which on 40 points
# of these batches is nearly every series.  The filters run on three columns,
# the all-NaN one of "ties" among them, so that both answers are common.
FILTER_COLUMNS = [mc.COLAGG_NAN_COLUMN - 1, mc.COLAGG_NAN_COLUMN,
                  mc.COLAGG_NAN_COLUMN + 1]


def _cols(a):
    return np.ascontiguousarray(a[:, FILTER_COLUMNS])


def _on_bound_rows(values, group_of, on, n_rows=2):
    """Put samples exactly on a bound: the first n_rows member rows of
    groups 7 and up (63 members or more, finite bounds nearly everywhere)
    take `on[group]` at every point; the second of them then steps one ulp
    out at its last finite point."""
    v = values.copy()
    picked = [s for s in range(len(group_of)) if group_of[s] >= 7][:n_rows]
    for s in picked:
        v[s] = on[group_of[s]]
    s = picked[-1]
    g = np.flatnonzero(np.isfinite(v[s]))[-1]
    v[s, g] = np.nextafter(v[s, g], math.inf)
    return v, picked


@pytest.mark.parametrize("kind", mc.KINDS)
def test_filter_iqr_on_class(engine, kind):
    """Bounds of the class batch: NaN (the all-NaN column, the empty group)
    and infinite ones included; group_of holds -1 for the rows of no group;
    a sample on the upper bound is no outlier, one ulp above it is."""
    values = _cols(mc.colagg_batch(kind)[0])
    lower, upper = map(_cols, mc.oracle_colagg("iqr_bounds", 0.0, kind))
    group_of = mc.colagg_group_of(kind)
    assert (group_of == -1).sum() == mc.COLAGG_LOOSE_ROWS
    v, picked = _on_bound_rows(values, group_of, upper)
    got = engine.colagg_filter("iqr", v, group_of, lower, upper)
    np.testing.assert_array_equal(
        got, oracle.colagg_filter("iqr", v, group_of, lower, upper))
    np.testing.assert_array_equal(
        got, mr.colagg_filter("iqr", v, group_of, lower, upper))
    assert got[picked[0]] == 0 and got[picked[-1]] == 1
    assert not got[group_of == -1].any()
    assert 0.05 < got.mean() < 0.95


@pytest.mark.parametrize("kind", mc.KINDS)
def test_filter_mad_on_class(engine, kind):
    """outliers_mad with the corrected mad: |v - median| == 3 mad is no
    outlier, one ulp further is."""
    values = _cols(mc.colagg_batch(kind)[0])
    med = _cols(mc.oracle_colagg("median", 0.0, kind))
    tol = _cols(mc.oracle_colagg("mad", 0.0, kind)) * 3.0
    group_of = mc.colagg_group_of(kind)
    with np.errstate(invalid="ignore"):
        on = med + tol
        exact = np.abs(on - med) == tol         # the sum was exact
    on = np.where(exact, on, med)
    assert exact[7:].mean() > 0.5
    v, picked = _on_bound_rows(values, group_of, on)
    got = engine.colagg_filter("mad", v, group_of, med, tol)
    np.testing.assert_array_equal(
        got, oracle.colagg_filter("mad", v, group_of, med, tol))
    np.testing.assert_array_equal(
        got, mr.colagg_filter("mad", v, group_of, med, tol))
    assert got[picked[0]] == 0 and got[picked[-1]] == 1
    assert not got[group_of == -1].any()
    assert 0.05 < got.mean() < 0.95


# ---- launch shapes ------------------------------------------------------------

N_TILES = 1025      # 4100 groups of 2 members x 128 points


@pytest.mark.parametrize("case", [("quantile", 0.3), ("share", 0.0)],
                         ids=_case_id)
def test_colagg_second_trip(engine, case):
    """More outputs than colagg_kernel launches threads: the second trip of
    its loop, which reuses the thread's scratch slot."""
    op, phi = case
    v, rows, offsets = mc.tile_colagg(N_TILES)
    n_groups = len(offsets) - 1
    assert n_groups == 4100 and v.shape[1] == 128
    assert n_groups * v.shape[1] > mc.COLAGG_MAX_THREADS
    assert v.nbytes < 40e6
    got = engine.colagg(op, v, rows, offsets, phi=phi)
    small = oracle.colagg(op, *mc.colagg_small(), phi=phi)
    _assert_bits(got, np.tile(small, (N_TILES, 1)), f"{op} tiled")
    _assert_bits(got, oracle.colagg(op, v, rows, offsets, phi=phi), op)


@pytest.mark.parametrize("op", ["median", "mad"])
def test_colagg_scratch_cap(engine, op):
    """One group of 520 members at full launch width asks for more than
    2 GiB of scratch; vmgpu_colagg halves its blocks once, so every thread
    makes at least two trips on a slot of 520 doubles."""
    big = 520
    v, rows, offsets = mc.tile_colagg(N_TILES, big_group=big)
    n_groups = len(offsets) - 1
    assert n_groups * v.shape[1] > mc.COLAGG_MAX_THREADS
    assert mc.COLAGG_MAX_THREADS * big * 8 > mc.COLAGG_SCRATCH_CAP
    assert mc.COLAGG_MAX_THREADS // 2 * big * 8 <= mc.COLAGG_SCRATCH_CAP
    assert v.nbytes < 40e6
    got = engine.colagg(op, v, rows, offsets)
    small = oracle.colagg(op, *mc.colagg_small())
    _assert_bits(got[:-1], np.tile(small, (N_TILES, 1)), f"{op} tiled")
    _assert_bits(got, oracle.colagg(op, v, rows, offsets), op)
    assert np.isfinite(got[-1]).all()


@pytest.mark.parametrize("mode", ["iqr", "mad"])
def test_filter_second_trip(engine, mode):
    n_series = mc.COLAGG_MAX_THREADS + 1
    v, group_of, b1, b2 = mc.filter_small()
    assert n_series == 524_289 and v.shape[1] == 2
    assert n_series > mc.COLAGG_MAX_THREADS
    reps = -(-n_series // len(v))
    tv = np.tile(v, (reps, 1))[:n_series]
    tgo = np.tile(group_of, reps)[:n_series]
    small = mr.colagg_filter(mode, v, group_of, b1, b2)
    assert small.any() and not small.all() and (group_of == -1).any()
    got = engine.colagg_filter(mode, tv, tgo, b1, b2)
    np.testing.assert_array_equal(got, np.tile(small, reps)[:n_series])
    np.testing.assert_array_equal(
        got, oracle.colagg_filter(mode, tv, tgo, b1, b2))
