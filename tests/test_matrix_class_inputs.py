"""The class batches of matrix_classes.py on the references alone.

Three things are shown here, without a GPU:

* The C oracle agrees with the plain reference of matrix_reference.py on
  every batch.  The oracle restates the kernels line for line, so this is
  where an error the two share comes out: mad over a column with an infinite
  median was NaN in both (the NaN deviations stayed in the second sort) where
  the reference's quantile() drops them.  On [+Inf, 1, +Inf, 2] the median is
  +Inf, the deviations are [NaN, Inf, NaN, Inf] and mad is +Inf.
* The inputs are not trivial: a function that is constant or NaN nearly
  everywhere would pass the device comparison whatever the device computes.
  On "ties" every case shows at least 8 distinct finite values and at most
  50 % NaN; on "inf" every case shows finite and non-finite values.  The
  exceptions are listed with their reasons.
* The histogram batch takes every branch of the three walks at least 8
  times, bar one branch that cannot be taken at all.
"""
import math

import numpy as np
import pytest

import oracle
import matrix_classes as mc
import matrix_reference as mr

NAN = mc.NAN

MIN_DISTINCT = 8
MAX_NAN = 0.5
MIN_BRANCH_HITS = 8


def _case_id(case):
    return "-".join(str(c) for c in case)


def _assert_same(got, exp, context):
    bad = mr.same_arrays(got, exp)
    assert not bad.any(), (f"{context}: {int(bad.sum())} differ, first at "
                           f"{np.argwhere(bad)[0]}: {got[bad][0]!r} != "
                           f"{exp[bad][0]!r}")


def _assert_pow_close(got, exp, context):
    assert np.array_equal(np.isnan(got), np.isnan(exp)), context
    ok = ~np.isnan(exp)
    inf = ok & np.isinf(exp)
    assert np.array_equal(got[inf], exp[inf]), context
    fin = ok & ~inf
    np.testing.assert_allclose(got[fin], exp[fin], rtol=1e-12, atol=0,
                               err_msg=context)


# ---- the batches are what they claim to be ---------------------------------

def test_alphabet():
    a = mc.ALPHABET
    assert len(a) >= 12 and len(np.unique(a)) >= 12
    assert np.signbit(a[a == 0]).any() and (~np.signbit(a[a == 0])).any()
    assert (a < 0).any() and a.max() >= 1e15


@pytest.mark.parametrize("kind", mc.KINDS)
def test_colagg_batch_shape(kind):
    v, rows, offsets = mc.colagg_batch(kind)
    sizes = np.diff(offsets.astype(np.int64))
    assert tuple(sizes) == (0, 1, 2, 3, 4, 5, 8, 63, 64, 65, 257)
    assert v.shape[1] == 40
    assert len(np.unique(rows)) == len(rows) == sizes.sum()
    assert (~mc.colagg_member_mask(kind)).sum() == mc.COLAGG_LOOSE_ROWS
    # members interleave: no group of more than two is a run of rows
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        r = np.sort(rows[int(lo):int(hi)].astype(np.int64))
        if len(r) > 2:
            assert (np.diff(r) != 1).any()
    if kind == "ties":
        assert 0.17 < np.isnan(v).mean() < 0.27
        assert np.isnan(v[:, mc.COLAGG_NAN_COLUMN]).all()
        assert not np.isinf(v).any()
    else:
        assert not np.isnan(v).any()
        assert 0.08 < np.isposinf(v).mean() < 0.12
        assert 0.04 < np.isneginf(v).mean() < 0.08


@pytest.mark.parametrize("kind", mc.KINDS)
def test_transform_batch_shape(kind):
    for n_grid in mc.TRANSFORM_N_GRIDS:
        v = mc.transform_batch(kind, n_grid)
        assert v.shape[1] == n_grid
        assert np.isnan(v).all(axis=1).any()              # an all-NaN row
        assert (np.isfinite(v).sum(axis=1) == 1).any()    # a lone value
        if kind == "inf":
            assert np.isposinf(v[:, 0]).any() and np.isneginf(v[:, 0]).any()
            assert np.isposinf(v[:, -1]).any() and np.isneginf(v[:, -1]).any()
    v = mc.transform_batch(kind, 64)
    fin = ~np.isnan(v)
    assert (fin[:, 0] & ~fin[:, 1:].any(axis=1)).any()    # head only
    assert (fin[:, -1] & ~fin[:, :-1].any(axis=1)).any()  # tail only
    assert (~fin[:, 0] & fin[:, 1:].all(axis=1)).any()    # a NaN first
    assert ((v[:, 1:] == v[:, :-1]).mean(axis=1) > 0.4).any()   # plateaus
    with np.errstate(invalid="ignore"):      # Inf - Inf
        drops = v[:, :-1] - v[:, 1:]
    small = (drops > 0) & (drops * 8 < v[:, :-1])
    big = (drops > 0) & (drops * 8 >= v[:, :-1]) & (v[:, :-1] > 0)
    assert (small.any(axis=1) & big.any(axis=1)).any()    # both reset kinds
    if kind == "inf":
        inner = np.isinf(v[:, 1:-1]) & np.isnan(v[:, :-2]) & np.isnan(v[:, 2:])
        assert inner.any()                                # Inf in a NaN gap
    sf = mc.smoothing_factors(64)
    assert (sf == 0).any() and (sf == 1).any() and (sf < 0).any()
    assert (sf > 1).any() and np.isnan(sf).any()


def test_hist_batch_shape():
    bv, les, offsets = mc.hist_batch()
    groups = [list(les[int(lo):int(hi)])
              for lo, hi in zip(offsets[:-1], offsets[1:])]
    sizes = {len(g) for g in groups}
    assert {0, 1, 2, 3, 12, 33} <= sizes
    assert [math.inf] in groups                                   # only +Inf
    assert any(len(g) == 2 and g[1] == math.inf for g in groups)  # [x, +Inf]
    assert any(len(set(g)) < len(g) for g in groups)              # duplicate
    assert any(g and math.inf not in g for g in groups)           # no +Inf
    body = np.delete(bv, [mc.HIST_ZERO_COLUMN, mc.HIST_NAN_COLUMN], axis=1)
    fin = body[~np.isnan(body)]
    assert (fin == np.round(fin)).all() and (fin >= 0).all()      # counts
    assert 0.03 < np.isnan(body).mean() < 0.08
    assert (bv[:, mc.HIST_ZERO_COLUMN] == 0).all()
    assert np.isnan(bv[:, mc.HIST_NAN_COLUMN]).all()
    plateaus = leading = broken = 0
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        blk = body[int(lo):int(hi)]
        if len(blk) < 2:
            continue
        plateaus += int(((blk[1:] == blk[:-1]) & (blk[1:] > 0)).sum())
        leading += int(((blk[0] == 0) & (blk[-1] > 0)).sum())
        broken += int((blk[1:] < blk[:-1]).sum())
    assert plateaus > 100 and leading > 50
    assert 0.02 < broken / body.size < 0.06
    req = mc.hist_le_req()
    finite_les = les[np.isfinite(les)]
    assert np.isin(req, finite_les).sum() >= 12                   # exact hits
    between = np.isfinite(req) & (req > 0) & ~np.isin(req, finite_les)
    assert between.sum() >= 8
    assert (req == 0).any() and (req == -1).any()
    assert np.isposinf(req).any() and np.isnan(req).any()


# ---- column aggregates: oracle against the plain reference ------------------

def _colagg_outputs(op, phi, kind):
    o, p = mc.oracle_colagg(op, phi, kind), mc.plain_colagg(op, phi, kind)
    if op in mc.PER_SERIES_OPS:
        m = mc.colagg_member_mask(kind)
        return [(o[m], p[m])]
    if op == "iqr_bounds":
        return list(zip(o, p))
    return [(o, p)]


@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("case", mc.COLAGG_CASES, ids=_case_id)
def test_colagg_oracle_matches_plain(case, kind):
    op, phi = case
    for o, p in _colagg_outputs(op, phi, kind):
        if op == "geomean":
            _assert_pow_close(o, p, f"{op} {kind}")
        else:
            _assert_same(o, p, f"{op} phi={phi} {kind}")
    if op in mc.SUM_OPS:
        bad = mr.colagg_fsum_check(op, *mc.colagg_batch(kind),
                                   mc.oracle_colagg(op, phi, kind))
        assert not bad, f"{op} {kind}: beyond the summation bound: {bad[:3]}"


# (op, phi) -> why the 8-distinct / 50 %-NaN bar does not apply on "ties"
COLAGG_TRIVIAL = {
    ("group", 0.0): "group() is 1 wherever the group has a sample",
    ("quantile", -0.5): "phi < 0 is -Inf by definition",
    ("quantile", 1.5): "phi > 1 is +Inf by definition",
    ("quantile", NAN): "phi = NaN is NaN by definition",
}
# ops whose answer is finite whatever the samples are
COLAGG_ALWAYS_FINITE = {"count": "a count", "distinct": "a count",
                        "group": "the constant 1"}


def _non_empty(a):
    """Drop the empty group's row of a per-group output."""
    sizes = np.asarray(mc.COLAGG_GROUP_SIZES)
    return a[sizes > 0] if a.shape[0] == len(sizes) else a


@pytest.mark.parametrize("case", mc.COLAGG_CASES, ids=_case_id)
def test_colagg_not_trivial(case):
    op, phi = case
    for o, _ in _colagg_outputs(op, phi, "ties"):
        o = _non_empty(o)
        finite = o[np.isfinite(o)]
        if case in COLAGG_TRIVIAL:
            if op == "group":
                assert set(np.unique(finite)) == {1.0} and np.isnan(o).any()
            else:
                assert len(finite) == 0
            continue
        assert len(np.unique(finite)) >= MIN_DISTINCT, \
            f"{op}: {len(np.unique(finite))} distinct finite values"
        assert np.isnan(o).mean() <= MAX_NAN, f"{op}: {np.isnan(o).mean():.0%} NaN"


@pytest.mark.parametrize("case", mc.COLAGG_CASES, ids=_case_id)
def test_colagg_inf_mixes_finite_and_not(case):
    op, phi = case
    for o, _ in _colagg_outputs(op, phi, "inf"):
        o = _non_empty(o)
        if op in COLAGG_ALWAYS_FINITE:
            assert np.isfinite(o).all(), op
        elif op == "quantile" and case in COLAGG_TRIVIAL:
            assert not np.isfinite(o).any(), case
        else:
            assert np.isfinite(o).any() and (~np.isfinite(o)).any(), case


def test_inf_batch_has_infinite_medians():
    """Where the median is infinite and a finite sample stands next to it,
    the deviations of the infinite samples are NaN and leave; mad is the
    median of the rest, +Inf."""
    med = mc.plain_colagg("median", 0.0, "inf")
    mad = mc.plain_colagg("mad", 0.0, "inf")
    assert (np.isposinf(med) & np.isposinf(mad)).any()
    assert np.isposinf(med).sum() >= 5 and np.isneginf(med).sum() >= 5
    # (a column whose only deviation left is one Inf answers NaN all the
    # same: quantileSorted weighs it Inf * 1 + Inf * 0)
    assert (np.isinf(med) & np.isnan(mad)).any()


def test_mad_of_the_issue_column():
    v = np.asarray([[math.inf], [1.0], [math.inf], [2.0]])
    rows, offsets = np.arange(4, dtype=np.uint32), np.asarray([0, 4], np.uint64)
    assert oracle.colagg("median", v, rows, offsets)[0, 0] == math.inf
    assert oracle.colagg("mad", v, rows, offsets)[0, 0] == math.inf
    assert mr.mad([float(x) for x in v[:, 0]]) == math.inf
    out, _ = oracle.tf_apply(mc.series_func_id("range_mad"), v.T.copy())
    assert (out == math.inf).all()


@pytest.mark.parametrize("kind", mc.KINDS)
def test_colagg_mad_equals_mad_over_time(kind):
    """Single-column groups: the aggregate and the rollup function are the
    same mad() of the reference and have to agree bit for bit."""
    v, rows, offsets = mc.colagg_batch(kind)
    got = mc.oracle_colagg("mad", 0.0, kind)
    ts = np.arange(v.shape[0], dtype=np.int64)
    for grp in range(len(offsets) - 1):
        members = rows[int(offsets[grp]):int(offsets[grp + 1])]
        for g in range(v.shape[1]):
            col = v[members, g]
            col = col[~np.isnan(col)]     # a rollup window holds no NaN
            exp = (oracle.call_rollup_fn("mad_over_time", col, ts[:len(col)])
                   if len(col) else NAN)
            assert np.float64(got[grp, g]).view(np.int64) == \
                np.float64(exp).view(np.int64) or \
                (math.isnan(got[grp, g]) and math.isnan(exp)), (grp, g)


@pytest.mark.parametrize("kind", mc.KINDS)
def test_range_mad_equals_mad_over_time(kind):
    for n_grid in mc.TRANSFORM_N_GRIDS:
        v = mc.transform_batch(kind, n_grid)
        got, _ = mc.oracle_transform("range_mad", 0.0, kind, n_grid)
        ts = np.arange(n_grid, dtype=np.int64)
        for s in range(v.shape[0]):
            exp = oracle.call_rollup_fn("mad_over_time", v[s], ts)
            for x in got[s]:
                assert (math.isnan(x) and math.isnan(exp)) or \
                    np.float64(x).view(np.int64) == \
                    np.float64(exp).view(np.int64), (n_grid, s)


# ---- series transforms -------------------------------------------------------

@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("case", mc.TRANSFORM_CASES, ids=_case_id)
def test_transform_oracle_matches_plain(case, kind):
    func, scalar = case
    for n_grid in mc.TRANSFORM_N_GRIDS:
        o, okeep = mc.oracle_transform(func, scalar, kind, n_grid)
        p, pkeep = mc.plain_transform(func, scalar, kind, n_grid)
        assert np.array_equal(okeep, pkeep), (func, n_grid)
        _assert_same(o, p, f"{func} {scalar} {kind} n_grid={n_grid}")


@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("func", mc.CLAMP_FUNCS)
def test_clamp_oracle_matches_plain(func, kind):
    for n_grid in mc.TRANSFORM_N_GRIDS:
        _assert_same(mc.oracle_clamp(func, kind, n_grid),
                     mc.plain_clamp(func, kind, n_grid),
                     f"{func} {kind} n_grid={n_grid}")


# (func, scalar) -> why the bar does not apply on "ties"; these cases still
# have to show both a kept sample and a trimmed one
TRANSFORM_TRIVIAL = {
    ("range_trim_zscore", 0.0): "z = 0 trims every sample off the mean",
    ("range_trim_outliers", 0.0): "k = 0 trims every sample off the median",
    ("range_trim_outliers", -1.5): "k < 0 trims all but mad = 0 rows",
    ("range_trim_spikes", 1.0): "phi = 0.5 keeps the median only",
    ("range_trim_spikes", 2.0): "phi = 1 swaps the bounds: constant rows stay",
    ("range_quantile", -0.5): "phi < 0 is -Inf by definition",
    ("range_quantile", 1.5): "phi > 1 is +Inf by definition",
}


@pytest.mark.parametrize("case", mc.TRANSFORM_CASES, ids=_case_id)
def test_transform_not_trivial(case):
    """Measured on the 64-point batch; the narrower ones are edge shapes."""
    func, scalar = case
    o, _ = mc.plain_transform(func, scalar, "ties", 64)
    finite = o[np.isfinite(o)]
    if case in TRANSFORM_TRIVIAL:
        if func == "range_quantile":
            assert len(finite) == 0 and np.isinf(o).any()
        else:
            assert len(finite) and np.isnan(o).mean() > MAX_NAN
        return
    assert len(np.unique(finite)) >= MIN_DISTINCT, \
        f"{case}: {len(np.unique(finite))} distinct finite values"
    assert np.isnan(o).mean() <= MAX_NAN, f"{case}: {np.isnan(o).mean():.0%} NaN"


@pytest.mark.parametrize("case", mc.TRANSFORM_CASES, ids=_case_id)
def test_transform_inf_mixes_finite_and_not(case):
    func, scalar = case
    o, _ = mc.plain_transform(func, scalar, "inf", 64)
    if func == "range_quantile" and case in TRANSFORM_TRIVIAL:
        assert not np.isfinite(o).any()
    else:
        assert np.isfinite(o).any() and (~np.isfinite(o)).any(), case


# ---- histograms ---------------------------------------------------------------

HIST_CASES = ([("stat", m) for m in mc.HSTAT_MODES] + [("share", None)]
              + [("quantile", phi) for phi in mc.HQ_PHIS])
# (name, arg, output index) -> why the bar does not apply
HIST_TRIVIAL = {
    ("quantile", NAN, 0): "phi = NaN is NaN", ("quantile", NAN, 1): "same",
    ("quantile", NAN, 2): "same",
    ("quantile", -1.0, 0): "phi < 0 is -Inf",
    ("quantile", -1.0, 1): "phi < 0: lower is -Inf",
    ("quantile", -1.0, 2): "phi < 0: upper is the first bucket's count, "
                           "a few small integers",
    ("quantile", 2.0, 0): "phi > 1 is +Inf",
    ("quantile", 2.0, 2): "phi > 1: upper is +Inf",
}


@pytest.mark.parametrize("case", HIST_CASES, ids=_case_id)
def test_hist_oracle_matches_plain(case):
    outs, (plain, _) = mc.oracle_hist(*case), mc.plain_hist(*case)
    for i, (o, p) in enumerate(zip(outs, plain)):
        _assert_same(o, p, f"{case} output {i}")


@pytest.mark.parametrize("case", HIST_CASES, ids=_case_id)
def test_hist_not_trivial(case):
    """Over the groups with at least two finite les."""
    two = mc.hist_two_finite_les()
    assert two.sum() >= 8
    plain, _ = mc.plain_hist(*case)
    for i, p in enumerate(plain):
        sel = p[two]
        finite = sel[np.isfinite(sel)]
        if case + (i,) in HIST_TRIVIAL:
            assert len(np.unique(finite)) < MIN_DISTINCT
            continue
        assert len(np.unique(finite)) >= MIN_DISTINCT, (case, i)
        assert np.isnan(sel).mean() <= MAX_NAN, (case, i)


HQ_UNREACHABLE = "hq: plateau v == vPrev"
BRANCHES = {
    "stat": {"stat: infinite le skipped", "stat: finite le",
             "stat: zero weight", "stat: avg",
             "stat: negative variance clamped", "stat: variance kept"},
    "share": {"share: NaN le_req or no les", "share: le_req < 0",
              "share: le_req +Inf", "share: le_req >= le",
              "share: exit at the +Inf bucket", "share: lePrev == le_req",
              "share: interpolated", "share: le_req beyond every le"},
    "quantile": {"hq: NaN phi", "hq: empty histogram", "hq: phi < 0",
                 "hq: phi > 1", "hq: v <= 0 skipped", "hq: v < vReq",
                 "hq: exit at the +Inf bucket", "hq: interpolated",
                 "hq: tail, last finite le", "hq: tail, no finite le"},
}


@pytest.mark.parametrize("name", list(BRANCHES))
def test_hist_branches_taken(name):
    """Every branch of the restated walk, at least 8 times over the batch.
    The plateau exit of histogram_quantile is the exception: it is dead code
    in the reference, the kernel and the oracle alike (see
    matrix_reference.histogram_quantile), so its count has to stay 0."""
    hits = sum((mc.plain_hist(*c)[1] for c in HIST_CASES if c[0] == name),
               start=type(mc.plain_hist(*HIST_CASES[0])[1])())
    assert set(hits) - {HQ_UNREACHABLE} == BRANCHES[name]
    for branch in BRANCHES[name]:
        assert hits[branch] >= MIN_BRANCH_HITS, (branch, hits[branch])
    assert hits[HQ_UNREACHABLE] == 0
