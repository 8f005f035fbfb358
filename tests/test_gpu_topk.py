"""The topk family (csrc/topk.hip) against the CPU oracle where selection
kernels go wrong: ties at the boundary, all-NaN columns, more values in one
1/16-binade than any fixed candidate list holds, grids narrower than a wave,
NaN summaries that get selected, and group-relayouted batches.

Every matrix reaches the device as one sample per grid timestamp under
last_over_time with window=STEP, so the resident output IS the matrix; a NaN
cell is a sample left out of the CSR.  Each test checks that first.  Where
values tie, which of the tied rows survives is open in the reference too
(unstable sort), so the comparison goes through topk_check.py.
"""
import math

import numpy as np
import pytest

import oracle
from seriesgen import assert_parity
from topk_check import assert_topk_pointwise, assert_topk_range

pytestmark = pytest.mark.gpu

START = 1_000_000_000_000
STEP = 15_000
SUMMARIES = ("avg", "min", "max", "median", "last")


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


class _Resident:
    """A matrix made resident as a batch's evaluated output."""

    def __init__(self, engine, M, group_ids=None, n_groups=0):
        M = np.ascontiguousarray(M, dtype=np.float64)
        n_grid = M.shape[1]
        present = ~np.isnan(M)
        grid = START + np.arange(n_grid, dtype=np.int64) * STEP
        ts = np.broadcast_to(grid, M.shape)[present]
        vals = M[present]
        offsets = np.concatenate(
            [[0], np.cumsum(present.sum(axis=1))]).astype(np.uint64)
        self.plan = engine.RollupPlan("last_over_time", START,
                                      START + (n_grid - 1) * STEP, STEP,
                                      window=STEP)
        self.batch = engine.SeriesBatch(ts, vals, offsets, group_ids,
                                        n_groups)
        self.host_out, _, _ = self.batch.exec(self.plan)
        out_nan = np.isnan(self.host_out)
        assert (out_nan == ~present).all(), \
            f"resident NaN cells differ at {np.argwhere(out_nan == present)[:5]}"
        assert np.array_equal(self.host_out.view(np.int64)[present],
                              M.view(np.int64)[present]), \
            "resident output is not the intended matrix"

    def reload(self):
        """topk_pointwise NaN-fills the resident output in place."""
        self.batch.exec(self.plan, download=False)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.batch.close()


def _check_pointwise(engine, res, k, reverse, exact, context):
    res.reload()
    got = engine.topk_pointwise(res.batch, k, reverse=reverse)
    ref = oracle.topk_pointwise(res.host_out, k, reverse=reverse)
    assert_topk_pointwise(res.host_out, got, ref, context=context)
    if exact:
        assert_parity(got, ref, exact=True, context=context)


# ---- pointwise ----

@pytest.fixture(scope="module")
def dense_bin():
    """8200 x 3 distinct values in [100, 101): every key of a column shares
    its top 16 bits, and there are 8 more of them than 8192."""
    rng = np.random.default_rng(8200)
    M = rng.uniform(100.0, 101.0, size=(8200, 3))
    for g in range(M.shape[1]):
        assert np.unique(M[:, g]).size == M.shape[0]
    top16 = M.view(np.uint64) >> np.uint64(48)
    assert (top16 == top16[0, 0]).all()
    return M


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("k", [1, 10, 8199])
def test_pointwise_dense_bin(engine, dense_bin, k, reverse):
    with _Resident(engine, dense_bin) as res:
        _check_pointwise(engine, res, k, reverse, exact=True,
                         context=f"dense bin k={k} rev={reverse}")


@pytest.mark.parametrize("reverse", [False, True])
def test_pointwise_zeros_and_nan_columns(engine, reverse):
    rng = np.random.default_rng(41)
    n = 8200
    M = np.full((n, 4), np.nan)
    M[:, 0] = 0.0
    M[rng.choice(n, 5, replace=False), 0] = [0.25, 3.0, 1e-300, 7.5, 1e9]
    # column 1 stays all NaN; column 2 has three values, fewer than k
    M[[17, 4099, 8199], 2] = [2.5, -1.0, 0.0]
    M[:, 3] = rng.choice([-0.0, 0.0, np.inf, -np.inf], size=n,
                         p=[0.45, 0.45, 0.05, 0.05])
    M[rng.choice(n, 6, replace=False), 3] = [1.5, -1.5, 5e-324, -5e-324,
                                             1e308, -1e308]
    with _Resident(engine, M) as res:
        _check_pointwise(engine, res, 10, reverse, exact=False,
                         context=f"zeros/NaN columns rev={reverse}")


@pytest.fixture(scope="module")
def tied_matrix():
    rng = np.random.default_rng(65)
    M = rng.integers(0, 8, size=(300, 65)).astype(np.float64)
    M[rng.random(M.shape) < 0.2] = np.nan
    return M


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("k", [1, 7, 64, 299])
def test_pointwise_ties(engine, tied_matrix, k, reverse):
    with _Resident(engine, tied_matrix) as res:
        _check_pointwise(engine, res, k, reverse, exact=False,
                         context=f"ties k={k} rev={reverse}")


@pytest.mark.parametrize("reverse", [False, True])
def test_pointwise_k_edges(engine, reverse):
    """Non-integer and out-of-range k follow getIntK."""
    rng = np.random.default_rng(50)
    M = rng.standard_normal((50, 5)) * 10
    M[rng.random(M.shape) < 0.1] = np.nan
    with _Resident(engine, M) as res:
        for k in (0, 0.5, -1, math.nan, 49, 50, 51, math.inf):
            _check_pointwise(engine, res, k, reverse, exact=True,
                             context=f"k={k} rev={reverse}")


# ---- range ----

@pytest.mark.parametrize("n_grid", [1, 63, 64, 65, 129])
def test_range_narrow_and_edge_grids(engine, n_grid):
    """Values are multiples of 1/8 in [-64, 64]: sums of up to 200 x 129 of
    them are exact in any order, so neither the device's tree-sum avg nor
    its atomic remaining sum can differ from the oracle's by rounding."""
    rng = np.random.default_rng(1000 + n_grid)
    n, k = 200, 17
    M = rng.integers(-512, 513, size=(n, n_grid)) / 8.0
    M[rng.random(M.shape) < 0.15] = np.nan
    M[[5, 77, 199], :] = np.nan
    M[40, :] = 3.25
    M[141, :] = -17.5
    with _Resident(engine, M) as res:
        for summary in SUMMARIES:
            for rev in (False, True):
                sel, rem = engine.topk_range(res.batch, k, summary=summary,
                                             reverse=rev, remaining=True)
                ref_sel, ref_rem = oracle.topk_range(
                    res.host_out, k, summary, reverse=rev, remaining=True)
                assert len(sel) == len(set(sel.tolist())) == k
                assert_topk_range(
                    res.host_out, summary, sel, rem, ref_sel, ref_rem,
                    context=f"n_grid={n_grid} {summary} rev={rev}")


def test_range_all_tied(engine):
    """5000 identical rows: every summary ties, the ties quota alone decides
    how many rows are selected, and the remaining sum does not depend on
    which ones were."""
    n, n_grid, k, c, hole = 5000, 6, 100, 3.25, 2
    M = np.full((n, n_grid), c)
    M[:, hole] = np.nan
    exp_rem = np.full(n_grid, (n - k) * c)
    exp_rem[hole] = np.nan
    with _Resident(engine, M) as res:
        for summary in SUMMARIES:
            for rev in (False, True):
                sel, rem = engine.topk_range(res.batch, k, summary=summary,
                                             reverse=rev, remaining=True)
                ctx = f"{summary} rev={rev}"
                assert len(sel) == k, ctx
                assert len(set(sel.tolist())) == k, ctx
                assert sel.min() >= 0 and sel.max() < n, ctx
                assert np.isnan(rem[hole]), ctx
                keep = np.arange(n_grid) != hole
                assert np.array_equal(rem[keep], exp_rem[keep]), \
                    f"{ctx}: remaining {rem}"


def test_range_nan_summaries_selected(engine):
    """k above the number of rows with a summary: the rest of the selection
    is filled with all-NaN rows, after the others."""
    rng = np.random.default_rng(90)
    n, n_grid, k = 100, 5, 20
    live = np.sort(rng.choice(n, 10, replace=False))
    M = np.full((n, n_grid), np.nan)
    # every summary of live row j is 10*j + a constant: all distinct
    for j, r in enumerate(rng.permutation(live)):
        M[r] = 10.0 * j + np.array([2.0, 0.0, 4.0, 1.0, 3.0])
    with _Resident(engine, M) as res:
        for summary in SUMMARIES:
            for rev in (False, True):
                sel, _ = engine.topk_range(res.batch, k, summary=summary,
                                           reverse=rev)
                ref_sel, _ = oracle.topk_range(res.host_out, k, summary,
                                               reverse=rev)
                ctx = f"{summary} rev={rev}"
                assert len(sel) == k and len(set(sel.tolist())) == k, ctx
                assert sel[:10].tolist() == ref_sel[:10].tolist(), ctx
                assert set(ref_sel[:10].tolist()) == set(live.tolist()), ctx
                assert not set(sel[10:].tolist()) & set(live.tolist()), ctx
                assert sel.min() >= 0 and sel.max() < n, ctx


# ---- group-relayouted batch ----

def test_topk_on_relayouted_batch(engine):
    """A batch built with interleaved group ids is physically permuted; the
    selected ids and the pointwise matrix must still speak of the caller's
    series order."""
    rng = np.random.default_rng(64)
    n, n_grid = 64, 20
    M = rng.permutation(n * n_grid).reshape(n, n_grid) / 4.0
    gids = (np.arange(n) % 7).astype(np.int32)
    with _Resident(engine, M, group_ids=gids, n_groups=7) as res:
        assert res.batch._perm is not None
        for summary in SUMMARIES:
            for rev in (False, True):
                sel, rem = engine.topk_range(res.batch, 10, summary=summary,
                                             reverse=rev, remaining=True)
                ref_sel, ref_rem = oracle.topk_range(
                    res.host_out, 10, summary, reverse=rev, remaining=True)
                ctx = f"relayout {summary} rev={rev}"
                assert_topk_range(res.host_out, summary, sel, rem, ref_sel,
                                  ref_rem, context=ctx)
                # no two rows share a summary: the ids are pinned one by one
                assert len({oracle.topk_summary(summary, r) for r in M}) == n
                assert sel.tolist() == ref_sel.tolist(), ctx
        for rev in (False, True):
            _check_pointwise(engine, res, 5, rev, exact=True,
                             context=f"relayout pointwise rev={rev}")
