"""The tie-aware topk comparators (topk_check.py) against hand-made results:
they must accept every legal answer and reject every wrong one, or the GPU
suite built on them pins nothing."""
import numpy as np
import pytest

import oracle
from topk_check import assert_topk_pointwise, assert_topk_range

K = 3


def _matrix():
    """8 rows x 3 columns.  Column 0: the boundary value 5.0 of topk(3) is
    carried by rows 2, 4 and 6, of which one is kept beside 9.0 and 7.0.
    Column 1: distinct values with a NaN.  Column 2: -0.0 and +0.0 tied at
    the boundary."""
    X = np.array([
        [9.0, 1.5, 3.0],
        [7.0, 2.5, 0.0],
        [5.0, np.nan, -0.0],
        [1.0, 4.5, -1.0],
        [5.0, 0.5, 0.0],
        [2.0, 8.5, 2.0],
        [5.0, 6.5, -0.0],
        [np.nan, 3.5, -2.0],
    ])
    return X, oracle.topk_pointwise(X, K)


def test_pointwise_oracle_vs_oracle_passes():
    X, R = _matrix()
    assert_topk_pointwise(X, R, R)
    Rb = oracle.topk_pointwise(X, K, reverse=True)
    assert_topk_pointwise(X, Rb, Rb)


def test_pointwise_swapped_boundary_ties_pass():
    X, R = _matrix()
    G = R.copy()
    kept = [i for i in (2, 4, 6) if not np.isnan(R[i, 0])]
    assert len(kept) == 1, "the matrix must have a tie across the boundary"
    other = next(i for i in (2, 4, 6) if i != kept[0])
    G[kept[0], 0], G[other, 0] = np.nan, X[other, 0]
    # column 2: a kept zero handed to a dropped zero of the other sign
    zk = [i for i in (1, 2, 4, 6) if not np.isnan(R[i, 2])]
    zd = [i for i in (1, 2, 4, 6) if np.isnan(R[i, 2])]
    assert zk and zd
    src = zk[0]
    dst = next(i for i in zd if np.signbit(X[i, 2]) != np.signbit(X[src, 2]))
    G[src, 2], G[dst, 2] = np.nan, X[dst, 2]
    assert_topk_pointwise(X, G, R)


def test_pointwise_wrong_row_kept_fails():
    X, R = _matrix()
    G = R.copy()
    assert not np.isnan(R[1, 0]) and np.isnan(R[5, 0])
    G[1, 0], G[5, 0] = np.nan, X[5, 0]  # 7.0 dropped, 2.0 kept: same count
    with pytest.raises(AssertionError, match="kept values differ"):
        assert_topk_pointwise(X, G, R)


def test_pointwise_one_ulp_fails():
    X, R = _matrix()
    G = R.copy()
    G[0, 0] = np.nextafter(G[0, 0], np.inf)
    with pytest.raises(AssertionError, match="not the input's bits"):
        assert_topk_pointwise(X, G, R)
    # a kept zero with its sign flipped: == the input, but not its bits
    G = R.copy()
    i = next(i for i in range(8) if R[i, 2] == 0)
    G[i, 2] = -R[i, 2]
    with pytest.raises(AssertionError, match="not the input's bits"):
        assert_topk_pointwise(X, G, R)


def test_pointwise_count_mismatch_fails():
    X, R = _matrix()
    G = R.copy()
    G[0, 1] = np.nan if not np.isnan(R[0, 1]) else X[0, 1]
    with pytest.raises(AssertionError, match="kept counts differ"):
        assert_topk_pointwise(X, G, R)


def _range_matrix():
    """6 rows x 4 columns; rows 1, 3 and 4 share avg 2.0, which is the
    boundary of topk_avg(3)."""
    return np.array([
        [9.0, 9.0, 9.0, 9.0],
        [2.0, 2.0, np.nan, 2.0],
        [5.0, 5.0, 5.0, 5.0],
        [1.0, 3.0, 1.0, 3.0],
        [2.0, np.nan, 2.0, 2.0],
        [0.0, 0.0, 0.0, 0.0],
    ])


def test_range_oracle_vs_oracle_and_tied_boundary_pass():
    V = _range_matrix()
    for summary in ("avg", "min", "max", "median", "last"):
        for rev in (False, True):
            sel, rem = oracle.topk_range(V, 3, summary, reverse=rev,
                                         remaining=True)
            assert_topk_range(V, summary, sel, rem, sel, rem)
    ref_sel, ref_rem = oracle.topk_range(V, 3, "avg", remaining=True)
    assert list(ref_sel[:2]) == [0, 2] and ref_sel[2] in (1, 3, 4)
    for tied in (1, 3, 4):
        # another tied row at the boundary: its remaining row differs from
        # the oracle's and is not compared
        sel = np.array([0, 2, tied], dtype=np.int64)
        keep = np.ones(6, bool)
        keep[sel] = False
        rem = np.nansum(V[keep], axis=0)
        assert_topk_range(V, "avg", sel, rem, ref_sel, ref_rem)


def test_range_wrong_selection_fails():
    V = _range_matrix()
    ref_sel, ref_rem = oracle.topk_range(V, 2, "avg", remaining=True)
    assert list(ref_sel) == [0, 2]
    with pytest.raises(AssertionError, match="value order differs"):
        assert_topk_range(V, "avg", np.array([2, 0]), ref_rem, ref_sel,
                          ref_rem)
    with pytest.raises(AssertionError, match="value order differs"):
        assert_topk_range(V, "avg", np.array([0, 5]), ref_rem, ref_sel,
                          ref_rem)
    wrong_rem = ref_rem.copy()
    wrong_rem[1] += 1.0
    with pytest.raises(AssertionError, match="remaining"):
        assert_topk_range(V, "avg", ref_sel, wrong_rem, ref_sel, ref_rem)
