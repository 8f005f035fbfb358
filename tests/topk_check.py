"""Tie-aware comparators for the topk family.

The reference sorts with an unstable sort, so where several rows carry the
boundary value it leaves open which of them is kept.  The oracle keeps the
larger row id, the device keeps whoever wins an atomic; both are legal.
These helpers pin everything else.
"""
import numpy as np

import oracle


def assert_topk_pointwise(X, G, R, context=""):
    """X: the input matrix, G: the result under test, R: the oracle's result
    for the same k and direction.  Per column: every kept G is the bit
    pattern of X at that cell, G keeps as many values as R, and the kept
    values are the same multiset under == (so -0.0 and +0.0 may stand in
    for each other, as they do under lessWithNaNs)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    G = np.ascontiguousarray(G, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    assert G.shape == X.shape == R.shape, \
        f"{context}: shapes {G.shape} / {X.shape} / {R.shape}"
    kept_g, kept_r = ~np.isnan(G), ~np.isnan(R)
    bits_differ = kept_g & (G.view(np.int64) != X.view(np.int64))
    assert not bits_differ.any(), \
        f"{context}: kept values are not the input's bits at " \
        f"{np.argwhere(bits_differ)[:5].tolist()}"
    ng, nr = kept_g.sum(axis=0), kept_r.sum(axis=0)
    bad = np.flatnonzero(ng != nr)
    assert bad.size == 0, \
        f"{context}: kept counts differ at columns {bad[:5].tolist()}: " \
        f"{ng[bad][:5].tolist()} vs {nr[bad][:5].tolist()}"
    # np.sort puts NaN last, so with equal counts the kept values line up
    sg, sr = np.sort(G, axis=0), np.sort(R, axis=0)
    differ = ~np.isnan(sr) & ~(sg == sr)
    assert not differ.any(), \
        f"{context}: kept values differ at (rank, column) " \
        f"{np.argwhere(differ)[:5].tolist()}: {sg[differ][:3]} vs " \
        f"{sr[differ][:3]}"


def range_boundary_is_unambiguous(values, summary, sel):
    """True when the selection holds every row whose summary equals the
    last selected one, i.e. no tie straddles the boundary."""
    sv = [oracle.topk_summary(summary, values[i]) for i in sel]
    if not sv:
        return True
    boundary = sv[-1]
    all_vals = [oracle.topk_summary(summary, values[i])
                for i in range(values.shape[0])]
    return sv.count(boundary) == sum(1 for v in all_vals if v == boundary)


def assert_topk_range(values, summary, sel, rem, ref_sel, ref_rem,
                      context=""):
    """values: the matrix both selections were made from; (sel, rem): the
    result under test; (ref_sel, ref_rem): the oracle's.  For selections
    without NaN summaries."""
    # the selected summary-value sequences must be identical;
    # WHICH rows carry a boundary-tied value is unspecified in
    # the reference too (unstable sort), so compare ids only
    # away from the boundary value.
    sv = [oracle.topk_summary(summary, values[i]) for i in sel]
    rv = [oracle.topk_summary(summary, values[i]) for i in ref_sel]
    assert sv == rv, f"{context}: value order differs"
    boundary = sv[-1] if sv else None
    ids_g = {i for i, v in zip(sel, sv) if v != boundary}
    ids_r = {i for i, v in zip(ref_sel, rv) if v != boundary}
    assert ids_g == ids_r, f"{context}"
    if rem is None and ref_rem is None:
        return
    if range_boundary_is_unambiguous(values, summary, sel):
        # no boundary tie ambiguity: remaining sums comparable
        gn, rn = np.isnan(rem), np.isnan(ref_rem)
        assert (gn == rn).all()
        assert np.allclose(rem[~gn], ref_rem[~rn], rtol=1e-9,
                           atol=0), f"{context} remaining"
