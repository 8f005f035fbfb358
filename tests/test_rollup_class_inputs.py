"""The class batches of rollup_classes.py are not trivial inputs.

Runs the oracle alone.  test_gpu_rollup_classes.py compares the device with
these same references; a function that is constant, or NaN nearly
everywhere, on a batch would make that comparison pass whatever the device
computes (a `==` written as `<=` passes where no two samples are equal).  So
every function has to show at least 8 distinct finite values and at most 50 %
NaN on every class batch, with the exceptions spelled out below.
"""
import numpy as np
import pytest

import oracle
from rollup_classes import (ALL_FUNCS, ARGS, CLASSES, END, KINDSETS, LBD,
                            N_GRID, REF_LEN, START, STEP, WINDOW_SAMPLES,
                            class_batch, class_reference, class_window,
                            series_labels)

# NaN is their answer by construction: one of the two is NaN at every point
PRESENCE_FUNCS = {"present_over_time", "absent_over_time"}
# NaN unless the last sample is an outlier
IQR_FUNCS = {"outlier_iqr_over_time", "iqr_over_time"}
EQ_FUNCS = {"count_eq_over_time", "share_eq_over_time", "sum_eq_over_time"}

CASES = [(c, w) for c in CLASSES for w in WINDOW_SAMPLES]


@pytest.mark.parametrize("cls,wid", CASES)
def test_batch_shape(cls, wid):
    ts, vals, offsets = class_batch(cls, wid, "ties")
    window = class_window(cls, wid)
    labels = series_labels(cls, "ties")
    assert len(offsets) - 1 == len(labels)
    lens = np.diff(offsets.astype(np.int64))
    assert list(lens) == [n for n, _ in labels]
    stale = oracle.stale_nan()
    stale_bits = np.float64(stale).view(np.int64)
    for s, (n, kind) in enumerate(labels):
        t = ts[int(offsets[s]):int(offsets[s + 1])]
        v = vals[int(offsets[s]):int(offsets[s + 1])]
        assert (np.diff(t) >= 0).all(), (n, kind)
        if n >= 63:
            # spans the grid and its first window: grid points read from
            # the head and from the tail of the column
            assert t[0] < START, (n, kind)
            assert t[-1] > END - window - 2 * STEP, (n, kind)
        is_stale = v.view(np.int64) == stale_bits
        # ordinary NaN is not storable
        assert not (np.isnan(v) & ~is_stale).any(), (n, kind)
        if n < 63:
            continue
        if kind == "dup_ts":
            frac = (np.diff(t) == 0).mean()
            assert 0.15 < frac < 0.45, (n, frac)
        elif kind == "gap":
            # longer than the window plus the lookback of the plan shapes
            assert np.diff(t).max() > window + LBD, n
        elif kind == "stale":
            assert is_stale.any(), n
        elif kind in ("alphabet", "counter"):
            assert (np.diff(v) == 0).mean() > 0.3, (n, kind)


def test_inf_batch_holds_both_infinities():
    for cls, wid in CASES:
        _, vals, _ = class_batch(cls, wid, "inf")
        assert np.isposinf(vals).any() and np.isneginf(vals).any(), (cls, wid)
        assert not np.isnan(vals).any(), (cls, wid)
        # some windows have an infinite median next to finite samples: the
        # deviations |v - median| of the infinite samples are NaN there and
        # mad_over_time is the median of the rest, +Inf
        med, _ = class_reference("median_over_time", cls, wid, "inf")
        mad, _ = class_reference("mad_over_time", cls, wid, "inf")
        assert (np.isposinf(med) & np.isposinf(mad)).any(), (cls, wid)


def test_window_sizes():
    """The class windows hold about 12 and 64 samples of the reference
    length, and one of each class's windows is off the step multiple."""
    for cls, wid in CASES:
        window = class_window(cls, wid)
        cadence = ((N_GRID - 1) * STEP + window) // (REF_LEN[cls] - 1)
        per_window = window / cadence
        want = WINDOW_SAMPLES[wid]
        assert 0.8 * want <= per_window <= 1.25 * want, (cls, wid, per_window)
    for cls in CLASSES:
        assert any(class_window(cls, w) % STEP for w in WINDOW_SAMPLES), cls


@pytest.mark.parametrize("cls,wid", CASES)
@pytest.mark.parametrize("func", ALL_FUNCS)
def test_reference_not_trivial(func, cls, wid):
    ref, scanned = class_reference(func, cls, wid, "ties")
    assert scanned > 0
    finite = ref[np.isfinite(ref)]
    nan_frac = np.isnan(ref).mean()
    context = f"{func} {cls} {wid}"
    if func in PRESENCE_FUNCS:
        assert (ref == 1.0).any() and np.isnan(ref).any(), context
        assert set(np.unique(finite)) == {1.0}, context
        return
    # stale_samples_over_time counts markers that one sample in twenty
    # carries: a window of 12 samples shows the counts 0..3 and seldom more,
    # so its bar is 4 distinct counts, one of them nonzero
    want = 4 if func == "stale_samples_over_time" else 8
    assert len(np.unique(finite)) >= want, \
        f"{context}: {len(np.unique(finite))} distinct finite values"
    if func not in IQR_FUNCS:
        assert nan_frac <= 0.5, f"{context}: {nan_frac:.0%} NaN"
    if func == "stale_samples_over_time":
        assert (finite != 0).any(), context
    if func in EQ_FUNCS:
        nonzero = (finite != 0).sum() / ref.size
        assert nonzero >= 0.10, f"{context}: nonzero at {nonzero:.1%}"


def test_args_cover_every_parameterised_function():
    assert len(ARGS) == 16
    assert set(ARGS) <= set(ALL_FUNCS)
    assert len(ALL_FUNCS) == len(set(ALL_FUNCS)) == 71
    assert set(KINDSETS) == {"ties", "inf"}
