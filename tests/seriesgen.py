"""Irregular series batches for parity tests (test infrastructure)."""
import numpy as np

import oracle


def ragged_batch(n_series, max_samples, start, step=15_000, seed=1234,
                 stale_p=0.0, dup_p=0.0, include_empty=True):
    """Varying lengths (including empty series), optional Prometheus stale
    NaNs and duplicate timestamps — the edge cases the reference tests."""
    rng = np.random.default_rng(seed)
    ts_parts, val_parts = [], []
    offsets = [0]
    for s in range(n_series):
        if include_empty and s % 17 == 0:
            offsets.append(offsets[-1])
            continue
        n = int(rng.integers(1, max_samples + 1))
        t = start + np.cumsum(rng.integers(1, 2 * step, n)).astype(np.int64)
        if dup_p > 0:
            dup = rng.random(n) < dup_p
            t[dup] = np.roll(t, 1)[dup]
            t = np.sort(t)
        if rng.random() < 0.5:
            # counter-like with resets
            v = np.cumsum(np.abs(rng.standard_normal(n)))
            r = rng.random(n) < 0.05
            base = np.maximum.accumulate(np.where(r, v, -np.inf))
            v = v - np.where(np.isfinite(base), base, 0.0)
        else:
            v = np.abs(np.cumsum(rng.standard_normal(n))) * 10
        if stale_p > 0:
            sm = rng.random(n) < stale_p
            v = np.where(sm, oracle.stale_nan(), v)
        ts_parts.append(t)
        val_parts.append(v)
        offsets.append(offsets[-1] + n)
    ts = np.concatenate(ts_parts) if ts_parts else np.empty(0, np.int64)
    vals = np.concatenate(val_parts) if val_parts else np.empty(0, np.float64)
    return (ts.astype(np.int64), vals.astype(np.float64),
            np.asarray(offsets, dtype=np.uint64))


TIE_KINDS = ("alphabet", "counter", "gauge", "dup_ts", "gap", "stale")
INF_KIND = "inf"


def _alphabet_runs(rng, n):
    """Integers 0..5 held over runs of repeats (mean run length 2.5)."""
    v = rng.integers(0, 6, n).astype(np.float64)
    hold = rng.random(n) < 0.6
    hold[0] = False
    src = np.maximum.accumulate(np.where(hold, 0, np.arange(n)))
    return v[src]


def _plateau_counter(rng, n):
    """Integer counter whose increments are zero half the time (plateaus),
    dropping to zero at one third and two thirds of its length."""
    inc = rng.poisson(1.5, n) * (rng.random(n) < 0.5)
    v = np.cumsum(inc).astype(np.float64)
    if n >= 6:
        v[n // 3:] -= v[n // 3]
        v[2 * n // 3:] -= v[2 * n // 3]
    return v


def _gauge(rng, n):
    """Continuous positive walk; about one sample in twelve repeats its
    predecessor to within 3e-13 relative, alternately above and below, which
    is inside the 1e-12 near-equality skip of changes / increases /
    decreases."""
    v = np.abs(np.cumsum(rng.standard_normal(n))) * 10 + 1.0
    near = np.flatnonzero(rng.random(n) < 0.08)
    for m, k in enumerate(near[near > 0]):
        v[k] = v[k - 1] * (1 + (3e-13 if m % 2 == 0 else -3e-13))
    return v


def tie_batch(lengths, start, n_grid, window, step=15_000, kinds=TIE_KINDS,
              gap=None, seed=4242):
    """One series per (length, kind), lengths outermost: the inputs on which
    the rollup functions stop being trivial.

      alphabet  integers 0..5 in runs of repeats: equal samples in every
                window (count_eq, distinct, mode, tmin/tmax ties, constant
                windows for deriv)
      counter   integer counter with zero increments (plateaus) and two resets
      gauge     continuous positive walk with a few near-equal neighbours
      dup_ts    alphabet values; about 30 % of the samples carry their
                predecessor's timestamp
      gap       plateau counter with one hole of `gap` ms at mid-series
                (default window + 7 * step, longer than the window plus any
                lookback the suites use)
      stale     alphabet runs with about 5 % Prometheus stale NaNs
      inf       alphabet values with about 2 % +Inf and 2 % -Inf (Inf is
                storable, ordinary NaN is not), plus one run of +Inf over a
                sixth of the series and one of -Inf over a twelfth, so some
                windows have an infinite median

    Every series spans the grid and its first window whatever its length:
    sample k sits at start - window + k * cadence plus an in-order jitter,
    cadence = ((n_grid - 1) * step + window) // (n - 1), so grid points read
    from every part of a long column.  Returns flat ts, vals, offsets."""
    rng = np.random.default_rng(seed)
    if gap is None:
        gap = window + 7 * step
    span = (n_grid - 1) * step + window
    ts_parts, val_parts = [], []
    offsets = [0]
    for n in lengths:
        for kind in kinds:
            holed = kind == "gap" and n >= 4
            room = span - gap if holed else span
            assert room >= n - 1, f"{n} samples do not fit {room} ms"
            if n == 1:
                t = np.array([start - window + span // 2], dtype=np.int64)
            else:
                cadence = room // (n - 1)
                t = start - window + np.arange(n, dtype=np.int64) * cadence
                t += rng.integers(0, max(1, cadence // 2), n)
            if holed:
                t[n // 2:] += gap
            if kind == "dup_ts":
                dup = rng.random(n) < 0.3
                dup[0] = False
                t = t[np.maximum.accumulate(np.where(dup, 0, np.arange(n)))]
            if kind in ("alphabet", "stale"):
                v = _alphabet_runs(rng, n)
            elif kind in ("counter", "gap"):
                v = _plateau_counter(rng, n)
            elif kind == "gauge":
                v = _gauge(rng, n)
            elif kind in ("dup_ts", INF_KIND):
                v = rng.integers(0, 6, n).astype(np.float64)
            else:
                raise ValueError(f"unknown series kind {kind!r}")
            if kind == "stale":
                v = np.where(rng.random(n) < 0.05, oracle.stale_nan(), v)
            if kind == INF_KIND:
                u = rng.random(n)
                v = np.where(u < 0.02, np.inf, np.where(u > 0.98, -np.inf, v))
                if n >= 12:
                    # windows whose median is itself infinite
                    v[n // 2:n // 2 + n // 6] = np.inf
                    v[3 * n // 4:3 * n // 4 + n // 12] = -np.inf
            ts_parts.append(t)
            val_parts.append(v)
            offsets.append(offsets[-1] + n)
    return (np.concatenate(ts_parts).astype(np.int64),
            np.concatenate(val_parts).astype(np.float64),
            np.asarray(offsets, dtype=np.uint64))


def assert_parity(got, ref, exact=True, rtol=1e-12, atol=0.0, context=""):
    """NaN==NaN; exact bit equality for arithmetic-only funcs, else rtol
    (+ optional atol floor: cross-series float sums of near-cancelling
    columns — e.g. sum(zscore_over_time) ~ 0 — carry addition-order noise
    at machine epsilon that no relative tolerance can bound; the reference
    itself sums in nondeterministic worker order)."""
    assert got.shape == ref.shape, f"{context}: shape {got.shape} vs {ref.shape}"
    gn, rn = np.isnan(got), np.isnan(ref)
    assert (gn == rn).all(), \
        f"{context}: NaN placement differs at {np.argwhere(gn != rn)[:5]}"
    g, r = got[~gn], ref[~rn]
    if exact:
        bad = g != r
        assert not bad.any(), \
            f"{context}: {bad.sum()} exact mismatches; first diffs " \
            f"{g[bad][:3]} vs {r[bad][:3]}"
    else:
        ok = np.isclose(g, r, rtol=rtol, atol=atol)
        assert ok.all(), \
            f"{context}: {np.sum(~ok)} mismatches beyond rtol={rtol}; " \
            f"first {g[~ok][:3]} vs {r[~ok][:3]}"
