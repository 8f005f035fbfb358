"""Multi-series rollup functions (rollup.go:1490-1560).

`count_values_over_time` and `histogram_over_time` emit a DATA-DEPENDENT
number of output series per input series — one per observed formatted value
/ non-zero vmrange bucket — via the timeseriesMap side channel
(newTimeseriesMap, rollup.go:629; DoTimeseriesMap, rollup.go:700).  They do
not fit the one-value-per-(series, grid point) kernel contract.

Both have a device path over a resident SeriesBatch, on the same sparse
contract (mark pass, row scan, count pass):
`histogram_over_time_batch` -> SeriesBatch.histogram_over_time ->
csrc/hot.hip keys rows on the 488 vmrange codes;
`count_values_over_time_batch` -> SeriesBatch.count_values_over_time ->
csrc/cvot.hip keys rows on the value's bits.  The reference's key,
strconv.FormatFloat(v,'g',-1,64), is the shortest round-trip form: a pure
function of the bits, injective on non-NaN doubles (-0 and 0 differ) and
"NaN" for every NaN.  So the device finds a series' distinct values with a
sort over canonicalised bits and the host formats one label per output row,
not one per sample.  The per-column host functions below stay as the
references and as the path for callers that have no batch.  The per-point
windows are the doInternal windows (seekFirstTimestampIdxAfter semantics)
for an explicit lookbehind window.

Neither function is in rollupFuncsCanAdjustWindow, so the window is the
range selector's literal duration (required: both take m[d]).  Neither is
in rollupFuncsKeepMetricName, so the output metric group resets unless the
query carries keep_metric_names.  Stale NaNs are dropped (neither is in the
keep set, eval.go:2108).
"""
import math

import numpy as np

from .aggregate import (_H_LOWER, _H_UPPER, _histogram_ranges,
                        _histogram_update)
from .binary_op import Series
from .decimal import STALE_NAN_BITS


def format_go_float_g(v):
    """strconv.FormatFloat(v, 'g', -1, 64): shortest digits; scientific
    form when the decimal exponent is < -4 or >= 6 (strconv/ftoa.go:
    `if shortest { eprec = 6 }`), with a 2+-digit exponent."""
    if v != v:
        return "NaN"
    if math.isinf(v):
        return "+Inf" if v > 0 else "-Inf"
    if v == 0:
        return "-0" if math.copysign(1.0, v) < 0 else "0"
    sci = np.format_float_scientific(v, unique=True, trim="-")
    mant, _, es = sci.partition("e")
    exp = int(es)
    neg = mant.startswith("-")
    digits = mant.lstrip("-").replace(".", "").rstrip("0") or "0"
    if exp < -4 or exp >= 6:
        m = digits[0] + ("." + digits[1:] if len(digits) > 1 else "")
        return f"{'-' if neg else ''}{m}e{'+' if exp >= 0 else '-'}{abs(exp):02d}"
    # positional form
    return np.format_float_positional(v, unique=True, trim="-")


def _drop_stale(ts_col, vals_col):
    bits = np.asarray(vals_col, dtype=np.float64).view(np.uint64)
    keep = bits != STALE_NAN_BITS
    if keep.all():
        return ts_col, vals_col
    return ts_col[keep], vals_col[keep]


def _windows(ts_col, start, end, step, window):
    """Per-grid-point [i, j) half-open sample ranges: i/j = first index with
    ts > (t_end - window) / t_end (seekFirstTimestampIdxAfter,
    rollup.go:825)."""
    if window <= 0:
        raise ValueError("multi-series rollups need an explicit window "
                         "(m[d] range selector)")
    n_grid = 1 + (int(end) - int(start)) // int(step)
    t_end = np.asarray(start, dtype=np.int64) + \
        np.arange(n_grid, dtype=np.int64) * int(step)
    j = np.searchsorted(ts_col, t_end, side="right")
    i = np.searchsorted(ts_col, t_end - int(window), side="right")
    return i, j, n_grid


def _base_mn(mn, keep_metric_names):
    out = mn.copy()
    if not keep_metric_names:
        out.reset_metric_group()
    return out


def count_values_over_time(label_name, ts_col, vals_col, mn, start, end,
                           step, window, keep_metric_names=False,
                           drop_stale=True):
    """newRollupCountValues (rollup.go:1490): per grid point, count each
    distinct window value, one output series per distinct
    strconv 'g'-formatted value under label_name.  Returns
    (list[Series], samples_scanned)."""
    ts_col = np.ascontiguousarray(ts_col, dtype=np.int64)
    vals_col = np.ascontiguousarray(vals_col, dtype=np.float64)
    if drop_stale:
        ts_col, vals_col = _drop_stale(ts_col, vals_col)
    i, j, n_grid = _windows(ts_col, start, end, step, window)
    base = _base_mn(mn, keep_metric_names)
    out = {}
    order = []
    scanned = 0
    for g in range(n_grid):
        lo, hi = int(i[g]), int(j[g])
        scanned += hi - lo
        for v in vals_col[lo:hi]:
            key = format_go_float_g(float(v))
            s = out.get(key)
            if s is None:
                m2 = base.copy()
                m2.remove_tag(label_name)
                m2.add_tag(label_name, key)
                s = Series(m2, np.full(n_grid, math.nan))
                out[key] = s
                order.append(key)
            cur = s.values[g]
            s.values[g] = 1.0 if math.isnan(cur) else cur + 1.0
    return [out[k] for k in order], scanned


def histogram_over_time(ts_col, vals_col, mn, start, end, step, window,
                        keep_metric_names=False, drop_stale=True):
    """rollupHistogram (rollup.go:1525): per grid point, a VictoriaMetrics
    metrics.Histogram over the window values; each non-zero vmrange bucket
    becomes an output series labeled vmrange=<range> with the count at that
    point (NaN elsewhere — the timeseriesMap origin is NaN-filled).
    Returns (list[Series], samples_scanned)."""
    ts_col = np.ascontiguousarray(ts_col, dtype=np.int64)
    vals_col = np.ascontiguousarray(vals_col, dtype=np.float64)
    if drop_stale:
        ts_col, vals_col = _drop_stale(ts_col, vals_col)
    i, j, n_grid = _windows(ts_col, start, end, step, window)
    base = _base_mn(mn, keep_metric_names)
    ranges = _histogram_ranges()
    out = {}
    order = []
    scanned = 0
    for g in range(n_grid):
        lo, hi = int(i[g]), int(j[g])
        scanned += hi - lo
        buckets = {}
        for v in vals_col[lo:hi]:
            _histogram_update(buckets, float(v))
        for key, count in buckets.items():
            if count == 0:
                continue  # VisitNonZeroBuckets
            if key == "lower":
                vmrange = _H_LOWER
            elif key == "upper":
                vmrange = _H_UPPER
            else:
                vmrange = ranges[key]
            s = out.get(vmrange)
            if s is None:
                m2 = base.copy()
                m2.remove_tag("vmrange")
                m2.add_tag("vmrange", vmrange)
                s = Series(m2, np.full(n_grid, math.nan))
                out[vmrange] = s
                order.append(vmrange)
            s.values[g] = float(count)
    return [out[k] for k in order], scanned


# --- device path of histogram_over_time -----------------------------------

VMRANGE_N_THRESHOLDS = 487
VMRANGE_CODE_UPPER = 487


def _vmrange_code(v):
    """Class of v under _histogram_update: None = contributes nothing,
    0 = lower, 1..486 = bucket idx 0..485, 487 = upper."""
    b = {}
    _histogram_update(b, float(v))
    if not b:
        return None
    key = next(iter(b))
    if key == "lower":
        return 0
    if key == "upper":
        return VMRANGE_CODE_UPPER
    return key + 1


_vmrange_thresholds = None


def vmrange_bucket_thresholds():
    """The 487 thresholds of the vmrange step function: entry j is the
    smallest double whose code is >= j + 1, found by bisecting on the bit
    pattern against _histogram_update itself (the formula is not restated
    here), so code(v) = #{j : thr[j] <= v} for every non-negative double.
    This table is what the device classifier uses (csrc/vmrange_bucket.h);
    the host function is monotone in v, which tests/
    test_vmrange_bucket_table.py checks around every threshold."""
    global _vmrange_thresholds
    if _vmrange_thresholds is None:
        one = np.empty(1, dtype=np.uint64)

        def at(bits):
            one[0] = bits
            return _vmrange_code(one.view(np.float64)[0])

        inf_bits = int(np.float64(np.inf).view(np.uint64))
        thr = np.empty(VMRANGE_N_THRESHOLDS, dtype=np.uint64)
        lo_bound = 1  # smallest subnormal: code 0
        for k in range(1, VMRANGE_N_THRESHOLDS + 1):
            # invariant: code(lo) < k <= code(hi)
            lo, hi = lo_bound, inf_bits
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if at(mid) >= k:
                    hi = mid
                else:
                    lo = mid
            thr[k - 1] = hi
            lo_bound = lo
        _vmrange_thresholds = thr.view(np.float64)
        _vmrange_thresholds.setflags(write=False)
    return _vmrange_thresholds


def vmrange_code_lookup(v, thresholds=None):
    """Table-lookup twin of _vmrange_code — the arithmetic the device
    classifier performs."""
    v = float(v)
    if v != v or v < 0:
        return None
    thr = vmrange_bucket_thresholds() if thresholds is None else thresholds
    return int(np.searchsorted(thr, v, side="right"))


def vmrange_label(code):
    if code == 0:
        return _H_LOWER
    if code == VMRANGE_CODE_UPPER:
        return _H_UPPER
    return _histogram_ranges()[code - 1]


def histogram_over_time_batch(batch, metric_names, start, end, step, window,
                              keep_metric_names=False, drop_stale=True):
    """histogram_over_time over every series of a resident SeriesBatch in
    one device call.  metric_names[s] is the MetricName of series s.
    Returns (list[Series], samples_scanned); series come out ordered by
    (series id, ascending vmrange bucket) — the reference's order is Go map
    order and carries no meaning.  Naming is the host function's: the
    metric group resets unless keep_metric_names, any existing vmrange tag
    is replaced."""
    row_series, row_bucket, values, scanned = batch.histogram_over_time(
        start, end, step, window, drop_stale=drop_stale)
    out = []
    bases = {}
    for i in np.argsort(row_series, kind="stable"):
        s = int(row_series[i])
        base = bases.get(s)
        if base is None:
            base = bases[s] = _base_mn(metric_names[s], keep_metric_names)
        m2 = base.copy()
        m2.remove_tag("vmrange")
        m2.add_tag("vmrange", vmrange_label(int(row_bucket[i])))
        out.append(Series(m2, values[i]))
    return out, scanned


# --- device path of count_values_over_time --------------------------------

_NAN_BITS = 0x7FF8000000000000


def count_values_order_key(v):
    """The u64 by which the device orders (and tells apart) the values of
    one series — host twin of cvot_order_key in csrc/value_key.h.  On the
    value's bits u, every NaN first mapped to 0x7FF8000000000000:
    (u >> 63) ? ~u : u | 1 << 63.  Unsigned-ascending is
    -Inf ... -0 < 0 ... +Inf < NaN; equal keys <=> equal 'g' labels."""
    u = int(np.asarray(v, dtype=np.float64).reshape(1).view(np.uint64)[0])
    if (u & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000:
        u = _NAN_BITS
    if u >> 63:
        return ~u & 0xFFFFFFFFFFFFFFFF
    return u | (1 << 63)


def count_values_over_time_batch(label_name, batch, metric_names, start, end,
                                 step, window, keep_metric_names=False,
                                 drop_stale=True, max_rows=None):
    """count_values_over_time over every series of a resident SeriesBatch in
    one device call.  metric_names[s] is the MetricName of series s.
    Returns (list[Series], samples_scanned); series come out ordered by
    (series id, ascending value) — the reference's order is Go map order and
    carries no meaning.  Naming is the host function's: the metric group
    resets unless keep_metric_names, any existing label_name tag is
    replaced, the label value is format_go_float_g of the row's value (one
    call per row).  max_rows bounds the number of output series; None takes
    limits.max_series_per_aggr_func, the flag the reference applies to
    count_values, 0 is unlimited.  Above the bound the device call raises
    VmGpuError before it allocates any output."""
    if max_rows is None:
        from . import limits
        max_rows = limits.max_series_per_aggr_func
    row_series, row_value, values, scanned = batch.count_values_over_time(
        start, end, step, window, drop_stale=drop_stale, max_rows=max_rows)
    out = []
    bases = {}
    for i in np.argsort(row_series, kind="stable"):
        s = int(row_series[i])
        base = bases.get(s)
        if base is None:
            base = bases[s] = _base_mn(metric_names[s], keep_metric_names)
        m2 = base.copy()
        m2.remove_tag(label_name)
        m2.add_tag(label_name, format_go_float_g(float(row_value[i])))
        out.append(Series(m2, values[i]))
    return out, scanned
