"""Plain references for the column aggregates, the series transforms and the
histogram walks, in pure Python over one column or row at a time.  Test
infrastructure.

oracle/colagg.c, oracle/transform.c and oracle/hstat.c restate the device
kernels statement by statement (same insertion sort, same helpers), so parity
between the two cannot see an error both share.  This module is written from
the semantics of the reference's aggr.go / transform.go / rollup.go instead:
NaN is dropped with a comprehension, order statistics go through sorted(),
mode and distinct through itertools.groupby, and mad through quantile(), as
the reference's own mad() does.

What may be compared how
------------------------
Python floats are IEEE doubles, Python never contracts a*b+c, division and
math.sqrt are correctly rounded, and both the device library and the oracle
are built with -ffp-contract=off.  A recurrence written here in the same
order therefore gives the same bits, and `same()` asserts exactly that
(NaN equals NaN, -0.0 equals 0.0).  The exceptions:

* geomean ends in pow(), which differs between libms by an ulp: rtol 1e-12,
  the project's bar for pow-based functions.
* sum, avg, sum2 and share are also held to math.fsum, the correctly rounded
  sum.  Recursive summation of n terms x_i in any order is off by at most
  (n - 1) * 2**-53 * sum(|x_i|) (Higham, Accuracy and Stability of Numerical
  Algorithms, eq. 4.4, first order), where n counts the non-NaN members.
  The bound is derived, not measured; `sum_bound()` states it.
"""
import itertools
import math
from collections import Counter

import numpy as np

NAN = math.nan
INF = math.inf
U = 2.0 ** -53


# ---- IEEE arithmetic where Python raises instead ---------------------------

def _div(a, b):
    if b == 0:
        if a != a or b != b or a == 0:
            return NAN
        neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -INF if neg else INF
    return a / b


def _sqrt(x):
    return NAN if (x != x or x < 0) else math.sqrt(x)


def _pow(x, y):
    with np.errstate(all="ignore"):
        return float(np.power(np.float64(x), np.float64(y)))


def _isnan(x):
    return x != x


def _seq_sum(terms):
    """Left-to-right recursive summation (newer builtin sum()s compensate)."""
    total = 0.0
    for x in terms:
        total += x
    return total


def same(a, b):
    """Bit equality with NaN == NaN and -0.0 == 0.0."""
    return (a != a and b != b) or a == b


def same_arrays(got, exp):
    """Elementwise same() over numpy arrays; returns the mismatch mask."""
    got = np.asarray(got, np.float64)
    exp = np.asarray(exp, np.float64)
    return ~((np.isnan(got) & np.isnan(exp)) | (got == exp))


def sum_bound(terms):
    """(n - 1) * 2**-53 * sum(|x_i|) over the finite, non-NaN terms."""
    return (len(terms) - 1) * U * math.fsum(abs(x) for x in terms)


# ---- order statistics ------------------------------------------------------

def quantile_sorted(phi, a):
    """quantileSorted (aggr.go): linear interpolation between the two ranks
    around phi * (n - 1); -Inf below 0, +Inf above 1."""
    n = len(a)
    if n == 0 or _isnan(phi):
        return NAN
    if phi < 0:
        return -INF
    if phi > 1:
        return INF
    rank = phi * (n - 1)
    lo = max(0, math.floor(rank))
    hi = min(n - 1, lo + 1)
    w = rank - math.floor(rank)
    return a[lo] * (1.0 - w) + a[hi] * w


def quantile(phi, values):
    """quantile() (rollup.go): NaN dropped, then sorted."""
    return quantile_sorted(phi, sorted(v for v in values if not _isnan(v)))


def mad(values):
    """mad() (rollup.go): the median of |v - median|, each through
    quantile(), so a NaN deviation (Inf - Inf) is dropped like a NaN sample."""
    med = quantile(0.5, values)
    return quantile(0.5, [abs(v - med) for v in values])


def _runs(values):
    """(value, length) of the runs of equal values, ascending."""
    return [(k, len(list(g))) for k, g in
            itertools.groupby(sorted(v for v in values if not _isnan(v)))]


def mode(values):
    """modeNoNaNs: the most frequent value, the smallest among equals."""
    runs = _runs(values)
    if not runs:
        return NAN
    return max(runs, key=lambda r: r[1])[0]     # max() keeps the first


def distinct(values):
    n = len(_runs(values))
    return float(n) if n else NAN


def welford(values):
    """(avg, count, q) of the reference's streaming variance."""
    avg = count = q = 0.0
    for v in values:
        if _isnan(v):
            continue
        count += 1.0
        avg_new = avg + (v - avg) / count
        q += (v - avg) * (v - avg_new)
        avg = avg_new
    return avg, count, q


def stdvar(values):
    _, count, q = welford(values)
    return NAN if count == 0 else q / count


# ---- column aggregates -----------------------------------------------------

def _reduce(op, col, phi):
    vals = [v for v in col if not _isnan(v)]
    if op == "median":
        return quantile(0.5, col)
    if op == "quantile":
        return quantile(phi, col)
    if op == "mad":
        return mad(col)
    if op == "stdvar":
        return stdvar(col)
    if op == "stddev":
        return _sqrt(stdvar(col))
    if op == "mode":
        return mode(col)
    if op == "distinct":
        return distinct(col)
    if not vals:
        return NAN
    if op == "sum":
        return _seq_sum(vals)
    if op == "sum2":
        return _seq_sum(v * v for v in vals)
    if op == "avg":
        return _seq_sum(vals) / len(vals)
    if op == "min":
        return min(vals)
    if op == "max":
        return max(vals)
    if op == "count":
        return float(len(vals))
    if op == "group":
        return 1.0
    if op == "geomean":
        prod = 1.0
        for v in vals:
            prod *= v
        return _pow(prod, 1.0 / len(vals))
    raise ValueError(op)


def _columns(values, group_rows, group_offsets):
    n_grid = values.shape[1]
    for grp in range(len(group_offsets) - 1):
        rows = [int(r) for r in
                group_rows[int(group_offsets[grp]):int(group_offsets[grp + 1])]]
        for g in range(n_grid):
            yield grp, g, rows, [float(values[r, g]) for r in rows]


def colagg(op, values, group_rows, group_offsets, phi=0.0):
    """Same shapes as oracle.colagg.  Rows of no group stay NaN in the
    per-series outputs; the caller compares member rows only."""
    n_groups = len(group_offsets) - 1
    n_grid = values.shape[1]
    if op in ("share", "zscore"):
        out = np.full(values.shape, NAN)
        for grp, g, rows, col in _columns(values, group_rows, group_offsets):
            if op == "share":
                # aggrFuncShare: NaN and negative members take no part
                total = _seq_sum(v for v in col if v >= 0)
                for r, v in zip(rows, col):
                    out[r, g] = _div(v, total) if v >= 0 else NAN
            else:
                avg, count, q = welford(col)
                if count == 0:
                    continue          # all NaN: passes through as NaN
                sd = _sqrt(q / count)
                for r, v in zip(rows, col):
                    out[r, g] = v if _isnan(v) else _div(v - avg, sd)
        return out
    if op == "iqr_bounds":
        lower = np.empty((n_groups, n_grid))
        upper = np.empty((n_groups, n_grid))
        for grp, g, _, col in _columns(values, group_rows, group_offsets):
            q25, q75 = quantile(0.25, col), quantile(0.75, col)
            iqr = 1.5 * (q75 - q25)
            lower[grp, g] = q25 - iqr
            upper[grp, g] = q75 + iqr
        return lower, upper
    out = np.empty((n_groups, n_grid))
    for grp, g, _, col in _columns(values, group_rows, group_offsets):
        out[grp, g] = _reduce(op, col, phi)
    return out


def colagg_fsum_check(op, values, group_rows, group_offsets, got):
    """Hold sum / avg / sum2 / share to math.fsum within sum_bound().
    Returns a list of violations (empty when fine).  Columns with an
    infinite term are left to the bit comparison."""
    bad = []
    for grp, g, rows, col in _columns(values, group_rows, group_offsets):
        if op == "share":
            terms = [v for v in col if v >= 0]
        elif op == "sum2":
            terms = [v * v for v in col if not _isnan(v)]
        else:
            terms = [v for v in col if not _isnan(v)]
        if not terms or not all(math.isfinite(t) for t in terms):
            continue
        exact = math.fsum(terms)
        bound = sum_bound(terms)
        if op == "share":
            # any sum within the bound, then one rounding of the division
            lo_s, hi_s = exact - bound, exact + bound
            if lo_s <= 0:
                continue
            for r, v in zip(rows, col):
                if not v >= 0:
                    continue
                x = float(got[r, g])
                lo, hi = v / hi_s, v / lo_s
                slack = 2 * U * abs(hi)
                if not lo - slack <= x <= hi + slack:
                    bad.append((grp, g, r, x, lo, hi))
            continue
        x = float(got[grp, g])
        if op == "avg":
            n = len(terms)
            # the sum's bound over n, plus the rounding of the division
            if abs(x - exact / n) > bound / n + 2 * U * abs(exact / n):
                bad.append((grp, g, x, exact / n, bound / n))
        elif abs(x - exact) > bound:
            bad.append((grp, g, x, exact, bound))
    return bad


def colagg_filter(mode_name, values, group_of, b1, b2):
    """outliers_iqr: any point above upper or below lower; outliers_mad:
    any point further than b2 from b1.  A NaN on either side compares
    false, so it never flags."""
    flags = np.zeros(values.shape[0], np.uint8)
    for s, grp in enumerate(group_of):
        if grp < 0:
            continue
        for g in range(values.shape[1]):
            v, x1, x2 = float(values[s, g]), float(b1[grp, g]), float(b2[grp, g])
            if mode_name == "iqr":
                hit = v > x2 or v < x1
            else:
                hit = abs(v - x1) > x2
            if hit:
                flags[s] = 1
                break
    return flags


# ---- series transforms -----------------------------------------------------

def _first(row):
    return next((i for i, v in enumerate(row) if not _isnan(v)), None)


def _last(row):
    return next((i for i in range(len(row) - 1, -1, -1)
                 if not _isnan(row[i])), None)


def _set_last_values(row):
    """setLastValues: the last non-NaN value everywhere."""
    i = _last(row)
    return row if i is None else [row[i]] * len(row)


def _running(func, row):
    lo = _first(row)
    if lo is None:
        return row
    out = list(row)
    prev = row[lo]
    for i in range(lo + 1, len(row)):
        v = row[i]
        if not _isnan(v):
            if func == "sum":
                prev = prev + v
            elif func == "min":
                prev = prev if prev < v else v
            elif func == "max":
                prev = prev if prev > v else v
            else:   # the divisor counts positions, NaN ones included
                prev = prev + (v - prev) / float(i - lo + 1)
        out[i] = prev
    return out


def _mean(row):
    vals = [v for v in row if not _isnan(v)]
    return _div(_seq_sum(vals), float(len(vals)))


def series_transform(func, row, ts=None, arg1=None, scalar=0.0):
    """One row through one transform function; returns (row, keep)."""
    row = [float(v) for v in row]
    n = len(row)
    if func == "keep_last_value":
        out, last = [], row[0]
        for v in row:
            if not _isnan(v):
                last = v
            out.append(last)
        return out, 1
    if func == "keep_next_value":
        out, _ = series_transform("keep_last_value", row[::-1])
        return out[::-1], 1
    if func == "interpolate":
        lo, hi = _first(row), _last(row)
        out = list(row)
        if lo is None:
            return out, 1
        i = lo
        while i <= hi:
            if not _isnan(row[i]):
                i += 1
                continue
            j = i
            while _isnan(row[j]):
                j += 1
            prev, nxt = row[i - 1], row[j]
            delta = (nxt - prev) / float(j - i + 1)
            for k in range(i, j):
                prev += delta
                out[k] = prev
            i = j
        return out, 1
    if func.startswith("running_"):
        return _running(func[8:], row), 1
    if func in ("range_sum", "range_min", "range_max", "range_avg"):
        return _set_last_values(_running(func[6:], row)), 1
    if func == "range_first":
        i = _first(row)
        return (row if i is None else [row[i]] * n), 1
    if func == "range_last":
        return _set_last_values(row), 1
    if func == "range_normalize":
        vals = [v for v in row if not _isnan(v)]
        vmin = min(vals, default=INF)
        vmax = max(vals, default=-INF)
        d = vmax - vmin
        if math.isinf(d):
            return row, 0
        return [_div(v - vmin, d) for v in row], 1
    if func in ("range_zscore", "range_trim_zscore"):
        sd = _sqrt(stdvar(row))
        avg = _mean(row)
        if func == "range_zscore":
            return [_div(v - avg, sd) for v in row], 1
        z = abs(scalar)
        return [NAN if _div(abs(v - avg), sd) > z else v for v in row], 1
    if func == "range_stdvar":
        return [stdvar(row)] * n, 1
    if func == "range_stddev":
        return [_sqrt(stdvar(row))] * n, 1
    if func == "range_linear_regression":
        t0 = int(ts[0])
        ms = [float(int(t) - t0) for t in ts]
        dts = [m / 1e3 for m in ms]
        if all(v == row[0] for v in row[1:]):
            v0, k = row[0], 0.0
        else:
            pts = [(dt, v) for dt, v in zip(dts, row) if not _isnan(v)]
            if not pts:
                v0 = k = NAN
            else:
                cnt = float(len(pts))
                vsum = tsum = tvsum = ttsum = 0.0
                for dt, v in pts:
                    vsum += v
                    tsum += dt
                    tvsum += dt * v
                    ttsum += dt * dt
                k = 0.0
                tdiff = ttsum - tsum * tsum / cnt
                if abs(tdiff) >= 1e-6:
                    k = (tvsum - tsum * vsum / cnt) / tdiff
                v0 = vsum / cnt - k * tsum / cnt
        return [v0 + k * m / 1e3 for m in ms], 1
    if func == "range_mad":
        return [mad(row)] * n, 1
    if func == "range_trim_outliers":
        med = quantile(0.5, row)
        dmax = scalar * mad(row)
        return [NAN if abs(v - med) > dmax else v for v in row], 1
    if func == "range_trim_spikes":
        phi = scalar / 2.0
        vmax = quantile(1.0 - phi, row)
        vmin = quantile(phi, row)
        return [NAN if (v > vmax or v < vmin) else v for v in row], 1
    if func == "range_quantile":
        # the quantile is stored over the last non-NaN sample and then
        # spread by setLastValues: a NaN quantile exposes the sample before
        out = list(row)
        i = _last(row)
        if i is not None:
            out[i] = quantile(scalar, row)
        return _set_last_values(out), 1
    if func == "smooth_exponential":
        out = list(row)
        lo = _first(row)
        while lo is not None and lo < n and math.isinf(row[lo]):
            lo += 1
        if lo is None or lo >= n:
            return out, 1
        avg = row[lo]
        for i in range(lo + 1, n):
            v = row[i]
            if _isnan(v):
                continue
            if math.isinf(v):
                out[i] = avg
                continue
            sf = 1.0 if arg1 is None else float(arg1[i])
            if _isnan(sf):
                sf = 1.0
            sf = min(1.0, max(0.0, sf))
            avg = avg * (1.0 - sf) + v * sf
            out[i] = avg
        return out, 1
    if func == "remove_resets":
        out = list(row)
        lo = _first(row)
        if lo is None:
            return out, 1
        corr, prev = 0.0, row[lo]
        for i in range(lo, n):
            v = row[i]
            if _isnan(v):
                continue
            d = v - prev
            if d < 0:
                # a drop of less than 1/8 is a glitch: add back the drop
                corr += (prev - v) if (-d * 8.0) < prev else prev
            prev = v
            out[i] = v + corr
        return out, 1
    raise ValueError(func)


def transform(func, values, ts=None, arg1=None, scalar=0.0):
    out = np.empty(values.shape)
    keep = np.ones(values.shape[0], np.uint8)
    for s in range(values.shape[0]):
        out[s], keep[s] = series_transform(func, values[s], ts=ts, arg1=arg1,
                                           scalar=scalar)
    return out, keep


def clamp(func, values, lo, hi=None):
    out = np.empty(values.shape)
    for s in range(values.shape[0]):
        for g in range(values.shape[1]):
            v = float(values[s, g])
            if func in ("clamp", "clamp_min") and v < lo[g]:
                v = float(lo[g])
            bound = hi if func == "clamp" else lo
            if func in ("clamp", "clamp_max") and v > bound[g]:
                v = float(bound[g])
            out[s, g] = v
    return out


# ---- histogram walks, one counter per branch -------------------------------

def _groups(les, group_offsets):
    for grp in range(len(group_offsets) - 1):
        lo, hi = int(group_offsets[grp]), int(group_offsets[grp + 1])
        yield grp, lo, [float(le) for le in les[lo:hi]]


def _fixed(col):
    """fixBrokenBuckets: a NaN or decreasing bucket takes the one before;
    a NaN first bucket is 0."""
    out, prev = [], 0.0
    for j, v in enumerate(col):
        if j == 0:
            prev = 0.0 if _isnan(v) else v
        elif not (_isnan(v) or prev > v):
            prev = v
        out.append(prev)
    return out


def histogram_stat(mode_name, bv, les, group_offsets, hits=None):
    """histogram_avg / stddev / stdvar: moments of the bucket midpoints,
    weighted by the raw (unfixed) bucket increments; infinite les skipped."""
    hits = Counter() if hits is None else hits
    n_grid = bv.shape[1]
    out = np.empty((len(group_offsets) - 1, n_grid))
    for grp, lo, gles in _groups(les, group_offsets):
        for g in range(n_grid):
            le_prev = v_prev = total = total2 = wt = 0.0
            for j, le in enumerate(gles):
                if math.isinf(le):
                    hits["stat: infinite le skipped"] += 1
                    continue
                hits["stat: finite le"] += 1
                v = float(bv[lo + j, g])
                mid = (le + le_prev) / 2
                w = v - v_prev
                total += mid * w
                total2 += mid * mid * w
                wt += w
                le_prev, v_prev = le, v
            if wt == 0:
                hits["stat: zero weight"] += 1
                r = NAN
            elif mode_name == "avg":
                hits["stat: avg"] += 1
                r = total / wt
            else:
                avg = total / wt
                sv = total2 / wt - avg * avg
                if sv < 0:
                    hits["stat: negative variance clamped"] += 1
                    sv = 0.0
                else:
                    hits["stat: variance kept"] += 1
                r = _sqrt(sv) if mode_name == "stddev" else sv
            out[grp, g] = r
    return out


def histogram_share(le_req, bv, les, group_offsets, hits=None):
    """histogram_share: the share of samples at or below le_req, with its
    lower and upper bound."""
    hits = Counter() if hits is None else hits
    n_grid = bv.shape[1]
    shape = (len(group_offsets) - 1, n_grid)
    out, out_lo, out_hi = np.empty(shape), np.empty(shape), np.empty(shape)
    for grp, lo, gles in _groups(les, group_offsets):
        for g in range(n_grid):
            req = float(le_req[g])
            if _isnan(req) or not gles:
                hits["share: NaN le_req or no les"] += 1
                res = (NAN, NAN, NAN)
            elif req < 0:
                hits["share: le_req < 0"] += 1
                res = (0.0, 0.0, 0.0)
            elif req == INF:
                hits["share: le_req +Inf"] += 1
                res = (1.0, 1.0, 1.0)
            else:
                col = _fixed([float(bv[lo + j, g]) for j in range(len(gles))])
                v_last = col[-1]
                vp = lep = 0.0
                res = None
                for v, le in zip(col, gles):
                    if req >= le:
                        hits["share: le_req >= le"] += 1
                        vp, lep = v, le
                        continue
                    lb = _div(vp, v_last)
                    if le == INF:
                        hits["share: exit at the +Inf bucket"] += 1
                        res = (lb, lb, 1.0)
                    elif lep == req:
                        hits["share: lePrev == le_req"] += 1
                        res = (lb, lb, lb)
                    else:
                        hits["share: interpolated"] += 1
                        q = lb + _div(_div(v - vp, v_last) * (req - lep),
                                      le - lep)
                        res = (q, lb, _div(v, v_last))
                    break
                if res is None:
                    hits["share: le_req beyond every le"] += 1
                    res = (1.0, 1.0, 1.0)
            out[grp, g], out_lo[grp, g], out_hi[grp, g] = res
    return out, out_lo, out_hi


def histogram_quantile(phi, bv, les, group_offsets, hits=None):
    """histogram_quantile with boundsLabel: (q, lower, upper).

    `v == vPrev` is the reference's plateau exit.  It cannot be taken:
    vPrev is either its initial 0, and v <= 0 has been skipped before, or a
    bucket with vPrev < vReq, and the walk only gets there with v >= vReq.
    The branch is kept, counted, and test_matrix_class_inputs.py asserts
    that the count stays 0."""
    hits = Counter() if hits is None else hits
    n_grid = bv.shape[1]
    shape = (len(group_offsets) - 1, n_grid)
    out, out_lo, out_hi = np.empty(shape), np.empty(shape), np.empty(shape)
    for grp, lo, gles in _groups(les, group_offsets):
        for g in range(n_grid):
            raw = [float(bv[lo + j, g]) for j in range(len(gles))]
            col = _fixed(raw)
            v_last = col[-1] if col else 0.0
            if _isnan(phi):
                hits["hq: NaN phi"] += 1
                res = (NAN, NAN, NAN)
            elif v_last == 0:
                hits["hq: empty histogram"] += 1
                res = (NAN, NAN, NAN)
            elif phi < 0:
                hits["hq: phi < 0"] += 1
                res = (-INF, -INF, 0.0 if _isnan(raw[0]) else raw[0])
            elif phi > 1:
                hits["hq: phi > 1"] += 1
                res = (INF, v_last, INF)
            else:
                v_req = v_last * phi
                vp = lep = 0.0
                res = None
                for v, le in zip(col, gles):
                    if v <= 0:
                        hits["hq: v <= 0 skipped"] += 1
                        lep = le
                        continue
                    if v < v_req:
                        hits["hq: v < vReq"] += 1
                        vp, lep = v, le
                        continue
                    if math.isinf(le):
                        hits["hq: exit at the +Inf bucket"] += 1
                        break
                    if v == vp:
                        hits["hq: plateau v == vPrev"] += 1
                        res = (lep, lep, v)
                        break
                    hits["hq: interpolated"] += 1
                    res = (lep + _div((le - lep) * (v_req - vp), v - vp),
                           lep, le)
                    break
                if res is None:
                    finite = [le for le in gles if not math.isinf(le)]
                    if finite:
                        hits["hq: tail, last finite le"] += 1
                        res = (finite[-1], finite[-1], INF)
                    else:
                        hits["hq: tail, no finite le"] += 1
                        res = (NAN, NAN, INF)
            out[grp, g], out_lo[grp, g], out_hi[grp, g] = res
    return out, out_lo, out_hi
