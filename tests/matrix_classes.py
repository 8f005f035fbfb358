"""Edge-class inputs for the column aggregates (csrc/aggrcol.hip), the series
transforms (csrc/transform.hip) and the histogram walks (csrc/hstat.hip),
shared by test_matrix_class_inputs.py (CPU: the references agree and the
inputs are not trivial) and the three test_gpu_*_classes.py files (GPU: the
device on those same inputs).  Test infrastructure.

Every value comes from a small alphabet, so equal pairs, plateaus, -0.0 next
to 0.0 and one value large enough to swallow its neighbours in a sum turn up
in every column.  "ties" batches add NaN holes, "inf" batches add +Inf and
-Inf.  All generators take fixed integer seeds and all arrays are read-only
and built once.
"""
import functools
import math

import numpy as np

NAN = math.nan
INF = math.inf

KINDS = ("ties", "inf")
ALPHABET = np.array([-0.0, 0.0, -3.0, -1.0, 0.5, 1.0, 2.0, 2.5, 3.0, 4.0,
                     7.0, 10.0, 1e15])
PHIS = (0.0, 0.3, 0.5, 1.0, -0.5, 1.5, NAN)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _fill(rng, shape, kind):
    """Alphabet values; "ties": 20 % NaN; "inf": 10 % +Inf and 6 % -Inf."""
    v = rng.choice(ALPHABET, size=shape)
    r = rng.random(shape)
    if kind == "ties":
        v[r < 0.20] = NAN
    else:
        v[r < 0.10] = INF
        v[(r >= 0.10) & (r < 0.16)] = -INF
    return v


# ---- column aggregates ----------------------------------------------------

COLAGG_GROUP_SIZES = (0, 1, 2, 3, 4, 5, 8, 63, 64, 65, 257)
COLAGG_N_GRID = 40
COLAGG_LOOSE_ROWS = 6      # rows that belong to no group
COLAGG_NAN_COLUMN = 17     # "ties": NaN in every row
REDUCE_OPS = ("median", "quantile", "mad", "stddev", "stdvar", "mode",
              "distinct", "sum", "min", "max", "avg", "count", "sum2",
              "geomean", "group")
PER_SERIES_OPS = ("share", "zscore")
COLAGG_OPS = REDUCE_OPS + PER_SERIES_OPS + ("iqr_bounds",)
SUM_OPS = ("sum", "avg", "sum2", "share")


@functools.lru_cache(maxsize=None)
def colagg_batch(kind):
    """values [n_series x n_grid], group_rows, group_offsets.  group_rows is
    a random permutation of the rows, so the members of a group interleave
    with those of the others, and its last COLAGG_LOOSE_ROWS rows are left
    out of every group."""
    rng = np.random.default_rng(4100 + KINDS.index(kind))
    n_members = sum(COLAGG_GROUP_SIZES)
    n_series = n_members + COLAGG_LOOSE_ROWS
    v = _fill(rng, (n_series, COLAGG_N_GRID), kind)
    if kind == "ties":
        v[:, COLAGG_NAN_COLUMN] = NAN
    perm = rng.permutation(n_series).astype(np.uint32)
    rows = perm[:n_members].copy()
    offsets = np.concatenate([[0], np.cumsum(COLAGG_GROUP_SIZES)]).astype(np.uint64)
    return _frozen(v, rows, offsets)


def colagg_member_mask(kind):
    """Rows that belong to a group.  share and zscore write only those; what
    a row in no group receives is undefined today (the device and the oracle
    both leave their output buffer as allocated), so the per-series
    comparisons look at member rows only."""
    v, rows, _ = colagg_batch(kind)
    mask = np.zeros(v.shape[0], bool)
    mask[rows] = True
    return mask


def colagg_group_of(kind):
    """Group index per row, -1 for the rows of no group."""
    v, rows, offsets = colagg_batch(kind)
    gof = np.full(v.shape[0], -1, np.int32)
    for grp in range(len(offsets) - 1):
        gof[rows[int(offsets[grp]):int(offsets[grp + 1])]] = grp
    return gof


# ---- series transforms ----------------------------------------------------

TRANSFORM_N_GRIDS = (1, 2, 3, 64)
TRANSFORM_RANDOM_ROWS = 24
TS_START = 1_000_000_000_000
TS_STEP = 15_000
SERIES_FUNCS = ("keep_last_value", "keep_next_value", "interpolate",
                "running_sum", "running_min", "running_max", "running_avg",
                "range_sum", "range_min", "range_max", "range_avg",
                "range_first", "range_last", "range_normalize",
                "range_zscore", "range_trim_zscore", "range_stddev",
                "range_stdvar", "range_linear_regression", "range_mad",
                "range_trim_outliers", "range_trim_spikes", "range_quantile",
                "smooth_exponential", "remove_resets")
# the scalar argument of the functions that take one; the first value is the
# one the non-triviality bars are measured at
SCALARS = {
    "range_quantile": (0.5, 0.0, 0.3, 1.0, -0.5, 1.5, NAN),
    "range_trim_spikes": (0.2, 0.0, 1.0, 2.0),
    "range_trim_outliers": (3.0, 0.0, -1.5, NAN),
    "range_trim_zscore": (3.0, 0.0, -1.5, NAN),
}
CLAMP_FUNCS = ("clamp", "clamp_min", "clamp_max")


def transform_ts(n_grid):
    return (TS_START + np.arange(n_grid) * TS_STEP).astype(np.int64)


def _shape_rows(n, kind):
    """The hand-made rows at width n (narrow widths fold several of them
    into the same row, which is harmless)."""
    mid = n // 2
    rows = []

    def row(fill=NAN):
        r = np.full(n, fill)
        rows.append(r)
        return r

    row()                                   # all NaN
    row()[0] = 2.5                          # one value at the head
    row()[mid] = 2.5                        # ... in the middle
    row()[n - 1] = 2.5                      # ... at the tail
    row(4.0)                                # constant
    row(4.0)[0] = NAN                       # constant with a NaN first
    r = row(1.0)                            # leading NaN run
    r[:max(1, n // 4)] = NAN
    r[mid:] = 3.0
    r = row(7.0)                            # trailing NaN run
    r[n - max(1, n // 4):] = NAN
    r = row()                               # inner NaN runs of length 1, 2, 5
    r[:] = np.resize([1.0, NAN, 2.0, NAN, NAN, 4.0, 4.0, NAN, NAN, NAN, NAN,
                      NAN, 10.0, 0.5], n)
    # a counter with resets: a small drop (100 -> 90, less than 1/8 of 100,
    # which remove_resets adds back as the drop) and a full reset (-> 1)
    r = row()
    r[:] = np.resize([10.0, 50.0, 100.0, 90.0, 90.0, 120.0, 1.0, 3.0, NAN,
                      3.0, 2.0, 40.0], n)
    r = row()                               # plateaus
    r[:] = np.repeat([0.0, 2.0, 2.0, -0.0, 7.0, 7.0, 1e15, 3.0],
                     max(1, -(-n // 8)))[:n]
    if kind == "inf":
        row(1.0)[0] = INF                   # +Inf first
        row(1.0)[0] = -INF                  # -Inf first
        row(2.0)[n - 1] = INF               # +Inf last
        row(2.0)[n - 1] = -INF              # -Inf last
        for inf in (INF, -INF):             # inside a NaN gap
            r = row(3.0)
            lo, hi = max(0, mid - 2), min(n, mid + 3)
            r[lo:hi] = NAN
            r[mid] = inf
            if n > 4:
                r[n - 1] = 0.5
    return rows


@functools.lru_cache(maxsize=None)
def transform_batch(kind, n_grid):
    """values [n_series x n_grid]: the hand-made rows, then random rows."""
    rng = np.random.default_rng(4200 + 10 * TRANSFORM_N_GRIDS.index(n_grid)
                                + KINDS.index(kind))
    rows = _shape_rows(n_grid, kind)
    rand = _fill(rng, (TRANSFORM_RANDOM_ROWS, n_grid), kind)
    # every random row keeps to its own 3 to 8 letters of the alphabet, so
    # the per-row extremes and quantiles differ from row to row
    for r in rand:
        letters = rng.choice(ALPHABET, rng.integers(3, 9), replace=False)
        own = np.isin(r, ALPHABET)
        r[own] = rng.choice(letters, own.sum())
    if kind == "inf" and n_grid >= 3:
        # a few holes too, so the infinities meet the NaN handling
        rand[::4][rng.random(rand[::4].shape) < 0.15] = NAN
    v = np.vstack(rows + [rand])
    return _frozen(v)[0]


@functools.lru_cache(maxsize=None)
def smoothing_factors(n_grid):
    """0, 1, below 0, above 1 and NaN, cycling."""
    return _frozen(np.resize([0.3, 0.0, 1.0, -0.5, 1.5, NAN, 0.7, 0.05],
                             n_grid).astype(np.float64))[0]


@functools.lru_cache(maxsize=None)
def clamp_bounds(n_grid):
    """Per-point min and max rows from the alphabet: equal to samples, in
    the wrong order at some points, NaN and infinite at others."""
    rng = np.random.default_rng(4290 + n_grid)
    lo = rng.choice([-3.0, -1.0, -0.0, 0.5, 2.0, NAN, -INF], n_grid)
    hi = rng.choice([0.0, 1.0, 2.5, 4.0, 10.0, NAN, INF, -1.0], n_grid)
    return _frozen(lo, hi)


# ---- histograms -----------------------------------------------------------

HIST_N_GRID = 48
HIST_ZERO_COLUMN = 5
HIST_NAN_COLUMN = 11
HQ_PHIS = (0.0, 0.25, 0.5, 0.99, 1.0, -1.0, 2.0, NAN)


def _hist_les(rng):
    """le rows of every group: 0 les; only +Inf; [x, +Inf]; 3, 12 and 33
    les; a duplicated le; no +Inf bucket.  Two of each non-empty shape."""
    def grid(n):     # n - 1 finite les on a quarter grid, then +Inf
        return list(np.sort(rng.choice(np.arange(1, 400), n - 1,
                                       replace=False)) * 0.25) + [INF]
    groups = [[]]
    for _ in range(2):
        groups += [[INF], [float(rng.integers(1, 9))] + [INF], grid(3),
                   grid(12), grid(33), [1.0, 2.0, 2.0, 5.0, INF],
                   [0.5, 1.0, 2.5, 5.0]]
    groups.insert(9, [])
    return groups


@functools.lru_cache(maxsize=None)
def hist_batch():
    """bucket_values [n_rows x n_grid], les [n_rows], group_offsets.
    Integer cumulative counts with plateaus and leading zero buckets, about
    5 % NaN and about 3 % broken (decreasing) buckets (25 % in one group),
    one all-zero column and one all-NaN column."""
    rng = np.random.default_rng(4300)
    groups = _hist_les(rng)
    blocks = []
    for les in groups:
        n = len(les)
        inc = rng.choice([0.0, 0.0, 0.0, 1.0, 2.0, 5.0, 40.0],
                         size=(n, HIST_N_GRID))
        # leading zero buckets at about a third of the grid points
        lead = rng.integers(0, 4, HIST_N_GRID) * (rng.random(HIST_N_GRID) < 0.35)
        for g in range(HIST_N_GRID):
            inc[:min(n, int(lead[g])), g] = 0.0
        bv = np.cumsum(inc, axis=0)
        r = rng.random(bv.shape)
        # the second 12-le group is broken at every fourth bucket: raw
        # decreasing counts are negative weights for histogram_stddev, whose
        # variance then goes below zero and is clamped
        rate = 0.25 if (n == 12 and len(blocks) > 8) else 0.03
        broken = (r < rate) & (bv > 0)
        bv[broken] = np.maximum(0.0, bv[broken] - rng.integers(1, 4, bv.shape)[broken])
        if rate > 0.03:
            bv[broken] = np.floor(bv[broken] * 0.2)     # deep drops
        bv[(r >= rate) & (r < rate + 0.05)] = NAN
        blocks.append(bv)
    bv = np.vstack(blocks)
    bv[:, HIST_ZERO_COLUMN] = 0.0
    bv[:, HIST_NAN_COLUMN] = NAN
    les = np.asarray([le for g in groups for le in g], np.float64)
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint64)
    assert (np.diff(offsets.astype(np.int64)) > 0).any()
    return _frozen(bv, les, offsets)


@functools.lru_cache(maxsize=None)
def hist_le_req():
    """One le_req per grid point: the les themselves (exact hits), points
    between them, 0, -1, +Inf and NaN."""
    rng = np.random.default_rng(4301)
    _, les, _ = hist_batch()
    finite = np.unique(les[np.isfinite(les)])
    between = (finite[:-1] + finite[1:]) / 2
    req = np.empty(HIST_N_GRID)
    for g in range(HIST_N_GRID):
        k = g % 8
        if k < 3:
            req[g] = rng.choice(finite[finite <= 6])    # hits in most groups
        elif k == 3:
            req[g] = rng.choice(finite)
        elif k < 6:
            req[g] = rng.choice(between[between <= 30])
        else:
            req[g] = rng.choice([0.0, -1.0, INF, NAN, 1e6])
    req[:5] = [0.0, -1.0, INF, NAN, 1.0]
    return _frozen(req)[0]


def hist_two_finite_les():
    """Groups with at least two finite les: where the histogram functions
    have something to interpolate."""
    _, les, offsets = hist_batch()
    return np.asarray([np.isfinite(les[int(lo):int(hi)]).sum() >= 2
                       for lo, hi in zip(offsets[:-1], offsets[1:])])


# ---- references, computed once and shared ----------------------------------
# `oracle_*` is the C oracle, `plain_*` the pure-Python reference of
# matrix_reference.py.  The NaN arguments are the module's NAN object, so the
# caches hit.

COLAGG_CASES = ([(op, 0.0) for op in COLAGG_OPS if op != "quantile"]
                + [("quantile", phi) for phi in PHIS])
TRANSFORM_CASES = [(f, s) for f in SERIES_FUNCS
                   for s in SCALARS.get(f, (0.0,))]
HSTAT_MODES = ("avg", "stddev", "stdvar")


def _frozen_result(r):
    for a in (r if isinstance(r, tuple) else (r,)):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def oracle_colagg(op, phi, kind):
    import oracle
    return _frozen_result(oracle.colagg(op, *colagg_batch(kind), phi=phi))


@functools.lru_cache(maxsize=None)
def plain_colagg(op, phi, kind):
    import matrix_reference as mr
    return _frozen_result(mr.colagg(op, *colagg_batch(kind), phi=phi))


def series_func_id(func):
    from victoriametrics_amd import transform as tf
    return {**tf._CLAMP, **tf._SERIES}[func]


def _transform_args(func, n_grid):
    ts = transform_ts(n_grid) if func == "range_linear_regression" else None
    arg1 = smoothing_factors(n_grid) if func == "smooth_exponential" else None
    return ts, arg1


@functools.lru_cache(maxsize=None)
def oracle_transform(func, scalar, kind, n_grid):
    import oracle
    ts, arg1 = _transform_args(func, n_grid)
    return _frozen_result(oracle.tf_apply(
        series_func_id(func), transform_batch(kind, n_grid).copy(), ts=ts,
        arg1=arg1, scalar=scalar))


@functools.lru_cache(maxsize=None)
def plain_transform(func, scalar, kind, n_grid):
    import matrix_reference as mr
    ts, arg1 = _transform_args(func, n_grid)
    return _frozen_result(mr.transform(func, transform_batch(kind, n_grid),
                                       ts=ts, arg1=arg1, scalar=scalar))


@functools.lru_cache(maxsize=None)
def oracle_clamp(func, kind, n_grid):
    import oracle
    lo, hi = clamp_bounds(n_grid)
    args = {"clamp": (lo, hi), "clamp_min": (lo, None), "clamp_max": (hi, None)}
    a1, a2 = args[func]
    return _frozen_result(oracle.tf_apply(
        series_func_id(func), transform_batch(kind, n_grid).copy(),
        arg1=a1, arg2=a2)[0])


@functools.lru_cache(maxsize=None)
def plain_clamp(func, kind, n_grid):
    import matrix_reference as mr
    lo, hi = clamp_bounds(n_grid)
    v = transform_batch(kind, n_grid)
    if func == "clamp":
        return _frozen_result(mr.clamp(func, v, lo, hi))
    return _frozen_result(mr.clamp(func, v, lo if func == "clamp_min" else hi))


@functools.lru_cache(maxsize=None)
def oracle_hist(name, arg):
    """name: "stat" (arg: mode), "share" (arg unused), "quantile" (arg:
    phi).  Returns a tuple of outputs."""
    import oracle
    bv, les, offsets = hist_batch()
    if name == "stat":
        return _frozen_result((oracle.histogram_stat(
            HSTAT_MODES.index(arg), bv, les, offsets),))
    if name == "share":
        return _frozen_result(oracle.histogram_share(hist_le_req(), bv, les,
                                                     offsets))
    return _frozen_result(oracle.histogram_quantile(arg, bv, les, offsets,
                                                    bounds=True))


@functools.lru_cache(maxsize=None)
def plain_hist(name, arg):
    """As oracle_hist, plus the Counter of branches taken."""
    import collections
    import matrix_reference as mr
    bv, les, offsets = hist_batch()
    hits = collections.Counter()
    if name == "stat":
        out = (mr.histogram_stat(arg, bv, les, offsets, hits),)
    elif name == "share":
        out = mr.histogram_share(hist_le_req(), bv, les, offsets, hits)
    else:
        out = mr.histogram_quantile(arg, bv, les, offsets, hits)
    return _frozen_result(out), hits


# ---- launch shapes: small batches to tile -----------------------------------
# The kernels launch a bounded grid and loop.  The launch-shape tests tile one
# of these small batches with np.tile until the outputs exceed the launch, so
# the expected output is the small result tiled.

COLAGG_MAX_THREADS = 2048 * 256     # colagg_kernel, colagg_filter_kernel
WIDE_MAX_THREADS = 4096 * 256       # hstat.hip kernels, both transform kernels
COLAGG_SCRATCH_CAP = 2 << 30        # bytes; vmgpu_colagg halves blocks above


@functools.lru_cache(maxsize=None)
def colagg_small():
    """8 rows x 128 points in 4 interleaved groups of 2."""
    rng = np.random.default_rng(4400)
    v = _fill(rng, (8, 128), "ties")
    rows = rng.permutation(8).astype(np.uint32)
    offsets = (np.arange(5) * 2).astype(np.uint64)
    return _frozen(v, rows, offsets)


def tile_colagg(n_tiles, big_group=0):
    """colagg_small() n_tiles times over, then one group of big_group rows."""
    v, rows, offsets = colagg_small()
    n, per = v.shape[0], len(rows)
    tv = np.tile(v, (n_tiles, 1))
    trows = (np.tile(rows, n_tiles)
             + np.repeat(np.arange(n_tiles, dtype=np.uint32) * n, per))
    toff = np.arange(4 * n_tiles + 1, dtype=np.uint64) * 2
    if big_group:
        rng = np.random.default_rng(4401)
        tv = np.vstack([tv, _fill(rng, (big_group, v.shape[1]), "ties")])
        trows = np.concatenate([trows, tv.shape[0] - big_group
                                + rng.permutation(big_group)])
        toff = np.concatenate([toff, [toff[-1] + big_group]])
    return tv, trows.astype(np.uint32), toff.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def filter_small():
    """16 series x 2 points, 3 groups and some series of no group; bounds
    from the alphabet with NaN and infinite entries; a few samples exactly
    on a bound."""
    rng = np.random.default_rng(4402)
    v = _fill(rng, (16, 2), "ties")
    group_of = rng.integers(-1, 3, 16).astype(np.int32)
    b1 = np.array([[-1.0, 0.5], [NAN, -3.0], [-INF, 2.0]])
    b2 = np.array([[4.0, 2.5], [7.0, NAN], [3.0, INF]])
    return _frozen(v, group_of, b1, b2)


@functools.lru_cache(maxsize=None)
def hist_small():
    """3 groups of 3 les x 128 points, counts as in hist_batch."""
    rng = np.random.default_rng(4403)
    les = np.array([1.0, 2.5, INF, 0.25, 4.0, 8.0, 2.0, 2.0, INF])
    offsets = np.array([0, 3, 6, 9], np.uint64)
    bv = np.vstack([np.cumsum(rng.choice([0.0, 0.0, 1.0, 2.0, 5.0],
                                         size=(3, 128)), axis=0)
                    for _ in range(3)])
    r = rng.random(bv.shape)
    bv[r < 0.05] = NAN
    bv[(r > 0.97) & (bv > 0)] -= 1.0
    req = rng.choice([0.0, 0.25, 1.0, 1.5, 2.0, 3.0, 8.0, 9.0, -1.0, INF, NAN],
                     128)
    return _frozen(bv, les, offsets, req)


def tile_hist(n_tiles):
    bv, les, offsets, req = hist_small()
    return (np.tile(bv, (n_tiles, 1)), np.tile(les, n_tiles),
            np.arange(3 * n_tiles + 1, dtype=np.uint64) * 3, req)
