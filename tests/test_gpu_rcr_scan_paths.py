"""One set of removeCounterResets shapes through every scan of the engine.

csrc/vmgpu.hip holds four scans: two with one sample per lane, which share
rcr_round_single, and two with two samples per lane, which each carry their
own copy of the pair round.  Series length and the presence of stale NaNs
pick the scan:

  129, 200, 256   pipe kernel: rcr_scan_pairs for a series at an even sample
                  offset; rcr_scan_wave<2> behind the compaction for one at an
                  odd offset (every other 129-sample series leaves its
                  successor at one) and for one with stale NaNs
  300, 500        wave kernel: load_rcr_fused_wave; rcr_scan_wave<1> behind
                  the compaction when the series holds stale NaNs
  700, 2000       block kernel: rcr_scan_col_pairs on the LDS column
  4200            huge kernel: rcr_scan_col_pairs on the global column

Every series spans the grid and its first window, whatever its length, so
the grid points read corrected values from every round of the scan, not only
from the first few.  Results are compared bit for bit with the oracle.
"""
import functools

import numpy as np
import pytest

import oracle
from seriesgen import assert_parity
from test_gpu_pipe_edges import (_fractional_counter, _oracle_batch,
                                 _rcr_model_clamps)

pytestmark = pytest.mark.gpu

START = 1_000_000_000_000
STEP = 15_000
LBD = 5 * STEP                      # staleness interval = LBD + window
PLANS = {"fused_w20": (130, 20 * STEP), "jcache_w64": (65, 64 * STEP)}
LENGTHS = {"pipe": (129, 200, 256), "long": (300, 500, 700, 2000, 4200)}
SEED = 78


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


def _shapes(rng, n, n_grid, window):
    """The scan shapes at one length: list of (ts, vals), and the indices of
    the fractional counters among them."""
    gap = LBD + window + STEP
    cadence = ((n_grid - 1) * STEP + window) // (n - 1)
    base_t = START - window + np.arange(n, dtype=np.int64) * cadence
    mono = np.cumsum(rng.poisson(150.0, n).astype(np.float64)) + 1000.0

    def with_gaps(at):
        t = base_t.copy()
        for k in sorted({k for k in at if k < n}):
            t[k:] += gap
        return t

    full = mono.copy()
    full[n // 3:] -= full[n // 3] - 1.0
    full[2 * n // 3:] -= full[2 * n // 3]
    part = mono.copy()
    a, b = n // 4, n // 2 + 1
    part[a:] -= 0.05 * part[a - 1]          # -d*8 < prev: partial reset
    part[b:] -= 0.04 * part[b - 1]
    assert 0 < (part[a - 1] - part[a]) * 8 < part[a - 1]
    assert 0 < (part[b - 1] - part[b]) * 8 < part[b - 1]
    nan_v = mono.copy()                     # ordinary NaN, not the stale one
    r1, r2 = n // 2, 3 * n // 4
    nan_v[r1:] -= nan_v[r1] - 1.0
    nan_v[r1 - 1] = np.nan                  # right before a reset
    nan_v[r2:] -= nan_v[r2] - 1.0
    nan_v[r2 + 1] = np.nan                  # right after one
    negz = np.zeros(n)
    negz[::3] = -0.0
    negz[3 * n // 5:] = np.cumsum(np.ones(n - 3 * n // 5))

    series = [(base_t, mono), (base_t, full), (base_t, part)]
    frac = []
    # the clamp fires in most but not all p = 0.2 series at 300 samples
    for p in [0.2] * (4 if n <= 300 else 2) + [0.0]:
        frac.append(len(series))
        series.append((base_t, _fractional_counter(rng, n, p)))
    series += [
        (with_gaps((63, 127, n - 1)), full),
        (with_gaps((64, 128)), part),
        (with_gaps((65, 129)), mono),
        (base_t, nan_v), (base_t, negz),
    ]
    return series, frac


@functools.lru_cache(maxsize=None)
def _batch(kind, plan_id, stale):
    """Flat columns + offsets of one batch; the same draws for every plan and
    with or without stale NaNs."""
    n_grid, window = PLANS[plan_id]
    rng = np.random.default_rng(SEED)
    series = []
    for n in LENGTHS[kind]:
        shapes, frac = _shapes(rng, n, n_grid, window)
        # the reference alone: its monotonic clamp changes some fractional
        # counter of this length and leaves another one as it is
        clamps = [_rcr_model_clamps(shapes[k][1], shapes[k][0], 0)
                  for k in frac]
        assert any(clamps), f"n={n}: no series engages the clamp"
        assert not all(clamps), f"n={n}: no series takes the clamp shortcut"
        series += shapes
    assert len(series) <= 62
    if stale:
        srng = np.random.default_rng(SEED + 1)
        marked = []
        for t, v in series:
            v = v.copy()
            v[srng.choice(len(v), 3, replace=False)] = oracle.stale_nan()
            marked.append((t, v))
        series = marked
    offsets = np.zeros(len(series) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(t) for t, _ in series])
    if kind == "pipe" and not stale:
        assert (offsets[:-1] & 1).any() and not (offsets[:-1] & 1).all()
    ts = np.concatenate([t for t, _ in series]).astype(np.int64)
    vals = np.concatenate([v for _, v in series]).astype(np.float64)
    return ts, vals, offsets


@pytest.mark.parametrize("stale", [False, True], ids=["clean", "stale_nans"])
@pytest.mark.parametrize("plan_id", list(PLANS))
@pytest.mark.parametrize("kind", list(LENGTHS))
def test_scan_paths(engine, kind, plan_id, stale):
    n_grid, window = PLANS[plan_id]
    ts, vals, offsets = _batch(kind, plan_id, stale)
    end = START + (n_grid - 1) * STEP
    for func in ("rate", "deriv_fast"):
        plan = engine.RollupPlan(func, START, end, STEP, window=window,
                                 lookback_delta=LBD)
        out, _, scanned = engine.rollup_eval(plan, ts, vals, offsets)
        ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets)
        context = f"{kind} {plan_id} {func} stale={stale}"
        assert scanned == ref_scanned, context
        assert np.isfinite(ref).any(), context
        assert_parity(out, ref, exact=True, context=context)
