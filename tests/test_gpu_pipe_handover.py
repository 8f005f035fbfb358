"""Series-to-series handover of the pipelined rate kernel
(rollup_pipe_kernel): while a wave evaluates series k it has the data of
series k+1 in flight into the staging registers and the descriptors of
series k+2 in flight into scalar registers, and it waits for the staged
data exactly once, at the top of the next iteration.

VMGPU_PIPE_BLOCKS=1 launches one block, so wave w of its four waves walks the
series w, w+4, w+8, ... of the kernel's series list: a few dozen series are
enough to put every kind of series behind every other kind on one wave.
Results are compared bit for bit with the oracle, samples_scanned included.
"""
import numpy as np
import pytest

import oracle
from seriesgen import assert_parity
from test_gpu_pipe_edges import START, STEP, _counter, _oracle_batch

pytestmark = pytest.mark.gpu

WAVES = 4            # waves of one block
FILLER = 513         # odd and above the wave kernels' 512-sample cap

KINDS = ["full256", "n129", "n128", "n1", "empty", "odd", "stale", "wide",
         "resets"]


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


def _make(kind, rng):
    """One series of the given kind -> (ts, vals)."""
    t0 = START - 20 * STEP + int(rng.integers(0, 40)) * STEP
    if kind == "full256":
        return _counter(rng, 256, t0 - 40 * STEP, reset_p=0.0)
    if kind == "n129":
        return _counter(rng, 129, t0, reset_p=0.0)
    if kind == "n128":
        return _counter(rng, 128, t0, reset_p=0.0)
    if kind == "n1":
        return _counter(rng, 1, START + 30 * STEP, reset_p=0.0)
    if kind == "empty":
        return np.empty(0, np.int64), np.empty(0, np.float64)
    if kind == "odd":      # placed at an odd sample offset by _layout
        return _counter(rng, int(rng.integers(150, 257)), t0, reset_p=0.0)
    if kind == "stale":    # compacted from global memory, count < raw count
        t, v = _counter(rng, 200, t0, reset_p=0.0)
        v[rng.choice(200, 9, replace=False)] = oracle.stale_nan()
        return t, v
    if kind == "wide":     # span >= 2^31 ms: the cold two-probe loop
        far = START - (1 << 31) - 50 * STEP + np.arange(50, dtype=np.int64) * STEP
        near = START - 20 * STEP + np.arange(150, dtype=np.int64) * STEP
        t = np.concatenate([far, near])
        assert t[-1] - t[0] >= 1 << 31
        v = np.cumsum(rng.poisson(150.0, len(t)).astype(np.float64))
        return t, v
    if kind == "resets":   # the scan's slow path
        return _counter(rng, 220, t0, reset_p=0.1)
    raise AssertionError(kind)


def _all_pairs_cycle(k):
    """Cyclic sequence over range(k) in which every ordered pair (a, b),
    a == b included, occurs exactly once as neighbours: an Euler circuit of
    the complete directed graph with loops (Hierholzer)."""
    nxt = {a: list(range(k)) for a in range(k)}
    stack, circuit = [0], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == k * k + 1 and circuit[0] == circuit[-1]
    return circuit[:-1]


def _handover_kinds():
    """Kinds in kernel-list order such that, with four waves walking the
    list at stride four, every ordered pair of kinds is a (k, k+1) handover
    on some wave.  81 pairs need four chains of 22 series: 88 series."""
    cyc = _all_pairs_cycle(len(KINDS))
    per_wave = -(-len(cyc) // WAVES)            # handovers per wave: 21
    chains = [[cyc[(w * per_wave + j) % len(cyc)] for j in range(per_wave + 1)]
              for w in range(WAVES)]
    kinds = [KINDS[chains[i % WAVES][i // WAVES]]
             for i in range(WAVES * (per_wave + 1))]
    seen = {(kinds[i], kinds[i + WAVES]) for i in range(len(kinds) - WAVES)}
    assert seen == {(a, b) for a in KINDS for b in KINDS}
    return kinds


def _layout(kinds, rng):
    """Flat columns for the kinds.  A series of kind "odd" starts at an odd
    sample offset and every other one at an even offset; where the running
    offset has the wrong parity a 513-sample filler series goes in front.
    Fillers are too long for the pipe kernel (they run through the block
    kernel), so they are not on its series list: the list order is the
    order of `kinds`, read through the selection list."""
    series, pos = [], 0
    for kind in kinds:
        if (pos & 1) != int(kind == "odd"):
            series.append(_counter(rng, FILLER, START - 100 * STEP,
                                   reset_p=0.01))
            pos += FILLER
        t, v = _make(kind, rng)
        series.append((t, v))
        pos += len(t)
    return _flat(series)


def _flat(series):
    offsets = np.zeros(len(series) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(t) for t, _ in series])
    ts = np.concatenate([np.asarray(t, np.int64) for t, _ in series])
    vals = np.concatenate([np.asarray(v, np.float64) for _, v in series])
    return ts, vals, offsets


def _check(engine, cols, n_grid, ratio, func="rate", context=""):
    ts, vals, offsets = cols
    end = START + (n_grid - 1) * STEP
    plan = engine.RollupPlan(func, START, end, STEP, window=ratio * STEP)
    out, _, scanned = engine.rollup_eval(plan, ts, vals, offsets)
    ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets)
    assert scanned == ref_scanned, context
    assert_parity(out, ref, exact=True, context=context)
    return out


# (n_grid, window/step): 130 points are three rounds of 64, 65 two and 2 one,
# so the number of row stores behind the staged loads differs; 20 takes the
# fused seek+eval loop, 64 the j-cache loop
SHAPES = {"rate": [(130, 20), (130, 64), (2, 20), (65, 20), (65, 64)],
          "deriv_fast": [(130, 20), (130, 64)]}


@pytest.mark.parametrize("func", ["rate", "deriv_fast"])
def test_handover_sequences(engine, monkeypatch, func):
    """Every ordered pair of series kinds as (k, k+1) on one wave."""
    monkeypatch.setenv("VMGPU_PIPE_BLOCKS", "1")
    cols = _layout(_handover_kinds(), np.random.default_rng(2024))
    for n_grid, ratio in SHAPES[func]:
        _check(engine, cols, n_grid, ratio, func=func,
               context=f"handover {func} n_grid={n_grid} w/s={ratio}")


@pytest.mark.parametrize("n_series", [4, 5, 7, 8])
def test_handover_last_series(engine, monkeypatch, n_series):
    """One block: with 4 series no wave has a next series; with 5, 7 and 8
    the next (and last) series of a wave is empty, at an odd sample offset,
    a single sample, or full."""
    monkeypatch.setenv("VMGPU_PIPE_BLOCKS", "1")
    rng = np.random.default_rng(50 + n_series)
    series = [_counter(rng, 256, START - 60 * STEP),
              _counter(rng, 129, START - 20 * STEP),
              _counter(rng, 200, START - 20 * STEP, reset_p=0.1),
              _counter(rng, 128, START - 20 * STEP),
              (np.empty(0, np.int64), np.empty(0, np.float64)),
              _counter(rng, 201, START - 20 * STEP),    # starts at 713: odd
              _counter(rng, 1, START + 30 * STEP),
              _counter(rng, 256, START - 60 * STEP)][:n_series]
    cols = _flat(series)
    if n_series > 5:
        assert int(cols[2][5]) & 1
    for n_grid, ratio in ((130, 20), (65, 64)):
        _check(engine, cols, n_grid, ratio,
               context=f"last series n={n_series} n_grid={n_grid}")


@pytest.mark.parametrize("aggr", ["sum", "avg"])
def test_handover_grouped(engine, monkeypatch, aggr):
    """The grouped instantiation over the same sequence, three groups.
    Group ids rise with the series index, so the batch's by-group layout
    keeps the series order (float-sum bar: atomic order varies)."""
    monkeypatch.setenv("VMGPU_PIPE_BLOCKS", "1")
    ts, vals, offsets = _layout(_handover_kinds(), np.random.default_rng(2025))
    n = len(offsets) - 1
    n_groups = 3
    gids = (np.arange(n) * n_groups // n).astype(np.int32)
    for n_grid, ratio in ((130, 20), (130, 64)):
        end = START + (n_grid - 1) * STEP
        plan = engine.RollupPlan("rate", START, end, STEP, window=ratio * STEP,
                                 aggr=aggr)
        with engine.SeriesBatch(ts, vals, offsets, gids, n_groups) as b:
            perm = getattr(b, "_perm", None)
            assert perm is None or np.array_equal(perm, np.arange(n))
            out, _, scanned = b.exec(plan)
        ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets,
                                            group_ids=gids, n_groups=n_groups,
                                            aggr=aggr)
        assert scanned == ref_scanned
        assert_parity(out, ref, exact=False, rtol=1e-9,
                      context=f"grouped {aggr} n_grid={n_grid} w/s={ratio}")


def test_many_series_default_grid(engine, monkeypatch):
    """24,000 series on the default grid (no override): more series than
    waves resident at any occupancy, so every wave hands over several times
    whatever the device holds.  Lengths are
    uniform in 0..256 and about 2 % of the series start at an odd offset.
    Ten more launches over the resident batch must reproduce the first one
    byte for byte: a staged value consumed before it has landed would differ
    from launch to launch."""
    monkeypatch.delenv("VMGPU_PIPE_BLOCKS", raising=False)
    rng = np.random.default_rng(24000)
    n_series = 24000
    lens = np.empty(n_series, dtype=np.int64)
    pos = odd_starts = 0
    for s in range(n_series):
        n = int(rng.integers(0, 129)) * 2                 # even, 0..256
        if pos & 1:                                       # back to even
            odd_starts += 1
            n = max(n - 1, 1)
        elif rng.random() < 0.02:                         # next starts odd
            n = max(n - 1, 1)
        lens[s] = n
        pos += n
    assert 0.01 < odd_starts / n_series < 0.04
    assert lens.min() == 0 and lens.max() == 256
    offsets = np.zeros(n_series + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    total = int(offsets[-1])
    # jittered cadence per series, counters with a few resets
    first = np.repeat(offsets[:-1].astype(np.int64), lens)
    k = np.arange(total, dtype=np.int64) - first
    t0 = START - 20 * STEP + rng.integers(0, 40, n_series) * STEP
    ts = np.repeat(t0, lens) + k * STEP + rng.integers(-500, 501, total)
    inc = rng.poisson(150.0, total).astype(np.float64)
    run = np.cumsum(inc)
    vals = run - run[first] + 1.0
    drop = np.flatnonzero(rng.random(total) < 0.01)
    vals[drop] = 1.0                                      # counter resets
    n_grid = 70
    plan = engine.RollupPlan("rate", START, START + (n_grid - 1) * STEP, STEP,
                             window=20 * STEP)
    ref, _, ref_scanned = _oracle_batch(plan, ts, vals, offsets)
    with engine.SeriesBatch(ts, vals, offsets) as b:
        out, _, scanned = b.exec(plan)
        assert scanned == ref_scanned
        assert_parity(out, ref, exact=True, context="24000 series")
        first_bytes = out.tobytes()
        for rep in range(10):
            again, _, scanned = b.exec(plan)
            assert scanned == ref_scanned
            assert again.tobytes() == first_bytes, f"launch {rep + 2} differs"


@pytest.mark.parametrize("value", ["0", "1", "1000000000", "garbage"])
def test_block_override_clamp(engine, monkeypatch, value):
    """VMGPU_PIPE_BLOCKS is clamped into the valid range and anything that
    is not a number is ignored."""
    monkeypatch.setenv("VMGPU_PIPE_BLOCKS", value)
    rng = np.random.default_rng(9)
    series = [_counter(rng, 2 * int(rng.integers(0, 129)), START - 20 * STEP)
              for _ in range(40)]
    _check(engine, _flat(series), 130, 20, context=f"PIPE_BLOCKS={value}")
