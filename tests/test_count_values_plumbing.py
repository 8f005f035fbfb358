"""Host side of the device count_values_over_time path, without a device:
the order key the device sorts on (rollup_multi.count_values_order_key) and
the row -> Series step (rollup_multi.count_values_over_time_batch) driven by
a stand-in batch that returns fixed rows."""
import numpy as np
import pytest

from victoriametrics_amd import limits, rollup_multi
from victoriametrics_amd.decimal import STALE_NAN_BITS
from victoriametrics_amd.metric_name import MetricName


def _from_bits(bits):
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


NAN_PAYLOADS = [_from_bits(b) for b in (0x7FF8000000000000,
                                        0xFFF8000000000000,
                                        0x7FF8000000000123, STALE_NAN_BITS)]


def test_order_key_is_strictly_increasing():
    vals = [-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300,
            np.inf, np.nan]
    keys = [rollup_multi.count_values_order_key(v) for v in vals]
    assert all(0 <= k < 1 << 64 for k in keys)
    assert all(a < b for a, b in zip(keys, keys[1:])), keys


def test_order_key_folds_every_nan():
    keys = {rollup_multi.count_values_order_key(v) for v in NAN_PAYLOADS}
    assert keys == {0xFFF8000000000000}
    # and stays clear of the device's "no row" sentinel
    assert max(keys) < 0xFFFFFFFFFFFFFFFF


def test_order_key_tells_apart_what_the_label_tells_apart():
    rng = np.random.default_rng(1490)
    vals = np.concatenate([np.exp(rng.normal(0.0, 5.0, 500)),
                           -np.exp(rng.normal(0.0, 5.0, 500)),
                           [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324,
                            np.nextafter(1.0, 2.0), 1.0, np.nextafter(1.0, 0.0)]])
    order = sorted(range(len(vals)),
                   key=lambda i: rollup_multi.count_values_order_key(vals[i]))
    srt = vals[order]
    for a, b in zip(srt, srt[1:]):
        assert a < b or (a == 0 and b == 0 and np.signbit(a) and not np.signbit(b))
    labels = {rollup_multi.format_go_float_g(float(v)) for v in vals}
    keys = {rollup_multi.count_values_order_key(v) for v in vals}
    assert len(labels) == len(keys) == len(vals)


ROW_VALUES = np.array([-0.0, 0.0, 1e6, 123456.0, 1e-5, np.inf, -np.inf,
                       np.nan])
ROW_LABELS = [b"-0", b"0", b"1e+06", b"123456", b"1e-05", b"+Inf", b"-Inf",
              b"NaN"]
ROW_SERIES = np.array([2, 2, 2, 0, 0, 0, 1, 1], dtype=np.uint32)
N_GRID = 3


class _StandInBatch:
    """Answers count_values_over_time with fixed rows and records the call."""

    def __init__(self):
        self.calls = []
        self.values = np.arange(len(ROW_VALUES) * N_GRID,
                                dtype=np.float64).reshape(-1, N_GRID) + 1.0
        self.values[1, 2] = np.nan

    def count_values_over_time(self, start, end, step, window,
                               drop_stale=True, max_rows=0):
        self.calls.append(dict(start=start, end=end, step=step, window=window,
                               drop_stale=drop_stale, max_rows=max_rows))
        return ROW_SERIES.copy(), ROW_VALUES.copy(), self.values.copy(), 77


def _mns():
    return [MetricName(b"m0", [(b"job", b"a")]),
            MetricName(b"m1", [(b"code", b"old"), (b"job", b"b")]),
            MetricName(b"m2", [(b"job", b"c")])]


@pytest.mark.parametrize("keep_metric_names", [False, True])
def test_batch_function_names_rows(keep_metric_names):
    batch = _StandInBatch()
    got, scanned = rollup_multi.count_values_over_time_batch(
        "code", batch, _mns(), 1000, 1200, 100, 300,
        keep_metric_names=keep_metric_names)
    assert scanned == 77
    assert len(got) == len(ROW_VALUES)
    jobs = [b"a", b"b", b"c"]
    seen = set()
    for s in got:
        label = s.mn.get_tag_value(b"code")
        row = ROW_LABELS.index(label)
        seen.add(row)
        src = int(ROW_SERIES[row])
        # attributed to metric_names[row_series], group handled, tag replaced
        assert s.mn.get_tag_value(b"job") == jobs[src]
        assert s.mn.metric_group == ((b"m%d" % src) if keep_metric_names
                                     else b"")
        assert [k for k, _ in s.mn.tags].count(b"code") == 1
        assert np.array_equal(
            np.asarray(s.values).view(np.uint64),
            batch.values[row].view(np.uint64))
    assert seen == set(range(len(ROW_VALUES)))
    # ordered by series id, a series' rows in the order the batch gave them
    assert [int(ROW_SERIES[ROW_LABELS.index(s.mn.get_tag_value(b"code"))])
            for s in got] == sorted(ROW_SERIES.tolist())
    # the source names are untouched
    assert _mns()[1].get_tag_value(b"code") == b"old"


def test_batch_function_passes_the_grid_and_the_limit(monkeypatch):
    batch = _StandInBatch()
    rollup_multi.count_values_over_time_batch(
        "code", batch, _mns(), 1000, 1200, 100, 300, drop_stale=False)
    assert batch.calls[-1] == dict(
        start=1000, end=1200, step=100, window=300, drop_stale=False,
        max_rows=limits.max_series_per_aggr_func)
    monkeypatch.setattr(limits, "max_series_per_aggr_func", 1234)
    rollup_multi.count_values_over_time_batch(
        "code", batch, _mns(), 1000, 1200, 100, 300)
    assert batch.calls[-1]["max_rows"] == 1234
    assert batch.calls[-1]["drop_stale"] is True
    rollup_multi.count_values_over_time_batch(
        "code", batch, _mns(), 1000, 1200, 100, 300, max_rows=0)
    assert batch.calls[-1]["max_rows"] == 0


def test_series_batch_has_the_device_entry_point():
    from victoriametrics_amd import engine
    assert callable(engine.SeriesBatch.count_values_over_time)
