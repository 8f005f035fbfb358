"""CPU-side checks of the count_values() aggregate's entry points: the
symbols exist, the Python layer rejects malformed arrays and limits before
it takes a pointer, and without a device the calls fail loudly."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO_ROOT
from victoriametrics_amd import aggregate, engine
from victoriametrics_amd.binary_op import Series
from victoriametrics_amd.metric_name import MetricName

LIB = os.path.join(REPO_ROOT, "victoriametrics_amd", "libvmgpu.so")
HEADER = os.path.join(REPO_ROOT, "include", "vmgpu.h")
SYMBOLS = ("vmgpu_aggr_count_values_exec",
           "vmgpu_batch_aggr_count_values_exec",
           "vmgpu_aggr_count_values_fetch")


def test_symbols_exported_and_declared():
    lib = ctypes.CDLL(LIB)
    header = open(HEADER).read()
    declared = re.findall(r"^int\s+(vmgpu_\w+)\(", header, re.M)
    for sym in SYMBOLS:
        assert sym in declared, f"{sym} not declared in vmgpu.h"
        assert hasattr(lib, sym), f"libvmgpu.so does not export {sym}"


@pytest.fixture
def no_native(monkeypatch):
    """Any attempt to reach the library fails the test."""
    def boom(*a, **k):
        raise AssertionError("native layer reached with malformed input")
    monkeypatch.setattr(engine, "_load_lib", boom)
    monkeypatch.setattr(engine, "init", boom)


def _good():
    return (np.ones((3, 4)), np.asarray([0, 1, 2], np.uint32),
            np.asarray([0, 2, 3], np.uint64), 1000)


@pytest.mark.parametrize("which,bad,exc", [
    (0, np.ones((3, 4), np.float32), TypeError),
    (0, [[1.0, 2.0]], TypeError),
    (0, np.ones(12), ValueError),
    (0, np.ones((3, 8))[:, ::2], ValueError),
    (0, np.ones((4, 3)).T, ValueError),
    (1, np.asarray([0, 1, 2], np.int64), TypeError),
    (1, np.asarray([[0, 1, 2]], np.uint32), ValueError),
    (1, np.arange(6, dtype=np.uint32)[::2], ValueError),
    (1, np.asarray([0, 1], np.uint32), ValueError),   # offsets run past it
    (2, np.asarray([0, 2, 3], np.int64), TypeError),
    (2, np.asarray([0.0, 2.0, 3.0]), TypeError),
    (2, np.empty(0, np.uint64), ValueError),
    (2, np.arange(6, dtype=np.uint64)[::2], ValueError),
    (3, 0, ValueError),
    (3, -1, ValueError),
    (3, 2 ** 24 + 1, ValueError),
    (3, 2 ** 32, ValueError),
])
def test_aggr_count_values_rejects_malformed(no_native, which, bad, exc):
    args = list(_good())
    args[which] = bad
    with pytest.raises(exc):
        engine.aggr_count_values(*args)


def _bare_batch(n_series):
    b = engine.SeriesBatch.__new__(engine.SeriesBatch)
    b.n_series = n_series
    b.handle = 0
    b._perm = None
    return b


@pytest.mark.parametrize("group_of,n_groups,limit,exc", [
    (np.zeros(4, np.int64), 1, 10, TypeError),
    ([0, 0, 0, 0], 1, 10, TypeError),
    (np.zeros((4, 1), np.int32), 1, 10, ValueError),
    (np.zeros(8, np.int32)[::2], 1, 10, ValueError),
    (np.zeros(3, np.int32), 1, 10, ValueError),                  # wrong length
    (np.asarray([0, 1, 2, 0], np.int32), 2, 10, ValueError),     # id >= n_groups
    (np.asarray([0, -2, 0, 0], np.int32), 1, 10, ValueError),
    (np.zeros(4, np.int32), 1, 0, ValueError),
    (np.zeros(4, np.int32), 1, 2 ** 24 + 1, ValueError),
])
def test_batch_aggr_count_values_rejects_malformed(no_native, group_of,
                                                   n_groups, limit, exc):
    with pytest.raises(exc):
        _bare_batch(4).aggr_count_values(group_of, n_groups, limit)


def test_batch_aggr_count_values_after_grouped_exec(no_native):
    b = _bare_batch(4)
    b._last_grouped = True
    with pytest.raises(engine.VmGpuError):
        b.aggr_count_values(np.zeros(4, np.int32), 1, 10)


def test_limit_error_is_a_vmgpu_error():
    assert issubclass(engine.CountValuesLimitError, engine.VmGpuError)


def test_wrappers_reject_bad_limit(no_native):
    series = [Series(MetricName(b"m", [(b"s", b"%d" % i)]), np.ones(4))
              for i in range(3)]
    for bad in (0, 2 ** 24 + 1):
        with pytest.raises(ValueError):
            aggregate.count_values_device("v", series, max_series_per_aggr=bad)


def test_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; loud-failure path not applicable")
    try:
        engine.init()  # the library's own view of the machine
    except engine.VmGpuError:
        pass
    else:
        pytest.skip("GPU present; loud-failure path not applicable")
    with pytest.raises(engine.VmGpuError):
        engine.aggr_count_values(*_good())
    series = [Series(MetricName(b"m", [(b"s", b"%d" % i)]), np.ones(4))
              for i in range(3)]
    with pytest.raises(engine.VmGpuError):
        aggregate.count_values_device("v", series)
    # the C ABI itself, never initialised in this process
    lib = ctypes.CDLL(LIB)
    errbuf = ctypes.create_string_buffer(256)
    rc = lib.vmgpu_aggr_count_values_fetch(None, None, None, errbuf,
                                           ctypes.c_size_t(len(errbuf)))
    assert rc != 0 and b"not initialized" in errbuf.value
    n_rows = ctypes.c_uint64(0)
    rc = lib.vmgpu_aggr_count_values_exec(
        None, ctypes.c_uint32(0), ctypes.c_int32(1), None, None,
        ctypes.c_uint32(0), ctypes.c_uint32(10), ctypes.byref(n_rows), errbuf,
        ctypes.c_size_t(len(errbuf)))
    assert rc != 0 and b"not initialized" in errbuf.value
