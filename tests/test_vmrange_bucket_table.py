"""The vmrange threshold table behind the device histogram_over_time
classifier (rollup_multi.vmrange_bucket_thresholds, csrc/vmrange_bucket.h).

The device never calls log10: it counts the thresholds <= v.  These tests
pin that this lookup is, for every double tried, the class the host function
aggregate._histogram_update assigns — 0 = lower, 1..486 = bucket idx 0..485,
487 = upper, None = contributes nothing.  No GPU needed."""
import math

import numpy as np
import pytest

from victoriametrics_amd.aggregate import _histogram_update
from victoriametrics_amd.rollup_multi import (vmrange_bucket_thresholds,
                                              vmrange_code_lookup)


def _host_code(v):
    b = {}
    _histogram_update(b, float(v))
    if not b:
        return None
    ((key, count),) = b.items()
    assert count == 1
    if key == "lower":
        return 0
    if key == "upper":
        return 487
    return key + 1


@pytest.fixture(scope="module")
def thr():
    return vmrange_bucket_thresholds()


def test_table_shape(thr):
    assert thr.dtype == np.float64 and thr.shape == (487,)
    assert np.all(thr > 0) and np.all(np.isfinite(thr))
    assert np.all(np.diff(thr) > 0)
    # strictly increasing as bit patterns too (positive doubles)
    assert np.all(np.diff(thr.view(np.uint64).astype(np.int64)) > 0)


def test_lookup_matches_host_around_every_threshold(thr):
    bits = thr.view(np.uint64).astype(np.int64)
    for k in range(487):
        around = (bits[k] + np.arange(-64, 65)).astype(np.uint64)
        vs = around.view(np.float64)
        for v in vs:
            assert vmrange_code_lookup(v, thr) == _host_code(v), (k, float(v).hex())
        # the threshold is the first double of class k + 1
        assert _host_code(vs[64]) == k + 1
        assert _host_code(vs[63]) == k


def test_lookup_matches_host_log_uniform(thr):
    rng = np.random.default_rng(20240611)
    vs = 10.0 ** rng.uniform(-11.0, 20.0, 100_000)
    got = np.searchsorted(thr, vs, side="right")
    want = np.fromiter((_host_code(v) for v in vs), dtype=np.int64, count=len(vs))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(vs[i]).hex(), got[i], want[i]) for i in bad[:5]]
    assert want.min() == 0 and want.max() == 487  # both tails exercised


def test_lookup_special_values(thr):
    specials = [0.0, -0.0, 5e-324, 1e-9, 1e19, math.inf]
    specials += [float("1e%d" % n) for n in range(-9, 19)]
    for v in specials:
        assert vmrange_code_lookup(v, thr) == _host_code(v), v
    assert vmrange_code_lookup(0.0, thr) == 0
    assert vmrange_code_lookup(-0.0, thr) == 0
    assert vmrange_code_lookup(5e-324, thr) == 0
    assert vmrange_code_lookup(1e-9, thr) == 1          # bucket 0
    for n in range(-8, 18):                              # 10^n -> 18(n+9)-1
        assert vmrange_code_lookup(float("1e%d" % n), thr) == 18 * (n + 9)
    assert vmrange_code_lookup(1e18, thr) == 487
    assert vmrange_code_lookup(1e19, thr) == 487
    assert vmrange_code_lookup(math.inf, thr) == 487
    # the run of doubles above 1.0 whose log10 product is an exact integer
    assert vmrange_code_lookup(1.0000000000000020, thr) == 162
    assert vmrange_code_lookup(1.0000000000000022, thr) == 163
    for v in (math.nan, -1.0, -5e-324, -math.inf):
        assert vmrange_code_lookup(v, thr) is None
        assert _host_code(v) is None


def test_batch_histogram_over_time_fails_loudly_without_device():
    """SeriesBatch.histogram_over_time has no CPU fallback: with no device
    (or, on a GPU box, with no such batch) it raises VmGpuError."""
    import os
    import subprocess
    from conftest import REPO_ROOT
    from victoriametrics_amd import engine
    pkg = os.path.join(REPO_ROOT, "victoriametrics_amd")
    if not os.path.exists(os.path.join(pkg, "libvmgpu.so")):
        subprocess.run(["sh", "build.sh"], cwd=os.path.join(pkg, "csrc"),
                       check=True)
    batch = object.__new__(engine.SeriesBatch)
    batch.handle = 0
    batch.n_series = 1
    batch._perm = None
    with pytest.raises(engine.VmGpuError):
        batch.histogram_over_time(0, 100, 10, 50)
