"""hstat_kernel, hshare_kernel and hq_kernel (csrc/hstat.hip) on the
histogram class batch of matrix_classes.py, and with more outputs than they
launch threads.

Integer counts with plateaus, leading zero buckets, NaN and broken buckets;
groups of 0 les, +Inf only, one finite le, a duplicated le and no +Inf
bucket; a per-point le_req that hits les exactly.
test_matrix_class_inputs.py shows on the CPU that the batch takes every
branch of the three walks (bar the plateau exit of histogram_quantile, which
cannot be taken) and that the outputs are not trivial.  The device is held to
the C oracle (equal bits, NaN payloads aside) and to the restated walks of
matrix_reference.py (equal values, -0.0 == 0.0).
"""
import numpy as np
import pytest

import oracle
import matrix_classes as mc
import matrix_reference as mr

pytestmark = pytest.mark.gpu

NAN = mc.NAN

HIST_CASES = ([("stat", m) for m in mc.HSTAT_MODES] + [("share", None)]
              + [("quantile", phi) for phi in mc.HQ_PHIS])


@pytest.fixture(scope="module")
def engine():
    from victoriametrics_amd import engine as e
    e.init()
    return e


def _bits(a):
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = NAN
    return a.view(np.int64)


def _assert_bits(got, exp, context):
    bad = _bits(got) != _bits(exp)
    assert not bad.any(), (f"{context}: {int(bad.sum())} differ from the "
                           f"oracle, first at {np.argwhere(bad)[0]}: "
                           f"{got[bad][0]!r} != {exp[bad][0]!r}")


def _assert_same(got, exp, context):
    bad = mr.same_arrays(got, exp)
    assert not bad.any(), (f"{context}: {int(bad.sum())} differ from the "
                           f"plain reference, first at {np.argwhere(bad)[0]}: "
                           f"{got[bad][0]!r} != {exp[bad][0]!r}")


def _device(engine, name, arg, bv, les, offsets, req):
    if name == "stat":
        return (engine.histogram_stat(arg, bv, les, offsets),)
    if name == "share":
        return engine.histogram_share(req, bv, les, offsets, bounds=True)
    return engine.histogram_quantile(arg, bv, les, offsets, bounds=True)


def _oracle(name, arg, bv, les, offsets, req):
    if name == "stat":
        return (oracle.histogram_stat(mc.HSTAT_MODES.index(arg), bv, les,
                                      offsets),)
    if name == "share":
        return oracle.histogram_share(req, bv, les, offsets)
    return oracle.histogram_quantile(arg, bv, les, offsets, bounds=True)


@pytest.mark.parametrize("case", HIST_CASES,
                         ids=lambda c: "-".join(str(x) for x in c))
def test_hist_on_class(engine, case):
    got = _device(engine, *case, *mc.hist_batch(), mc.hist_le_req())
    ref = mc.oracle_hist(*case)
    plain, _ = mc.plain_hist(*case)
    for i, (g, r, p) in enumerate(zip(got, ref, plain)):
        _assert_bits(g, r, f"{case} output {i}")
        _assert_same(g, p, f"{case} output {i}")


N_TILES = 2731      # 8193 groups of 3 les x 128 points


@pytest.mark.parametrize("case", [("stat", "stddev"), ("share", None),
                                  ("quantile", 0.5)],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_hist_second_trip(engine, case):
    bv, les, offsets, req = mc.tile_hist(N_TILES)
    n_groups = len(offsets) - 1
    assert n_groups == 8193 and bv.shape == (3 * 8193, 128)
    assert n_groups * bv.shape[1] > mc.WIDE_MAX_THREADS
    assert bv.nbytes < 40e6
    got = _device(engine, *case, bv, les, offsets, req)
    s_bv, s_les, s_off, _ = mc.hist_small()
    small = _oracle(*case, s_bv, s_les, s_off, req)
    full = _oracle(*case, bv, les, offsets, req)
    for i, (g, s, f) in enumerate(zip(got, small, full)):
        if i == 0:      # the small batch is no constant either
            assert len(np.unique(s[np.isfinite(s)])) >= 8, case
        _assert_bits(g, np.tile(s, (N_TILES, 1)), f"{case} output {i} tiled")
        _assert_bits(g, f, f"{case} output {i}")
