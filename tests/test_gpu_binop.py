"""GPU binary-operator kernels vs the oracle, bit-exact: the elementwise
pair kernel over all 18 ops (+ bool modifier, fills, dropNaNRight), the
set-op mask kernel, the `or` merge-walk kernel, and the full host dispatch
run GPU-vs-oracle on identical inputs."""
import math
import zlib

import numpy as np
import pytest

import oracle
from victoriametrics_amd import engine
from victoriametrics_amd.binary_op import BinOpSpec, Series, binary_op_eval
from victoriametrics_amd.metric_name import MetricName

pytestmark = pytest.mark.gpu

NAN = math.nan
ALL_OPS = ["+", "-", "*", "/", "%", "^", "atan2", "==", "!=", ">", "<",
           ">=", "<=", "default", "if", "ifnot", "and", "or"]


def _rand(rng, n, nan_frac=0.2):
    v = rng.standard_normal(n) * 100
    v[rng.random(n) < nan_frac] = NAN
    return v


# pow/atan2 are software transcendentals: the device (OCML) and host
# (glibc, and Go's own FDLIBM ports) implementations legitimately differ in
# the last ulps.  The reference's own tests compare these with tolerance
# (exec_test.go timeseriesEqual); everything else is bit-exact.
ULP_OPS = {"^", "atan2"}


def _assert_op_equal(op, got, exp, msg):
    if op in ULP_OPS:
        both_nan = np.isnan(got) & np.isnan(exp)
        np.testing.assert_allclose(got[~both_nan], exp[~both_nan],
                                   rtol=1e-12, atol=0, err_msg=msg)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), msg
    else:
        np.testing.assert_array_equal(got.view(np.int64), exp.view(np.int64),
                                      err_msg=msg)


@pytest.mark.parametrize("op", ALL_OPS)
@pytest.mark.parametrize("is_bool", [False, True])
def test_pairs_kernel_all_ops(op, is_bool):
    if is_bool and op not in ("==", "!=", ">", "<", ">=", "<="):
        pytest.skip("bool modifier only applies to comparisons")
    rng = np.random.default_rng(zlib.crc32(op.encode()))
    n_pairs, n_grid = 37, 240
    a = np.stack([_rand(rng, n_grid) for _ in range(n_pairs)])
    b = np.stack([_rand(rng, n_grid) for _ in range(n_pairs)])
    from victoriametrics_amd.binary_op import OP_IDS
    got = engine.binop_eval(OP_IDS[op], is_bool, False, a,
                            np.arange(n_pairs, dtype=np.uint32), b,
                            np.arange(n_pairs, dtype=np.uint32))
    for p in range(n_pairs):
        exp = oracle.binop_apply(op, a[p], b[p], is_bool=is_bool)
        _assert_op_equal(op, got[p], exp, f"{op} bool={is_bool} row {p}")


def test_pairs_kernel_fills_and_dropnan():
    rng = np.random.default_rng(7)
    a = np.stack([_rand(rng, 100) for _ in range(8)])
    b = np.stack([_rand(rng, 100) for _ in range(8)])
    idx = np.arange(8, dtype=np.uint32)
    from victoriametrics_amd.binary_op import OP_IDS
    for fl, fr, dnr in [(None, 5.0, False), (3.0, None, False),
                        (1.0, 2.0, False), (None, None, True),
                        (None, 9.0, True)]:
        got = engine.binop_eval(OP_IDS[">"], False, dnr, a, idx, b, idx,
                                fill_left=fl, fill_right=fr)
        for p in range(8):
            exp = oracle.binop_apply(">", a[p], b[p], drop_nan_right=dnr,
                                     fill_left=fl, fill_right=fr)
            np.testing.assert_array_equal(got[p].view(np.int64),
                                          exp.view(np.int64))


def test_pairs_kernel_idx_indirection():
    # scalar broadcast: all pairs read the same right row
    rng = np.random.default_rng(8)
    a = np.stack([_rand(rng, 50) for _ in range(6)])
    b = _rand(rng, 50)[None, :]
    from victoriametrics_amd.binary_op import OP_IDS
    got = engine.binop_eval(OP_IDS["+"], False, False, a,
                            np.arange(6, dtype=np.uint32), b,
                            np.zeros(6, dtype=np.uint32))
    for p in range(6):
        exp = oracle.binop_apply("+", a[p], b[0])
        np.testing.assert_array_equal(got[p].view(np.int64),
                                      exp.view(np.int64))


def S(name, tags, values):
    return Series(MetricName(name, tags), np.asarray(values, np.float64))


def _mk_series(rng, n_series, n_grid, name="m", extra=()):
    out = []
    for i in range(n_series):
        out.append(S(name, [("pod", f"p{i}"), *extra],
                     _rand(rng, n_grid)))
    return out


def _oracle_fns():
    """test-infra executors mirroring the Go loops (same as the CPU tests)"""
    from victoriametrics_amd.binary_op import (OP_IDS, MASK_AND, MASK_UNLESS,
                                               MASK_DEFAULT)

    def apply_fn(spec, left, right, dst, drop_nan_right):
        for tl, tr, td in zip(left, right, dst):
            td.values = oracle.binop_apply(
                OP_IDS[spec.op], tl.values, tr.values,
                is_bool=spec.bool_modifier, drop_nan_right=drop_nan_right,
                fill_left=spec.fill_left, fill_right=spec.fill_right)
        return dst

    def mask_fn(mode, lrows, lgroup, grows, goff):
        for t, gi in zip(lrows, lgroup):
            rights = grows[goff[gi]:goff[gi + 1]]
            for i in range(len(t.values)):
                has = any(not math.isnan(r.values[i]) for r in rights)
                if mode == MASK_AND and not has:
                    t.values[i] = NAN
                elif mode == MASK_UNLESS and has:
                    t.values[i] = NAN
                elif mode == MASK_DEFAULT and math.isnan(t.values[i]):
                    for r in rights:
                        if not math.isnan(r.values[i]):
                            t.values[i] = r.values[i]
                            break

    def or_fn(groups):
        for tss_left, tss_right, cm in groups:
            for li, tl in enumerate(tss_left):
                for i in range(len(tl.values)):
                    left_nan = math.isnan(tl.values[i])
                    for ri, tr in enumerate(tss_right):
                        mergeable = bool(cm[li, ri])
                        if left_nan and mergeable:
                            tl.values[i] = tr.values[i]
                        if not left_nan or mergeable:
                            tr.values[i] = NAN

    return apply_fn, mask_fn, or_fn


def _compare_results(gpu_out, cpu_out):
    assert len(gpu_out) == len(cpu_out)
    gm = {t.mn.marshal_sorted(): t.values for t in gpu_out}
    cm = {t.mn.marshal_sorted(): t.values for t in cpu_out}
    assert sorted(gm) == sorted(cm)
    for k in gm:
        np.testing.assert_array_equal(gm[k].view(np.int64),
                                      np.asarray(cm[k]).view(np.int64),
                                      err_msg=repr(k))


def _clone(tss):
    return [Series(t.mn.copy(), t.values.copy()) for t in tss]


@pytest.mark.parametrize("op", ["+", "/", ">", "and", "or", "unless", "if",
                                "ifnot", "default"])
def test_full_dispatch_gpu_vs_oracle(op):
    rng = np.random.default_rng(11)
    left = _mk_series(rng, 23, 120, "a")
    right = _mk_series(rng, 17, 120, "b")  # partial key overlap
    spec = BinOpSpec(op)
    a_fn, m_fn, o_fn = _oracle_fns()
    exp = binary_op_eval(spec, _clone(left), _clone(right),
                         apply_fn=a_fn, mask_fn=m_fn, or_fn=o_fn)
    got = binary_op_eval(BinOpSpec(op), _clone(left), _clone(right))
    _compare_results(got, exp)


def test_full_dispatch_group_left_gpu():
    rng = np.random.default_rng(12)
    left = [S("req", [("pod", f"p{i}"), ("node", f"n{i % 3}")],
              _rand(rng, 64)) for i in range(12)]
    right = [S("info", [("node", f"n{j}")], _rand(rng, 64, 0.05))
             for j in range(3)]
    spec = dict(group_op="on", group_tags=["node"], join_op="group_left")
    a_fn, m_fn, o_fn = _oracle_fns()
    exp = binary_op_eval(BinOpSpec("*", **spec), _clone(left), _clone(right),
                         apply_fn=a_fn, mask_fn=m_fn, or_fn=o_fn)
    got = binary_op_eval(BinOpSpec("*", **spec), _clone(left), _clone(right))
    _compare_results(got, exp)


def test_or_merge_walk_gpu():
    # mergeable names in the same key group exercise binop_or_kernel's
    # consume-and-fill order
    rng = np.random.default_rng(13)
    left, right = [], []
    for i in range(9):
        v = _rand(rng, 80, 0.5)
        w = _rand(rng, 80, 0.3)
        left.append(S("m", [("pod", f"p{i}")], v))
        right.append(S("m", [("pod", f"p{i}")], w))
    a_fn, m_fn, o_fn = _oracle_fns()
    exp = binary_op_eval(BinOpSpec("or"), _clone(left), _clone(right),
                         apply_fn=a_fn, mask_fn=m_fn, or_fn=o_fn)
    got = binary_op_eval(BinOpSpec("or"), _clone(left), _clone(right))
    _compare_results(got, exp)


def test_histogram_quantile_pipeline_on_device():
    """End-to-end §8f(3) motivation: rate -> sum by (le) -> ratio with
    binop divide, all sample math on device."""
    from victoriametrics_amd import synth
    from victoriametrics_amd.engine import RollupPlan, SeriesBatch
    n_series, n_samples = 256, 120
    ts, vals, offsets = synth.counter_batch(n_series, n_samples,
                                            1_000_000_000_000)
    start = int(ts[0]) + 60_000
    plan = RollupPlan("rate", start, start + 30 * 15_000, 15_000,
                      window=300_000)
    batch = SeriesBatch(ts, vals, offsets)
    grid, _, _ = batch.exec(plan)
    n_grid = grid.shape[1]
    # a / (a + 1) ratio via the binop kernel
    from victoriametrics_amd.binary_op import OP_IDS
    ones = np.ones_like(grid)
    s = engine.binop_eval(OP_IDS["+"], False, False, grid,
                          np.arange(n_series, dtype=np.uint32), ones,
                          np.arange(n_series, dtype=np.uint32))
    ratio = engine.binop_eval(OP_IDS["/"], False, False, grid,
                              np.arange(n_series, dtype=np.uint32), s,
                              np.arange(n_series, dtype=np.uint32))
    exp = grid / (grid + 1.0)
    np.testing.assert_allclose(ratio, exp, rtol=0, atol=0)
