"""transform_series_kernel and the elementwise kernel (csrc/transform.hip) on
the class batches of matrix_classes.py, and with more rows than either
launches threads.

The series functions and the clamp family are held to the C oracle (equal
bits, NaN payloads aside) and to the plain reference of matrix_reference.py
(equal values, -0.0 == 0.0).  The arithmetic-only one-argument functions are
held to the oracle by bits, the libm ones at rtol 1e-12 as in
test_gpu_transform.py.  test_matrix_class_inputs.py shows on the CPU that the
inputs are not trivial.

range_mad and range_trim_outliers shared the mad error of the column
aggregates: a row with an infinite median, such as [+Inf, 1, +Inf, 2], gave
NaN and now gives +Inf, as the reference's mad() does.
"""
import math

import numpy as np
import pytest

import oracle
import matrix_classes as mc
import matrix_reference as mr
from victoriametrics_amd import transform as tf

pytestmark = pytest.mark.gpu

NAN = mc.NAN

EXACT_ELEMENTWISE = ["abs", "ceil", "floor", "sqrt", "deg", "rad", "sgn"]
ULP_FUNCS = ["exp", "ln", "log2", "log10", "sin", "cos", "tan", "asin",
             "acos", "atan", "sinh", "cosh", "tanh", "asinh", "acosh",
             "atanh"]


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


def _case_id(case):
    return "-".join(str(c) for c in case)


def _device(func, values, scalar=0.0):
    """(values, keep) of one series function on the device."""
    n_grid = values.shape[1]
    args = [mc.smoothing_factors(n_grid)] if func == "smooth_exponential" else ()
    out = tf.transform(func, values.copy(), ts=mc.transform_ts(n_grid),
                       args=args, scalar=scalar)
    if func == "range_normalize":
        return out
    return out, np.ones(values.shape[0], np.uint8)


# ---- every series function on every class batch ------------------------------

@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("case", mc.TRANSFORM_CASES, ids=_case_id)
def test_series_func_on_class(case, kind):
    func, scalar = case
    for n_grid in mc.TRANSFORM_N_GRIDS:
        got, keep = _device(func, mc.transform_batch(kind, n_grid), scalar)
        ref, rkeep = mc.oracle_transform(func, scalar, kind, n_grid)
        plain, pkeep = mc.plain_transform(func, scalar, kind, n_grid)
        context = f"{func} {scalar} {kind} n_grid={n_grid}"
        np.testing.assert_array_equal(keep, rkeep, err_msg=context)
        np.testing.assert_array_equal(keep, pkeep, err_msg=context)
        _assert_bits(got, ref, context)
        _assert_same(got, plain, context)


def test_range_mad_of_an_infinite_median():
    row = np.asarray([[math.inf, 1.0, math.inf, 2.0]])
    assert (tf.transform("range_mad", row.copy()) == math.inf).all()
    # nothing is further than 3 * Inf from the median: the row stays
    out = tf.transform("range_trim_outliers", row.copy(), scalar=3.0)
    ref, _ = oracle.tf_apply(mc.series_func_id("range_trim_outliers"),
                             row.copy(), scalar=3.0)
    _assert_bits(out, ref, "range_trim_outliers")
    _assert_same(out, mr.transform("range_trim_outliers", row, scalar=3.0)[0],
                 "range_trim_outliers")


# ---- the elementwise kernel ---------------------------------------------------

@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("func", mc.CLAMP_FUNCS)
def test_clamp_on_class(func, kind):
    for n_grid in mc.TRANSFORM_N_GRIDS:
        lo, hi = mc.clamp_bounds(n_grid)
        args = {"clamp": [lo, hi], "clamp_min": [lo], "clamp_max": [hi]}[func]
        got = tf.transform(func, mc.transform_batch(kind, n_grid).copy(),
                           args=args)
        context = f"{func} {kind} n_grid={n_grid}"
        _assert_bits(got, mc.oracle_clamp(func, kind, n_grid), context)
        _assert_same(got, mc.plain_clamp(func, kind, n_grid), context)


@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("func", EXACT_ELEMENTWISE)
def test_elementwise_exact_on_class(func, kind):
    v = mc.transform_batch(kind, 64)
    exp, _ = oracle.tf_apply(tf._ELEMENTWISE[func], v.copy())
    _assert_bits(tf.transform(func, v.copy()), exp, f"{func} {kind}")


@pytest.mark.parametrize("kind", mc.KINDS)
@pytest.mark.parametrize("func", ULP_FUNCS)
def test_elementwise_libm_on_class(func, kind):
    """-0.0, 1e15, the infinities and the domain edges (ln 0, atanh 1,
    acosh below 1) of device libm against glibc."""
    v = mc.transform_batch(kind, 64)
    exp, _ = oracle.tf_apply(tf._ELEMENTWISE[func], v.copy())
    got = tf.transform(func, v.copy())
    context = f"{func} {kind}"
    assert np.array_equal(np.isnan(got), np.isnan(exp)), context
    inf = np.isinf(exp)
    assert np.array_equal(got[inf], exp[inf]), context
    fin = np.isfinite(exp)
    np.testing.assert_allclose(got[fin], exp[fin], rtol=1e-12, atol=1e-300,
                               err_msg=context)


# ---- launch shapes ------------------------------------------------------------

N_ROWS = mc.WIDE_MAX_THREADS + 1


def _tiled_rows():
    small = mc.transform_batch("inf", 2)
    reps = -(-N_ROWS // len(small))
    return small, reps, np.tile(small, (reps, 1))[:N_ROWS]


@pytest.mark.parametrize("func", ["range_mad", "running_sum"])
def test_series_kernel_second_trip(func):
    """More rows than transform_series_kernel launches threads; range_mad
    sorts in its scratch row, running_sum scans."""
    small, reps, v = _tiled_rows()
    assert v.shape == (1_048_577, 2)
    assert v.shape[0] > mc.WIDE_MAX_THREADS
    assert v.nbytes < 40e6
    got = tf.transform(func, v.copy())
    plain, _ = mc.plain_transform(func, 0.0, "inf", 2)
    _assert_same(got, np.tile(plain, (reps, 1))[:N_ROWS], f"{func} tiled")
    ref, _ = oracle.tf_apply(mc.series_func_id(func), v.copy())
    _assert_bits(got, ref, func)


def test_elementwise_kernel_second_trip():
    small, reps, v = _tiled_rows()
    assert v.size > mc.WIDE_MAX_THREADS
    assert v.shape == (1_048_577, 2)
    lo, hi = mc.clamp_bounds(2)
    got = tf.transform("clamp", v.copy(), args=[lo, hi])
    plain = mc.plain_clamp("clamp", "inf", 2)
    assert mr.same_arrays(plain, small).mean() > 0.1      # it does clamp
    _assert_same(got, np.tile(plain, (reps, 1))[:N_ROWS], "clamp tiled")
    ref, _ = oracle.tf_apply(mc.series_func_id("clamp"), v.copy(), arg1=lo,
                             arg2=hi)
    _assert_bits(got, ref, "clamp")
