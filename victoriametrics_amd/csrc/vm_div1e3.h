/* vm_div1e3.h — exact x / 1e3 without a division, for small integers.
 *
 * For every integer-valued double x with |x| < 2^32,
 *
 *     q  = x * 0.001
 *     r  = fma(-q, 1e3, x)        (exact residual of the first guess)
 *     q' = fma(r, 0.001, q)
 *
 * equals the correctly rounded x / 1e3 bit for bit (checked exhaustively
 * over the whole range by tests/test_div1e3_host.py; the bare multiply alone
 * is off by one ulp for about one x in seven).  The sequence is odd in x, so
 * the negative half follows from the positive one.  (-0.0, which no integer
 * converts to, would come back as +0.0.)
 *
 * Plain C/C++: the rate evaluator (vmgpu.hip) and the host check compile this
 * very expression.  The FMAs are explicit builtins because the engine is
 * built with -ffp-contract=off.
 */
#ifndef VM_DIV1E3_H
#define VM_DIV1E3_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VM_DIV1E3_FN static __host__ __device__ __forceinline__
#else
#define VM_DIV1E3_FN static inline
#endif

/* x must be integer-valued with |x| < 2^32. */

VM_DIV1E3_FN double vm_div1e3_small(double x) {
  double q = x * 0.001;
  double r = __builtin_fma(-q, 1e3, x);
  return __builtin_fma(r, 0.001, q);
}

#endif /* VM_DIV1E3_H */
