/* vmrange bucket classifier (metrics.Histogram.Update, histogram.go:88).
 *
 * The host reference (aggregate._histogram_update) computes
 * (log10(v) + 9) * 18 and decrements exact-integer results, which no device
 * log10 reproduces bit-for-bit.  It is, however, a monotone step function of
 * v with 487 steps, so the device classifies by table lookup: thr[j] is the
 * smallest double whose code is >= j + 1, built ONCE on the host from the
 * reference's own arithmetic (rollup_multi.vmrange_bucket_thresholds) and
 * uploaded.  code(v) = #{ j : thr[j] <= v }.
 *
 * Codes: 0 = lower, 1..486 = bucket idx 0..485, 487 = upper; NaN and v < 0
 * contribute nothing (VMRANGE_CODE_NONE).  488 codes => a presence mask is
 * 16 x u32.
 */
#ifndef VMGPU_VMRANGE_BUCKET_H
#define VMGPU_VMRANGE_BUCKET_H

#include <stdint.h>

#define VMRANGE_N_THRESHOLDS 487
#define VMRANGE_N_CODES 488
#define VMRANGE_MASK_WORDS 16
#define VMRANGE_CODE_NONE 0xFFFFu
/* the table is padded with NaN to a power of two so the search below needs
 * no bounds test: `NaN <= v` is false, i.e. a pad sorts above every value,
 * +Inf included */
#define VMRANGE_TABLE_PAD 512

#if defined(__HIPCC__)
#define VMRANGE_FN __host__ __device__ __forceinline__
#else
#define VMRANGE_FN static inline
#endif

/* thr: VMRANGE_TABLE_PAD doubles (LDS on the device).  Branchless 9-step
 * lower-bound search; the code of v when v is neither NaN nor negative (0
 * for those, to be discarded by the caller).  On its own for callers that
 * run several searches side by side. */
VMRANGE_FN uint32_t vmrange_bucket_search(const double* thr, double v) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t step = VMRANGE_TABLE_PAD / 2; step; step >>= 1)
    pos += (thr[pos + step - 1] <= v) ? step : 0;
  return pos;
}

VMRANGE_FN uint32_t vmrange_bucket_code(const double* thr, double v) {
  if (v != v || v < 0) return VMRANGE_CODE_NONE; /* -0.0 is not < 0 */
  return vmrange_bucket_search(thr, v);
}

#endif /* VMGPU_VMRANGE_BUCKET_H */
