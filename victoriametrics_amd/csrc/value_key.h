/* Rows keyed on a double's value: the order key, the bitonic sort and the
 * search that cvot.hip (count_values_over_time, per series) and aggrcv.hip
 * (the count_values() aggregate, per group) share.  aggrtopk.hip (grouped
 * topk) uses the sort and the size classes with a key of its own.
 *
 * Order key of value bits u (all NaNs first folded to HOT_NAN_BITS):
 *   (u >> 63) ? ~u : u | 1 << 63
 * unsigned-ascending = -Inf ... -0 < 0 ... +Inf < NaN.  The largest real key
 * is NaN's 0xFFF8000000000000, so all-ones is free for CVOT_KEY_NONE, which
 * sorts behind every row.
 *
 * The sort is the normalised bitonic network: every comparator orders its
 * pair ascending, so an index >= n can stand for +max without being stored
 * (such a comparator never moves anything) and n needs no padding.
 */
#ifndef VMGPU_VALUE_KEY_H
#define VMGPU_VALUE_KEY_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hot_common.h"

/* one wave sorts this many keys in a 2 KiB slab: 8 KiB a workgroup, so LDS
 * never limits the short class's occupancy; covers the 240-sample shape */
#define CVOT_WAVE_CAP 256
/* one workgroup sorts this many keys in 16 KiB of LDS: eight such
 * workgroups, the CU's 32 waves, still fit its 160 KiB */
#define CVOT_BLOCK_CAP 2048
#define CVOT_KEY_NONE 0xFFFFFFFFFFFFFFFFULL

static HOT_DEV uint64_t cvot_order_key(double v) {
  uint64_t u = (uint64_t)__double_as_longlong(v);
  if (v != v) u = HOT_NAN_BITS;
  return (u >> 63) ? ~u : (u | (1ULL << 63));
}

static HOT_DEV double cvot_key_value(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k ^ (1ULL << 63)) : ~k;
  return __longlong_as_double((long long)u);
}

template <bool WAVE>
static HOT_DEV void cvot_sync() {
  if (WAVE) hot_wave_sync();
  else __syncthreads();
}

static HOT_DEV void cvot_cmpxchg(uint64_t* keys, uint64_t a, uint64_t b) {
  const uint64_t x = keys[a], y = keys[b];
  if (x > y) {
    keys[a] = y;
    keys[b] = x;
  }
}

/* Ascending sort of keys[0..n) by nthr cooperating threads (one wave on its
 * slab, or one workgroup on LDS or global memory).  The caller has made
 * keys visible; the sort ends on a sync.  All trip counts are uniform. */
template <bool WAVE>
static HOT_DEV void cvot_sort(uint64_t* keys, uint64_t n, uint32_t tid,
                              uint32_t nthr) {
  if (n < 2) return;
  uint64_t P = 2;
  while (P < n) P <<= 1;
  const uint64_t pairs = P >> 1;
  for (uint64_t k = 2; k <= P; k <<= 1) {
    const uint64_t half = k >> 1;
    /* flip: pair x of a k-block meets its mirror image k-1-x */
    for (uint64_t t = tid; t < pairs; t += nthr) {
      const uint64_t a = ((t & ~(half - 1)) << 1) | (t & (half - 1));
      const uint64_t b = a ^ (k - 1);
      if (b < n) cvot_cmpxchg(keys, a, b);
    }
    cvot_sync<WAVE>();
    for (uint64_t j = half >> 1; j; j >>= 1) {
      for (uint64_t t = tid; t < pairs; t += nthr) {
        const uint64_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint64_t b = a | j;
        if (b < n) cvot_cmpxchg(keys, a, b);
      }
      cvot_sync<WAVE>();
    }
  }
}

/* first index in sorted keys[0..R) whose key is not below key */
static HOT_DEV uint32_t cvot_lower_bound(const uint64_t* keys, uint32_t R,
                                         uint64_t key) {
  uint32_t lo = 0, hi = R;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

#endif
