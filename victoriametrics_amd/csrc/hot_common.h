/* What the sparse multi-series rollups share: hot.hip (histogram_over_time)
 * and cvot.hip (count_values_over_time) both mark, scan and count over a
 * resident batch, one wavefront per series, on the same grid arithmetic and
 * with the same batch-owned grow-only buffers. */
#ifndef VMGPU_HOT_COMMON_H
#define VMGPU_HOT_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_common.h"

#define HOT_WAVE 64
#define HOT_BLOCK_THREADS 256
#define HOT_WAVES_PER_BLOCK (HOT_BLOCK_THREADS / HOT_WAVE)
#define HOT_MAX_BLOCKS 4096
#define HOT_STALE_NAN_BITS 0x7FF0000000000002ULL
#define HOT_NAN_BITS 0x7FF8000000000000ULL

struct HotParams {
  int64_t start, step, window;
  int32_t n_grid;
  int32_t drop_stale;
};

#define HOT_DEV __device__ __forceinline__
#define HOT_MIN(a, b) ((a) < (b) ? (a) : (b))
#define HOT_MAX(a, b) ((a) > (b) ? (a) : (b))

/* one wavefront's LDS phase barrier: DS ops are lgkm-counted and issue in
 * order, so waiting them out (plus the compiler barrier) gives cross-lane
 * visibility inside the wave without a workgroup barrier */
static HOT_DEV void hot_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

/* Clamped grid range [g0, g1] of a sample; false when it is in no window.
 * True floor division for negative numerators; 32-bit divides when the
 * operands fit (the common case: ts within +-24 days of start). */
static HOT_DEV bool hot_grid_range(const HotParams& p, int64_t ts,
                                   int32_t& g0, int32_t& g1) {
  int64_t a = ts - p.start;
  int64_t q, r;
  if (a >= 0 && a <= 0xFFFFFFFFLL && p.step <= 0xFFFFFFFFLL) {
    uint32_t qq = (uint32_t)a / (uint32_t)p.step;
    q = qq;
    r = a - (int64_t)qq * p.step;
  } else {
    q = a / p.step;
    r = a - q * p.step;
    if (r < 0) { q -= 1; r += p.step; }
  }
  /* now a = q*step + r, 0 <= r < step */
  int64_t lo = q + (r > 0 ? 1 : 0);
  uint64_t x = (uint64_t)r + (uint64_t)(p.window - 1);
  int64_t hi = q + (int64_t)((x <= 0xFFFFFFFFULL && p.step <= 0xFFFFFFFFLL)
                                 ? (uint64_t)((uint32_t)x / (uint32_t)p.step)
                                 : x / (uint64_t)p.step);
  if (lo < 0) lo = 0;
  if (hi > (int64_t)p.n_grid - 1) hi = (int64_t)p.n_grid - 1;
  if (lo > hi) return false;
  g0 = (int32_t)lo;
  g1 = (int32_t)hi;
  return true;
}

/* hot.hip: exclusive scan of row_counts[n] into row_start[n + 1] on stream
 * st (hot_scan_kernel; the library is built without relocatable device
 * code, so other files reach the kernel through this launcher) */
void hot_scan_launch(const uint32_t* row_counts, uint32_t n,
                     uint64_t* row_start, hipStream_t st);

/* hot.hip: the device copy of the table vmgpu_vmrange_thresholds_set
 * uploaded (VMRANGE_TABLE_PAD doubles, NaN-padded), NULL before the first
 * upload.  The caller holds the context lock. */
const double* vm_hot_thresholds(void);

/* Grow-only reservation with plain hipMalloc.  Deliberately NOT the
 * stream-ordered pool of devalloc.h: the result size changes from call to
 * call, and a free-then-larger-malloc cycle through the pool right before
 * the kernels run is the one pattern under which a result came back with a
 * zero-filled hole (see profiles/histogram_over_time.md).  These buffers
 * live as long as the batch, so allocation cost is paid once. */
template <class T>
inline hipError_t hot_reserve(T** p, size_t* cap, size_t bytes) {
  if (*p && *cap >= bytes) return hipSuccess;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  hipError_t e = hipMalloc((void**)p, bytes);
  if (e == hipSuccess) *cap = bytes;
  return e;
}

#endif
