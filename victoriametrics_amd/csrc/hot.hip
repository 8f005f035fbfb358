/* hot.hip — histogram_over_time (rollupHistogram, rollup.go:1525) on the
 * device, over a resident batch.
 *
 * The function emits a DATA-DEPENDENT number of rows per series (one per
 * vmrange bucket that is non-zero at some grid point), so it does not fit
 * the one-value-per-(series, grid point) contract of the rollup kernels.
 * This file adds the sparse contract as two passes over the batch's
 * resident columns, one wavefront per series in both:
 *
 *   hot_mark_kernel   classifies every sample (vmrange_bucket.h), ORs the
 *       code into the series' 488-bit presence mask, sums samples_scanned
 *       as the clamped grid-range length of every in-window sample, caches
 *       the code as u16 (VMRANGE_CODE_NONE = contributes nothing), and
 *       emits the per-series row count = popcount(mask).
 *   hot_scan_kernel   exclusive scan of the row counts -> first output row
 *       of every series, and the total n_rows.
 *   hot_count_kernel  per series, a +-1 difference array per row in LDS
 *       (tiled over the grid when rows x n_grid exceeds the wave's LDS
 *       slab), an in-place running sum (one lane per row), then a flat
 *       f64 write that turns 0 into NaN.  Cost O(samples + rows * n_grid), independent of
 *       window / step.  Counts are integers: any order is exact.
 *
 * A sample at ts belongs to grid points g with
 *   t_end[g] - window < ts <= t_end[g],  t_end[g] = start + g * step
 * i.e. g in [ceil((ts-start)/step), floor((ts+window-1-start)/step)],
 * clamped to [0, n_grid).  Both passes derive the range from ts alone, so
 * they need no sortedness and agree with each other by construction.
 *
 * No [n_series x 488 x n_grid] buffer exists anywhere: the only dense
 * state is the per-wave LDS tile.  The result rows and the pass-to-pass
 * scratch (codes, masks, row counts, row starts) belong to the batch and
 * only ever grow (vm_hot_state, batch_access.h), so a repeated query
 * allocates nothing.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "batch_access.h"
#include "devalloc.h"
#include "hot_common.h"
#include "vmrange_bucket.h"
#include "../../include/vmgpu.h"

/* per-wave difference-array slab, in i32 elements (6 KiB; 24 KiB a block) */
#define HOT_TILE_ELEMS 1536
#define HOT_SCAN_THREADS 1024

__global__ __launch_bounds__(HOT_BLOCK_THREADS) void hot_mark_kernel(
    HotParams p, const int64_t* __restrict__ ts,
    const double* __restrict__ vals, const uint64_t* __restrict__ offsets,
    const double* __restrict__ thr_g, uint32_t n_series,
    uint16_t* __restrict__ codes, uint32_t* __restrict__ masks,
    uint32_t* __restrict__ row_counts, unsigned long long* scanned) {
  __shared__ double s_thr[VMRANGE_TABLE_PAD];
  __shared__ uint32_t s_mask[HOT_WAVES_PER_BLOCK][VMRANGE_MASK_WORDS];
  for (int i = threadIdx.x; i < VMRANGE_TABLE_PAD; i += HOT_BLOCK_THREADS)
    s_thr[i] = thr_g[i];
  __syncthreads();
  const int lane = threadIdx.x % HOT_WAVE;
  const int wv = threadIdx.x / HOT_WAVE;
  const uint32_t wid = blockIdx.x * HOT_WAVES_PER_BLOCK + wv;
  const uint32_t stride = gridDim.x * HOT_WAVES_PER_BLOCK;
  unsigned long long sc = 0;
  for (uint32_t s = wid; s < n_series; s += stride) {
    const uint64_t lo = offsets[s];
    const uint64_t n = offsets[s + 1] - lo;
    if (lane < VMRANGE_MASK_WORDS) s_mask[wv][lane] = 0;
    hot_wave_sync();
    for (uint64_t k = lane; k < n; k += HOT_WAVE) {
      const int64_t t = ts[lo + k];
      const double v = vals[lo + k];
      uint32_t code = VMRANGE_CODE_NONE;
      const bool stale = p.drop_stale &&
          (unsigned long long)__double_as_longlong(v) == HOT_STALE_NAN_BITS;
      int32_t g0, g1;
      if (!stale && hot_grid_range(p, t, g0, g1)) {
        sc += (unsigned long long)(g1 - g0 + 1);
        code = vmrange_bucket_code(s_thr, v);
        if (code != VMRANGE_CODE_NONE)
          atomicOr(&s_mask[wv][code >> 5], 1u << (code & 31));
      }
      codes[lo + k] = (uint16_t)code;
    }
    hot_wave_sync();
    const uint32_t m = lane < VMRANGE_MASK_WORDS ? s_mask[wv][lane] : 0u;
    uint32_t rows = __popc(m);
    for (int d = 8; d; d >>= 1) rows += __shfl_xor(rows, d);
    if (lane < VMRANGE_MASK_WORDS)
      masks[(uint64_t)s * VMRANGE_MASK_WORDS + lane] = m;
    if (lane == 0) row_counts[s] = rows;
    hot_wave_sync();
  }
  for (int d = 32; d; d >>= 1) sc += __shfl_xor(sc, d);
  if (lane == 0 && sc) atomicAdd(scanned, sc);
}

/* exclusive scan of row_counts[n] into row_start[n + 1]: one workgroup
 * walks the array 4096 elements a round (16 B per lane, coalesced), wave
 * shuffles inside a wave, 16 wave totals through LDS (double-buffered, so
 * one barrier a round), a running carry across rounds */
__global__ __launch_bounds__(HOT_SCAN_THREADS) void hot_scan_kernel(
    const uint32_t* __restrict__ row_counts, uint32_t n,
    uint64_t* __restrict__ row_start) {
  constexpr int NW = HOT_SCAN_THREADS / HOT_WAVE;
  __shared__ uint32_t s_wave[2][NW];
  const uint32_t t = threadIdx.x;
  const uint32_t lane = t % HOT_WAVE;
  const uint32_t wv = t / HOT_WAVE;
  uint64_t carry = 0;
  int buf = 0;
  for (uint64_t base = 0; base < n; base += 4 * HOT_SCAN_THREADS, buf ^= 1) {
    const uint64_t i = base + (uint64_t)t * 4;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (i + 3 < n) {
      const uint4 v = *reinterpret_cast<const uint4*>(row_counts + i);
      c0 = v.x; c1 = v.y; c2 = v.z; c3 = v.w;
    } else {
      if (i < n) c0 = row_counts[i];
      if (i + 1 < n) c1 = row_counts[i + 1];
      if (i + 2 < n) c2 = row_counts[i + 2];
    }
    const uint32_t sum = c0 + c1 + c2 + c3;
    uint32_t incl = sum;
    for (int d = 1; d < HOT_WAVE; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if ((int)lane >= d) incl += up;
    }
    if (lane == HOT_WAVE - 1) s_wave[buf][wv] = incl;
    __syncthreads();
    uint64_t run = carry;
    uint64_t tot = 0;
    for (uint32_t w = 0; w < NW; w++) {
      const uint32_t x = s_wave[buf][w];
      if (w < wv) run += x;
      tot += x;
    }
    run += incl - sum;
    if (i < n) row_start[i] = run;
    run += c0;
    if (i + 1 < n) row_start[i + 1] = run;
    run += c1;
    if (i + 2 < n) row_start[i + 2] = run;
    run += c2;
    if (i + 3 < n) row_start[i + 3] = run;
    carry += tot;
  }
  if (t == 0) row_start[n] = carry;
}

__global__ __launch_bounds__(HOT_BLOCK_THREADS) void hot_count_kernel(
    HotParams p, const int64_t* __restrict__ ts,
    const uint16_t* __restrict__ codes, const uint64_t* __restrict__ offsets,
    const uint32_t* __restrict__ masks, const uint64_t* __restrict__ row_start,
    uint32_t n_series, double* __restrict__ out,
    uint32_t* __restrict__ row_series, uint16_t* __restrict__ row_code) {
  __shared__ __align__(16) int32_t s_diff[HOT_WAVES_PER_BLOCK][HOT_TILE_ELEMS];
  __shared__ uint32_t s_mask[HOT_WAVES_PER_BLOCK][VMRANGE_MASK_WORDS];
  __shared__ uint32_t s_pre[HOT_WAVES_PER_BLOCK][VMRANGE_MASK_WORDS];
  const int lane = threadIdx.x % HOT_WAVE;
  const int wv = threadIdx.x / HOT_WAVE;
  const uint32_t wid = blockIdx.x * HOT_WAVES_PER_BLOCK + wv;
  const uint32_t stride = gridDim.x * HOT_WAVES_PER_BLOCK;
  int32_t* diff = s_diff[wv];
  const double dnan = __longlong_as_double((long long)HOT_NAN_BITS);
  for (uint32_t s = wid; s < n_series; s += stride) {
    const uint64_t row0 = row_start[s];
    const uint32_t R = (uint32_t)(row_start[s + 1] - row0);
    if (R == 0 || R > VMRANGE_N_CODES) continue; /* wave-uniform */
    const uint64_t lo = offsets[s];
    const uint64_t n = offsets[s + 1] - lo;

    /* presence mask + per-word exclusive popcount prefix: the local row of
     * code c is the number of present codes below c */
    const uint32_t m = lane < VMRANGE_MASK_WORDS
        ? masks[(uint64_t)s * VMRANGE_MASK_WORDS + lane] : 0u;
    const uint32_t pc = __popc(m);
    uint32_t incl = pc;
    for (int d = 1; d < VMRANGE_MASK_WORDS; d <<= 1) {
      uint32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    hot_wave_sync();
    if (lane < VMRANGE_MASK_WORDS) {
      s_mask[wv][lane] = m;
      s_pre[wv][lane] = incl - pc;
    }
    hot_wave_sync();
    for (uint32_t c = lane; c < VMRANGE_N_CODES; c += HOT_WAVE) {
      const uint32_t w = s_mask[wv][c >> 5];
      if ((w >> (c & 31)) & 1u) {
        const uint32_t r = s_pre[wv][c >> 5] + __popc(w & ((1u << (c & 31)) - 1u));
        if (r < R) {
          row_series[row0 + r] = s;
          row_code[row0 + r] = (uint16_t)c;
        }
      }
    }

    /* grid tile: R rows of gt points + one slot for the closing -1; an odd
     * row stride keeps the lane-per-row running sum off a single bank */
    const int32_t gt = HOT_MIN(p.n_grid, (int32_t)(HOT_TILE_ELEMS / R) - 2);
    const uint32_t W = (uint32_t)(gt + 1) | 1u;
    for (int32_t G0 = 0; G0 < p.n_grid; G0 += gt) {
      const int32_t gw = HOT_MIN(gt, p.n_grid - G0);
      {
        /* R * W <= HOT_TILE_ELEMS, a multiple of 4: 16 B stores may round up */
        int4* d4 = reinterpret_cast<int4*>(diff);
        const uint32_t n4 = (R * W + 3) / 4;
        for (uint32_t e = lane; e < n4; e += HOT_WAVE) d4[e] = make_int4(0, 0, 0, 0);
      }
      hot_wave_sync();
      for (uint64_t k = lane; k < n; k += HOT_WAVE) {
        const uint32_t c = codes[lo + k];
        if (c >= VMRANGE_N_CODES) continue;
        int32_t g0, g1;
        if (!hot_grid_range(p, ts[lo + k], g0, g1)) continue;
        g0 = HOT_MAX(g0, G0) - G0;
        g1 = HOT_MIN(g1, G0 + gw - 1) - G0;
        if (g0 > g1) continue;
        const uint32_t w = s_mask[wv][c >> 5];
        const uint32_t r = s_pre[wv][c >> 5] + __popc(w & ((1u << (c & 31)) - 1u));
        if (r >= R) continue;
        atomicAdd(&diff[r * W + g0], 1);
        atomicSub(&diff[r * W + g1 + 1], 1);
      }
      hot_wave_sync();
      /* running sum in place, one lane per row */
      for (uint32_t r = lane; r < R; r += HOT_WAVE) {
        int32_t run = 0;
        for (int32_t j = 0; j < gw; j++) {
          run += diff[r * W + j];
          diff[r * W + j] = run;
        }
      }
      hot_wave_sync();
      /* flat write of the [R x gw] tile: with one tile (gw == n_grid) the
       * series' whole output block is contiguous */
      const uint32_t tot = R * (uint32_t)gw;
      const float inv_gw = 1.0f / (float)gw;
      for (uint32_t e = lane; e < tot; e += HOT_WAVE) {
        /* e < HOT_TILE_ELEMS is exact in f32; the quotient is off by at most
         * one */
        uint32_t r = (uint32_t)((float)e * inv_gw);
        if (r * (uint32_t)gw > e) r--;
        else if ((r + 1) * (uint32_t)gw <= e) r++;
        const uint32_t j = e - r * (uint32_t)gw;
        const int32_t cnt = diff[r * W + j];
        out[(row0 + r) * (uint64_t)p.n_grid + (uint64_t)(G0 + (int32_t)j)] =
            cnt ? (double)cnt : dnan;
      }
      hot_wave_sync();
    }
  }
}

/* ------------------------------------------------------------------ */
/* host side                                                          */
/* ------------------------------------------------------------------ */

namespace {

double* g_d_thr = nullptr; /* VMRANGE_TABLE_PAD doubles, NaN-padded */

}  // namespace

void hot_scan_launch(const uint32_t* row_counts, uint32_t n,
                     uint64_t* row_start, hipStream_t st) {
  hipLaunchKernelGGL(hot_scan_kernel, dim3(1), dim3(HOT_SCAN_THREADS), 0, st,
                     row_counts, n, row_start);
}

void vm_hot_state_free(vm_hot_state* h) {
  (void)hipFree(h->d_out);
  (void)hipFree(h->d_row_series);
  (void)hipFree(h->d_row_code);
  (void)hipFree(h->d_codes);
  (void)hipFree(h->d_masks);
  (void)hipFree(h->d_row_counts);
  (void)hipFree(h->d_row_start);
  (void)hipFree(h->d_scanned);
  *h = vm_hot_state();
}

const double* vm_hot_thresholds(void) { return g_d_thr; }

void vm_hot_shutdown(void) {
  (void)vm_dev_free(g_d_thr);
  g_d_thr = nullptr;
}

extern "C" {

int vmgpu_vmrange_thresholds_set(const double* thresholds, uint32_t n,
                                 char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  if (!thresholds || n != VMRANGE_N_THRESHOLDS)
    return vm_set_err(errbuf, errbuf_len,
                       "vmgpu: vmrange table must have 487 thresholds");
  for (uint32_t i = 0; i < n; i++) {
    bool ok = thresholds[i] > 0 && (i == 0 || thresholds[i] > thresholds[i - 1]);
    if (!ok)
      return vm_set_err(errbuf, errbuf_len,
                         "vmgpu: vmrange thresholds must be positive and "
                         "strictly increasing");
  }
  double padded[VMRANGE_TABLE_PAD];
  memcpy(padded, thresholds, n * sizeof(double));
  for (uint32_t i = n; i < VMRANGE_TABLE_PAD; i++) padded[i] = __builtin_nan("");
  hipStream_t st = vm_ctx_stream();
  if (!g_d_thr)
    VM_HIP_TRY(vm_dev_malloc(&g_d_thr, sizeof(padded)), "alloc vmrange table");
  VM_HIP_TRY(hipMemcpyAsync(g_d_thr, padded, sizeof(padded), hipMemcpyHostToDevice, st),
          "upload vmrange table");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync vmrange table");
  return 0;
}

int vmgpu_histogram_over_time_exec(uint64_t handle, int64_t start, int64_t end,
                                   int64_t step, int64_t window,
                                   int32_t drop_stale, uint64_t* out_n_rows,
                                   uint64_t* out_samples_scanned,
                                   char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  vm_batch_cols b;
  if (vm_batch_cols_get(handle, &b) != 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  if (window <= 0)
    return vm_set_err(errbuf, errbuf_len,
                       "vmgpu: histogram_over_time needs an explicit window "
                       "(m[d] range selector)");
  if (step <= 0 || end < start)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad grid");
  int64_t n_grid64 = 1 + (end - start) / step;
  if (n_grid64 > (int64_t)1 << 30)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: grid too large");
  if (!g_d_thr)
    return vm_set_err(errbuf, errbuf_len,
                       "vmgpu: vmrange threshold table not uploaded "
                       "(vmgpu_vmrange_thresholds_set)");
  HotParams p;
  p.start = start;
  p.step = step;
  p.window = window;
  p.n_grid = (int32_t)n_grid64;
  p.drop_stale = drop_stale ? 1 : 0;

  hipStream_t st = vm_ctx_stream();
  hipEvent_t ev_start, ev_stop;
  vm_ctx_events(&ev_start, &ev_stop);
  const uint32_t ns = b.n_series;

  vm_hot_state& h = *b.hot;
  h.valid = false; /* the earlier result is replaced from here on */
  {
    /* scratch is sized by the batch, so each piece is allocated once */
    size_t cap = 0;
    if (!h.d_codes)
      VM_HIP_TRY(hot_reserve(&h.d_codes, &cap, (size_t)b.n_samples * 2 + 16), "alloc codes");
    if (!h.d_masks)
      VM_HIP_TRY(hot_reserve(&h.d_masks, &cap, (size_t)ns * VMRANGE_MASK_WORDS * 4),
              "alloc masks");
    if (!h.d_row_counts)
      VM_HIP_TRY(hot_reserve(&h.d_row_counts, &cap, (size_t)ns * 4), "alloc row counts");
    if (!h.d_row_start)
      VM_HIP_TRY(hot_reserve(&h.d_row_start, &cap, ((size_t)ns + 1) * 8), "alloc row start");
    if (!h.d_scanned)
      VM_HIP_TRY(hot_reserve(&h.d_scanned, &cap, 8), "alloc scanned");
  }
  VM_HIP_TRY(hipMemsetAsync(h.d_scanned, 0, 8, st), "zero scanned");

  const uint32_t blocks = std::min<uint32_t>(
      (ns + HOT_WAVES_PER_BLOCK - 1) / HOT_WAVES_PER_BLOCK, HOT_MAX_BLOCKS);

  VM_HIP_TRY(hipEventRecord(ev_start, st), "event start");
  hipLaunchKernelGGL(hot_mark_kernel, dim3(blocks), dim3(HOT_BLOCK_THREADS), 0, st,
                     p, b.d_ts, b.d_vals, b.d_offsets, g_d_thr, ns,
                     h.d_codes, h.d_masks, h.d_row_counts, h.d_scanned);
  hot_scan_launch(h.d_row_counts, ns, h.d_row_start, st);
  /* the output size is data-dependent: the host learns n_rows here */
  uint64_t n_rows = 0;
  unsigned long long scanned_h = 0;
  VM_HIP_TRY(hipMemcpyAsync(&n_rows, h.d_row_start + ns, 8, hipMemcpyDeviceToHost, st),
          "download n_rows");
  VM_HIP_TRY(hipMemcpyAsync(&scanned_h, h.d_scanned, 8, hipMemcpyDeviceToHost, st),
          "download scanned");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync mark");
  {
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "mark kernel", kerr);
  }
  if (n_rows > (uint64_t)ns * VMRANGE_N_CODES)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: inconsistent row count");

  h.n_rows = n_rows;
  h.n_grid = p.n_grid;
  if (n_rows) {
    VM_HIP_TRY(hot_reserve(&h.d_out, &h.out_cap, (size_t)n_rows * p.n_grid * 8),
            "alloc histogram rows");
    VM_HIP_TRY(hot_reserve(&h.d_row_series, &h.row_series_cap, (size_t)n_rows * 4),
            "alloc row series");
    VM_HIP_TRY(hot_reserve(&h.d_row_code, &h.row_code_cap, (size_t)n_rows * 2),
            "alloc row codes");
    hipLaunchKernelGGL(hot_count_kernel, dim3(blocks), dim3(HOT_BLOCK_THREADS), 0, st,
                       p, b.d_ts, h.d_codes, b.d_offsets, h.d_masks,
                       h.d_row_start, ns, h.d_out, h.d_row_series,
                       h.d_row_code);
  }
  VM_HIP_TRY(hipEventRecord(ev_stop, st), "event stop");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync count");
  VM_HIP_TRY(hipGetLastError(), "count kernel");
  float ms = 0;
  VM_HIP_TRY(hipEventElapsedTime(&ms, ev_start, ev_stop), "event elapsed");
  vm_ctx_set_last_kernel_ms((double)ms);
  h.valid = true;
  if (out_n_rows) *out_n_rows = n_rows;
  if (out_samples_scanned) *out_samples_scanned = (uint64_t)scanned_h;
  return 0;
}

int vmgpu_histogram_over_time_fetch(uint64_t handle, uint32_t* row_series,
                                    uint16_t* row_bucket, double* out,
                                    char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  vm_batch_cols b;
  if (vm_batch_cols_get(handle, &b) != 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  const vm_hot_state& h = *b.hot;
  if (!h.valid)
    return vm_set_err(errbuf, errbuf_len,
                       "vmgpu: no histogram_over_time result on this batch");
  if (h.n_rows == 0) return 0;
  hipStream_t st = vm_ctx_stream();
  if (row_series)
    VM_HIP_TRY(hipMemcpyAsync(row_series, h.d_row_series, h.n_rows * 4,
                           hipMemcpyDeviceToHost, st), "download row series");
  if (row_bucket)
    VM_HIP_TRY(hipMemcpyAsync(row_bucket, h.d_row_code, h.n_rows * 2,
                           hipMemcpyDeviceToHost, st), "download row buckets");
  if (out)
    VM_HIP_TRY(hipMemcpyAsync(out, h.d_out, (size_t)h.n_rows * h.n_grid * 8,
                           hipMemcpyDeviceToHost, st), "download histogram rows");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync fetch");
  if (row_series && b.perm)
    for (uint64_t i = 0; i < h.n_rows; i++) {
      uint32_t phys = row_series[i];
      if (phys >= b.n_series)
        return vm_set_err(errbuf, errbuf_len, "vmgpu: corrupt row series");
      row_series[i] = b.perm[phys];
    }
  return 0;
}

}  // extern "C"
