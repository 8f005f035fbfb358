/* cvot.hip — count_values_over_time (newRollupCountValues, rollup.go:1490)
 * on the device, over a resident batch.
 *
 * The reference keys its output series on strconv.FormatFloat(v,'g',-1,64),
 * the shortest round-trip form: injective on non-NaN doubles (-0 and 0
 * differ) and "NaN" for every NaN.  So the label is a pure function of the
 * value's bits with all NaNs folded into one, the device keys rows on those
 * bits, and the host formats one label per ROW instead of one per sample.
 *
 * Same sparse contract and pass structure as hot.hip (hot_common.h), but
 * the key set is unbounded: a series has up to one row per sample, so the
 * distinct keys come from a per-series sort instead of a presence mask.
 *
 *   cvot_mark_kernel       one wavefront per series of at most CVOT_WAVE_CAP
 *       samples: the order key of every covered sample (CVOT_KEY_NONE for
 *       the rest), samples_scanned as in hot_mark_kernel, the keys that
 *       differ from their predecessor's into the wave's LDS slab (a value
 *       held for a run is sorted once), a bitonic sort, then the runs of
 *       equal keys: the
 *       series' distinct keys go to row_keys[offsets[s] + r] (a series has
 *       no more rows than samples, so the slot always exists), the run
 *       count to row_counts[s], and every sample's local row (a binary
 *       search of its key among the distinct keys) to local_row.  Longer
 *       series are appended to a list for
 *   cvot_mark_long_kernel  one workgroup per listed series: the same steps
 *       with the keys in the workgroup's LDS up to CVOT_BLOCK_CAP samples,
 *       and in place in the series' own row_keys slice above that.
 *   hot_scan_launch        row_counts -> row_start, n_rows (hot.hip).
 *   cvot_count_kernel      per series, +-1 difference arrays in LDS, running
 *       sum, f64 write with 0 -> NaN, as hot_count_kernel, but tiled over
 *       rows as well as over the grid; also row_series and row_value.
 *
 * The order key, the bitonic sort and the search are value_key.h's, shared
 * with the count_values() aggregate (aggrcv.hip).
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <mutex>

#include "batch_access.h"
#include "devalloc.h"
#include "hot_common.h"
#include "value_key.h"
#include "../../include/vmgpu.h"

/* workgroups of the long-series kernel: 8 per CU on 256 CUs; with an empty
 * list they read one word and leave */
#define CVOT_LONG_BLOCKS 2048
/* per-wave difference-array slab in i32 elements, as HOT_TILE_ELEMS */
#define CVOT_TILE_ELEMS 1536
/* rows per tile once rows x grid exceed the slab: leaves 62 grid points a
 * row, so a tile row is still a ~500-byte contiguous output write */
#define CVOT_ROW_TILE 24
#define CVOT_ROW_NONE 0xFFFFFFFFu

/* order key of a covered sample (adding its grid-range length to sc), or
 * CVOT_KEY_NONE for a dropped stale NaN or a sample in no window */
static HOT_DEV uint64_t cvot_sample_key(const HotParams& p, int64_t t, double v,
                                        unsigned long long& sc) {
  if (p.drop_stale &&
      (unsigned long long)__double_as_longlong(v) == HOT_STALE_NAN_BITS)
    return CVOT_KEY_NONE;
  int32_t g0, g1;
  if (!hot_grid_range(p, t, g0, g1)) return CVOT_KEY_NONE;
  sc += (unsigned long long)(g1 - g0 + 1);
  return cvot_order_key(v);
}

__global__ __launch_bounds__(HOT_BLOCK_THREADS) void cvot_mark_kernel(
    HotParams p, const int64_t* __restrict__ ts,
    const double* __restrict__ vals, const uint64_t* __restrict__ offsets,
    uint32_t n_series, uint32_t* __restrict__ local_row,
    uint64_t* __restrict__ row_keys, uint32_t* __restrict__ row_counts,
    uint32_t* __restrict__ long_list, unsigned long long* small) {
  constexpr int Q = CVOT_WAVE_CAP / HOT_WAVE;
  __shared__ uint64_t s_keys[HOT_WAVES_PER_BLOCK][CVOT_WAVE_CAP];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = threadIdx.x / HOT_WAVE;
  const uint32_t wid = blockIdx.x * HOT_WAVES_PER_BLOCK + wv;
  const uint32_t stride = gridDim.x * HOT_WAVES_PER_BLOCK;
  uint64_t* keys = s_keys[wv];
  unsigned long long sc = 0;
  for (uint32_t s = wid; s < n_series; s += stride) {
    const uint64_t lo = offsets[s];
    const uint64_t n64 = offsets[s + 1] - lo;
    if (n64 > CVOT_WAVE_CAP) { /* wave-uniform */
      if (lane == 0)
        long_list[atomicAdd(reinterpret_cast<uint32_t*>(small + 1), 1u)] = s;
      continue;
    }
    const uint32_t n = (uint32_t)n64;
    uint64_t mine[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const uint32_t k = lane + q * HOT_WAVE;
      mine[q] = CVOT_KEY_NONE;
      if (k < n) mine[q] = cvot_sample_key(p, ts[lo + k], vals[lo + k], sc);
    }
    /* only a sample whose key differs from its predecessor's goes into the
     * sort: the distinct keys are the same, and a value held for a run (an
     * enum, a state) costs one slot however long the run is */
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const uint32_t k = lane + q * HOT_WAVE;
      const uint64_t up = __shfl_up((unsigned long long)mine[q], 1);
      const uint64_t wrap =
          q ? __shfl((unsigned long long)mine[q ? q - 1 : 0], HOT_WAVE - 1) : 0;
      const uint64_t prev = lane ? up : wrap;
      const bool first = k < n && (k == 0 || mine[q] != prev);
      const unsigned long long fm = __ballot(first);
      if (first) keys[m + __popcll(fm & ((1ULL << lane) - 1ULL))] = mine[q];
      m += __popcll(fm);
    }
    hot_wave_sync();
    cvot_sort<true>(keys, m, lane, HOT_WAVE);
    /* heads of the runs of equal keys; every read of the slab comes before
     * the compaction below overwrites it */
    uint64_t cur[Q];
    bool head[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const uint32_t k = lane + q * HOT_WAVE;
      cur[q] = CVOT_KEY_NONE;
      head[q] = false;
      if (k < m) {
        cur[q] = keys[k];
        head[q] = cur[q] != CVOT_KEY_NONE && (k == 0 || keys[k - 1] != cur[q]);
      }
    }
    hot_wave_sync();
    uint32_t R = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const unsigned long long m = __ballot(head[q]);
      if (head[q]) {
        const uint32_t r = R + __popcll(m & ((1ULL << lane) - 1ULL));
        keys[r] = cur[q];
        row_keys[lo + r] = cur[q];
      }
      R += __popcll(m);
    }
    hot_wave_sync();
    if (lane == 0) row_counts[s] = R;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const uint32_t k = lane + q * HOT_WAVE;
      if (k < n)
        local_row[lo + k] = mine[q] == CVOT_KEY_NONE
            ? CVOT_ROW_NONE : cvot_lower_bound(keys, R, mine[q]);
    }
    hot_wave_sync();
  }
  for (int d = 32; d; d >>= 1) sc += __shfl_xor(sc, d);
  if (lane == 0 && sc) atomicAdd(small, sc);
}

/* One series of n > CVOT_WAVE_CAP samples by a whole workgroup.  keys is the
 * sort area: the workgroup's LDS, or dst itself (the series' row_keys
 * slice) when n is above CVOT_BLOCK_CAP.  The compaction walks the sorted
 * keys HOT_BLOCK_THREADS at a time and writes run r at dst[r], r <= i, only
 * after the whole chunk and its predecessor (carry) have been read, so it is
 * safe in place. */
static HOT_DEV void cvot_long_series(
    const HotParams& p, const int64_t* __restrict__ ts,
    const double* __restrict__ vals, uint64_t n, uint64_t* keys, uint64_t* dst,
    uint32_t* __restrict__ local_row, uint32_t* row_count, uint32_t* s_wcnt,
    uint64_t* s_carry, unsigned long long& sc) {
  const uint32_t t = threadIdx.x;
  const uint32_t lane = t % HOT_WAVE;
  const uint32_t wv = t / HOT_WAVE;
  for (uint64_t k = t; k < n; k += HOT_BLOCK_THREADS)
    keys[k] = cvot_sample_key(p, ts[k], vals[k], sc);
  __syncthreads();
  cvot_sort<false>(keys, n, t, HOT_BLOCK_THREADS);
  uint32_t R = 0;
  for (uint64_t base = 0; base < n; base += HOT_BLOCK_THREADS) {
    const uint64_t i = base + t;
    uint64_t cur = CVOT_KEY_NONE;
    bool head = false;
    if (i < n) {
      cur = keys[i];
      const uint64_t prev =
          i == 0 ? CVOT_KEY_NONE : (t == 0 ? *s_carry : keys[i - 1]);
      head = cur != CVOT_KEY_NONE && (i == 0 || prev != cur);
    }
    const unsigned long long m = __ballot(head);
    if (lane == 0) s_wcnt[wv] = __popcll(m);
    __syncthreads();
    uint32_t r = R + __popcll(m & ((1ULL << lane) - 1ULL));
    uint32_t tot = 0;
    for (uint32_t w = 0; w < HOT_WAVES_PER_BLOCK; w++) {
      const uint32_t c = s_wcnt[w];
      if (w < wv) r += c;
      tot += c;
    }
    if (head) dst[r] = cur;
    if (t == HOT_BLOCK_THREADS - 1) *s_carry = cur;
    R += tot;
    __syncthreads();
  }
  if (t == 0) *row_count = R;
  for (uint64_t k = t; k < n; k += HOT_BLOCK_THREADS) {
    unsigned long long unused = 0;
    const uint64_t key = cvot_sample_key(p, ts[k], vals[k], unused);
    local_row[k] = key == CVOT_KEY_NONE ? CVOT_ROW_NONE
                                        : cvot_lower_bound(dst, R, key);
  }
  __syncthreads();
}

__global__ __launch_bounds__(HOT_BLOCK_THREADS) void cvot_mark_long_kernel(
    HotParams p, const int64_t* __restrict__ ts,
    const double* __restrict__ vals, const uint64_t* __restrict__ offsets,
    uint32_t* __restrict__ local_row, uint64_t* row_keys,
    uint32_t* __restrict__ row_counts, const uint32_t* __restrict__ long_list,
    unsigned long long* small) {
  __shared__ uint64_t s_keys[CVOT_BLOCK_CAP];
  __shared__ uint32_t s_wcnt[HOT_WAVES_PER_BLOCK];
  __shared__ uint64_t s_carry;
  const uint32_t n_long = *reinterpret_cast<const uint32_t*>(small + 1);
  unsigned long long sc = 0;
  for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
    const uint32_t s = long_list[i];
    const uint64_t lo = offsets[s];
    const uint64_t n = offsets[s + 1] - lo;
    if (n <= CVOT_BLOCK_CAP)
      cvot_long_series(p, ts + lo, vals + lo, n, s_keys, row_keys + lo,
                       local_row + lo, row_counts + s, s_wcnt, &s_carry, sc);
    else
      cvot_long_series(p, ts + lo, vals + lo, n, row_keys + lo, row_keys + lo,
                       local_row + lo, row_counts + s, s_wcnt, &s_carry, sc);
  }
  for (int d = 32; d; d >>= 1) sc += __shfl_xor(sc, d);
  if (threadIdx.x % HOT_WAVE == 0 && sc) atomicAdd(small, sc);
}

__global__ __launch_bounds__(HOT_BLOCK_THREADS) void cvot_count_kernel(
    HotParams p, const int64_t* __restrict__ ts,
    const uint32_t* __restrict__ local_row,
    const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ row_keys,
    const uint64_t* __restrict__ row_start, uint32_t n_series,
    double* __restrict__ out, uint32_t* __restrict__ row_series,
    double* __restrict__ row_value) {
  __shared__ __align__(16) int32_t s_diff[HOT_WAVES_PER_BLOCK][CVOT_TILE_ELEMS];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = threadIdx.x / HOT_WAVE;
  const uint32_t wid = blockIdx.x * HOT_WAVES_PER_BLOCK + wv;
  const uint32_t stride = gridDim.x * HOT_WAVES_PER_BLOCK;
  int32_t* diff = s_diff[wv];
  const double dnan = __longlong_as_double((long long)HOT_NAN_BITS);
  for (uint32_t s = wid; s < n_series; s += stride) {
    const uint64_t row0 = row_start[s];
    const uint32_t R = (uint32_t)(row_start[s + 1] - row0);
    if (R == 0) continue; /* wave-uniform */
    const uint64_t lo = offsets[s];
    const uint64_t n = offsets[s + 1] - lo;
    for (uint32_t r = lane; r < R; r += HOT_WAVE) {
      row_series[row0 + r] = s;
      row_value[row0 + r] = cvot_key_value(row_keys[lo + r]);
    }

    /* tile: rt rows of gt grid points + one slot for the closing -1; an odd
     * row stride keeps the lane-per-row running sum off a single bank.
     * W <= gt + 2, so rt * W <= CVOT_TILE_ELEMS. */
    const uint32_t rt =
        (uint64_t)R * ((uint64_t)p.n_grid + 2) <= CVOT_TILE_ELEMS
            ? R : HOT_MIN(R, (uint32_t)CVOT_ROW_TILE);
    const int32_t gt = HOT_MIN(p.n_grid, (int32_t)(CVOT_TILE_ELEMS / rt) - 2);
    const uint32_t W = (uint32_t)(gt + 1) | 1u;
    for (uint32_t R0 = 0; R0 < R; R0 += rt) {
      const uint32_t rw = HOT_MIN(rt, R - R0);
      for (int32_t G0 = 0; G0 < p.n_grid; G0 += gt) {
        const int32_t gw = HOT_MIN(gt, p.n_grid - G0);
        {
          /* rw * W <= CVOT_TILE_ELEMS, a multiple of 4: 16 B stores may
           * round up */
          int4* d4 = reinterpret_cast<int4*>(diff);
          const uint32_t n4 = (rw * W + 3) / 4;
          for (uint32_t e = lane; e < n4; e += HOT_WAVE)
            d4[e] = make_int4(0, 0, 0, 0);
        }
        hot_wave_sync();
        for (uint64_t k = lane; k < n; k += HOT_WAVE) {
          const uint32_t lr = local_row[lo + k];
          if (lr == CVOT_ROW_NONE || lr < R0 || lr - R0 >= rw) continue;
          int32_t g0, g1;
          if (!hot_grid_range(p, ts[lo + k], g0, g1)) continue;
          g0 = HOT_MAX(g0, G0) - G0;
          g1 = HOT_MIN(g1, G0 + gw - 1) - G0;
          if (g0 > g1) continue;
          const uint32_t r = lr - R0;
          atomicAdd(&diff[r * W + g0], 1);
          atomicSub(&diff[r * W + g1 + 1], 1);
        }
        hot_wave_sync();
        /* running sum in place, one lane per row */
        for (uint32_t r = lane; r < rw; r += HOT_WAVE) {
          int32_t run = 0;
          for (int32_t j = 0; j < gw; j++) {
            run += diff[r * W + j];
            diff[r * W + j] = run;
          }
        }
        hot_wave_sync();
        /* flat write of the [rw x gw] tile */
        const uint32_t tot = rw * (uint32_t)gw;
        const float inv_gw = 1.0f / (float)gw;
        for (uint32_t e = lane; e < tot; e += HOT_WAVE) {
          /* e < CVOT_TILE_ELEMS is exact in f32; the quotient is off by at
           * most one */
          uint32_t r = (uint32_t)((float)e * inv_gw);
          if (r * (uint32_t)gw > e) r--;
          else if ((r + 1) * (uint32_t)gw <= e) r++;
          const uint32_t j = e - r * (uint32_t)gw;
          const int32_t cnt = diff[r * W + j];
          out[(row0 + R0 + r) * (uint64_t)p.n_grid + (uint64_t)(G0 + (int32_t)j)] =
              cnt ? (double)cnt : dnan;
        }
        hot_wave_sync();
      }
    }
  }
}

/* ------------------------------------------------------------------ */
/* host side                                                          */
/* ------------------------------------------------------------------ */

void vm_cvot_state_free(vm_cvot_state* h) {
  (void)hipFree(h->d_out);
  (void)hipFree(h->d_row_series);
  (void)hipFree(h->d_row_value);
  (void)hipFree(h->d_local_row);
  (void)hipFree(h->d_row_keys);
  (void)hipFree(h->d_row_counts);
  (void)hipFree(h->d_row_start);
  (void)hipFree(h->d_long_list);
  (void)hipFree(h->d_small);
  *h = vm_cvot_state();
}

extern "C" {

int vmgpu_count_values_over_time_exec(uint64_t handle, int64_t start, int64_t end,
                                      int64_t step, int64_t window,
                                      int32_t drop_stale, uint64_t max_rows,
                                      uint64_t* out_n_rows,
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
                       "vmgpu: count_values_over_time needs an explicit window "
                       "(m[d] range selector)");
  if (step <= 0 || end < start)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad grid");
  int64_t n_grid64 = 1 + (end - start) / step;
  if (n_grid64 > (int64_t)1 << 30)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: grid too large");
  if (b.n_samples >= CVOT_ROW_NONE)
    return vm_set_err(errbuf, errbuf_len,
                       "vmgpu: batch too large for count_values_over_time");
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

  vm_cvot_state& h = *b.cvot;
  h.valid = false; /* the earlier result is replaced from here on */
  {
    /* scratch is sized by the batch, so each piece is allocated once */
    size_t cap = 0;
    if (!h.d_local_row)
      VM_HIP_TRY(hot_reserve(&h.d_local_row, &cap, (size_t)b.n_samples * 4 + 16),
              "alloc local rows");
    if (!h.d_row_keys)
      VM_HIP_TRY(hot_reserve(&h.d_row_keys, &cap, (size_t)b.n_samples * 8 + 16),
              "alloc row keys");
    if (!h.d_row_counts)
      VM_HIP_TRY(hot_reserve(&h.d_row_counts, &cap, (size_t)ns * 4 + 16),
              "alloc row counts");
    if (!h.d_row_start)
      VM_HIP_TRY(hot_reserve(&h.d_row_start, &cap, ((size_t)ns + 1) * 8), "alloc row start");
    if (!h.d_long_list)
      VM_HIP_TRY(hot_reserve(&h.d_long_list, &cap, (size_t)ns * 4 + 16),
              "alloc long-series list");
    if (!h.d_small)
      VM_HIP_TRY(hot_reserve(&h.d_small, &cap, 16), "alloc counters");
  }
  VM_HIP_TRY(hipMemsetAsync(h.d_small, 0, 16, st), "zero counters");

  const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(
      (ns + HOT_WAVES_PER_BLOCK - 1) / HOT_WAVES_PER_BLOCK, HOT_MAX_BLOCKS));
  const uint32_t long_blocks =
      std::max<uint32_t>(1, std::min<uint32_t>(ns, CVOT_LONG_BLOCKS));

  VM_HIP_TRY(hipEventRecord(ev_start, st), "event start");
  hipLaunchKernelGGL(cvot_mark_kernel, dim3(blocks), dim3(HOT_BLOCK_THREADS), 0, st,
                     p, b.d_ts, b.d_vals, b.d_offsets, ns, h.d_local_row,
                     h.d_row_keys, h.d_row_counts, h.d_long_list, h.d_small);
  hipLaunchKernelGGL(cvot_mark_long_kernel, dim3(long_blocks),
                     dim3(HOT_BLOCK_THREADS), 0, st, p, b.d_ts, b.d_vals,
                     b.d_offsets, h.d_local_row, h.d_row_keys, h.d_row_counts,
                     h.d_long_list, h.d_small);
  hot_scan_launch(h.d_row_counts, ns, h.d_row_start, st);
  /* the output size is data-dependent: the host learns n_rows here */
  uint64_t n_rows = 0;
  unsigned long long scanned_h = 0;
  VM_HIP_TRY(hipMemcpyAsync(&n_rows, h.d_row_start + ns, 8, hipMemcpyDeviceToHost, st),
          "download n_rows");
  VM_HIP_TRY(hipMemcpyAsync(&scanned_h, h.d_small, 8, hipMemcpyDeviceToHost, st),
          "download scanned");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync mark");
  {
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "mark kernel", kerr);
  }
  if (n_rows > b.n_samples)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: inconsistent row count");
  if (max_rows && n_rows > max_rows) {
    if (errbuf && errbuf_len)
      snprintf(errbuf, errbuf_len,
               "vmgpu: count_values_over_time produces %llu output rows, "
               "above the limit of %llu",
               (unsigned long long)n_rows, (unsigned long long)max_rows);
    return 1;
  }

  h.n_rows = n_rows;
  h.n_grid = p.n_grid;
  if (n_rows) {
    VM_HIP_TRY(hot_reserve(&h.d_out, &h.out_cap, (size_t)n_rows * p.n_grid * 8),
            "alloc count_values rows");
    VM_HIP_TRY(hot_reserve(&h.d_row_series, &h.row_series_cap, (size_t)n_rows * 4),
            "alloc row series");
    VM_HIP_TRY(hot_reserve(&h.d_row_value, &h.row_value_cap, (size_t)n_rows * 8),
            "alloc row values");
    hipLaunchKernelGGL(cvot_count_kernel, dim3(blocks), dim3(HOT_BLOCK_THREADS), 0, st,
                       p, b.d_ts, h.d_local_row, b.d_offsets, h.d_row_keys,
                       h.d_row_start, ns, h.d_out, h.d_row_series,
                       h.d_row_value);
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

int vmgpu_count_values_over_time_fetch(uint64_t handle, uint32_t* row_series,
                                       double* row_value, double* out,
                                       char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  vm_batch_cols b;
  if (vm_batch_cols_get(handle, &b) != 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  const vm_cvot_state& h = *b.cvot;
  if (!h.valid)
    return vm_set_err(errbuf, errbuf_len,
                       "vmgpu: no count_values_over_time result on this batch");
  if (h.n_rows == 0) return 0;
  hipStream_t st = vm_ctx_stream();
  if (row_series)
    VM_HIP_TRY(hipMemcpyAsync(row_series, h.d_row_series, h.n_rows * 4,
                           hipMemcpyDeviceToHost, st), "download row series");
  if (row_value)
    VM_HIP_TRY(hipMemcpyAsync(row_value, h.d_row_value, h.n_rows * 8,
                           hipMemcpyDeviceToHost, st), "download row values");
  if (out)
    VM_HIP_TRY(hipMemcpyAsync(out, h.d_out, (size_t)h.n_rows * h.n_grid * 8,
                           hipMemcpyDeviceToHost, st), "download count_values rows");
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
