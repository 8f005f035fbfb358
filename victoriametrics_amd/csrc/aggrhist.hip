/* aggrhist.hip — the histogram() aggregate (aggrFuncHistogram, aggr.go:316)
 * on the device.
 *
 * Input: a device matrix vals[n_in_rows x n_grid] (f64, row-major) and a
 * member CSR (group_offsets u64[n_groups + 1], group_rows u32[n_members]).
 * Per (group, grid point) the reference runs a metrics.Histogram over the
 * member values and emits one series per vmrange bucket that is non-zero at
 * some grid point.  The output is therefore SPARSE like hot.hip's: one row
 * per (group, vmrange code) present anywhere in the group, ordered by group
 * and then by ascending code, with the count as f64 and 0.0 (not NaN) where
 * a code is absent at a grid point — the reference starts its rows from
 * zeros.
 *
 * The shape follows hot.hip, turned from per-series windows to per-group
 * columns.  The host cuts every group into chunks of at most
 * AH_CHUNK_MEMBERS members; a work item is (chunk, tile of 64 columns) and
 * belongs to one wavefront, lanes owning columns, so one huge group spreads
 * over the machine and so do a million tiny ones.
 *
 *   ah_mark_kernel       classifies every member value (vmrange_bucket.h,
 *       table staged in LDS), caches the code as u16 in codes[row x n_grid]
 *       and ORs it into the wave's 16-word mask; one global atomicOr per
 *       non-zero word into masks[group x 16].
 *   ah_row_count_kernel  row_counts[g] = popcount(mask of g);
 *       hot_scan_launch  row_start; the host reads n_rows back.
 *   ah_row_fill_kernel   row_group / row_code of every output row.
 *   ah_count_kernel      per work item a u32 LDS tile [band rows x 64
 *       columns]; a lane only ever touches its own column, so increments
 *       are plain LDS read-modify-writes on distinct banks.  The local row
 *       of a code is its rank in the group's mask.  Non-zero counters are
 *       added into a zeroed u32 matrix [n_rows x n_grid] with integer
 *       atomicAdd — any arrival order gives the same bits.  A group with
 *       more rows than the tile holds is counted in bands of AH_BAND_ROWS.
 *   ah_u32_to_f64_kernel counters -> f64 result.
 *
 * The chunk list, the CSR checks and the counter conversion know nothing
 * about vmrange codes: they live in aggr_sparse.h, and the count_values()
 * aggregate (aggrcv.hip) uses them with its own row discovery.
 *
 * Result and scratch live in one file-static slot (the aggregate has no
 * batch of its own to hang them on), grow-only, plain hipMalloc through
 * hot_reserve, guarded by the context lock.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "aggr_sparse.h"
#include "batch_access.h"
#include "hot_common.h"
#include "vmrange_bucket.h"
#include "../../include/vmgpu.h"

/* Members of one group per work item.  Smaller chunks give one huge group
 * more wavefronts; larger ones flush fewer counters into the rows all the
 * chunks of a group share.  Measured in profiles/histogram_aggregate.md. */
#define AH_CHUNK_MEMBERS 128
/* member rows a lane keeps in flight */
#define AH_UNROLL 8
#define AH_TILE_COLS HOT_WAVE
/* Rows of the count tile.  64 rows x 64 columns x 4 B = 16 KiB a wave; with
 * two waves a workgroup that is 32 KiB, so four workgroups share a CU's
 * 160 KiB.  A taller band saves re-reads of the codes for wide groups but
 * leaves fewer waves to hide their latency. */
#define AH_BAND_ROWS 64
#define AH_MARK_THREADS 256
#define AH_COUNT_THREADS 128
#define AH_MARK_WAVES (AH_MARK_THREADS / HOT_WAVE)
#define AH_COUNT_WAVES (AH_COUNT_THREADS / HOT_WAVE)

/* cache the code of one value and note it in the wave's mask */
static HOT_DEV void ah_mark_put(uint32_t* s_mask, uint32_t code,
                                uint16_t* code_out) {
  *code_out = (uint16_t)code;
  if (code != VMRANGE_CODE_NONE) {
    const uint32_t bit = 1u << (code & 31);
    /* most bits are set after the first few members: test before the atomic */
    if (!(s_mask[code >> 5] & bit)) atomicOr(&s_mask[code >> 5], bit);
  }
}

__global__ __launch_bounds__(AH_MARK_THREADS) void ah_mark_kernel(
    const double* __restrict__ vals, uint32_t n_grid,
    const uint32_t* __restrict__ group_rows, const AhChunk* __restrict__ chunks,
    uint64_t n_items, uint32_t n_tiles, const double* __restrict__ thr_g,
    uint16_t* __restrict__ codes, uint32_t* masks) {
  __shared__ double s_thr[VMRANGE_TABLE_PAD];
  __shared__ uint32_t s_mask[AH_MARK_WAVES][VMRANGE_MASK_WORDS];
  for (int i = threadIdx.x; i < VMRANGE_TABLE_PAD; i += AH_MARK_THREADS)
    s_thr[i] = thr_g[i];
  __syncthreads();
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t stride = (uint64_t)gridDim.x * AH_MARK_WAVES;
  for (uint64_t it = (uint64_t)blockIdx.x * AH_MARK_WAVES + wv; it < n_items;
       it += stride) {
    const AhChunk ch = chunks[it / n_tiles];
    const uint32_t col = (uint32_t)(it % n_tiles) * AH_TILE_COLS + lane;
    if (lane < VMRANGE_MASK_WORDS) s_mask[wv][lane] = 0;
    hot_wave_sync();
    if (col < n_grid) {
      const uint32_t* rows = group_rows + ch.begin;
      uint32_t k = 0;
      /* AH_UNROLL member rows at a time: a wave's time is a chain of
       * latencies (a global load, then nine dependent LDS reads a search),
       * so the loads go out together and the searches run side by side */
      for (; k + AH_UNROLL <= ch.n; k += AH_UNROLL) {
        uint64_t idx[AH_UNROLL];
        double v[AH_UNROLL];
#pragma unroll
        for (int u = 0; u < AH_UNROLL; u++)
          idx[u] = (uint64_t)rows[k + u] * n_grid + col;
#pragma unroll
        for (int u = 0; u < AH_UNROLL; u++) v[u] = vals[idx[u]];
        uint32_t code[AH_UNROLL];
#pragma unroll
        for (int u = 0; u < AH_UNROLL; u++)
          code[u] = vmrange_bucket_search(s_thr, v[u]);
#pragma unroll
        for (int u = 0; u < AH_UNROLL; u++) {
          if (v[u] != v[u] || v[u] < 0) code[u] = VMRANGE_CODE_NONE;
          ah_mark_put(s_mask[wv], code[u], &codes[idx[u]]);
        }
      }
      for (; k < ch.n; k++) {
        const uint64_t i0 = (uint64_t)rows[k] * n_grid + col;
        ah_mark_put(s_mask[wv], vmrange_bucket_code(s_thr, vals[i0]), &codes[i0]);
      }
    }
    hot_wave_sync();
    if (lane < VMRANGE_MASK_WORDS) {
      const uint32_t m = s_mask[wv][lane];
      if (m) atomicOr(&masks[(uint64_t)ch.group * VMRANGE_MASK_WORDS + lane], m);
    }
    hot_wave_sync();
  }
}

__global__ __launch_bounds__(256) void ah_row_count_kernel(
    const uint32_t* __restrict__ masks, uint32_t n_groups,
    uint32_t* __restrict__ row_counts) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
       g < n_groups; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint4* m4 = reinterpret_cast<const uint4*>(masks + g * VMRANGE_MASK_WORDS);
    uint32_t rows = 0;
    for (int j = 0; j < VMRANGE_MASK_WORDS / 4; j++) {
      const uint4 m = m4[j];
      rows += __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
    }
    row_counts[g] = rows;
  }
}

/* one thread per (group, mask word): the rows of its set bits */
__global__ __launch_bounds__(256) void ah_row_fill_kernel(
    const uint32_t* __restrict__ masks, const uint64_t* __restrict__ row_start,
    uint32_t n_groups, uint32_t* __restrict__ row_group,
    uint16_t* __restrict__ row_code) {
  const uint64_t total = (uint64_t)n_groups * VMRANGE_MASK_WORDS;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t g = (uint32_t)(t / VMRANGE_MASK_WORDS);
    const uint32_t w = (uint32_t)(t % VMRANGE_MASK_WORDS);
    const uint32_t* gm = masks + (uint64_t)g * VMRANGE_MASK_WORDS;
    uint32_t m = gm[w];
    if (!m) continue;
    uint64_t row = row_start[g];
    for (uint32_t j = 0; j < w; j++) row += __popc(gm[j]);
    const uint64_t row_end = row_start[g + 1];
    while (m && row < row_end) {
      const uint32_t b = __ffs(m) - 1;
      row_group[row] = g;
      row_code[row] = (uint16_t)(w * 32 + b);
      row++;
      m &= m - 1;
    }
  }
}

/* local row of code c in a group: its rank among the present codes */
static HOT_DEV uint32_t ah_rank(const uint32_t* s_mask, const uint32_t* s_pre,
                                uint32_t c) {
  const uint32_t w = s_mask[c >> 5];
  return s_pre[c >> 5] + __popc(w & ((1u << (c & 31)) - 1u));
}

__global__ __launch_bounds__(AH_COUNT_THREADS) void ah_count_kernel(
    const uint16_t* __restrict__ codes, uint32_t n_grid,
    const uint32_t* __restrict__ group_rows, const AhChunk* __restrict__ chunks,
    uint64_t n_items, uint32_t n_tiles, const uint32_t* __restrict__ masks,
    const uint64_t* __restrict__ row_start, uint32_t* cnt) {
  __shared__ uint32_t s_tile[AH_COUNT_WAVES][AH_BAND_ROWS * AH_TILE_COLS];
  __shared__ uint32_t s_mask[AH_COUNT_WAVES][VMRANGE_MASK_WORDS];
  __shared__ uint32_t s_pre[AH_COUNT_WAVES][VMRANGE_MASK_WORDS];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t stride = (uint64_t)gridDim.x * AH_COUNT_WAVES;
  /* column `lane` of the tile: no other lane reads or writes it */
  uint32_t* tile = s_tile[wv] + lane;
  for (uint64_t it = (uint64_t)blockIdx.x * AH_COUNT_WAVES + wv; it < n_items;
       it += stride) {
    const AhChunk ch = chunks[it / n_tiles];
    const uint32_t col = (uint32_t)(it % n_tiles) * AH_TILE_COLS + lane;
    const uint64_t row0 = row_start[ch.group];
    const uint64_t R64 = row_start[ch.group + 1] - row0;
    if (R64 == 0 || R64 > VMRANGE_N_CODES) continue; /* wave-uniform */
    const uint32_t R = (uint32_t)R64;

    const uint32_t m = lane < VMRANGE_MASK_WORDS
        ? masks[(uint64_t)ch.group * VMRANGE_MASK_WORDS + lane] : 0u;
    const uint32_t pc = __popc(m);
    uint32_t incl = pc;
    for (int d = 1; d < VMRANGE_MASK_WORDS; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if ((int)lane >= d) incl += up;
    }
    hot_wave_sync();
    if (lane < VMRANGE_MASK_WORDS) {
      s_mask[wv][lane] = m;
      s_pre[wv][lane] = incl - pc;
    }
    hot_wave_sync();
    if (col < n_grid) { /* nothing inside crosses lanes */
      const uint32_t* rows = group_rows + ch.begin;
      for (uint32_t band0 = 0; band0 < R; band0 += AH_BAND_ROWS) {
        const uint32_t bh = HOT_MIN((uint32_t)AH_BAND_ROWS, R - band0);
        for (uint32_t r = 0; r < bh; r++) tile[r * AH_TILE_COLS] = 0;
        uint32_t k = 0;
        for (; k + AH_UNROLL <= ch.n; k += AH_UNROLL) {
          uint32_t cc[AH_UNROLL];
#pragma unroll
          for (int u = 0; u < AH_UNROLL; u++)
            cc[u] = codes[(uint64_t)rows[k + u] * n_grid + col];
          /* the ranks side by side, then the increments */
          uint32_t rr[AH_UNROLL];
#pragma unroll
          for (int u = 0; u < AH_UNROLL; u++) {
            const bool counts = cc[u] < VMRANGE_N_CODES;
            const uint32_t r = ah_rank(s_mask[wv], s_pre[wv], counts ? cc[u] : 0u);
            rr[u] = counts ? r - band0 : 0xFFFFFFFFu;
          }
#pragma unroll
          for (int u = 0; u < AH_UNROLL; u++)
            if (rr[u] < bh) tile[rr[u] * AH_TILE_COLS] += 1;
        }
        for (; k < ch.n; k++) {
          const uint32_t c = codes[(uint64_t)rows[k] * n_grid + col];
          if (c >= VMRANGE_N_CODES) continue;
          const uint32_t r = ah_rank(s_mask[wv], s_pre[wv], c) - band0;
          if (r < bh) tile[r * AH_TILE_COLS] += 1;
        }
        for (uint32_t r = 0; r < bh; r++) {
          const uint32_t v = tile[r * AH_TILE_COLS];
          if (v) atomicAdd(&cnt[(row0 + band0 + r) * n_grid + col], v);
        }
      }
    }
  }
}

/* ------------------------------------------------------------------ */
/* host side                                                          */
/* ------------------------------------------------------------------ */

namespace {

/* result of the last exec + pass-to-pass scratch; every buffer grow-only */
struct AhState {
  /* result */
  double* d_out = nullptr;          /* [n_rows x n_grid] */
  uint32_t* d_row_group = nullptr;  /* [n_rows] */
  uint16_t* d_row_code = nullptr;   /* [n_rows] */
  size_t out_cap = 0, row_group_cap = 0, row_code_cap = 0; /* bytes */
  uint64_t n_rows = 0;
  int32_t n_grid = 0;
  bool valid = false;
  /* input staging */
  double* d_vals = nullptr;         /* host-matrix form only */
  uint32_t* d_group_rows = nullptr;
  AhChunk* d_chunks = nullptr;
  size_t vals_cap = 0, group_rows_cap = 0, chunks_cap = 0;
  /* scratch */
  uint16_t* d_codes = nullptr;      /* [n_in_rows x n_grid] */
  uint32_t* d_masks = nullptr;      /* [n_groups x 16] */
  uint32_t* d_row_counts = nullptr; /* [n_groups] */
  uint64_t* d_row_start = nullptr;  /* [n_groups + 1] */
  uint32_t* d_cnt = nullptr;        /* [n_rows x n_grid] */
  size_t codes_cap = 0, masks_cap = 0, row_counts_cap = 0, row_start_cap = 0,
         cnt_cap = 0;
};

AhState g_ah;

/* Argument checks shared by both entry points; nothing is launched or
 * allocated before they pass.  Returns 0 or the vm_set_err code. */
int ah_validate(uint32_t n_in_rows, int64_t n_grid, const uint32_t* group_rows,
                const uint64_t* group_offsets, uint32_t n_groups,
                char* errbuf, size_t errbuf_len) {
  if (int rc = ah_validate_csr("aggr histogram", n_in_rows, n_grid, group_rows,
                               group_offsets, n_groups, errbuf, errbuf_len))
    return rc;
  if (n_groups == 0) return 0;
  /* a group with members has at most 488 rows: bound the result before any
   * kernel runs */
  const uint64_t max_rows =
      std::min<uint64_t>(n_groups, group_offsets[n_groups]) * VMRANGE_N_CODES;
  if (max_rows > (uint64_t)INT64_MAX / 8 / (uint64_t)n_grid)
    return vm_set_err(errbuf, errbuf_len,
                      "vmgpu: aggr histogram: result size overflows");
  return 0;
}

/* the pipeline over a device matrix; the caller holds the context lock and
 * has validated the CSR */
int ah_run(const double* d_vals, uint32_t n_in_rows, int32_t n_grid,
           const uint32_t* group_rows, const uint64_t* group_offsets,
           uint32_t n_groups, uint64_t* out_n_rows, char* errbuf,
           size_t errbuf_len) {
  AhState& a = g_ah;
  a.valid = false; /* the earlier result is replaced from here on */
  a.n_rows = 0;
  a.n_grid = n_grid;
  const uint64_t n_members = n_groups ? group_offsets[n_groups] : 0;
  if (n_members == 0) {
    a.valid = true;
    if (out_n_rows) *out_n_rows = 0;
    return 0;
  }
  const double* d_thr = vm_hot_thresholds();
  if (!d_thr)
    return vm_set_err(errbuf, errbuf_len,
                      "vmgpu: vmrange threshold table not uploaded "
                      "(vmgpu_vmrange_thresholds_set)");
  std::vector<AhChunk> chunks;
  ah_build_chunks(group_offsets, n_groups, AH_CHUNK_MEMBERS, &chunks);
  const uint32_t n_tiles = ((uint32_t)n_grid + AH_TILE_COLS - 1) / AH_TILE_COLS;
  const uint64_t n_items = (uint64_t)chunks.size() * n_tiles;

  hipStream_t st = vm_ctx_stream();
  hipEvent_t ev_start, ev_stop;
  vm_ctx_events(&ev_start, &ev_stop);

  VM_HIP_TRY(hot_reserve(&a.d_group_rows, &a.group_rows_cap, (size_t)n_members * 4),
             "alloc group rows");
  VM_HIP_TRY(hot_reserve(&a.d_chunks, &a.chunks_cap, chunks.size() * sizeof(AhChunk)),
             "alloc chunks");
  VM_HIP_TRY(hot_reserve(&a.d_codes, &a.codes_cap,
                         (size_t)n_in_rows * (size_t)n_grid * 2), "alloc codes");
  VM_HIP_TRY(hot_reserve(&a.d_masks, &a.masks_cap,
                         (size_t)n_groups * VMRANGE_MASK_WORDS * 4), "alloc masks");
  VM_HIP_TRY(hot_reserve(&a.d_row_counts, &a.row_counts_cap, (size_t)n_groups * 4),
             "alloc row counts");
  VM_HIP_TRY(hot_reserve(&a.d_row_start, &a.row_start_cap, ((size_t)n_groups + 1) * 8),
             "alloc row start");
  /* blocking copies: the host arrays are free to go when they return */
  VM_HIP_TRY(hipMemcpy(a.d_group_rows, group_rows, (size_t)n_members * 4,
                       hipMemcpyHostToDevice), "upload group rows");
  VM_HIP_TRY(hipMemcpy(a.d_chunks, chunks.data(), chunks.size() * sizeof(AhChunk),
                       hipMemcpyHostToDevice), "upload chunks");
  VM_HIP_TRY(hipMemsetAsync(a.d_masks, 0, (size_t)n_groups * VMRANGE_MASK_WORDS * 4, st),
             "zero masks");

  VM_HIP_TRY(hipEventRecord(ev_start, st), "event start");
  hipLaunchKernelGGL(ah_mark_kernel, dim3(ah_blocks(n_items, AH_MARK_WAVES)),
                     dim3(AH_MARK_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                     a.d_group_rows, a.d_chunks, n_items, n_tiles, d_thr,
                     a.d_codes, a.d_masks);
  hipLaunchKernelGGL(ah_row_count_kernel, dim3(ah_blocks(n_groups, 256)), dim3(256),
                     0, st, a.d_masks, n_groups, a.d_row_counts);
  hot_scan_launch(a.d_row_counts, n_groups, a.d_row_start, st);
  /* the output size is data-dependent: the host learns n_rows here */
  uint64_t n_rows = 0;
  VM_HIP_TRY(hipMemcpyAsync(&n_rows, a.d_row_start + n_groups, 8,
                            hipMemcpyDeviceToHost, st), "download n_rows");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync mark");
  {
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "mark kernel", kerr);
  }
  if (n_rows > std::min<uint64_t>(n_groups, n_members) * VMRANGE_N_CODES)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: inconsistent row count");

  if (n_rows) {
    const uint64_t n_out = n_rows * (uint64_t)n_grid;
    VM_HIP_TRY(hot_reserve(&a.d_out, &a.out_cap, (size_t)n_out * 8),
               "alloc histogram rows");
    VM_HIP_TRY(hot_reserve(&a.d_cnt, &a.cnt_cap, (size_t)n_out * 4), "alloc counters");
    VM_HIP_TRY(hot_reserve(&a.d_row_group, &a.row_group_cap, (size_t)n_rows * 4),
               "alloc row groups");
    VM_HIP_TRY(hot_reserve(&a.d_row_code, &a.row_code_cap, (size_t)n_rows * 2),
               "alloc row codes");
    VM_HIP_TRY(hipMemsetAsync(a.d_cnt, 0, (size_t)n_out * 4, st), "zero counters");
    hipLaunchKernelGGL(ah_row_fill_kernel,
                       dim3(ah_blocks((uint64_t)n_groups * VMRANGE_MASK_WORDS, 256)),
                       dim3(256), 0, st, a.d_masks, a.d_row_start, n_groups,
                       a.d_row_group, a.d_row_code);
    hipLaunchKernelGGL(ah_count_kernel, dim3(ah_blocks(n_items, AH_COUNT_WAVES)),
                       dim3(AH_COUNT_THREADS), 0, st, a.d_codes, (uint32_t)n_grid,
                       a.d_group_rows, a.d_chunks, n_items, n_tiles, a.d_masks,
                       a.d_row_start, a.d_cnt);
    hipLaunchKernelGGL(ah_u32_to_f64_kernel<false>, dim3(ah_blocks(n_out, 256)), dim3(256),
                       0, st, a.d_cnt, n_out, a.d_out);
  }
  VM_HIP_TRY(hipEventRecord(ev_stop, st), "event stop");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync count");
  VM_HIP_TRY(hipGetLastError(), "count kernel");
  float ms = 0;
  VM_HIP_TRY(hipEventElapsedTime(&ms, ev_start, ev_stop), "event elapsed");
  vm_ctx_set_last_kernel_ms((double)ms);
  a.n_rows = n_rows;
  a.valid = true;
  if (out_n_rows) *out_n_rows = n_rows;
  return 0;
}

}  // namespace

void vm_aggrhist_shutdown(void) {
  AhState& a = g_ah;
  (void)hipFree(a.d_out);
  (void)hipFree(a.d_row_group);
  (void)hipFree(a.d_row_code);
  (void)hipFree(a.d_vals);
  (void)hipFree(a.d_group_rows);
  (void)hipFree(a.d_chunks);
  (void)hipFree(a.d_codes);
  (void)hipFree(a.d_masks);
  (void)hipFree(a.d_row_counts);
  (void)hipFree(a.d_row_start);
  (void)hipFree(a.d_cnt);
  a = AhState();
}

extern "C" {

int vmgpu_aggr_histogram_exec(const double* values, uint32_t n_series,
                              int32_t n_grid, const uint32_t* group_rows,
                              const uint64_t* group_offsets, uint32_t n_groups,
                              uint64_t* out_n_rows, char* errbuf,
                              size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  g_ah.valid = false;
  if (int rc = ah_validate(n_series, n_grid, group_rows, group_offsets, n_groups,
                           errbuf, errbuf_len))
    return rc;
  const bool has_members = n_groups && group_offsets[n_groups];
  if (has_members) {
    if (!values)
      return vm_set_err(errbuf, errbuf_len, "vmgpu: aggr histogram: bad args");
    const size_t vbytes = (size_t)n_series * (size_t)n_grid * 8;
    VM_HIP_TRY(hot_reserve(&g_ah.d_vals, &g_ah.vals_cap, vbytes), "alloc values");
    VM_HIP_TRY(hipMemcpy(g_ah.d_vals, values, vbytes, hipMemcpyHostToDevice),
               "upload values");
  }
  return ah_run(g_ah.d_vals, n_series, n_grid, group_rows, group_offsets,
                n_groups, out_n_rows, errbuf, errbuf_len);
}

int vmgpu_batch_aggr_histogram_exec(uint64_t handle, const uint32_t* group_rows,
                                    const uint64_t* group_offsets,
                                    uint32_t n_groups, uint64_t* out_n_rows,
                                    char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  g_ah.valid = false;
  vm_batch_cols b;
  if (vm_batch_cols_get(handle, &b) != 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  if (!b.d_out || b.last_rows == 0 || b.last_grid <= 0)
    return vm_set_err(errbuf, errbuf_len,
                      "vmgpu: no rollup output on this batch "
                      "(vmgpu_rollup_exec first)");
  if (int rc = ah_validate(b.last_rows, b.last_grid, group_rows, group_offsets,
                           n_groups, errbuf, errbuf_len))
    return rc;
  return ah_run(b.d_out, b.last_rows, b.last_grid, group_rows, group_offsets,
                n_groups, out_n_rows, errbuf, errbuf_len);
}

int vmgpu_aggr_histogram_fetch(uint32_t* row_group, uint16_t* row_code,
                               double* out, char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  const AhState& a = g_ah;
  if (!a.valid)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: no aggr histogram result");
  if (a.n_rows == 0) return 0;
  hipStream_t st = vm_ctx_stream();
  if (row_group)
    VM_HIP_TRY(hipMemcpyAsync(row_group, a.d_row_group, a.n_rows * 4,
                              hipMemcpyDeviceToHost, st), "download row groups");
  if (row_code)
    VM_HIP_TRY(hipMemcpyAsync(row_code, a.d_row_code, a.n_rows * 2,
                              hipMemcpyDeviceToHost, st), "download row codes");
  if (out)
    VM_HIP_TRY(hipMemcpyAsync(out, a.d_out, (size_t)a.n_rows * a.n_grid * 8,
                              hipMemcpyDeviceToHost, st), "download histogram rows");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync fetch");
  return 0;
}

}  // extern "C"
