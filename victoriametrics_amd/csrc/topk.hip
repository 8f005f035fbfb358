/* topk.hip — the topk family (aggr.go:646-741) over the resident output of
 * a batch's last vmgpu_rollup_exec.
 *
 *   vmgpu_topk_range      topk_avg/min/max/median/last and the bottomk_*
 *       twins: one summary key per series row, then the k-th largest key by
 *       16-bit histogram refinement; the optional "remaining sum" row adds
 *       up what was not selected.
 *   vmgpu_topk_pointwise  topk / bottomk: per grid column, the k-th largest
 *       key by the same 16-bit histogram refinement, one 65536-bin histogram
 *       per column and round; what lies below it is set to NaN in place.
 *
 * Reaches the batch through batch_access.h and runs on the context stream
 * under the context lock, like hot.hip.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <vector>

#include "batch_access.h"
#include "hot_common.h"
#include "rollup_device.h"
#include "../../include/vmgpu.h"

/* the launch geometry of vmgpu.hip */
#define WAVE 64
#define BLOCK_THREADS 256
#define WAVES_PER_BLOCK (BLOCK_THREADS / WAVE)

/* Order-preserving u64 key for f64 under lessWithNaNs / greaterWithNaNs
 * (aggr.go:1259-1279): selection always keeps the "k largest keys".  NaN
 * maps to the SMALLEST key in both directions — lessWithNaNs treats NaN as
 * smaller than any number (so topk never keeps it) and greaterWithNaNs
 * treats it as bigger (so it sorts to the FRONT of the bottomk order and
 * is again never kept). */
static VM_DEV unsigned long long vm_topk_key(double v, int reverse) {
  if (vm_isnan(v)) return 0ULL;
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
  unsigned long long ord = (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
  /* the NaN sentinels 0 and ~0 are unreachable for non-NaN doubles: their
   * preimages under the order map are NaN bit patterns */
  return reverse ? ~ord : ord;
}

/* inverse of vm_topk_key's order map (non-NaN keys only) */
static VM_DEV double vm_topk_key_inv(unsigned long long ord) {
  unsigned long long b = (ord & 0x8000000000000000ULL)
                             ? (ord ^ 0x8000000000000000ULL)
                             : ~ord;
  return __longlong_as_double((long long)b);
}

/* k-th smallest (0-based) non-NaN key of a row: 8 passes of 256-bin LDS
 * histogram refinement over the order-preserving u64 keys (exact — every
 * byte of the result is pinned by counts).  hist: per-wave uint32[256]. */
static __device__ unsigned long long topk_row_kth(
    const double* row, int32_t n_grid, uint32_t k, int lane, uint32_t* hist) {
  unsigned long long prefix = 0;
  for (int byte = 7; byte >= 0; byte--) {
    const int shift = byte * 8;
    for (int b = lane; b < 256; b += WAVE) hist[b] = 0;
    hot_wave_sync();
    const unsigned long long pmask =
        (byte == 7) ? 0ULL : (~0ULL << (shift + 8));
    for (int g = lane; g < n_grid; g += WAVE) {
      double v = row[g];
      if (vm_isnan(v)) continue;
      unsigned long long key = vm_topk_key(v, 0);
      if ((key & pmask) != prefix) continue;
      atomicAdd(&hist[(key >> shift) & 0xff], 1u);
    }
    hot_wave_sync();
    /* each lane owns 4 consecutive bins; exclusive wave prefix of totals */
    uint32_t b0 = hist[lane * 4], b1 = hist[lane * 4 + 1];
    uint32_t b2 = hist[lane * 4 + 2], b3 = hist[lane * 4 + 3];
    uint32_t lt = b0 + b1 + b2 + b3;
    uint32_t ex = lt;
    for (int d = 1; d < WAVE; d <<= 1) {
      uint32_t xo = __shfl_up(ex, d);
      if (lane >= d) ex += xo;
    }
    ex -= lt;
    uint32_t c0 = ex, c1 = c0 + b0, c2 = c1 + b1, c3 = c2 + b2;
    int pick = -1;
    if (k >= c0 && k < c0 + b0) pick = 0;
    else if (k >= c1 && k < c1 + b1) pick = 1;
    else if (k >= c2 && k < c2 + b2) pick = 2;
    else if (k >= c3 && k < c3 + b3) pick = 3;
    uint64_t mb = __ballot(pick >= 0);
    int srcl = __ffsll((unsigned long long)mb) - 1;
    int pickv = __shfl(pick, srcl);
    uint32_t below = __shfl(pickv == 0 ? c0 : pickv == 1 ? c1
                            : pickv == 2 ? c2 : c3, srcl);
    int bin = srcl * 4 + pickv;
    k -= below;
    prefix |= ((unsigned long long)(unsigned)bin) << shift;
    hot_wave_sync();
  }
  return prefix;
}

/* per-series range summaries (aggr.go:804-858), one wave per series row */
__global__ __launch_bounds__(BLOCK_THREADS) void topk_summary_kernel(
    const double* values, uint32_t n_series, int32_t n_grid, int32_t op,
    int32_t reverse, unsigned long long* keys) {
  __shared__ uint32_t sh_hist[WAVES_PER_BLOCK][256];
  const int wave_in_block = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  uint32_t wid = blockIdx.x * WAVES_PER_BLOCK + wave_in_block;
  uint32_t stride = gridDim.x * WAVES_PER_BLOCK;
  for (uint32_t s = wid; s < n_series; s += stride) {
    const double* row = values + (size_t)s * n_grid;
    double acc = vm_dnan();
    if (op == 0 || op == 1 || op == 2) { /* avg / min / max */
      double sum = 0, cnt = 0;
      double mn = vm_dnan(), mx = vm_dnan();
      for (int g = lane; g < n_grid; g += WAVE) {
        double v = row[g];
        if (vm_isnan(v)) continue;
        cnt += 1;
        sum += v;
        if (vm_isnan(mn) || v < mn) mn = v;
        if (vm_isnan(mx) || v > mx) mx = v;
      }
      for (int d = 32; d > 0; d >>= 1) {
        double so = __shfl_down(sum, d);
        double co = __shfl_down(cnt, d);
        double mno = __shfl_down(mn, d);
        double mxo = __shfl_down(mx, d);
        sum += so;
        cnt += co;
        if (vm_isnan(mn) || (!vm_isnan(mno) && mno < mn)) mn = mno;
        if (vm_isnan(mx) || (!vm_isnan(mxo) && mxo > mx)) mx = mxo;
      }
      if (op == 0) acc = (cnt == 0) ? vm_dnan() : sum / cnt;
      else if (op == 1) acc = mn;
      else acc = mx;
    } else if (op == 3) { /* median = quantile(0.5) (aggr.go:848,922) */
      uint32_t m = 0;
      for (int g = lane; g < n_grid; g += WAVE)
        if (!vm_isnan(row[g])) m++;
      for (int d = 32; d > 0; d >>= 1) m += __shfl_down(m, d);
      m = __shfl(m, 0);
      if (m > 0) {
        uint32_t li = (m - 1) / 2; /* floor(0.5*(m-1)) */
        unsigned long long kv =
            topk_row_kth(row, n_grid, li, lane, sh_hist[wave_in_block]);
        double vlo = vm_topk_key_inv(kv);
        if (m & 1) {
          acc = vlo; /* odd count: weight 0 */
        } else {
          /* upper = positional li+1 in the sorted row: equals vlo inside
           * an equal run, else the smallest key > kv */
          uint32_t cle = 0; /* #keys <= kv */
          unsigned long long nxt = ~0ULL;
          for (int g = lane; g < n_grid; g += WAVE) {
            double v = row[g];
            if (vm_isnan(v)) continue;
            unsigned long long key = vm_topk_key(v, 0);
            if (key <= kv) cle++;
            else if (key < nxt) nxt = key;
          }
          for (int d = 32; d > 0; d >>= 1) {
            cle += __shfl_down(cle, d);
            unsigned long long no = __shfl_down(nxt, d);
            if (no < nxt) nxt = no;
          }
          cle = __shfl(cle, 0);
          nxt = __shfl(nxt, 0);
          double vhi = (li + 1 < cle) ? vlo : vm_topk_key_inv(nxt);
          /* quantileSorted: v[lower]*(1-weight) + v[upper]*weight, w=0.5 */
          acc = vlo * 0.5 + vhi * 0.5;
        }
      }
    } else if (op == 4) { /* last non-NaN */
      int base = ((n_grid + WAVE - 1) / WAVE - 1) * WAVE;
      for (; base >= 0; base -= WAVE) {
        int g = base + lane;
        double v = (g < n_grid) ? row[g] : vm_dnan();
        uint64_t m = __ballot(!vm_isnan(v));
        if (m) {
          int hi = 63 - __clzll((unsigned long long)m);
          acc = __shfl(v, hi);
          break;
        }
      }
    }
    if (lane == 0) keys[s] = vm_topk_key(acc, reverse);
  }
}

__global__ void topk_hist_kernel(const unsigned long long* keys, uint32_t n,
                                 unsigned long long prefix, int shift,
                                 uint32_t* hist) {
  /* 16-bit histogram of keys whose bits above shift+16 equal prefix */
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t stride = gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    unsigned long long k = keys[i];
    if (shift < 48 && (k >> (shift + 16)) != prefix) continue;
    atomicAdd(&hist[(k >> shift) & 0xffff], 1u);
  }
}

__global__ void topk_collect_kernel(const unsigned long long* keys, uint32_t n,
                                    unsigned long long kstar, uint32_t ties_quota,
                                    uint32_t* counters, uint32_t* sel,
                                    uint32_t sel_cap) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t stride = gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    unsigned long long k = keys[i];
    if (k > kstar) {
      uint32_t slot = atomicAdd(&counters[0], 1u);
      if (slot < sel_cap) sel[slot] = i;
    } else if (k == kstar) {
      uint32_t t = atomicAdd(&counters[1], 1u);
      if (t < ties_quota) {
        uint32_t slot = atomicAdd(&counters[0], 1u);
        if (slot < sel_cap) sel[slot] = i;
      }
    }
  }
}

__global__ void topk_remaining_kernel(const double* values, uint32_t n_series,
                                      int32_t n_grid, const uint8_t* selected,
                                      double* rem_sum, double* rem_cnt) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)n_series * n_grid;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    uint32_t s = (uint32_t)(i / n_grid);
    int32_t g = (int32_t)(i % n_grid);
    if (selected[s]) continue;
    double v = values[i];
    if (vm_isnan(v)) continue;
    atomicAdd(&rem_sum[g], v);
    atomicAdd(&rem_cnt[g], 1.0);
  }
}

/* ---- pointwise topk over [n_series x n_grid] ---- */

/* One refinement round: per column, the 16-bit histogram of the key bits at
 * shift, over the keys whose bits above shift+16 equal the column's prefix
 * (every key in the first round, shift 48). */
__global__ void topk_col_hist_kernel(const double* values, uint32_t n_series,
                                     int32_t n_grid, int32_t reverse,
                                     const unsigned long long* prefix_of_col,
                                     int shift, uint32_t* hists) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)n_series * n_grid;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    int32_t g = (int32_t)(i % n_grid);
    unsigned long long k = vm_topk_key(values[i], reverse);
    if (shift < 48 && (k >> (shift + 16)) != prefix_of_col[g]) continue;
    atomicAdd(&hists[(size_t)g * 65536 + ((k >> shift) & 0xffff)], 1u);
  }
}

/* One block per column: walks the column's histogram from the top bin down
 * to the bin that holds the need-th largest key still in play, appends that
 * bin to the column's prefix and takes the keys above it off the need.
 * After the fourth round the prefix is the k-th largest key of the column
 * and the need is how many keys equal to it are kept.  k0 seeds the need in
 * the first round (first != 0). */
__global__ __launch_bounds__(BLOCK_THREADS) void topk_col_refine_kernel(
    const uint32_t* hists, int32_t n_grid, uint32_t k0, int32_t first,
    unsigned long long* prefix_of_col, uint32_t* need_of_col) {
  int g = blockIdx.x;
  if (g >= n_grid) return;
  const uint32_t* h = hists + (size_t)g * 65536;
  /* sh_sum[c]: total of the 256 bins [c*256, c*256+256) */
  __shared__ uint32_t sh_sum[BLOCK_THREADS];
  __shared__ uint32_t sh_bin[BLOCK_THREADS];
  __shared__ uint32_t sh_chunk, sh_cum;
  const int t = threadIdx.x;
  sh_sum[t] = 0;
  __syncthreads();
  for (int c = 0; c < 256; c++) {
    uint32_t v = h[c * 256 + t];
    if (v) atomicAdd(&sh_sum[c], v);
  }
  __syncthreads();
  const uint32_t need = first ? k0 : need_of_col[g];
  if (t == 0) {
    uint32_t cum = 0;
    int chunk = 0;
    for (int c = 255; c >= 0; c--) {
      uint32_t s = sh_sum[c];
      if (cum + s >= need) {
        chunk = c;
        break;
      }
      cum += s;
    }
    sh_chunk = (uint32_t)chunk;
    sh_cum = cum;
  }
  __syncthreads();
  sh_bin[t] = h[sh_chunk * 256 + t];
  __syncthreads();
  if (t == 0) {
    uint32_t cum = sh_cum;
    int bin = 0;
    for (int b = 255; b >= 0; b--) {
      uint32_t c = sh_bin[b];
      if (cum + c >= need) {
        bin = b;
        break;
      }
      cum += c;
    }
    unsigned long long prefix = first ? 0ULL : prefix_of_col[g];
    prefix_of_col[g] = (prefix << 16) | (unsigned long long)(sh_chunk * 256 + bin);
    need_of_col[g] = need - cum;
  }
}

/* NaN-fills what lies below the column's k-th largest key; of the keys equal
 * to it, the first ties_of_col[g] to arrive stay (the reference's sort is
 * unstable: which of several equal boundary values survives is unspecified
 * there too). */
__global__ void topk_col_fill_kernel(double* values, uint32_t n_series,
                                     int32_t n_grid, int32_t reverse,
                                     const unsigned long long* kstar_of_col,
                                     const uint32_t* ties_of_col,
                                     uint32_t* ties_taken) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)n_series * n_grid;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    int32_t g = (int32_t)(i % n_grid);
    unsigned long long key = vm_topk_key(values[i], reverse);
    if (key == 0) continue; /* NaN stays NaN whether kept or not */
    unsigned long long kstar = kstar_of_col[g];
    bool keep;
    if (key > kstar) {
      keep = true;
    } else if (key == kstar) {
      uint32_t t = atomicAdd(&ties_taken[g], 1u);
      keep = t < ties_of_col[g];
    } else {
      keep = false;
    }
    if (!keep) values[i] = vm_dnan();
  }
}

extern "C" {

int vmgpu_topk_range(uint64_t handle, double k, int32_t summary_op,
                     int32_t reverse, int64_t* out_sel, int64_t* out_n_sel,
                     double* out_remaining, char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited()) return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  vm_batch_cols b;
  if (vm_batch_cols_get(handle, &b) != 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  if (!b.d_out || b.last_rows == 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: no evaluated output on this batch");
  uint32_t n = b.last_rows;
  int32_t n_grid = b.last_grid;
  uint32_t kk = 0;
  if (k == k && k > 0) kk = (k > (double)n) ? n : (uint32_t)k;
  if (out_n_sel) *out_n_sel = 0;
  if (kk == 0) return 0;

  hipStream_t st = vm_ctx_stream();
  VmPoolBuf<unsigned long long> keys_buf;
  VmPoolBuf<uint32_t> hist_buf, misc_buf, sel_buf;
  VM_HIP_TRY(keys_buf.alloc((size_t)n * 8), "alloc keys");
  VM_HIP_TRY(hist_buf.alloc(65536 * 4), "alloc hist");
  VM_HIP_TRY(misc_buf.alloc(8), "alloc counters");
  VM_HIP_TRY(sel_buf.alloc((size_t)kk * 4), "alloc sel");
  unsigned long long* d_keys = keys_buf.p;
  uint32_t* d_hist = hist_buf.p;
  uint32_t* d_misc = misc_buf.p; /* counters */
  uint32_t* d_sel = sel_buf.p;
  uint32_t blocks = std::min<uint32_t>((n + BLOCK_THREADS - 1) / BLOCK_THREADS * WAVES_PER_BLOCK, 2048);
  hipLaunchKernelGGL(topk_summary_kernel, dim3(blocks), dim3(BLOCK_THREADS), 0, st,
                     b.d_out, n, n_grid, summary_op, reverse, d_keys);
  /* refine the k-th largest key threshold 16 bits at a time */
  unsigned long long prefix = 0;
  uint32_t need_above = kk; /* how many keys >= threshold so far required */
  std::vector<uint32_t> hist(65536);
  uint32_t above_total = 0;
  for (int shift = 48; shift >= 0; shift -= 16) {
    VM_HIP_TRY(hipMemsetAsync(d_hist, 0, 65536 * 4, st), "zero hist");
    uint32_t hblocks = std::min<uint32_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(topk_hist_kernel, dim3(hblocks), dim3(256), 0, st,
                       d_keys, n, prefix, shift, d_hist);
    VM_HIP_TRY(hipMemcpyAsync(hist.data(), d_hist, 65536 * 4, hipMemcpyDeviceToHost, st), "dl hist");
    VM_HIP_TRY(hipStreamSynchronize(st), "sync hist");
    uint32_t cum = 0;
    int bin = 0;
    for (int bb = 65535; bb >= 0; bb--) {
      uint32_t c = hist[bb];
      if (cum + c >= need_above - above_total) { bin = bb; break; }
      cum += c;
    }
    above_total += cum;
    prefix = (prefix << 16) | (unsigned long long)bin;
  }
  unsigned long long kstar = prefix;
  uint32_t ties_quota = need_above - above_total;
  VM_HIP_TRY(hipMemsetAsync(d_misc, 0, 8, st), "zero counters");
  uint32_t cblocks = std::min<uint32_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(topk_collect_kernel, dim3(cblocks), dim3(256), 0, st,
                     d_keys, n, kstar, ties_quota, d_misc, d_sel, kk);
  std::vector<uint32_t> sel(kk);
  uint32_t nsel_h[2];
  VM_HIP_TRY(hipMemcpyAsync(sel.data(), d_sel, (size_t)kk * 4, hipMemcpyDeviceToHost, st), "dl sel");
  VM_HIP_TRY(hipMemcpyAsync(nsel_h, d_misc, 8, hipMemcpyDeviceToHost, st), "dl counters");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync sel");
  uint32_t m = std::min<uint32_t>(nsel_h[0], kk);
  /* order the selection by key descending (reference output order after
   * reverseSeries): download keys of the selected rows */
  std::vector<unsigned long long> skeys(m);
  for (uint32_t x = 0; x < m; x++) {
    VM_HIP_TRY(hipMemcpyAsync(&skeys[x], d_keys + sel[x], 8, hipMemcpyDeviceToHost, st), "dl key");
  }
  VM_HIP_TRY(hipStreamSynchronize(st), "sync keys");
  std::vector<uint32_t> order(m);
  for (uint32_t x = 0; x < m; x++) order[x] = x;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t bx) {
    if (skeys[a] != skeys[bx]) return skeys[a] > skeys[bx];
    /* ties: descending row id, matching the oracle's reversed ascending
     * sort (the reference's own sort is unstable: tie order unspecified) */
    return sel[a] > sel[bx];
  });
  for (uint32_t x = 0; x < m; x++) out_sel[x] = (int64_t)sel[order[x]];
  if (out_n_sel) *out_n_sel = (int64_t)m;

  if (out_remaining) {
    VmPoolBuf<uint8_t> mask_buf;
    VmPoolBuf<double> rem_buf;
    VM_HIP_TRY(mask_buf.alloc(n), "alloc mask");
    VM_HIP_TRY(rem_buf.alloc((size_t)n_grid * 16), "alloc rem");
    uint8_t* d_mask = mask_buf.p;
    double* d_rem = rem_buf.p;
    VM_HIP_TRY(hipMemsetAsync(d_mask, 0, n, st), "zero mask");
    VM_HIP_TRY(hipMemsetAsync(d_rem, 0, (size_t)n_grid * 16, st), "zero rem");
    std::vector<uint8_t> mask(n, 0);
    for (uint32_t x = 0; x < m; x++) mask[sel[x]] = 1;
    VM_HIP_TRY(hipMemcpyAsync(d_mask, mask.data(), n, hipMemcpyHostToDevice, st), "ul mask");
    uint32_t rblocks = std::min<uint32_t>(
        (uint32_t)(((size_t)n * n_grid + 255) / 256), 4096u);
    hipLaunchKernelGGL(topk_remaining_kernel, dim3(rblocks), dim3(256), 0, st,
                       b.d_out, n, n_grid, d_mask, d_rem, d_rem + n_grid);
    std::vector<double> rem(2 * (size_t)n_grid);
    VM_HIP_TRY(hipMemcpyAsync(rem.data(), d_rem, (size_t)n_grid * 16, hipMemcpyDeviceToHost, st), "dl rem");
    VM_HIP_TRY(hipStreamSynchronize(st), "sync rem");
    for (int32_t g = 0; g < n_grid; g++)
      out_remaining[g] = (rem[n_grid + g] == 0) ? __builtin_nan("") : rem[g];
  }
  return 0;
}

int vmgpu_topk_pointwise(uint64_t handle, double k, int32_t reverse,
                         double* out, char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited()) return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  vm_batch_cols b;
  if (vm_batch_cols_get(handle, &b) != 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  if (!b.d_out || b.last_rows == 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: no evaluated output on this batch");
  uint32_t n = b.last_rows;
  int32_t n_grid = b.last_grid;
  uint32_t kk = 0;
  if (k == k && k > 0) kk = (k > (double)n) ? n : (uint32_t)k;
  hipStream_t st = vm_ctx_stream();
  if (kk >= n || n == 0) {
    if (out) {
      VM_HIP_TRY(hipMemcpyAsync(out, b.d_out, (size_t)n * n_grid * 8,
                             hipMemcpyDeviceToHost, st), "dl out");
      VM_HIP_TRY(hipStreamSynchronize(st), "sync");
    }
    return 0;
  }
  /* the k-th largest key of every column, 16 bits per round: five scans of
   * the matrix in all, for any number of equal or near-equal values */
  VmPoolBuf<uint32_t> hists_buf, small_buf;
  VmPoolBuf<unsigned long long> kstar_buf;
  VM_HIP_TRY(hists_buf.alloc((size_t)n_grid * 65536 * 4), "alloc col hists");
  VM_HIP_TRY(kstar_buf.alloc((size_t)n_grid * 8), "alloc kstar");
  VM_HIP_TRY(small_buf.alloc((size_t)n_grid * 8), "alloc small");
  uint32_t* d_hists = hists_buf.p;
  unsigned long long* d_kstar = kstar_buf.p; /* prefix while refining */
  uint32_t* d_need = small_buf.p;            /* ties to keep, at the end */
  uint32_t* d_taken = small_buf.p + n_grid;
  VM_HIP_TRY(hipMemsetAsync(d_taken, 0, (size_t)n_grid * 4, st), "zero taken");
  size_t total = (size_t)n * n_grid;
  uint32_t eblocks = (uint32_t)std::min<size_t>((total + 255) / 256, 4096);
  for (int shift = 48; shift >= 0; shift -= 16) {
    VM_HIP_TRY(hipMemsetAsync(d_hists, 0, (size_t)n_grid * 65536 * 4, st), "zero hists");
    hipLaunchKernelGGL(topk_col_hist_kernel, dim3(eblocks), dim3(256), 0, st,
                       b.d_out, n, n_grid, reverse, d_kstar, shift, d_hists);
    hipLaunchKernelGGL(topk_col_refine_kernel, dim3(n_grid),
                       dim3(BLOCK_THREADS), 0, st, d_hists, n_grid, kk,
                       shift == 48 ? 1 : 0, d_kstar, d_need);
  }
  hipLaunchKernelGGL(topk_col_fill_kernel, dim3(eblocks), dim3(256), 0, st,
                     b.d_out, n, n_grid, reverse, d_kstar, d_need, d_taken);
  if (out) {
    VM_HIP_TRY(hipMemcpyAsync(out, b.d_out, total * 8, hipMemcpyDeviceToHost, st), "dl out");
  }
  VM_HIP_TRY(hipStreamSynchronize(st), "sync fill");
  hipError_t kerr = hipGetLastError();
  if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "topk kernel", kerr);
  return 0;
}

}  /* extern "C" */
