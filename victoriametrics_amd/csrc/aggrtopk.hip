/* aggrtopk.hip — the grouped pointwise topk / bottomk aggregate
 * (`topk(k, q) by (...)`, newAggrFuncTopK, aggr.go:646-675) on the device.
 *
 * Input: a device matrix vals[n_in_rows x n_grid] (f64, row-major, only ever
 * read) and the member CSR of aggrhist.hip / aggrcv.hip.  Every (group, grid
 * column c) is a problem of its own: the group's members are numbered
 * p = 0..n-1 in CSR order, kn = getIntK(ks[c], n) of them are kept, and kept
 * are the kn largest under the composite order (value key, then p).  The
 * value key is topk.hip's order-preserving u64 (inverted for bottomk) with
 * -0.0 folded onto +0.0 first, since lessWithNaNs sees them equal; every NaN
 * has key 0, the smallest in both directions, and is never kept.  Of equal
 * values the member LATER in the member list wins, which is the oracle's
 * rule (oracle/topk.c cmp_kv), so the result is a pure function of the
 * input: no atomic decides anything here.
 *
 * The output is SPARSE: one row per member position that keeps at least one
 * value, ordered by group and then by member position; a kept cell carries
 * the input's own bits, every other cell HOT_NAN_BITS.
 *
 *   pass 1, threshold: per (group, column) the pair (kstar, pstar) with
 *       cell kept  <=>  key > kstar || (key == kstar && p >= pstar).
 *       kn == 0 gives (~0, ~0), which nothing passes; "every non-NaN" is
 *       (0, ~0).  Two classes, chosen per group on the host from
 *       K = min(n, max over c of getIntK(ks[c], inf)):
 *     list class, K <= AT_LIST_CAP (at_list_kernel): aggr_sparse.h's
 *       geometry, one wavefront per (chunk of AT_CHUNK_MEMBERS members, tile
 *       of 64 columns), lane = column.  The wave walks the chunk's members in
 *       order, one coalesced 512-byte read a member, AT_UNROLL of them in
 *       flight.  Each lane keeps its kn best (key, p) pairs in an unsorted
 *       LDS list laid out [slot][lane], so a lane's bank depends on the lane
 *       alone and lanes at different slots never conflict; the list's
 *       minimum lives in registers, so a value that does not enter costs one
 *       compare and no LDS traffic, and one that enters costs a rescan of kn
 *       slots.  A group of one chunk writes its thresholds directly; the
 *       chunks of a longer group write their lists to a partial buffer and
 *       at_merge_kernel (one lane per (group, column), the same list code)
 *       reduces them.
 *     sort class, K > AT_LIST_CAP (at_sort_kernel): per (group, column) the
 *       n keys are gathered and sorted ascending with cvot_sort in cvot.hip's
 *       three size classes (one wave in its LDS slab up to CVOT_WAVE_CAP, one
 *       workgroup in LDS up to CVOT_BLOCK_CAP, one workgroup in global
 *       scratch above).  kstar = sorted[n - kn], ties = kn - #(keys > kstar),
 *       and pstar is the position of the ties-th member from the END whose
 *       key equals kstar, found by a backward ballot count.
 *   pass 2, mark (at_mark_kernel): (chunk, tile) items again; a member with
 *       any kept lane stores 1 to row_counts[member] (the same value from
 *       every tile: a plain store).  hot_scan_launch turns the flags into
 *       output rows.
 *   pass 3, fill (at_fill_kernel): the kept members only, found 64 at a time
 *       by a ballot over the flags: out, row_group, row_src, row_last.
 *
 * LDS: at AT_LIST_CAP 16 a wave's lists take 16 x 64 x (8 + 4) = 12 KiB.
 * The list kernels run AT_LIST_THREADS = 128 threads, two waves and 24 KiB a
 * workgroup, so six workgroups (12 waves) fit the CU's 160 KiB.
 *
 * Global sort scratch: one slab of the longest global-class group per
 * workgroup in flight, at most AT_SORT_BLOCKS workgroups and at most
 * AT_SORT_SCRATCH_MIB MiB in all (never less than one slab).
 *
 * The result lives in one file-static slot, grow-only (hot_reserve), guarded
 * by the context lock; everything else is pool scratch freed on return.
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
#include "value_key.h"
#include "../../include/vmgpu.h"

/* members of one group per work item */
#define AT_CHUNK_MEMBERS 512
/* largest K a lane's LDS list holds; above it the group is sorted */
#define AT_LIST_CAP 16
/* member rows a lane keeps in flight */
#define AT_UNROLL 8
/* workgroup of the list and merge kernels: 2 waves, 24 KiB of LDS */
#define AT_LIST_THREADS 128
/* workgroups of the global sort class in flight */
#define AT_SORT_BLOCKS 256
/* bound of the global sort scratch */
#define AT_SORT_SCRATCH_MIB 1024
#define AT_TILE_COLS HOT_WAVE
#define AT_LIST_WAVES (AT_LIST_THREADS / HOT_WAVE)
#define AT_PART_DIRECT 0xFFFFFFFFu /* one chunk: thresholds written directly */
#define AT_PART_SORT 0xFFFFFFFEu   /* sort class */
#define AT_KEY_MAX 0xFFFFFFFFFFFFFFFFULL
#define AT_POS_MAX 0xFFFFFFFFu

/* vm_topk_key (topk.hip) with -0.0 folded onto +0.0; 0 for every NaN */
static HOT_DEV uint64_t at_key(double v, int reverse) {
  if (v != v) return 0ULL;
  if (v == 0.0) v = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint64_t ord = (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
  return reverse ? ~ord : ord;
}

/* getIntK clamped to the n members of the group (n < 2^32) */
static HOT_DEV uint32_t at_int_k(double k, uint32_t n) {
  if (!(k >= 1.0)) return 0; /* NaN, negatives and everything truncating to 0 */
  if (k >= (double)n) return n;
  return (uint32_t)k;
}

/* threshold of a (group, column) whose kn best are known: cnt of them were
 * found (fewer than kn only when the group has fewer non-NaN values), the
 * smallest being (minkey, minpos) */
static HOT_DEV void at_store_threshold(uint64_t* thr_key, uint32_t* thr_pos,
                                       uint64_t at, uint32_t kn, uint32_t cnt,
                                       uint64_t minkey, uint32_t minpos) {
  uint64_t kstar = minkey;
  uint32_t pstar = minpos;
  if (kn == 0) {
    kstar = AT_KEY_MAX;
    pstar = AT_POS_MAX;
  } else if (cnt < kn) {
    kstar = 0;
    pstar = AT_POS_MAX;
  }
  thr_key[at] = kstar;
  thr_pos[at] = pstar;
}

static HOT_DEV bool at_kept(uint64_t key, uint32_t p, uint64_t kstar,
                            uint32_t pstar) {
  return key > kstar || (key == kstar && p >= pstar);
}

/* a lane's list: column `lane` of keys[slot * 64 + lane] / pos[...] */
struct AtLane {
  uint64_t minkey;
  uint32_t minpos, minslot;
  uint32_t cnt, kn;
};

static HOT_DEV void at_list_push(AtLane& ln, uint64_t* keys, uint32_t* pos,
                                 uint64_t key, uint32_t p) {
  if (key == 0) return; /* a NaN is never kept */
  if (ln.cnt < ln.kn) {
    keys[ln.cnt * HOT_WAVE] = key;
    pos[ln.cnt * HOT_WAVE] = p;
    if (ln.cnt == 0 || key < ln.minkey || (key == ln.minkey && p < ln.minpos)) {
      ln.minkey = key;
      ln.minpos = p;
      ln.minslot = ln.cnt;
    }
    ln.cnt++;
    return;
  }
  /* the common case: one compare against registers */
  if (key < ln.minkey || (key == ln.minkey && p < ln.minpos)) return;
  keys[ln.minslot * HOT_WAVE] = key;
  pos[ln.minslot * HOT_WAVE] = p;
  ln.minkey = AT_KEY_MAX;
  ln.minpos = AT_POS_MAX;
  for (uint32_t j = 0; j < ln.kn; j++) {
    const uint64_t k2 = keys[j * HOT_WAVE];
    const uint32_t p2 = pos[j * HOT_WAVE];
    if (k2 < ln.minkey || (k2 == ln.minkey && p2 < ln.minpos)) {
      ln.minkey = k2;
      ln.minpos = p2;
      ln.minslot = j;
    }
  }
}

__global__ __launch_bounds__(AT_LIST_THREADS) void at_list_kernel(
    const double* __restrict__ vals, uint32_t n_grid,
    const uint32_t* __restrict__ group_rows, const AhChunk* __restrict__ chunks,
    uint64_t n_items, uint32_t n_tiles, const uint64_t* __restrict__ goff,
    const uint32_t* __restrict__ group_part, const double* __restrict__ ks,
    int reverse, uint64_t* __restrict__ thr_key, uint32_t* __restrict__ thr_pos,
    uint64_t* __restrict__ part_keys, uint32_t* __restrict__ part_pos,
    uint32_t* __restrict__ part_cnt) {
  __shared__ uint64_t s_keys[AT_LIST_WAVES][AT_LIST_CAP * HOT_WAVE];
  __shared__ uint32_t s_pos[AT_LIST_WAVES][AT_LIST_CAP * HOT_WAVE];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t stride = (uint64_t)gridDim.x * AT_LIST_WAVES;
  /* column `lane` of the lists: no other lane reads or writes it */
  uint64_t* keys = s_keys[wv] + lane;
  uint32_t* pos = s_pos[wv] + lane;
  for (uint64_t it = (uint64_t)blockIdx.x * AT_LIST_WAVES + wv; it < n_items;
       it += stride) {
    const AhChunk ch = chunks[it / n_tiles];
    const uint32_t part = group_part[ch.group];
    if (part == AT_PART_SORT) continue; /* wave-uniform */
    const uint32_t col = (uint32_t)(it % n_tiles) * AT_TILE_COLS + lane;
    if (col >= n_grid) continue; /* nothing below crosses lanes */
    const uint64_t g0 = goff[ch.group];
    const uint32_t n = (uint32_t)(goff[ch.group + 1] - g0);
    const uint32_t p0 = (uint32_t)(ch.begin - g0);
    AtLane ln;
    ln.minkey = AT_KEY_MAX;
    ln.minpos = AT_POS_MAX;
    ln.minslot = 0;
    ln.cnt = 0;
    /* the host put the group here because no column asks for more */
    ln.kn = HOT_MIN(at_int_k(ks[col], n), (uint32_t)AT_LIST_CAP);
    if (ln.kn) {
      const uint32_t* rows = group_rows + ch.begin;
      const double* vcol = vals + col;
      uint32_t k = 0;
      for (; k + AT_UNROLL <= ch.n; k += AT_UNROLL) {
        double v[AT_UNROLL];
#pragma unroll
        for (int u = 0; u < AT_UNROLL; u++)
          v[u] = vcol[(uint64_t)rows[k + u] * n_grid];
#pragma unroll
        for (int u = 0; u < AT_UNROLL; u++)
          at_list_push(ln, keys, pos, at_key(v[u], reverse), p0 + k + u);
      }
      for (; k < ch.n; k++)
        at_list_push(ln, keys, pos,
                     at_key(vcol[(uint64_t)rows[k] * n_grid], reverse), p0 + k);
    }
    if (part == AT_PART_DIRECT) {
      at_store_threshold(thr_key, thr_pos, (uint64_t)ch.group * n_grid + col,
                         ln.kn, ln.cnt, ln.minkey, ln.minpos);
    } else {
      const uint64_t pi = (uint64_t)part + p0 / AT_CHUNK_MEMBERS;
      part_cnt[pi * n_grid + col] = ln.cnt;
      for (uint32_t j = 0; j < ln.cnt; j++) {
        const uint64_t at = (pi * AT_LIST_CAP + j) * n_grid + col;
        part_keys[at] = keys[j * HOT_WAVE];
        part_pos[at] = pos[j * HOT_WAVE];
      }
    }
  }
}

/* the partial lists of a group of several chunks -> its thresholds; one lane
 * per (group, column), a wave per (group, tile) */
__global__ __launch_bounds__(AT_LIST_THREADS) void at_merge_kernel(
    const uint32_t* __restrict__ merge_groups, uint64_t n_items,
    uint32_t n_tiles, uint32_t n_grid, const uint64_t* __restrict__ goff,
    const uint32_t* __restrict__ group_part, const double* __restrict__ ks,
    const uint64_t* __restrict__ part_keys,
    const uint32_t* __restrict__ part_pos,
    const uint32_t* __restrict__ part_cnt, uint64_t* __restrict__ thr_key,
    uint32_t* __restrict__ thr_pos) {
  __shared__ uint64_t s_keys[AT_LIST_WAVES][AT_LIST_CAP * HOT_WAVE];
  __shared__ uint32_t s_pos[AT_LIST_WAVES][AT_LIST_CAP * HOT_WAVE];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t stride = (uint64_t)gridDim.x * AT_LIST_WAVES;
  uint64_t* keys = s_keys[wv] + lane;
  uint32_t* pos = s_pos[wv] + lane;
  for (uint64_t it = (uint64_t)blockIdx.x * AT_LIST_WAVES + wv; it < n_items;
       it += stride) {
    const uint32_t g = merge_groups[it / n_tiles];
    const uint32_t col = (uint32_t)(it % n_tiles) * AT_TILE_COLS + lane;
    if (col >= n_grid) continue;
    const uint32_t n = (uint32_t)(goff[g + 1] - goff[g]);
    const uint32_t n_parts = (n + AT_CHUNK_MEMBERS - 1) / AT_CHUNK_MEMBERS;
    const uint64_t part0 = group_part[g];
    AtLane ln;
    ln.minkey = AT_KEY_MAX;
    ln.minpos = AT_POS_MAX;
    ln.minslot = 0;
    ln.cnt = 0;
    ln.kn = HOT_MIN(at_int_k(ks[col], n), (uint32_t)AT_LIST_CAP);
    for (uint32_t q = 0; q < n_parts && ln.kn; q++) {
      const uint64_t pi = part0 + q;
      const uint32_t c = part_cnt[pi * n_grid + col];
      /* the part's whole list in flight at once, then the pushes: one load
       * latency a part instead of one an entry */
      uint64_t k[AT_LIST_CAP];
      uint32_t p[AT_LIST_CAP];
#pragma unroll
      for (uint32_t j = 0; j < AT_LIST_CAP; j++) {
        const uint64_t at = (pi * AT_LIST_CAP + j) * n_grid + col;
        k[j] = j < c ? part_keys[at] : 0; /* 0 is never pushed */
        p[j] = j < c ? part_pos[at] : 0;
      }
#pragma unroll
      for (uint32_t j = 0; j < AT_LIST_CAP; j++)
        at_list_push(ln, keys, pos, k[j], p[j]);
    }
    at_store_threshold(thr_key, thr_pos, (uint64_t)g * n_grid + col, ln.kn,
                       ln.cnt, ln.minkey, ln.minpos);
  }
}

/* first index in sorted keys[0..n) whose key is above key */
static HOT_DEV uint32_t at_upper_bound(const uint64_t* keys, uint32_t n,
                                       uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] <= key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

/* One (group, column) of the sort class by nthr cooperating threads (a wave
 * or a workgroup; its first wave finishes alone).  keys: room for n. */
template <bool WAVE>
static HOT_DEV void at_sort_item(uint64_t* keys, const double* __restrict__ vcol,
                                 uint32_t n_grid,
                                 const uint32_t* __restrict__ rows, uint32_t n,
                                 uint32_t kn, int reverse, uint32_t tid,
                                 uint32_t nthr, uint64_t* thr_key,
                                 uint32_t* thr_pos) {
  for (uint32_t i = tid; i < n; i += nthr)
    keys[i] = at_key(vcol[(uint64_t)rows[i] * n_grid], reverse);
  cvot_sync<WAVE>();
  cvot_sort<WAVE>(keys, n, tid, nthr);
  uint64_t kstar = 0;
  uint32_t ties = 0;
  const bool search = tid < HOT_WAVE && kn > 0 && kn < n;
  if (search) {
    kstar = keys[n - kn];
    ties = kn - (n - at_upper_bound(keys, n, kstar));
  }
  cvot_sync<WAVE>(); /* the keys may be overwritten from here on */
  if (tid >= HOT_WAVE) return;
  uint32_t pstar = AT_POS_MAX;
  if (kn == 0) {
    kstar = AT_KEY_MAX;
  } else if (kn >= n || kstar == 0) {
    kstar = 0; /* every non-NaN value */
  } else {
    /* the ties-th member from the end holding kstar; wave-uniform */
    uint32_t left = ties;
    for (uint32_t base = 0; base < n; base += HOT_WAVE) {
      const bool valid = base + tid < n;
      const uint32_t i = valid ? n - 1 - base - tid : 0;
      const bool hit =
          valid && at_key(vcol[(uint64_t)rows[i] * n_grid], reverse) == kstar;
      unsigned long long m = __ballot(hit);
      const uint32_t c = (uint32_t)__popcll(m);
      if (c >= left) {
        for (uint32_t s = 1; s < left; s++) m &= m - 1;
        pstar = n - 1 - base - (uint32_t)__builtin_ctzll(m);
        break;
      }
      left -= c;
    }
  }
  if (tid == 0) {
    *thr_key = kstar;
    *thr_pos = pstar;
  }
}

/* MODE 0: a wave per item in its LDS slab (n <= CVOT_WAVE_CAP); 1: a
 * workgroup per item in LDS (n <= CVOT_BLOCK_CAP); 2: a workgroup per item
 * in its slab of the global scratch.  Item = (listed group, column). */
template <int MODE>
__global__ __launch_bounds__(HOT_BLOCK_THREADS) void at_sort_kernel(
    const double* __restrict__ vals, uint32_t n_grid,
    const uint32_t* __restrict__ group_rows, const uint64_t* __restrict__ goff,
    const uint32_t* __restrict__ list, uint64_t n_items,
    const double* __restrict__ ks, int reverse, uint64_t* scratch,
    uint64_t scratch_stride, uint64_t* __restrict__ thr_key,
    uint32_t* __restrict__ thr_pos) {
  __shared__ uint64_t s_keys[MODE == 0 ? HOT_WAVES_PER_BLOCK * CVOT_WAVE_CAP
                                       : (MODE == 1 ? CVOT_BLOCK_CAP : 1)];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t first = MODE == 0 ? (uint64_t)blockIdx.x * HOT_WAVES_PER_BLOCK + wv
                                   : blockIdx.x;
  const uint64_t stride = MODE == 0 ? (uint64_t)gridDim.x * HOT_WAVES_PER_BLOCK
                                    : gridDim.x;
  uint64_t* keys = MODE == 0 ? s_keys + wv * CVOT_WAVE_CAP
                             : (MODE == 1 ? s_keys
                                          : scratch + blockIdx.x * scratch_stride);
  for (uint64_t it = first; it < n_items; it += stride) {
    const uint32_t g = list[it / n_grid];
    const uint32_t col = (uint32_t)(it % n_grid);
    const uint64_t g0 = goff[g];
    const uint32_t n = (uint32_t)(goff[g + 1] - g0);
    const uint32_t kn = at_int_k(ks[col], n);
    const uint64_t at = (uint64_t)g * n_grid + col;
    if (MODE == 0)
      at_sort_item<true>(keys, vals + col, n_grid, group_rows + g0, n, kn,
                         reverse, lane, HOT_WAVE, thr_key + at, thr_pos + at);
    else
      at_sort_item<false>(keys, vals + col, n_grid, group_rows + g0, n, kn,
                          reverse, threadIdx.x, HOT_BLOCK_THREADS, thr_key + at,
                          thr_pos + at);
  }
}

__global__ __launch_bounds__(HOT_BLOCK_THREADS) void at_mark_kernel(
    const double* __restrict__ vals, uint32_t n_grid,
    const uint32_t* __restrict__ group_rows, const AhChunk* __restrict__ chunks,
    uint64_t n_items, uint32_t n_tiles, const uint64_t* __restrict__ goff,
    int reverse, const uint64_t* __restrict__ thr_key,
    const uint32_t* __restrict__ thr_pos, uint32_t* __restrict__ row_counts) {
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t stride = (uint64_t)gridDim.x * HOT_WAVES_PER_BLOCK;
  for (uint64_t it = (uint64_t)blockIdx.x * HOT_WAVES_PER_BLOCK + wv;
       it < n_items; it += stride) {
    const AhChunk ch = chunks[it / n_tiles];
    const uint32_t col = (uint32_t)(it % n_tiles) * AT_TILE_COLS + lane;
    const bool live = col < n_grid;
    /* an idle lane reads column 0 and keeps nothing */
    const uint32_t c = live ? col : 0;
    const uint32_t p0 = (uint32_t)(ch.begin - goff[ch.group]);
    const uint64_t kstar = live ? thr_key[(uint64_t)ch.group * n_grid + c]
                                : AT_KEY_MAX;
    const uint32_t pstar = live ? thr_pos[(uint64_t)ch.group * n_grid + c]
                                : AT_POS_MAX;
    /* a tile in which no column keeps anything reads nothing */
    if (__ballot(kstar != AT_KEY_MAX) == 0) continue;
    const uint32_t* rows = group_rows + ch.begin;
    const double* vcol = vals + c;
    uint32_t k = 0;
    for (; k + AT_UNROLL <= ch.n; k += AT_UNROLL) {
      double v[AT_UNROLL];
#pragma unroll
      for (int u = 0; u < AT_UNROLL; u++)
        v[u] = vcol[(uint64_t)rows[k + u] * n_grid];
#pragma unroll
      for (int u = 0; u < AT_UNROLL; u++) {
        const bool keep =
            at_kept(at_key(v[u], reverse), p0 + k + u, kstar, pstar);
        if (__ballot(keep) != 0 && lane == 0) row_counts[ch.begin + k + u] = 1;
      }
    }
    for (; k < ch.n; k++) {
      const bool keep = at_kept(at_key(vcol[(uint64_t)rows[k] * n_grid], reverse),
                                p0 + k, kstar, pstar);
      if (__ballot(keep) != 0 && lane == 0) row_counts[ch.begin + k] = 1;
    }
  }
}

__global__ __launch_bounds__(HOT_BLOCK_THREADS) void at_fill_kernel(
    const double* __restrict__ vals, uint32_t n_grid,
    const uint32_t* __restrict__ group_rows, const AhChunk* __restrict__ chunks,
    uint64_t n_items, uint32_t n_tiles, const uint64_t* __restrict__ goff,
    int reverse, const uint64_t* __restrict__ thr_key,
    const uint32_t* __restrict__ thr_pos,
    const uint32_t* __restrict__ row_counts,
    const uint64_t* __restrict__ row_start, double* __restrict__ out,
    uint32_t* __restrict__ row_group, uint32_t* __restrict__ row_src,
    double* __restrict__ row_last) {
  const double dnan = __longlong_as_double((long long)HOT_NAN_BITS);
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t stride = (uint64_t)gridDim.x * HOT_WAVES_PER_BLOCK;
  for (uint64_t it = (uint64_t)blockIdx.x * HOT_WAVES_PER_BLOCK + wv;
       it < n_items; it += stride) {
    const AhChunk ch = chunks[it / n_tiles];
    const uint32_t tile = (uint32_t)(it % n_tiles);
    const uint32_t col = tile * AT_TILE_COLS + lane;
    const bool live = col < n_grid;
    const uint32_t c = live ? col : 0;
    const uint32_t p0 = (uint32_t)(ch.begin - goff[ch.group]);
    const uint64_t kstar = live ? thr_key[(uint64_t)ch.group * n_grid + c]
                                : AT_KEY_MAX;
    const uint32_t pstar = live ? thr_pos[(uint64_t)ch.group * n_grid + c]
                                : AT_POS_MAX;
    const uint32_t* rows = group_rows + ch.begin;
    for (uint32_t base = 0; base < ch.n; base += HOT_WAVE) {
      /* the kept members among the next 64, by their flags */
      const bool flag = base + lane < ch.n && row_counts[ch.begin + base + lane];
      unsigned long long m = __ballot(flag);
      if (m == 0) continue;
      uint64_t r = row_start[ch.begin + base];
      for (; m; m &= m - 1, r++) {
        const uint32_t k = base + (uint32_t)__builtin_ctzll(m);
        const double* vrow = vals + (uint64_t)rows[k] * n_grid;
        if (live) {
          const double v = vrow[col];
          out[r * n_grid + col] =
              at_kept(at_key(v, reverse), p0 + k, kstar, pstar) ? v : dnan;
        }
        if (tile == 0 && lane == 0) {
          row_group[r] = ch.group;
          row_src[r] = rows[k];
          row_last[r] = vrow[n_grid - 1];
        }
      }
    }
  }
}

/* ------------------------------------------------------------------ */
/* host side                                                          */
/* ------------------------------------------------------------------ */

namespace {

/* result of the last exec; every buffer grow-only */
struct AtState {
  double* d_out = nullptr;         /* [n_rows x n_grid] */
  uint32_t* d_row_group = nullptr; /* [n_rows] */
  uint32_t* d_row_src = nullptr;   /* [n_rows] input matrix row */
  double* d_row_last = nullptr;    /* [n_rows] input value, last column */
  size_t out_cap = 0, row_group_cap = 0, row_src_cap = 0, row_last_cap = 0;
  uint64_t n_rows = 0;
  int32_t n_grid = 0;
  bool valid = false;
};

AtState g_at;

/* what the host derives from the CSR and ks before anything runs */
struct AtPlan {
  std::vector<uint32_t> group_part; /* [n_groups] */
  std::vector<uint32_t> merge_groups;
  std::vector<uint32_t> sort_list[3]; /* wave, workgroup LDS, global */
  uint64_t n_parts = 0;
  uint64_t max_global_n = 0;
};

/* getIntK(k, inf), saturating */
uint64_t at_host_int_k(double k) {
  if (!(k >= 1.0)) return 0;
  if (k >= 9223372036854775808.0) return (uint64_t)1 << 63;
  return (uint64_t)k;
}

/* Argument checks and class choice shared by both entry points; nothing is
 * launched or allocated before they pass.  Returns 0 or 1. */
int at_validate(uint32_t n_in_rows, int64_t n_grid, const uint32_t* group_rows,
                const uint64_t* group_offsets, uint32_t n_groups,
                const double* ks, uint32_t n_ks, AtPlan* plan, char* errbuf,
                size_t errbuf_len) {
  static const char* op = "aggr topk";
  if (int rc = ah_validate_csr(op, n_in_rows, n_grid, group_rows, group_offsets,
                               n_groups, errbuf, errbuf_len))
    return rc;
  if (!ks) return ah_csr_err(errbuf, errbuf_len, op, "ks must not be NULL");
  if ((int64_t)n_ks != n_grid)
    return ah_csr_err(errbuf, errbuf_len, op, "n_ks must equal n_grid");
  const uint64_t n_members = n_groups ? group_offsets[n_groups] : 0;
  /* the thresholds, the partial lists and a result of every member */
  const uint64_t cell_limit = (uint64_t)INT64_MAX / 16 / (uint64_t)n_grid;
  if (n_members > cell_limit || n_groups > cell_limit)
    return ah_csr_err(errbuf, errbuf_len, op, "result size overflows");
  uint64_t k_max = 0;
  for (uint32_t c = 0; c < n_ks; c++)
    k_max = std::max(k_max, at_host_int_k(ks[c]));
  plan->group_part.assign(n_groups, AT_PART_DIRECT);
  for (uint32_t g = 0; g < n_groups; g++) {
    const uint64_t n = group_offsets[g + 1] - group_offsets[g];
    if (std::min(n, k_max) > AT_LIST_CAP) {
      plan->group_part[g] = AT_PART_SORT;
      if (n <= CVOT_WAVE_CAP) plan->sort_list[0].push_back(g);
      else if (n <= CVOT_BLOCK_CAP) plan->sort_list[1].push_back(g);
      else {
        plan->sort_list[2].push_back(g);
        plan->max_global_n = std::max(plan->max_global_n, n);
      }
    } else if (n > AT_CHUNK_MEMBERS) {
      plan->group_part[g] = (uint32_t)plan->n_parts;
      plan->merge_groups.push_back(g);
      plan->n_parts += (n + AT_CHUNK_MEMBERS - 1) / AT_CHUNK_MEMBERS;
    }
  }
  /* part indices are u32 and must stay clear of the two sentinels */
  if (plan->n_parts >= AT_PART_SORT ||
      plan->n_parts > cell_limit / AT_LIST_CAP)
    return ah_csr_err(errbuf, errbuf_len, op, "result size overflows");
  return 0;
}

template <class T>
hipError_t at_upload(VmPoolBuf<T>* buf, const T* src, size_t n, hipStream_t st) {
  hipError_t e = buf->alloc(std::max<size_t>(n, 1) * sizeof(T));
  if (e != hipSuccess || n == 0) return e;
  return hipMemcpyAsync(buf->p, src, n * sizeof(T), hipMemcpyHostToDevice, st);
}

/* the pipeline over a device matrix; the caller holds the context lock and
 * has validated the arguments into plan */
int at_run(const double* d_vals, int32_t n_grid, const uint32_t* group_rows,
           const uint64_t* group_offsets, uint32_t n_groups, const double* ks,
           int32_t reverse, const AtPlan& plan, uint64_t* out_n_rows,
           char* errbuf, size_t errbuf_len) {
  AtState& a = g_at;
  a.valid = false; /* the earlier result is replaced from here on */
  a.n_rows = 0;
  a.n_grid = n_grid;
  const uint64_t n_members = n_groups ? group_offsets[n_groups] : 0;
  if (n_members == 0) {
    a.valid = true;
    if (out_n_rows) *out_n_rows = 0;
    return 0;
  }
  std::vector<AhChunk> chunks;
  ah_build_chunks(group_offsets, n_groups, AT_CHUNK_MEMBERS, &chunks);
  const uint32_t n_tiles = ((uint32_t)n_grid + AT_TILE_COLS - 1) / AT_TILE_COLS;
  const uint64_t n_items = (uint64_t)chunks.size() * n_tiles;
  const uint64_t n_thr = (uint64_t)n_groups * (uint64_t)n_grid;
  const int rev = reverse ? 1 : 0;

  hipStream_t st = vm_ctx_stream();
  hipEvent_t ev_start, ev_stop;
  vm_ctx_events(&ev_start, &ev_stop);

  VmPoolBuf<uint32_t> d_group_rows, d_group_part, d_lists, d_thr_pos, d_part_pos,
      d_part_cnt, d_row_counts;
  VmPoolBuf<uint64_t> d_goff, d_thr_key, d_part_keys, d_row_start, d_scratch;
  VmPoolBuf<AhChunk> d_chunks;
  VmPoolBuf<double> d_ks;
  VM_HIP_TRY(at_upload(&d_group_rows, group_rows, (size_t)n_members, st),
             "upload group rows");
  VM_HIP_TRY(at_upload(&d_goff, group_offsets, (size_t)n_groups + 1, st),
             "upload group offsets");
  VM_HIP_TRY(at_upload(&d_chunks, chunks.data(), chunks.size(), st),
             "upload chunks");
  VM_HIP_TRY(at_upload(&d_group_part, plan.group_part.data(), (size_t)n_groups, st),
             "upload group classes");
  VM_HIP_TRY(at_upload(&d_ks, ks, (size_t)n_grid, st), "upload ks");
  /* merge groups, then the three sort lists */
  std::vector<uint32_t> lists(plan.merge_groups);
  size_t list_at[3];
  for (int m = 0; m < 3; m++) {
    list_at[m] = lists.size();
    lists.insert(lists.end(), plan.sort_list[m].begin(), plan.sort_list[m].end());
  }
  VM_HIP_TRY(at_upload(&d_lists, lists.data(), lists.size(), st), "upload lists");
  VM_HIP_TRY(d_thr_key.alloc((size_t)n_thr * 8), "alloc thresholds");
  VM_HIP_TRY(d_thr_pos.alloc((size_t)n_thr * 4), "alloc thresholds");
  const uint64_t n_part_cells = plan.n_parts * (uint64_t)n_grid;
  VM_HIP_TRY(d_part_keys.alloc(std::max<size_t>(n_part_cells * AT_LIST_CAP * 8, 8)),
             "alloc partial lists");
  VM_HIP_TRY(d_part_pos.alloc(std::max<size_t>(n_part_cells * AT_LIST_CAP * 4, 4)),
             "alloc partial lists");
  VM_HIP_TRY(d_part_cnt.alloc(std::max<size_t>(n_part_cells * 4, 4)),
             "alloc partial lists");
  VM_HIP_TRY(d_row_counts.alloc((size_t)n_members * 4), "alloc row counts");
  VM_HIP_TRY(d_row_start.alloc(((size_t)n_members + 1) * 8), "alloc row start");
  uint32_t sort_blocks = 0;
  if (!plan.sort_list[2].empty()) {
    const uint64_t slab = plan.max_global_n * 8;
    const uint64_t fit = ((uint64_t)AT_SORT_SCRATCH_MIB << 20) / slab;
    const uint64_t items = (uint64_t)plan.sort_list[2].size() * (uint64_t)n_grid;
    sort_blocks = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>({fit, items, (uint64_t)AT_SORT_BLOCKS}));
    VM_HIP_TRY(d_scratch.alloc((size_t)(slab * sort_blocks)), "alloc sort scratch");
  }
  /* the host arrays are free to go once the uploads have landed */
  VM_HIP_TRY(hipStreamSynchronize(st), "sync uploads");

  VM_HIP_TRY(hipEventRecord(ev_start, st), "event start");
  VM_HIP_TRY(hipMemsetAsync(d_row_counts.p, 0, (size_t)n_members * 4, st),
             "zero row counts");
  hipLaunchKernelGGL(at_list_kernel, dim3(ah_blocks(n_items, AT_LIST_WAVES)),
                     dim3(AT_LIST_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                     d_group_rows.p, d_chunks.p, n_items, n_tiles, d_goff.p,
                     d_group_part.p, d_ks.p, rev, d_thr_key.p, d_thr_pos.p,
                     d_part_keys.p, d_part_pos.p, d_part_cnt.p);
  if (!plan.merge_groups.empty()) {
    const uint64_t items = (uint64_t)plan.merge_groups.size() * n_tiles;
    hipLaunchKernelGGL(at_merge_kernel, dim3(ah_blocks(items, AT_LIST_WAVES)),
                       dim3(AT_LIST_THREADS), 0, st, d_lists.p, items, n_tiles,
                       (uint32_t)n_grid, d_goff.p, d_group_part.p, d_ks.p,
                       d_part_keys.p, d_part_pos.p, d_part_cnt.p, d_thr_key.p,
                       d_thr_pos.p);
  }
  if (!plan.sort_list[0].empty()) {
    const uint64_t items = (uint64_t)plan.sort_list[0].size() * (uint64_t)n_grid;
    hipLaunchKernelGGL(at_sort_kernel<0>,
                       dim3(ah_blocks(items, HOT_WAVES_PER_BLOCK)),
                       dim3(HOT_BLOCK_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                       d_group_rows.p, d_goff.p, d_lists.p + list_at[0], items,
                       d_ks.p, rev, (uint64_t*)nullptr, (uint64_t)0, d_thr_key.p,
                       d_thr_pos.p);
  }
  if (!plan.sort_list[1].empty()) {
    const uint64_t items = (uint64_t)plan.sort_list[1].size() * (uint64_t)n_grid;
    hipLaunchKernelGGL(at_sort_kernel<1>, dim3(ah_blocks(items, 1)),
                       dim3(HOT_BLOCK_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                       d_group_rows.p, d_goff.p, d_lists.p + list_at[1], items,
                       d_ks.p, rev, (uint64_t*)nullptr, (uint64_t)0, d_thr_key.p,
                       d_thr_pos.p);
  }
  if (sort_blocks) {
    const uint64_t items = (uint64_t)plan.sort_list[2].size() * (uint64_t)n_grid;
    hipLaunchKernelGGL(at_sort_kernel<2>, dim3(sort_blocks),
                       dim3(HOT_BLOCK_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                       d_group_rows.p, d_goff.p, d_lists.p + list_at[2], items,
                       d_ks.p, rev, d_scratch.p, plan.max_global_n, d_thr_key.p,
                       d_thr_pos.p);
  }
  hipLaunchKernelGGL(at_mark_kernel, dim3(ah_blocks(n_items, HOT_WAVES_PER_BLOCK)),
                     dim3(HOT_BLOCK_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                     d_group_rows.p, d_chunks.p, n_items, n_tiles, d_goff.p, rev,
                     d_thr_key.p, d_thr_pos.p, d_row_counts.p);
  hot_scan_launch(d_row_counts.p, (uint32_t)n_members, d_row_start.p, st);
  /* the output size is data-dependent: the host learns n_rows here */
  uint64_t n_rows = 0;
  VM_HIP_TRY(hipMemcpyAsync(&n_rows, d_row_start.p + n_members, 8,
                            hipMemcpyDeviceToHost, st), "download n_rows");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync mark");
  VM_HIP_TRY(hipGetLastError(), "mark kernel");
  if (n_rows > n_members)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: inconsistent row count");
  if (n_rows) {
    VM_HIP_TRY(hot_reserve(&a.d_out, &a.out_cap, (size_t)n_rows * n_grid * 8),
               "alloc topk rows");
    VM_HIP_TRY(hot_reserve(&a.d_row_group, &a.row_group_cap, (size_t)n_rows * 4),
               "alloc row groups");
    VM_HIP_TRY(hot_reserve(&a.d_row_src, &a.row_src_cap, (size_t)n_rows * 4),
               "alloc row sources");
    VM_HIP_TRY(hot_reserve(&a.d_row_last, &a.row_last_cap, (size_t)n_rows * 8),
               "alloc row last values");
    hipLaunchKernelGGL(at_fill_kernel,
                       dim3(ah_blocks(n_items, HOT_WAVES_PER_BLOCK)),
                       dim3(HOT_BLOCK_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                       d_group_rows.p, d_chunks.p, n_items, n_tiles, d_goff.p, rev,
                       d_thr_key.p, d_thr_pos.p, d_row_counts.p, d_row_start.p,
                       a.d_out, a.d_row_group, a.d_row_src, a.d_row_last);
  }
  VM_HIP_TRY(hipEventRecord(ev_stop, st), "event stop");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync fill");
  VM_HIP_TRY(hipGetLastError(), "fill kernel");
  float ms = 0;
  VM_HIP_TRY(hipEventElapsedTime(&ms, ev_start, ev_stop), "event elapsed");
  vm_ctx_set_last_kernel_ms((double)ms);
  a.n_rows = n_rows;
  a.valid = true;
  if (out_n_rows) *out_n_rows = n_rows;
  return 0;
}

}  // namespace

void vm_aggrtopk_shutdown(void) {
  AtState& a = g_at;
  (void)hipFree(a.d_out);
  (void)hipFree(a.d_row_group);
  (void)hipFree(a.d_row_src);
  (void)hipFree(a.d_row_last);
  a = AtState();
}

extern "C" {

int vmgpu_aggr_topk_exec(const double* values, uint32_t n_series, int32_t n_grid,
                         const uint32_t* group_rows, const uint64_t* group_offsets,
                         uint32_t n_groups, const double* ks, uint32_t n_ks,
                         int32_t reverse, uint64_t* out_n_rows,
                         char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  g_at.valid = false;
  AtPlan plan;
  if (int rc = at_validate(n_series, n_grid, group_rows, group_offsets, n_groups,
                           ks, n_ks, &plan, errbuf, errbuf_len))
    return rc;
  VmPoolBuf<double> d_vals;
  if (n_groups && group_offsets[n_groups]) {
    if (!values)
      return vm_set_err(errbuf, errbuf_len, "vmgpu: aggr topk: bad args");
    const size_t vbytes = (size_t)n_series * (size_t)n_grid * 8;
    VM_HIP_TRY(d_vals.alloc(vbytes), "alloc values");
    VM_HIP_TRY(hipMemcpyAsync(d_vals.p, values, vbytes, hipMemcpyHostToDevice,
                              vm_ctx_stream()), "upload values");
  }
  return at_run(d_vals.p, n_grid, group_rows, group_offsets, n_groups, ks,
                reverse, plan, out_n_rows, errbuf, errbuf_len);
}

int vmgpu_batch_aggr_topk_exec(uint64_t handle, const uint32_t* group_rows,
                               const uint64_t* group_offsets, uint32_t n_groups,
                               const double* ks, uint32_t n_ks, int32_t reverse,
                               uint64_t* out_n_rows, char* errbuf,
                               size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  g_at.valid = false;
  vm_batch_cols b;
  if (vm_batch_cols_get(handle, &b) != 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  if (!b.d_out || b.last_rows == 0 || b.last_grid <= 0)
    return vm_set_err(errbuf, errbuf_len,
                      "vmgpu: no rollup output on this batch "
                      "(vmgpu_rollup_exec first)");
  AtPlan plan;
  if (int rc = at_validate(b.last_rows, b.last_grid, group_rows, group_offsets,
                           n_groups, ks, n_ks, &plan, errbuf, errbuf_len))
    return rc;
  return at_run(b.d_out, b.last_grid, group_rows, group_offsets, n_groups, ks,
                reverse, plan, out_n_rows, errbuf, errbuf_len);
}

int vmgpu_aggr_topk_fetch(uint32_t* row_group, uint32_t* row_src, double* row_last,
                          double* out, char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  const AtState& a = g_at;
  if (!a.valid)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: no aggr topk result");
  if (a.n_rows == 0) return 0;
  hipStream_t st = vm_ctx_stream();
  if (row_group)
    VM_HIP_TRY(hipMemcpyAsync(row_group, a.d_row_group, a.n_rows * 4,
                              hipMemcpyDeviceToHost, st), "download row groups");
  if (row_src)
    VM_HIP_TRY(hipMemcpyAsync(row_src, a.d_row_src, a.n_rows * 4,
                              hipMemcpyDeviceToHost, st), "download row sources");
  if (row_last)
    VM_HIP_TRY(hipMemcpyAsync(row_last, a.d_row_last, a.n_rows * 8,
                              hipMemcpyDeviceToHost, st), "download row last values");
  if (out)
    VM_HIP_TRY(hipMemcpyAsync(out, a.d_out, (size_t)a.n_rows * a.n_grid * 8,
                              hipMemcpyDeviceToHost, st), "download topk rows");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync fetch");
  return 0;
}

}  // extern "C"
