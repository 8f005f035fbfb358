/* aggrcv.hip — the count_values() aggregate (aggrFuncCountValues,
 * aggr.go:566) on the device.
 *
 * Input: a device matrix vals[n_in_rows x n_grid] (f64, row-major) and the
 * member CSR of aggrhist.hip (group_offsets u64[n_groups + 1], group_rows
 * u32[n_members]).  Per group the reference keeps a map from value to output
 * series and counts, per grid point, the members holding that value.  The
 * output is SPARSE: one row per (group, distinct non-NaN value anywhere in
 * the group), ordered by group and then by ascending value, with the count
 * as f64 and NaN (not 0.0) where no member holds the value.  -0.0 and 0.0
 * are one row, as they are one key of the reference's map; row_value carries
 * the sign of the zero the reference would meet first (smallest member
 * position, then smallest grid index), because that zero names the series.
 *
 * Work items, lane ownership and the counting are aggrhist.hip's
 * (aggr_sparse.h): (chunk of CV_CHUNK_MEMBERS members, tile of 64 columns)
 * per wavefront, lanes owning columns.  The row discovery is new: the set of
 * distinct values of a group is unbounded, so it is collected in a
 * per-group open-addressing hash table of order keys (value_key.h) and then
 * sorted.
 *
 *   cv_insert_kernel  every non-NaN value's key into its group's table.  A
 *       slot only ever changes from empty to one key, so a non-empty read is
 *       final and a stale empty read is corrected by the compare-and-swap's
 *       return value: a key that is already present costs loads only, never
 *       an atomic.  In front of the table sit the key the lane handled last
 *       and a small per-wave LDS set of keys known to be present.  A
 *       successful insert bumps the group's distinct counter; a counter
 *       above max_rows_per_group, or a probe sequence that has visited the
 *       whole slice, records the group in the overflow word (atomicMin) and
 *       the lane stops inserting.  Zeros also atomicMin their
 *       ((member position * n_grid + column) << 1 | sign) into the group's
 *       zero word, once per lane and work item.
 *   hot_scan_launch   distinct counters -> row_start; the host reads n_rows
 *       and the overflow word.
 *   cv_rows_wave_kernel / cv_rows_block_kernel  the sorted keys of every
 *       group (cvot_sort).  Only occupied slots are sorted: a slice of at
 *       most CVOT_WAVE_CAP slots is gathered by one wave into an LDS slab;
 *       a larger one by one workgroup into LDS while the group has at most
 *       CVOT_BLOCK_CAP rows (the scan has counted them), and is sorted whole
 *       and in place above that (a power of two; the empty sentinel sorts
 *       last).  The host knows every slice size and builds both lists.  The
 *       R_g keys become row_key / row_group / row_value.
 *   cv_count_kernel   the local row of a value is the lower bound of its key
 *       among the group's sorted keys (staged in LDS up to CV_LDS_KEYS).
 *       Groups of at most CV_BAND_MAX_ROWS rows count in aggrhist.hip's
 *       banded u32 LDS tile and flush non-zero counters with integer
 *       atomicAdd; wider groups add straight into the u32 matrix, one
 *       atomicAdd a value, instead of re-reading their values once per band
 *       (measured in profiles/count_values_aggregate.md).
 *   ah_u32_to_f64_kernel<true>  counters -> f64, 0 -> NaN.
 *
 * Everything is integer counting into zeroed memory, so any arrival order
 * gives the same bits.
 *
 * Table size: per group the power of two >= 2 * min(limit + 1, members *
 * n_grid), at least CV_MIN_CAP, so the load factor stays at or below one
 * half until the limit is passed.  A group's slice is scanned, and above
 * CVOT_BLOCK_CAP rows sorted in global memory, by ONE workgroup: correct for
 * any limit up to 2^24, but meant for limits in the thousands.
 *
 * Result and scratch live in one file-static slot, grow-only, plain
 * hipMalloc through hot_reserve, guarded by the context lock.
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

/* members of one group per work item, as AH_CHUNK_MEMBERS */
#define CV_CHUNK_MEMBERS 128
/* member rows a lane keeps in flight */
#define CV_UNROLL 8
#define CV_TILE_COLS HOT_WAVE
/* rows of the count tile, as AH_BAND_ROWS: 16 KiB a wave */
#define CV_BAND_ROWS 64
/* widest group counted in bands; above it, one global atomicAdd a value */
#ifndef CV_BAND_MAX_ROWS
#define CV_BAND_MAX_ROWS 256
#endif
/* sorted keys of a group staged in LDS up to this many: 4 KiB a wave */
#define CV_LDS_KEYS 512
/* per-wave set of keys known to be in the table (direct-mapped) */
#define CV_SEEN 64
#define CV_MIN_CAP 64
#define CV_MAX_LIMIT (1u << 24)
#define CV_MAX_SLOTS (1ull << 31)
#define CV_INSERT_THREADS 256
#define CV_COUNT_THREADS 128
#define CV_INSERT_WAVES (CV_INSERT_THREADS / HOT_WAVE)
#define CV_COUNT_WAVES (CV_COUNT_THREADS / HOT_WAVE)
#define CV_ROWS_BLOCKS 2048
#define CV_NO_GROUP 0xFFFFFFFFu
#define CV_NO_ZERO 0xFFFFFFFFFFFFFFFFULL
/* order key of +0.0, which also stands for -0.0 */
#define CV_ZERO_KEY 0x8000000000000000ULL

/* All 64 bits take part: doubles such as 1.0, 2.0, 3.0 differ only in their
 * top bits, so key & mask alone would put a whole enum into one slot. */
static HOT_DEV uint32_t cv_hash(uint64_t k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDULL;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ULL;
  k ^= k >> 33;
  return (uint32_t)k;
}

/* row key of a value: CVOT_KEY_NONE for a NaN, -0 folded into 0 */
static HOT_DEV uint64_t cv_key(double v) {
  if (v != v) return CVOT_KEY_NONE;
  if (v == 0.0) return CV_ZERO_KEY;
  return cvot_order_key(v);
}

/* key into tab[0..mask]; false when the group has outgrown its limit or its
 * slice.  The load bypasses the CU's L1, which nothing refreshes while the
 * kernel runs. */
static HOT_DEV bool cv_insert(unsigned long long* tab, uint32_t mask,
                              uint64_t key, uint32_t h, uint32_t* counter,
                              uint32_t limit) {
  h &= mask;
  for (uint32_t probes = 0; probes <= mask; probes++) {
    unsigned long long cur = __hip_atomic_load(&tab[h], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return true;
    if (cur == CVOT_KEY_NONE) {
      cur = atomicCAS(&tab[h], (unsigned long long)CVOT_KEY_NONE,
                      (unsigned long long)key);
      if (cur == CVOT_KEY_NONE) return atomicAdd(counter, 1u) < limit;
      if (cur == key) return true;
    }
    h = (h + 1) & mask;
  }
  return false;
}

struct CvLane {
  uint64_t last;  /* key handled last */
  uint64_t zmin;  /* first zero met, coded for the zero word */
  bool dead;      /* the group overflowed under this lane */
};

static HOT_DEV uint64_t* cv_seen_slot(uint64_t* seen, uint32_t h) {
  return &seen[(h >> 16) % CV_SEEN];
}

/* One value whose key, hash and seen-set entry the caller has fetched (for a
 * batch of values side by side: the common case ends at one of the three
 * tests below without touching global memory). */
static HOT_DEV void cv_insert_value(CvLane& ln, double v, uint64_t key,
                                    uint32_t h, uint64_t seen_key,
                                    uint64_t cell, unsigned long long* tab,
                                    uint32_t mask, uint64_t* seen,
                                    uint32_t* counter, uint32_t limit,
                                    uint32_t group, uint32_t* overflow) {
  if (key == CVOT_KEY_NONE) return;
  if (key == CV_ZERO_KEY && ln.zmin == CV_NO_ZERO)
    ln.zmin = (cell << 1) | ((uint64_t)__double_as_longlong(v) >> 63);
  /* a value held along the members is looked up once */
  if (key == ln.last || ln.dead) return;
  ln.last = key;
  if (seen_key == key) return;
  if (cv_insert(tab, mask, key, h, counter, limit)) {
    *cv_seen_slot(seen, h) = key;
  } else {
    ln.dead = true;
    atomicMin(overflow, group);
  }
}

__global__ __launch_bounds__(CV_INSERT_THREADS) void cv_insert_kernel(
    const double* __restrict__ vals, uint32_t n_grid,
    const uint32_t* __restrict__ group_rows, const AhChunk* __restrict__ chunks,
    uint64_t n_items, uint32_t n_tiles, unsigned long long* table,
    const uint64_t* __restrict__ table_start, uint32_t limit,
    uint32_t* counters, unsigned long long* zero, uint32_t* overflow) {
  __shared__ uint64_t s_seen[CV_INSERT_WAVES][CV_SEEN];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t stride = (uint64_t)gridDim.x * CV_INSERT_WAVES;
  for (uint64_t it = (uint64_t)blockIdx.x * CV_INSERT_WAVES + wv; it < n_items;
       it += stride) {
    const AhChunk ch = chunks[it / n_tiles];
    const uint32_t col = (uint32_t)(it % n_tiles) * CV_TILE_COLS + lane;
    const uint64_t t0 = table_start[ch.group];
    const uint32_t mask = (uint32_t)(table_start[ch.group + 1] - t0) - 1u;
    unsigned long long* tab = table + t0;
    uint32_t* counter = counters + ch.group;
    /* the set is per group: keys of the item before mean nothing here */
    hot_wave_sync();
    for (uint32_t i = lane; i < CV_SEEN; i += HOT_WAVE)
      s_seen[wv][i] = CVOT_KEY_NONE;
    hot_wave_sync();
    /* a group already past its limit has been reported by the lane that
     * took it there: leave its full table alone */
    if (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >
        limit)
      continue;
    if (col >= n_grid) continue;
    CvLane ln;
    ln.last = CVOT_KEY_NONE;
    ln.zmin = CV_NO_ZERO;
    ln.dead = false;
    const uint32_t* rows = group_rows + ch.begin;
    uint32_t k = 0;
    for (; k + CV_UNROLL <= ch.n && !ln.dead; k += CV_UNROLL) {
      double v[CV_UNROLL];
#pragma unroll
      for (int u = 0; u < CV_UNROLL; u++)
        v[u] = vals[(uint64_t)rows[k + u] * n_grid + col];
      /* keys, hashes and seen-set reads of the batch side by side; an entry
       * that a value of this very batch adds is missed, which costs that
       * value a table load, nothing else */
      uint64_t key[CV_UNROLL], sk[CV_UNROLL];
      uint32_t h[CV_UNROLL];
#pragma unroll
      for (int u = 0; u < CV_UNROLL; u++) {
        key[u] = cv_key(v[u]);
        h[u] = cv_hash(key[u]);
      }
#pragma unroll
      for (int u = 0; u < CV_UNROLL; u++) sk[u] = *cv_seen_slot(s_seen[wv], h[u]);
#pragma unroll
      for (int u = 0; u < CV_UNROLL; u++)
        cv_insert_value(ln, v[u], key[u], h[u], sk[u],
                        (ch.begin + k + u) * n_grid + col, tab, mask,
                        s_seen[wv], counter, limit, ch.group, overflow);
    }
    for (; k < ch.n && !ln.dead; k++) {
      const double v = vals[(uint64_t)rows[k] * n_grid + col];
      const uint64_t key = cv_key(v);
      const uint32_t h = cv_hash(key);
      cv_insert_value(ln, v, key, h, *cv_seen_slot(s_seen[wv], h),
                      (ch.begin + k) * n_grid + col, tab, mask, s_seen[wv],
                      counter, limit, ch.group, overflow);
    }
    if (ln.zmin != CV_NO_ZERO) {
      unsigned long long* z = zero + ch.group;
      if (__hip_atomic_load(z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >
          ln.zmin)
        atomicMin(z, (unsigned long long)ln.zmin);
    }
  }
}

/* rows of group g from its sorted keys; the zero row takes its sign from
 * the zero word */
static HOT_DEV void cv_emit_rows(const uint64_t* keys, uint32_t R, uint32_t g,
                                 uint64_t row0, unsigned long long zero_word,
                                 uint32_t tid, uint32_t nthr,
                                 uint64_t* __restrict__ row_key,
                                 uint32_t* __restrict__ row_group,
                                 double* __restrict__ row_value) {
  for (uint32_t r = tid; r < R; r += nthr) {
    const uint64_t k = keys[r];
    double v = cvot_key_value(k);
    if (k == CV_ZERO_KEY && (zero_word & 1ULL)) v = -0.0;
    row_key[row0 + r] = k;
    row_group[row0 + r] = g;
    row_value[row0 + r] = v;
  }
}

/* one wave per listed group: a slice of at most CVOT_WAVE_CAP slots */
__global__ __launch_bounds__(HOT_BLOCK_THREADS) void cv_rows_wave_kernel(
    const uint32_t* __restrict__ list, uint32_t n_list,
    const unsigned long long* __restrict__ table,
    const uint64_t* __restrict__ table_start,
    const uint64_t* __restrict__ row_start,
    const unsigned long long* __restrict__ zero, uint64_t* __restrict__ row_key,
    uint32_t* __restrict__ row_group, double* __restrict__ row_value) {
  __shared__ uint64_t s_keys[HOT_WAVES_PER_BLOCK][CVOT_WAVE_CAP];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  uint64_t* keys = s_keys[wv];
  for (uint32_t i = blockIdx.x * HOT_WAVES_PER_BLOCK + wv; i < n_list;
       i += gridDim.x * HOT_WAVES_PER_BLOCK) {
    const uint32_t g = list[i];
    const uint64_t t0 = table_start[g];
    const uint32_t cap =
        HOT_MIN((uint32_t)(table_start[g + 1] - t0), (uint32_t)CVOT_WAVE_CAP);
    const uint64_t row0 = row_start[g];
    hot_wave_sync();
    /* only the occupied slots go into the sort: at most half the slice,
     * and for an enum a handful */
    uint32_t m = 0;
    for (uint32_t k0 = 0; k0 < cap; k0 += HOT_WAVE) {
      const uint64_t key = k0 + lane < cap ? table[t0 + k0 + lane] : CVOT_KEY_NONE;
      const bool used = key != CVOT_KEY_NONE;
      const unsigned long long um = __ballot(used);
      if (used) keys[m + __popcll(um & ((1ULL << lane) - 1ULL))] = key;
      m += __popcll(um);
    }
    hot_wave_sync();
    cvot_sort<true>(keys, m, lane, HOT_WAVE);
    const uint32_t R = HOT_MIN((uint32_t)(row_start[g + 1] - row0), m);
    cv_emit_rows(keys, R, g, row0, zero[g], lane, HOT_WAVE, row_key, row_group,
                 row_value);
  }
}

/* one workgroup per listed group: the occupied slots of the slice gathered
 * and sorted in LDS while there are at most CVOT_BLOCK_CAP of them (the row
 * scan has counted them), the whole slice sorted in place above that */
__global__ __launch_bounds__(HOT_BLOCK_THREADS) void cv_rows_block_kernel(
    const uint32_t* __restrict__ list, uint32_t n_list,
    unsigned long long* table, const uint64_t* __restrict__ table_start,
    const uint64_t* __restrict__ row_start,
    const unsigned long long* __restrict__ zero, uint64_t* __restrict__ row_key,
    uint32_t* __restrict__ row_group, double* __restrict__ row_value) {
  __shared__ uint64_t s_keys[CVOT_BLOCK_CAP];
  __shared__ uint32_t s_n;
  const uint32_t t = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < n_list; i += gridDim.x) {
    const uint32_t g = list[i];
    const uint64_t t0 = table_start[g];
    const uint64_t cap = table_start[g + 1] - t0;
    const uint64_t row0 = row_start[g];
    uint32_t R = (uint32_t)HOT_MIN(row_start[g + 1] - row0, cap);
    if (R <= CVOT_BLOCK_CAP) { /* workgroup-uniform */
      __syncthreads(); /* the rows of the group before have been read */
      if (t == 0) s_n = 0;
      __syncthreads();
      for (uint64_t k = t; k < cap; k += HOT_BLOCK_THREADS) {
        const uint64_t key = table[t0 + k];
        if (key == CVOT_KEY_NONE) continue;
        const uint32_t at = atomicAdd(&s_n, 1u); /* any order: sorted next */
        if (at < CVOT_BLOCK_CAP) s_keys[at] = key;
      }
      __syncthreads();
      R = HOT_MIN(R, s_n);
      cvot_sort<false>(s_keys, R, t, HOT_BLOCK_THREADS);
      cv_emit_rows(s_keys, R, g, row0, zero[g], t, HOT_BLOCK_THREADS, row_key,
                   row_group, row_value);
    } else {
      uint64_t* keys = reinterpret_cast<uint64_t*>(table + t0);
      cvot_sort<false>(keys, cap, t, HOT_BLOCK_THREADS);
      cv_emit_rows(keys, R, g, row0, zero[g], t, HOT_BLOCK_THREADS, row_key,
                   row_group, row_value);
    }
  }
}

/* local row of a key among the group's R sorted keys (R if absent) */
static HOT_DEV uint32_t cv_local_row(const uint64_t* s_keys,
                                     const uint64_t* g_keys, uint32_t R,
                                     uint64_t key) {
  if (key == CVOT_KEY_NONE) return 0xFFFFFFFFu;
  return R <= CV_LDS_KEYS ? cvot_lower_bound(s_keys, R, key)
                          : cvot_lower_bound(g_keys, R, key);
}

__global__ __launch_bounds__(CV_COUNT_THREADS) void cv_count_kernel(
    const double* __restrict__ vals, uint32_t n_grid,
    const uint32_t* __restrict__ group_rows, const AhChunk* __restrict__ chunks,
    uint64_t n_items, uint32_t n_tiles, const uint64_t* __restrict__ row_key,
    const uint64_t* __restrict__ row_start, uint32_t* cnt) {
  __shared__ uint32_t s_tile[CV_COUNT_WAVES][CV_BAND_ROWS * CV_TILE_COLS];
  __shared__ uint64_t s_keys[CV_COUNT_WAVES][CV_LDS_KEYS];
  const uint32_t lane = threadIdx.x % HOT_WAVE;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / HOT_WAVE);
  const uint64_t stride = (uint64_t)gridDim.x * CV_COUNT_WAVES;
  /* column `lane` of the tile: no other lane reads or writes it */
  uint32_t* tile = s_tile[wv] + lane;
  for (uint64_t it = (uint64_t)blockIdx.x * CV_COUNT_WAVES + wv; it < n_items;
       it += stride) {
    const AhChunk ch = chunks[it / n_tiles];
    const uint32_t col = (uint32_t)(it % n_tiles) * CV_TILE_COLS + lane;
    const uint64_t row0 = row_start[ch.group];
    const uint64_t R64 = row_start[ch.group + 1] - row0;
    if (R64 == 0 || R64 > CV_MAX_LIMIT) continue; /* wave-uniform */
    const uint32_t R = (uint32_t)R64;
    const uint64_t* g_keys = row_key + row0;
    hot_wave_sync();
    if (R <= CV_LDS_KEYS)
      for (uint32_t r = lane; r < R; r += HOT_WAVE) s_keys[wv][r] = g_keys[r];
    hot_wave_sync();
    if (col >= n_grid) continue; /* nothing below crosses lanes */
    const uint32_t* rows = group_rows + ch.begin;
    if (R > CV_BAND_MAX_ROWS) {
      /* wide group: straight into the counter matrix */
      uint32_t* ccol = cnt + row0 * n_grid + col;
      uint32_t k = 0;
      for (; k + CV_UNROLL <= ch.n; k += CV_UNROLL) {
        double v[CV_UNROLL];
#pragma unroll
        for (int u = 0; u < CV_UNROLL; u++)
          v[u] = vals[(uint64_t)rows[k + u] * n_grid + col];
        uint32_t rr[CV_UNROLL];
#pragma unroll
        for (int u = 0; u < CV_UNROLL; u++)
          rr[u] = cv_local_row(s_keys[wv], g_keys, R, cv_key(v[u]));
#pragma unroll
        for (int u = 0; u < CV_UNROLL; u++)
          if (rr[u] < R) atomicAdd(&ccol[(uint64_t)rr[u] * n_grid], 1u);
      }
      for (; k < ch.n; k++) {
        const uint32_t r = cv_local_row(
            s_keys[wv], g_keys, R, cv_key(vals[(uint64_t)rows[k] * n_grid + col]));
        if (r < R) atomicAdd(&ccol[(uint64_t)r * n_grid], 1u);
      }
      continue;
    }
    for (uint32_t band0 = 0; band0 < R; band0 += CV_BAND_ROWS) {
      const uint32_t bh = HOT_MIN((uint32_t)CV_BAND_ROWS, R - band0);
      for (uint32_t r = 0; r < bh; r++) tile[r * CV_TILE_COLS] = 0;
      uint32_t k = 0;
      for (; k + CV_UNROLL <= ch.n; k += CV_UNROLL) {
        double v[CV_UNROLL];
#pragma unroll
        for (int u = 0; u < CV_UNROLL; u++)
          v[u] = vals[(uint64_t)rows[k + u] * n_grid + col];
        /* the searches side by side, then the increments; a NaN's row and
         * a row below the band wrap to far above bh */
        uint32_t rr[CV_UNROLL];
#pragma unroll
        for (int u = 0; u < CV_UNROLL; u++)
          rr[u] = cv_local_row(s_keys[wv], g_keys, R, cv_key(v[u])) - band0;
#pragma unroll
        for (int u = 0; u < CV_UNROLL; u++)
          if (rr[u] < bh) tile[rr[u] * CV_TILE_COLS] += 1;
      }
      for (; k < ch.n; k++) {
        const uint32_t r =
            cv_local_row(s_keys[wv], g_keys, R,
                         cv_key(vals[(uint64_t)rows[k] * n_grid + col])) - band0;
        if (r < bh) tile[r * CV_TILE_COLS] += 1;
      }
      for (uint32_t r = 0; r < bh; r++) {
        const uint32_t c = tile[r * CV_TILE_COLS];
        if (c) atomicAdd(&cnt[(row0 + band0 + r) * n_grid + col], c);
      }
    }
  }
}

/* ------------------------------------------------------------------ */
/* host side                                                          */
/* ------------------------------------------------------------------ */

namespace {

/* result of the last exec + pass-to-pass scratch; every buffer grow-only */
struct CvState {
  /* result */
  double* d_out = nullptr;          /* [n_rows x n_grid] */
  uint32_t* d_row_group = nullptr;  /* [n_rows] */
  double* d_row_value = nullptr;    /* [n_rows] */
  size_t out_cap = 0, row_group_cap = 0, row_value_cap = 0; /* bytes */
  uint64_t n_rows = 0;
  int32_t n_grid = 0;
  bool valid = false;
  /* input staging */
  double* d_vals = nullptr;         /* host-matrix form only */
  uint32_t* d_group_rows = nullptr;
  AhChunk* d_chunks = nullptr;
  uint64_t* d_table_start = nullptr; /* [n_groups + 1] */
  uint32_t* d_lists = nullptr;       /* wave list, then block list */
  size_t vals_cap = 0, group_rows_cap = 0, chunks_cap = 0, table_start_cap = 0,
         lists_cap = 0;
  /* scratch */
  unsigned long long* d_table = nullptr; /* all groups' slices */
  uint32_t* d_row_counts = nullptr;      /* [n_groups] distinct counters,
                                          * then the overflow word */
  unsigned long long* d_zero = nullptr;  /* [n_groups] */
  uint64_t* d_row_start = nullptr;       /* [n_groups + 1] */
  uint64_t* d_row_key = nullptr;         /* [n_rows] */
  uint32_t* d_cnt = nullptr;             /* [n_rows x n_grid] */
  size_t table_cap = 0, row_counts_cap = 0, zero_cap = 0, row_start_cap = 0,
         row_key_cap = 0, cnt_cap = 0;
};

CvState g_cv;

/* what the host derives from the CSR and the limit before anything runs */
struct CvPlan {
  std::vector<uint64_t> table_start; /* [n_groups + 1] */
  std::vector<uint32_t> wave_list, block_list;
  uint64_t max_rows = 0;             /* sum of min(limit, members * n_grid) */
};

/* Argument checks and table layout shared by both entry points; nothing is
 * launched or allocated before they pass.  Returns 0 or 1. */
int cv_validate(uint32_t n_in_rows, int64_t n_grid, const uint32_t* group_rows,
                const uint64_t* group_offsets, uint32_t n_groups,
                uint32_t limit, CvPlan* plan, char* errbuf, size_t errbuf_len) {
  static const char* op = "aggr count_values";
  if (limit == 0 || limit > CV_MAX_LIMIT)
    return ah_csr_err(errbuf, errbuf_len, op,
                      "max_rows_per_group must lie in [1, 2^24]");
  if (int rc = ah_validate_csr(op, n_in_rows, n_grid, group_rows, group_offsets,
                               n_groups, errbuf, errbuf_len))
    return rc;
  plan->table_start.assign((size_t)n_groups + 1, 0);
  uint64_t slots = 0;
  bool too_many_slots = false;
  for (uint32_t g = 0; g < n_groups; g++) {
    const uint64_t members = group_offsets[g + 1] - group_offsets[g];
    /* members < 2^32, n_grid <= 2^30 */
    const uint64_t cells = members * (uint64_t)n_grid;
    const uint64_t rows = std::min<uint64_t>(limit, cells);
    /* bound the result before any kernel runs */
    if (rows > ((uint64_t)INT64_MAX / 8 / (uint64_t)n_grid) - plan->max_rows)
      return ah_csr_err(errbuf, errbuf_len, op, "result size overflows");
    plan->max_rows += rows;
    uint64_t cap = 0;
    if (members) {
      const uint64_t want = 2 * std::min<uint64_t>((uint64_t)limit + 1, cells);
      cap = CV_MIN_CAP;
      while (cap < want) cap <<= 1;
      if (cap <= CVOT_WAVE_CAP) plan->wave_list.push_back(g);
      else plan->block_list.push_back(g);
    }
    slots += cap;
    if (slots > CV_MAX_SLOTS) too_many_slots = true, slots = CV_MAX_SLOTS;
    plan->table_start[g + 1] = slots;
  }
  if (too_many_slots)
    return ah_csr_err(errbuf, errbuf_len, op,
                      "table size overflows 2^31 slots");
  return 0;
}

/* the pipeline over a device matrix; the caller holds the context lock and
 * has validated the arguments into plan */
int cv_run(const double* d_vals, int32_t n_grid, const uint32_t* group_rows,
           const uint64_t* group_offsets, uint32_t n_groups, uint32_t limit,
           const CvPlan& plan, uint64_t* out_n_rows, char* errbuf,
           size_t errbuf_len) {
  CvState& a = g_cv;
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
  ah_build_chunks(group_offsets, n_groups, CV_CHUNK_MEMBERS, &chunks);
  const uint32_t n_tiles = ((uint32_t)n_grid + CV_TILE_COLS - 1) / CV_TILE_COLS;
  const uint64_t n_items = (uint64_t)chunks.size() * n_tiles;
  const uint64_t n_slots = plan.table_start[n_groups];
  const uint32_t n_wave = (uint32_t)plan.wave_list.size();
  const uint32_t n_block = (uint32_t)plan.block_list.size();

  hipStream_t st = vm_ctx_stream();
  hipEvent_t ev_start, ev_stop;
  vm_ctx_events(&ev_start, &ev_stop);

  VM_HIP_TRY(hot_reserve(&a.d_group_rows, &a.group_rows_cap, (size_t)n_members * 4),
             "alloc group rows");
  VM_HIP_TRY(hot_reserve(&a.d_chunks, &a.chunks_cap, chunks.size() * sizeof(AhChunk)),
             "alloc chunks");
  VM_HIP_TRY(hot_reserve(&a.d_table_start, &a.table_start_cap,
                         ((size_t)n_groups + 1) * 8), "alloc table start");
  VM_HIP_TRY(hot_reserve(&a.d_lists, &a.lists_cap,
                         ((size_t)n_wave + n_block) * 4), "alloc sort lists");
  VM_HIP_TRY(hot_reserve(&a.d_table, &a.table_cap, (size_t)n_slots * 8),
             "alloc tables");
  VM_HIP_TRY(hot_reserve(&a.d_row_counts, &a.row_counts_cap,
                         ((size_t)n_groups + 1) * 4), "alloc row counts");
  VM_HIP_TRY(hot_reserve(&a.d_zero, &a.zero_cap, (size_t)n_groups * 8),
             "alloc zero words");
  VM_HIP_TRY(hot_reserve(&a.d_row_start, &a.row_start_cap, ((size_t)n_groups + 1) * 8),
             "alloc row start");
  uint32_t* d_overflow = a.d_row_counts + n_groups;
  /* blocking copies: the host arrays are free to go when they return */
  VM_HIP_TRY(hipMemcpy(a.d_group_rows, group_rows, (size_t)n_members * 4,
                       hipMemcpyHostToDevice), "upload group rows");
  VM_HIP_TRY(hipMemcpy(a.d_chunks, chunks.data(), chunks.size() * sizeof(AhChunk),
                       hipMemcpyHostToDevice), "upload chunks");
  VM_HIP_TRY(hipMemcpy(a.d_table_start, plan.table_start.data(),
                       ((size_t)n_groups + 1) * 8, hipMemcpyHostToDevice),
             "upload table start");
  if (n_wave)
    VM_HIP_TRY(hipMemcpy(a.d_lists, plan.wave_list.data(), (size_t)n_wave * 4,
                         hipMemcpyHostToDevice), "upload wave list");
  if (n_block)
    VM_HIP_TRY(hipMemcpy(a.d_lists + n_wave, plan.block_list.data(),
                         (size_t)n_block * 4, hipMemcpyHostToDevice),
               "upload block list");

  VM_HIP_TRY(hipEventRecord(ev_start, st), "event start");
  /* the table fill is part of the operator's cost: it is timed */
  VM_HIP_TRY(hipMemsetAsync(a.d_table, 0xFF, (size_t)n_slots * 8, st),
             "fill tables");
  VM_HIP_TRY(hipMemsetAsync(a.d_row_counts, 0, (size_t)n_groups * 4, st),
             "zero row counts");
  VM_HIP_TRY(hipMemsetAsync(d_overflow, 0xFF, 4, st), "reset overflow word");
  VM_HIP_TRY(hipMemsetAsync(a.d_zero, 0xFF, (size_t)n_groups * 8, st),
             "reset zero words");
  hipLaunchKernelGGL(cv_insert_kernel, dim3(ah_blocks(n_items, CV_INSERT_WAVES)),
                     dim3(CV_INSERT_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                     a.d_group_rows, a.d_chunks, n_items, n_tiles, a.d_table,
                     a.d_table_start, limit, a.d_row_counts, a.d_zero, d_overflow);
  hot_scan_launch(a.d_row_counts, n_groups, a.d_row_start, st);
  /* the output size is data-dependent: the host learns n_rows here */
  uint64_t n_rows = 0;
  uint32_t overflow_group = CV_NO_GROUP;
  VM_HIP_TRY(hipMemcpyAsync(&n_rows, a.d_row_start + n_groups, 8,
                            hipMemcpyDeviceToHost, st), "download n_rows");
  VM_HIP_TRY(hipMemcpyAsync(&overflow_group, d_overflow, 4,
                            hipMemcpyDeviceToHost, st), "download overflow word");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync insert");
  {
    hipError_t kerr = hipGetLastError();
    if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "insert kernel", kerr);
  }
  if (overflow_group != CV_NO_GROUP) {
    if (errbuf && errbuf_len)
      snprintf(errbuf, errbuf_len,
               "vmgpu: aggr count_values: group %u has more than %u distinct "
               "values", overflow_group, limit);
    return 1;
  }
  if (n_rows > plan.max_rows)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: inconsistent row count");

  if (n_rows) {
    const uint64_t n_out = n_rows * (uint64_t)n_grid;
    VM_HIP_TRY(hot_reserve(&a.d_out, &a.out_cap, (size_t)n_out * 8),
               "alloc count_values rows");
    VM_HIP_TRY(hot_reserve(&a.d_cnt, &a.cnt_cap, (size_t)n_out * 4), "alloc counters");
    VM_HIP_TRY(hot_reserve(&a.d_row_group, &a.row_group_cap, (size_t)n_rows * 4),
               "alloc row groups");
    VM_HIP_TRY(hot_reserve(&a.d_row_value, &a.row_value_cap, (size_t)n_rows * 8),
               "alloc row values");
    VM_HIP_TRY(hot_reserve(&a.d_row_key, &a.row_key_cap, (size_t)n_rows * 8),
               "alloc row keys");
    VM_HIP_TRY(hipMemsetAsync(a.d_cnt, 0, (size_t)n_out * 4, st), "zero counters");
    if (n_wave)
      hipLaunchKernelGGL(cv_rows_wave_kernel,
                         dim3(ah_blocks(n_wave, HOT_WAVES_PER_BLOCK)),
                         dim3(HOT_BLOCK_THREADS), 0, st, a.d_lists, n_wave,
                         a.d_table, a.d_table_start, a.d_row_start, a.d_zero,
                         a.d_row_key, a.d_row_group, a.d_row_value);
    if (n_block)
      hipLaunchKernelGGL(cv_rows_block_kernel,
                         dim3(std::min<uint32_t>(n_block, CV_ROWS_BLOCKS)),
                         dim3(HOT_BLOCK_THREADS), 0, st, a.d_lists + n_wave,
                         n_block, a.d_table, a.d_table_start, a.d_row_start,
                         a.d_zero, a.d_row_key, a.d_row_group, a.d_row_value);
    hipLaunchKernelGGL(cv_count_kernel, dim3(ah_blocks(n_items, CV_COUNT_WAVES)),
                       dim3(CV_COUNT_THREADS), 0, st, d_vals, (uint32_t)n_grid,
                       a.d_group_rows, a.d_chunks, n_items, n_tiles, a.d_row_key,
                       a.d_row_start, a.d_cnt);
    hipLaunchKernelGGL(ah_u32_to_f64_kernel<true>, dim3(ah_blocks(n_out, 256)),
                       dim3(256), 0, st, a.d_cnt, n_out, a.d_out);
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

void vm_aggrcv_shutdown(void) {
  CvState& a = g_cv;
  (void)hipFree(a.d_out);
  (void)hipFree(a.d_row_group);
  (void)hipFree(a.d_row_value);
  (void)hipFree(a.d_vals);
  (void)hipFree(a.d_group_rows);
  (void)hipFree(a.d_chunks);
  (void)hipFree(a.d_table_start);
  (void)hipFree(a.d_lists);
  (void)hipFree(a.d_table);
  (void)hipFree(a.d_row_counts);
  (void)hipFree(a.d_zero);
  (void)hipFree(a.d_row_start);
  (void)hipFree(a.d_row_key);
  (void)hipFree(a.d_cnt);
  a = CvState();
}

extern "C" {

int vmgpu_aggr_count_values_exec(const double* values, uint32_t n_series,
                                 int32_t n_grid, const uint32_t* group_rows,
                                 const uint64_t* group_offsets,
                                 uint32_t n_groups, uint32_t max_rows_per_group,
                                 uint64_t* out_n_rows, char* errbuf,
                                 size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  g_cv.valid = false;
  CvPlan plan;
  if (int rc = cv_validate(n_series, n_grid, group_rows, group_offsets, n_groups,
                           max_rows_per_group, &plan, errbuf, errbuf_len))
    return rc;
  const bool has_members = n_groups && group_offsets[n_groups];
  if (has_members) {
    if (!values)
      return vm_set_err(errbuf, errbuf_len, "vmgpu: aggr count_values: bad args");
    const size_t vbytes = (size_t)n_series * (size_t)n_grid * 8;
    VM_HIP_TRY(hot_reserve(&g_cv.d_vals, &g_cv.vals_cap, vbytes), "alloc values");
    VM_HIP_TRY(hipMemcpy(g_cv.d_vals, values, vbytes, hipMemcpyHostToDevice),
               "upload values");
  }
  return cv_run(g_cv.d_vals, n_grid, group_rows, group_offsets, n_groups,
                max_rows_per_group, plan, out_n_rows, errbuf, errbuf_len);
}

int vmgpu_batch_aggr_count_values_exec(uint64_t handle,
                                       const uint32_t* group_rows,
                                       const uint64_t* group_offsets,
                                       uint32_t n_groups,
                                       uint32_t max_rows_per_group,
                                       uint64_t* out_n_rows, char* errbuf,
                                       size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  g_cv.valid = false;
  vm_batch_cols b;
  if (vm_batch_cols_get(handle, &b) != 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  if (!b.d_out || b.last_rows == 0 || b.last_grid <= 0)
    return vm_set_err(errbuf, errbuf_len,
                      "vmgpu: no rollup output on this batch "
                      "(vmgpu_rollup_exec first)");
  CvPlan plan;
  if (int rc = cv_validate(b.last_rows, b.last_grid, group_rows, group_offsets,
                           n_groups, max_rows_per_group, &plan, errbuf,
                           errbuf_len))
    return rc;
  return cv_run(b.d_out, b.last_grid, group_rows, group_offsets, n_groups,
                max_rows_per_group, plan, out_n_rows, errbuf, errbuf_len);
}

int vmgpu_aggr_count_values_fetch(uint32_t* row_group, double* row_value,
                                  double* out, char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited())
    return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  const CvState& a = g_cv;
  if (!a.valid)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: no aggr count_values result");
  if (a.n_rows == 0) return 0;
  hipStream_t st = vm_ctx_stream();
  if (row_group)
    VM_HIP_TRY(hipMemcpyAsync(row_group, a.d_row_group, a.n_rows * 4,
                              hipMemcpyDeviceToHost, st), "download row groups");
  if (row_value)
    VM_HIP_TRY(hipMemcpyAsync(row_value, a.d_row_value, a.n_rows * 8,
                              hipMemcpyDeviceToHost, st), "download row values");
  if (out)
    VM_HIP_TRY(hipMemcpyAsync(out, a.d_out, (size_t)a.n_rows * a.n_grid * 8,
                              hipMemcpyDeviceToHost, st), "download count_values rows");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync fetch");
  return 0;
}

}  // extern "C"
