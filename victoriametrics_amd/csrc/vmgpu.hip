/* vmgpu.hip — MI355X-native (gfx950/CDNA4) rollup + aggregation engine.
 *
 * Replaces the reference's per-series worker fan-out
 * (netstorage.Results.RunParallel, netstorage.go:219 +
 * evalRollup{With,No}IncrementalAggregate, eval.go:1927/1968) with four HIP
 * kernels picked by series length, all sharing the device rollup set in
 * rollup_device.h:
 *
 *   rollup_wave_kernel  — series with <= CHUNK_WAVE samples: one 64-lane
 *       wavefront per series.  The wave stages the series' (ts, vals)
 *       columns into LDS with coalesced loads, optionally drops Prometheus
 *       stale NaNs (eval.go:2108) and applies removeCounterResets
 *       (rollup.go:921) as an EXACT-order fused scan (sparse sequential
 *       correction walk over ballot'd reset/gap events + segmented prefix
 *       max for the monotonic clamp), then evaluates the [start:end:step]
 *       grid with one lane per grid point (binary-search window seek in LDS,
 *       left-to-right serial window reductions => bit-exact vs the
 *       sequential reference semantics).
 *   rollup_pipe_kernel  — the wave kernel's software-pipelined variant for
 *       rate/deriv_fast over series of at most 256 samples (pipe_kernel.h):
 *       the next series' loads stay in flight while this one is evaluated.
 *   rollup_block_kernel — series up to CHUNK_BLOCK samples: one 256-thread
 *       workgroup per series, series staged in up to 128 KiB of LDS.
 *   rollup_huge_kernel  — longer series: per-series preprocessing into a
 *       global scratch column, grid evaluated from L2-cached global memory.
 *
 * Cross-series by-label aggregation (aggr_incremental.go) is fused into the
 * grid loop: identity-initialized [n_groups x n_grid] value/count matrices
 * updated with device-scope f64 atomics (CAS loops for min/max/product), so
 * the 1M-series rollup never materializes per-series grids in HBM.  The
 * multi-GPU merge all-reduces those matrices BEFORE the
 * finalize step; plan->skip_finalize exposes exactly that cut.
 *
 * This file also owns the context (stream, pool, events) and the resident
 * Batch with its one builder.  What runs over a batch or its output without
 * sharing these kernels lives in files of its own and reaches the context
 * through batch_access.h and devalloc.h: hot.hip, cvot.hip, topk.hip (the
 * topk family) and hstat.hip (the histogram transforms).
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <map>
#include <mutex>
#include <vector>

#include "batch_access.h"
#include "host_common.h"
#include "pipe_probe.h"
#include "rollup_device.h"
#include "vm_div1e3.h"
#include "../../include/vmgpu.h"

/* What rollup_pipe_kernel (pipe_kernel.h), the flagship rate kernel, relies
 * on.  The measurements behind each point are in profiles/.
 *   sentinel slab   two {t, v} records in front of sample 0 (t = INT64_MIN)
 *                   and two behind the last sample (t = INT64_MAX), so the
 *                   boundary probe and the rate evaluator index records
 *                   -2 .. count+1 without edge clamps
 *   count probe     the upper bound next to a hint is a sum of compares over
 *                   four records read in one LDS trip (pipe_probe.h); the
 *                   hint is one f64 accumulator advanced per 64-point round
 *   window / step   two 64-bit divisions, done once per wave: with a plan
 *                   window the quotient is the same for every series
 *   descriptors     selection entry, offsets, scrape interval and group id
 *                   are read through the constant address space, so they are
 *                   scalar loads, issued two series ahead
 *   staged loads    the b128 sample loads are inline asm the compiler does
 *                   not count; the one hand-placed wait is at the top of the
 *                   next iteration
 *   dt / 1e3        the exact multiply+fma sequence of vm_div1e3.h for
 *                   series whose span fits 31 bits (eval_rate_fused's dt32)
 * Shared with the wave and block kernels: removeCounterResets skips the
 * segmented prefix-max when the monotonic clamp is provably the identity
 * (vm_clamp_violates). */

#define WAVE 64
#define BLOCK_THREADS 256
#define WAVES_PER_BLOCK (BLOCK_THREADS / WAVE)
#define CHUNK_WAVE 512
/* block-kernel series cap: 16 B/sample of LDS + 16 B control word must stay
 * within the 64 KiB dynamic-LDS launch limit (the 160 KiB/CU budget is a
 * static-declaration property on gfx950) */
#define CHUNK_BLOCK 4064
#define MAX_WAVE_BLOCKS 4096

/* ------------------------------------------------------------------ */
/* device helpers                                                     */
/* ------------------------------------------------------------------ */

static VM_DEV void wave_lds_sync() {
  /* All DS and VMEM ops of this wave complete + compiler barrier: safe
   * cross-lane visibility within one wavefront for LDS *and* for the huge
   * kernel's global-scratch variant (no workgroup barrier needed).  Used
   * between phases only, never inside hot loops. */
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

static VM_DEV void wave_ds_sync() {
  /* LDS-only phase barrier for one wavefront: DS ops (including the
   * ds_bpermute behind __shfl) are lgkm-counted, so this gives cross-lane
   * LDS visibility while deliberately leaving prefetched global loads
   * (vmcnt) in flight — the point of the software-pipelined kernel. */
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

/* STR = element stride in int64 units: 1 for column layout, 2 for the pipe
 * kernel's (t, v) pair-interleaved LDS (one ds_read2/b128 per sample). */
template <int STR = 1>
static VM_DEV int vm_upper_bound(const int64_t* ts, int n, int64_t seek) {
  /* first index with ts[idx] > seek (seekFirstTimestampIdxAfter semantics,
   * rollup.go:825-855 — the reference's ±2 hint only narrows the range). */
  int i = 0, j = n;
  while (i < j) {
    int h = (i + j) >> 1;
    if (ts[h * STR] <= seek) i = h + 1;
    else j = h;
  }
  return i;
}

/* Per-lane upper bound from a density-interpolated guess: a bounded walk
 * resolves near-uniform sampling in 1-2 probes; anything irregular falls
 * back to a plain binary search.  Result identical to vm_upper_bound. */
template <int STR = 1>
static VM_DEV int vm_ub_hint(const int64_t* ts, int n, int64_t seek, int g) {
  if (g < 0) g = 0;
  if (g > n) g = n;
  for (int steps = 0; steps < 4; steps++) {
    bool gt_here = (g >= n) || (ts[g * STR] > seek);
    if (!gt_here) { g++; continue; }       /* result is above g */
    if (g == 0 || ts[(g - 1) * STR] <= seek) return g;
    g--;                                   /* result is below g */
  }
  return vm_upper_bound<STR>(ts, n, seek);
}

/* Branch-free variant: four independent probes decide among {g-1, g, g+1}
 * with pure selects; lanes outside the +-1 window (rare on real scrape
 * cadences) take a wave-coordinated binary-search fallback.  Result
 * identical to vm_upper_bound. */
template <int STR = 1>
static VM_DEV int vm_ub_hint_fast(const int64_t* ts, int n, int64_t seek, int g) {
  if (g < 0) g = 0;
  if (g > n) g = n;
  int i_m2 = g - 2 < 0 ? 0 : g - 2;
  int i_m1 = g - 1 < 0 ? 0 : g - 1;
  int i_0 = g < n - 1 ? g : (n - 1 < 0 ? 0 : n - 1);
  int i_p1 = g + 1 < n - 1 ? g + 1 : (n - 1 < 0 ? 0 : n - 1);
  int64_t t_m2 = ts[i_m2 * STR];
  int64_t t_m1 = ts[i_m1 * STR];
  int64_t t_0 = ts[i_0 * STR];
  int64_t t_p1 = ts[i_p1 * STR];
  bool le_m2 = (g - 2 < 0) || (t_m2 <= seek);  /* ts[g-2] <= seek (vacuous at edge) */
  bool le_m1 = (g - 1 < 0) || (g - 1 >= n) || (t_m1 <= seek);
  bool gt_m1 = (g - 1 >= 0) && (g - 1 < n) && (t_m1 > seek);
  bool le_0 = (g < n) && (t_0 <= seek);
  bool gt_0 = (g >= n) || (t_0 > seek);
  bool gt_p1 = (g + 1 >= n) || (t_p1 > seek);
  /* ok(x): (x==0 or ts[x-1]<=seek) and (x==n or ts[x]>seek) */
  bool ok_g = le_m1 && gt_0;
  bool ok_p1 = (g + 1 <= n) && le_0 && gt_p1;
  bool ok_m1 = (g - 1 >= 0) && le_m2 && gt_m1;
  int r = ok_g ? g : (ok_p1 ? g + 1 : (ok_m1 ? g - 1 : -1));
  if (__any(r < 0)) {
    if (r < 0) r = vm_upper_bound<STR>(ts, n, seek);
  }
  return r;
}

/* a wave-uniform 64-bit value moved to scalar registers */
static VM_DEV int64_t vm_uniform_i64(int64_t x) {
  uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
  uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

/* Sentinel records of the pipe kernel's pair-interleaved slab: two 16-byte
 * {t, v} records in front of sample 0 (t = INT64_MIN) and two behind sample
 * count-1 (t = INT64_MAX), v = 0 in all four. */
#define VM_SENT_RECS 2
#define VM_SENT_BYTES (2 * VM_SENT_RECS * 16)

/* The pipe kernel's boundary probe over its sentinel-padded slab (stride 2,
 * ts = sample 0): vm_probe_count4 reads the four records round the hint in
 * one LDS trip and answers with a sum of compares (derivation and edge cases
 * in pipe_probe.h); lanes whose hint missed take a wave-coordinated
 * binary-search fallback.  Result identical to vm_upper_bound<2>. */
static VM_DEV int vm_ub_pipe(const int64_t* ts, int n, int64_t seek, int g) {
  int r = vm_probe_count4(ts, n, seek, g);
  if (__any(r < 0)) {
    if (r < 0) r = vm_upper_bound<2>(ts, n, seek);
  }
  return r;
}

/* removeCounterResets clamp shortcut.  The monotonic clamp
 * x[k] = fmax(fin[k], x[k-1]) over a segment returns fin unchanged when
 * every non-boundary element already has fmax(fin[k], fin[k-1]) == fin[k]
 * bit for bit (induction over the segment: x[k-1] == fin[k-1]).  This is the
 * per-element violation test against the UNCLAMPED predecessor p: a NaN on
 * either side, a smaller value, or an equal compare with different bits
 * (+0.0 / -0.0, where fmax may return either) all count as violations and
 * keep the full prefix-max path. */
static VM_DEV bool vm_clamp_violates(double x, double p) {
  return !(x >= p) ||
         (x == p && __double_as_longlong(x) != __double_as_longlong(p));
}

static VM_DEV void vm_atomic_min_f64(double* addr, double val) {
  unsigned long long* p = (unsigned long long*)addr;
  unsigned long long old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (val < __longlong_as_double((long long)old)) {
    unsigned long long assumed = old;
    old = atomicCAS(p, assumed, (unsigned long long)__double_as_longlong(val));
    if (old == assumed) break;
  }
}

static VM_DEV void vm_atomic_max_f64(double* addr, double val) {
  unsigned long long* p = (unsigned long long*)addr;
  unsigned long long old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (val > __longlong_as_double((long long)old)) {
    unsigned long long assumed = old;
    old = atomicCAS(p, assumed, (unsigned long long)__double_as_longlong(val));
    if (old == assumed) break;
  }
}

static VM_DEV void vm_atomic_mul_f64(double* addr, double val) {
  unsigned long long* p = (unsigned long long*)addr;
  unsigned long long old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (true) {
    unsigned long long assumed = old;
    double cur = __longlong_as_double((long long)assumed);
    old = atomicCAS(p, assumed, (unsigned long long)__double_as_longlong(cur * val));
    if (old == assumed) break;
  }
}

/* Kernel-side plan (host plan flattened; all wave-uniform). */
struct KPlan {
  int64_t start, end, step;
  int64_t window;          /* plan window (0 => auto-adjust per series) */
  int64_t lookback_delta;
  int64_t min_staleness;
  int64_t max_staleness;   /* removeCounterResets staleness interval */
  int32_t n_grid;
  int32_t func;
  int32_t aggr;
  int32_t sspc;            /* samplesScannedPerCall */
  int32_t may_adjust;
  int32_t is_default;
  int32_t rcr;
  int32_t drop_stale;
  int32_t chunk_wave;      /* LDS samples per wave (wave kernel), 64-aligned */
  int32_t chunk_block;     /* LDS samples for the block kernel, sized to the
                              batch's longest block-class series */
  int32_t pre_func;        /* VMGPU_PRE_* value transform after rcr */
  int32_t jbuf_elems;      /* LDS boundary-cache elements for the rate paths */
  int32_t jbuf_mode;       /* 0 = none; 1 = u16 j-cache (shared-boundary);
                              2 = sample-scatter Et/Ev/J boundary map */
  double arg;
  double arg2;
};

/* Block-kernel LDS: 32B header + chunk_block*16 series data + 256B scratch
 * + (when it fits the 64 KiB dynamic limit and a rate j-cache is wanted)
 * n_grid u16 window-end indices.  Host sizing and kernel carve must agree. */
static __host__ __device__ inline size_t vm_block_lds_bytes(
    int32_t chunk_block, int32_t jbuf_mode, int32_t n_grid, int* has_jbuf) {
  size_t base = 32 + (size_t)chunk_block * 16 + 256;
  size_t jb = ((size_t)n_grid * 2 + 15) & ~(size_t)15;
  if (jbuf_mode >= 1 && base + jb <= 64 * 1024) {
    if (has_jbuf) *has_jbuf = 1;
    return base + jb;
  }
  if (has_jbuf) *has_jbuf = 0;
  return base;
}

/* LDS bytes for the rate boundary cache (host sizing and kernel carve must
 * agree) */
static __host__ __device__ inline size_t vm_jbuf_bytes(int32_t mode,
                                                       int32_t elems) {
  size_t a2 = ((size_t)elems * 2 + 15) & ~(size_t)15;
  if (mode == 2) return a2;            /* J u16 over [-dg, n_grid) */
  if (mode == 1) return a2;            /* J u16 over [0, n_grid) */
  return 0;
}

/* Per-wave LDS of the wave and pipe kernels without the boundary cache:
 * chunk_wave 16-byte sample slots + 256 B scratch.  The pipe kernel's slab
 * also carries the sentinel records (VM_SENT_BYTES: 32 B in front of sample
 * 0, 32 B of room behind the last slot for a full-length series).  The
 * kernel carves and the host sizing (launch LDS and the jbuf fit) all go
 * through here. */
static __host__ __device__ inline size_t vm_wave_slab_bytes(int32_t chunk_wave,
                                                            bool pipe) {
  return (size_t)chunk_wave * 16 + 256 + (pipe ? VM_SENT_BYTES : 0);
}

struct KIO {
  const int64_t* ts = nullptr;
  const double* vals = nullptr;
  const uint64_t* offsets = nullptr;
  const uint32_t* series_sel = nullptr; /* list of series ids for this kernel */
  uint32_t n_sel = 0;
  const int32_t* group_ids = nullptr;   /* may be null */
  const int64_t* series_si = nullptr;   /* batch scrape-interval index (raw
                                           0.6-quantile per series; 0 = use
                                           the plan default).  Valid only
                                           when no samples were dropped. */
  double* out = nullptr;                /* per-series [n_series x n_grid] or group values */
  double* out_counts = nullptr;         /* group counts */
  unsigned long long* samples_scanned = nullptr;
  /* huge-kernel scratch */
  int64_t* scr_ts = nullptr;
  double* scr_vals = nullptr;
  const uint64_t* scr_offsets = nullptr; /* per huge-series scratch base */
};

/* --- phase A: compacted load (executed by ONE wave) ----------------- */
/* Copies [g_ts,g_vals)[0..n) to dst, dropping stale NaNs if requested.
 * Returns new count. dst may be LDS or global. */
struct __align__(16) vm_i64x2 { int64_t x, y; };

template <int STR = 1>
static __device__ int load_compact_wave(const int64_t* g_ts, const double* g_vals,
                                        int64_t n, int64_t* d_ts, double* d_vals,
                                        bool drop_stale, int lane) {
  int count = 0;
  int64_t src = 0;
  /* vector fast path: 128-element tiles via 16-B loads/stores (the staging
   * loop is instruction-issue-bound, not bandwidth-bound — see profiles/).
   * Falls to the scalar tile path when stale NaNs must be compacted out or
   * the running count is odd (LDS b128 stores need 16-B alignment);
   * column layout only. */
  if (STR == 1 && (((uintptr_t)g_ts | (uintptr_t)g_vals) & 15) == 0) {
    const uint64_t lt_mask = (lane == 63) ? 0x7fffffffffffffffULL
                                          : ((1ULL << lane) - 1);
    while (src + 2 <= n) {
      int64_t pairs = (n - src) >> 1;
      if (pairs > 64) pairs = 64;
      bool act = lane < pairs;
      double2 v = {0.0, 0.0};
      vm_i64x2 t = {0, 0};
      if (act) {
        v = *(const double2*)(g_vals + src + 2 * lane);
        t = *(const vm_i64x2*)(g_ts + src + 2 * lane);
      }
      bool k0 = act && !(drop_stale && vm_is_stale_nan(v.x));
      bool k1 = act && !(drop_stale && vm_is_stale_nan(v.y));
      uint64_t m0 = __ballot(k0), m1 = __ballot(k1);
      uint64_t full = (pairs == 64) ? ~0ULL : ((1ULL << pairs) - 1);
      if ((m0 & m1) == full && (count & 1) == 0) {
        if (act) {
          *(double2*)(d_vals + count + 2 * lane) = v;
          *(vm_i64x2*)(d_ts + count + 2 * lane) = t;
        }
        count += (int)(2 * pairs);
      } else {
        int below = __popcll(m0 & lt_mask) + __popcll(m1 & lt_mask);
        int dst0 = count + below;
        if (k0) { d_ts[dst0] = t.x; d_vals[dst0] = v.x; }
        if (k1) { int d1 = dst0 + (k0 ? 1 : 0); d_ts[d1] = t.y; d_vals[d1] = v.y; }
        count += __popcll(m0) + __popcll(m1);
      }
      src += 2 * pairs;
    }
  }
  for (; src < n; src += WAVE) {
    int64_t k = src + lane;
    bool active = k < n;
    double v = 0.0;
    int64_t t = 0;
    if (active) {
      v = g_vals[k];
      t = g_ts[k];
    }
    bool keep = active && !(drop_stale && vm_is_stale_nan(v));
    uint64_t m = __ballot(keep);
    if (keep) {
      int dst = count + __popcll(m & ((lane == 63) ? 0x7fffffffffffffffULL
                                                   : ((1ULL << lane) - 1)));
      d_ts[dst * STR] = t;
      d_vals[dst * STR] = v;
    }
    count += __popcll(m);
  }
  return count;
}

/* --- phase B: removeCounterResets as a wave scan ---------------------- */
/* EXACT restatement of rollup.go:921-958; see file header.  The two scans
 * that hold one sample per lane, load_rcr_fused_wave and rcr_scan_wave,
 * share rcr_round_single: they only fetch, call the round and store.  The
 * round hands the lane's final value to the caller's `store(x, fast)` on
 * each of its two paths (fast = the round took the fast path: x = v + corr
 * with corr unchanged).
 * The two scans that hold two samples per lane, rcr_scan_pairs and
 * rcr_scan_col_pairs further down, each keep their own copy of the pair
 * round: every shared form of it that was built (values returned, values
 * handed to a callable, values stored by the round) made the flagship pipe
 * kernel 5 % slower, profiles/rcr_scan_unify.md.  A change to the scan rule
 * is made here and in those two. */

/* what a scan threads from one round to the next (all wave-uniform) */
struct RcrCarry {
  double corr = 0.0;      /* running correction */
  double prev_raw = 0.0;  /* raw value of the previous round's last sample */
  int64_t prev_ts = 0;    /* its timestamp */
  double prev_fin = 0.0;  /* its clamped output */
};

/* Single round: lane l holds sample l of a 64-sample round.  `first_round`
 * (wave-uniform) says that lane 0 holds element 0 of the series, `last` is
 * the lane of the round's last active sample.  Calls store(x, fast) with
 * the lane's final value and advances the carry. */
template <class Store>
static VM_DEV void rcr_round_single(double v, int64_t t, bool active,
                                    bool first_round, int last, int64_t msi,
                                    int lane, RcrCarry& cy, Store store) {
  double pv = __shfl_up(v, 1);
  int64_t pt = __shfl_up(t, 1);
  if (lane == 0) { pv = cy.prev_raw; pt = cy.prev_ts; }
  bool isfirst = first_round && lane == 0;
  double d = v - pv;
  double inc = 0.0;
  if (!isfirst && d < 0) inc = ((-d * 8) < pv) ? (pv - v) : pv;
  bool gap = (!isfirst && msi > 0 && (t - pt) > msi);
  /* corrections in exact sequential order: only reset/gap events change the
   * running correction, and f64 `c + 0.0` is an identity, so walking the
   * (rare) event lanes reproduces the serial left-to-right sum bitwise. */
  uint64_t em = __ballot(active && (gap || inc != 0.0));
  /* fast path: no events, no negative deltas, and the chunk starts at or
   * above the carried clamp level -> corrections are uniform and the
   * monotonic clamp is a no-op. */
  uint64_t dm = __ballot(active && !isfirst && d < 0);
  if (em == 0 && dm == 0 &&
      (first_round || __shfl(v, 0) + cy.corr >= cy.prev_fin)) {
    store(v + cy.corr, true);
    cy.prev_raw = __shfl(v, last);
    cy.prev_ts = __shfl(t, last);
    cy.prev_fin = cy.prev_raw + cy.corr;
    return;
  }
  double c = cy.corr;
  double mycorr = cy.corr;
  while (em) {
    int b = __ffsll((unsigned long long)em) - 1;
    em &= em - 1;
    double ib = __shfl(inc, b);
    int gb = __shfl((int)gap, b);
    double cn = gb ? 0.0 : (c + ib);
    if (lane >= b) mycorr = cn;
    c = cn;
  }
  double fin = v + mycorr;
  /* monotonic clamp (rollup.go:952-956) = segmented prefix max; a gap
   * element keeps its raw value and is exempt (the Go `continue`).  A NaN
   * element keeps its value and restarts the running max, as the
   * reference's `values[i] < values[i-1]` test does on either side of it. */
  bool bnd = isfirst || gap || vm_isnan(fin);
  double x = fin;
  /* clamp shortcut (vm_clamp_violates): one neighbour shuffle + ballot;
   * lanes past the series end sit above every active one and feed nothing
   * that is stored or carried, so they are left out */
  double pfin = __shfl_up(fin, 1);
  if (lane == 0) pfin = cy.prev_fin;
  const bool clamp_needed =
      __ballot(active && !bnd && vm_clamp_violates(fin, pfin)) != 0;
  if (clamp_needed) {
    int f = bnd ? 1 : 0;
    if (lane == 0 && !bnd) x = fmax(x, cy.prev_fin);
    for (int dlt = 1; dlt < WAVE; dlt <<= 1) {
      double xo = __shfl_up(x, dlt);
      int fo = __shfl_up(f, dlt);
      if (lane >= dlt) {
        if (!f) x = fmax(x, xo);
        f = f | fo;
      }
    }
  }
  /* store() comes before the carry update: an in-place caller's store reads
   * cy.corr, and must see the correction the round started with */
  store(x, false);
  cy.corr = c;
  cy.prev_raw = __shfl(v, last);
  cy.prev_ts = __shfl(t, last);
  cy.prev_fin = __shfl(x, last);
}

/* Fused staging + scan of the wave kernel: when no sample is dropped (no
 * stale NaNs — the overwhelmingly common case), the scan runs on the
 * staging registers, saving the whole LDS re-read pass.  Returns the kept
 * count on success, or -1 to signal "drops present, redo via
 * load_compact_wave + rcr_scan_wave" (wave-uniform). */
static __device__ int load_rcr_fused_wave(const int64_t* g_ts, const double* g_vals,
                                          int64_t n, int64_t* d_ts, double* d_vals,
                                          bool drop_stale, int64_t msi, int lane) {
  RcrCarry cy;
  for (int64_t base = 0; base < n; base += WAVE) {
    int64_t k = base + lane;
    bool active = k < n;
    double v = 0.0;
    int64_t t = 0;
    if (active) {
      v = g_vals[k];
      t = g_ts[k];
    }
    if (drop_stale && __ballot(active && vm_is_stale_nan(v)) != 0) return -1;
    if (active) d_ts[k] = t;
    int last = (int)(n - base - 1);
    if (last > 63) last = 63;
    rcr_round_single(v, t, active, base == 0, last, msi, lane, cy,
                     [&](double x, bool) {
                       if (active) d_vals[k] = x;
                     });
  }
  return (int)n;
}

/* In-place scan over a dense column (stride STR in int64 units): the wave
 * and pipe kernels' fallback behind load_compact_wave. */
template <int STR = 1>
static __device__ void rcr_scan_wave(int64_t* d_ts, double* d_vals, int count,
                                     int64_t msi, int lane) {
  RcrCarry cy;
  for (int base = 0; base < count; base += WAVE) {
    int k = base + lane;
    bool active = k < count;
    double v = active ? d_vals[k * STR] : 0.0;
    int64_t t = active ? d_ts[k * STR] : 0;
    int last = count - base - 1;
    if (last > 63) last = 63;
    /* a fast round with no correction leaves the column as it is */
    rcr_round_single(v, t, active, base == 0, last, msi, lane, cy,
                     [&](double x, bool fast) {
                       if (fast && cy.corr == 0.0) return;
                       if (active) d_vals[k * STR] = x;
                     });
  }
}

/* --- preFunc value transforms (rollup_* families) -------------------- */
/* deltaValues (rollup.go:960), derivValues (:976) and the
 * rollup_scrape_interval preFunc (:476), applied in place after
 * removeCounterResets exactly as getRollupConfigs composes them.  Fast
 * paths are wave-elementwise; derivValues' duplicate-timestamp carry is
 * replayed serially on lane 0 when duplicates exist (rare — dedup
 * upstream normally removes them). */
static VM_DEV void pre_func_wave(const int64_t* d_ts, double* d_vals,
                                 int count, int mode, int lane) {
  if (count <= 0 || mode == VMGPU_PRE_NONE) return;
  if (mode == VMGPU_PRE_SCRAPE_INTERVAL) {
    /* values[i] = ts[i]/1e3 - ts[i-1]/1e3 (NaN seed); values[0]=values[1] */
    for (int base = 0; base < count; base += WAVE) {
      int k = base + lane;
      if (k < count) {
        double cur = (double)d_ts[k] / 1000.0;
        double prev = (k > 0) ? (double)d_ts[k - 1] / 1000.0 : vm_dnan();
        d_vals[k] = cur - prev;
      }
      wave_lds_sync();
    }
    if (lane == 0 && count > 1) d_vals[0] = d_vals[1];
    wave_lds_sync();
    return;
  }
  if (mode == VMGPU_PRE_DELTA) {
    double last = 0.0;
    if (count >= 2) last = d_vals[count - 1] - d_vals[count - 2];
    for (int base = 0; base + 1 < count; base += WAVE) {
      int k = base + lane;
      double a = 0, b = 0;
      bool act = (k + 1 < count);
      if (act) {
        a = d_vals[k];
        b = d_vals[k + 1];
      }
      wave_lds_sync();      /* all reads land before any write */
      if (act) d_vals[k] = b - a;
      wave_lds_sync();
    }
    if (lane == 0) d_vals[count - 1] = last;
    wave_lds_sync();
    return;
  }
  /* VMGPU_PRE_DERIV */
  bool dup = false;
  for (int base = 0; base + 1 < count; base += WAVE) {
    int k = base + lane;
    bool d = (k + 1 < count) && (d_ts[k + 1] == d_ts[k]);
    if (__ballot(d) != 0) dup = true;
  }
  if (!dup) {
    double last = 0.0;
    if (count >= 2)
      last = (d_vals[count - 1] - d_vals[count - 2]) /
             ((double)(d_ts[count - 1] - d_ts[count - 2]) / 1e3);
    for (int base = 0; base + 1 < count; base += WAVE) {
      int k = base + lane;
      double a = 0, b = 0;
      int64_t ta = 0, tb = 0;
      bool act = (k + 1 < count);
      if (act) {
        a = d_vals[k];
        b = d_vals[k + 1];
        ta = d_ts[k];
        tb = d_ts[k + 1];
      }
      wave_lds_sync();
      if (act) d_vals[k] = (b - a) / ((double)(tb - ta) / 1e3);
      wave_lds_sync();
    }
    if (lane == 0) d_vals[count - 1] = last;
    wave_lds_sync();
    return;
  }
  if (lane == 0) {
    /* exact serial replay of derivValues with the duplicate-ts carry */
    double prev_deriv = 0.0;
    double prev_value = d_vals[0];
    int64_t prev_ts = d_ts[0];
    for (int i = 0; i + 1 < count; i++) {
      double v = d_vals[i + 1];
      int64_t t = d_ts[i + 1];
      if (t == prev_ts) {
        d_vals[i] = prev_deriv;
        continue;
      }
      double dt = (double)(t - prev_ts) / 1e3;
      prev_deriv = (v - prev_value) / dt;
      d_vals[i] = prev_deriv;
      prev_value = v;
      prev_ts = t;
    }
    d_vals[count - 1] = prev_deriv;
  }
  wave_lds_sync();
}

/* --- per-series window parameters (doInternal preamble) -------------- */
/* getScrapeInterval (rollup.go:871-897): 0.6 quantile of the last <=20
 * sample gaps, computed wave-cooperatively with a rank-based selection
 * (identical result to sort + quantileSorted). */
template <bool LDS_ONLY, int STR = 1>
static __device__ int64_t scrape_interval_wave_t(const int64_t* d_ts, int count,
                                                 int64_t default_interval, int lane,
                                                 double* scratch) {
  if (count < 2) return default_interval;
  int cnt = count - 1;
  if (cnt > 20) cnt = 20;
  bool active = lane < cnt;
  double gap = 0.0;
  if (active) gap = (double)(d_ts[(count - 1 - lane) * STR] -
                             d_ts[(count - 2 - lane) * STR]);
  if (active) scratch[lane] = gap;
  if (LDS_ONLY) wave_ds_sync(); else wave_lds_sync();
  /* rank of this lane's gap among the cnt gaps (ties broken by lane);
   * scratch broadcast keeps the cnt probes independent (one LDS round trip)
   * instead of cnt serial shuffles */
  int rank = 0;
  for (int i = 0; i < cnt; i++) {
    double gi = scratch[i];
    if (active && (gi < gap || (gi == gap && i < lane))) rank++;
  }
  double nn = (double)cnt;
  double q_rank = 0.6 * (nn - 1);
  int li = (int)fmax(0.0, floor(q_rank));
  int ui = (int)fmin(nn - 1, (double)(li + 1));
  double w = q_rank - floor(q_rank);
  uint64_t mlo = __ballot(active && rank == li);
  uint64_t mhi = __ballot(active && rank == ui);
  int lane_lo = __ffsll((unsigned long long)mlo) - 1;
  int lane_hi = __ffsll((unsigned long long)mhi) - 1;
  double lo = __shfl(gap, lane_lo);
  double hi = __shfl(gap, lane_hi);
  double q = lo * (1 - w) + hi * w;
  int64_t si = (int64_t)q;
  if (si <= 0) return default_interval;
  return si;
}

static __device__ int64_t scrape_interval_wave(const int64_t* d_ts, int count,
                                               int64_t default_interval, int lane,
                                               double* scratch) {
  return scrape_interval_wave_t<false>(d_ts, count, default_interval, lane, scratch);
}

/* Batch scrape-interval index: getScrapeInterval's 0.6-quantile is a pure
 * function of the series' immutable resident timestamps, so it is computed
 * ONCE at batch creation (like the length-partition lists) and each query
 * reads it instead of re-deriving it per series.  Stored RAW (0 = "fewer
 than 2 samples or non-positive quantile": the kernels substitute the
 * plan's default, exactly as rollup.go:871-897 does).  Queries that drop
 * stale NaNs fall back to the in-kernel computation whenever the compacted
 * count differs from the stored one (the quantile could differ). */
__global__ __launch_bounds__(BLOCK_THREADS) void si_prep_kernel(
    const int64_t* ts, const uint64_t* offsets, uint32_t n_series,
    int64_t* out_si) {
  __shared__ double scratch[WAVES_PER_BLOCK][32];
  const int lane = threadIdx.x % WAVE;
  const int wv = threadIdx.x / WAVE;
  uint32_t wid = blockIdx.x * WAVES_PER_BLOCK + wv;
  uint32_t stride = gridDim.x * WAVES_PER_BLOCK;
  for (uint32_t i = wid; i < n_series; i += stride) {
    uint64_t lo = offsets[i];
    int count = (int)(offsets[i + 1] - lo);
    int64_t si = scrape_interval_wave_t<false>(ts + lo, count, 0, lane, scratch[wv]);
    if (lane == 0) out_si[i] = si;
  }
}

static VM_DEV int64_t max_prev_interval_tiers(int64_t si) {
  /* getMaxPrevInterval (rollup.go:899-919) */
  if (si <= 2000) return si + 4 * si;
  if (si <= 4000) return si + 2 * si;
  if (si <= 8000) return si + si;
  if (si <= 16000) return si + si / 2;
  if (si <= 32000) return si + si / 4;
  return si + si / 8;
}

struct SeriesWindow {
  int64_t window;
  int64_t max_prev_interval;
};

static VM_DEV SeriesWindow series_window(const KPlan& p, int64_t scrape_interval_est) {
  /* doInternal window setup (rollup.go:719-756) */
  SeriesWindow sw;
  int64_t mpi = p.step;
  if (p.start < p.end) mpi = max_prev_interval_tiers(scrape_interval_est);
  if (p.lookback_delta > 0 && mpi > p.lookback_delta) mpi = p.lookback_delta;
  if (p.min_staleness > 0 && mpi < p.min_staleness) mpi = p.min_staleness;
  int64_t window = p.window;
  if (window <= 0) {
    window = p.step;
    if (p.may_adjust && window < mpi) window = mpi;
    if (p.is_default && p.lookback_delta > 0 && window > p.lookback_delta)
      window = p.lookback_delta;
  }
  sw.window = window;
  sw.max_prev_interval = mpi;
  return sw;
}

/* --- grid-point evaluation (one lane, one grid point) -----------------
 * FUNC_CT >= 0 folds the rollup-function dispatch at compile time (the hot
 * functions get specialized kernels with small register footprints);
 * FUNC_CT == -1 is the generic runtime-dispatch fallback. */
/* Route one grid value to the per-series matrix or the grouped aggregate
 * (the eval seam of evalRollupNoIncrementalAggregate vs
 * evalRollupWithIncrementalAggregate). */
static VM_DEV void vm_emit_value(const KPlan& p, const KIO& io, uint32_t s,
                                 int g, double v) {
  if (p.aggr == VMGPU_AGGR_NONE) {
    io.out[(size_t)s * (size_t)p.n_grid + (size_t)g] = v;
    return;
  }
  int grp = io.group_ids ? io.group_ids[s] : -1;
  if (grp >= 0 && !vm_isnan(v)) {
    double* gv = io.out + (size_t)grp * (size_t)p.n_grid + (size_t)g;
    double* gc = io.out_counts + (size_t)grp * (size_t)p.n_grid + (size_t)g;
    /* counts are true contribution counts only for avg (finalize divides);
     * every other op uses them as a presence gate, where an idempotent
     * plain store of 1.0 replaces the second atomic (cross-shard merge
     * still works: the all-reduce SUM of flags stays nonzero) */
    switch (p.aggr) {
      case VMGPU_AGGR_SUM: atomicAdd(gv, v); *gc = 1.0; break;
      case VMGPU_AGGR_AVG: atomicAdd(gv, v); atomicAdd(gc, 1.0); break;
      case VMGPU_AGGR_MIN: vm_atomic_min_f64(gv, v); *gc = 1.0; break;
      case VMGPU_AGGR_MAX: vm_atomic_max_f64(gv, v); *gc = 1.0; break;
      case VMGPU_AGGR_COUNT:
      case VMGPU_AGGR_GROUP: atomicAdd(gv, 1.0); *gc = 1.0; break;
      case VMGPU_AGGR_SUM2: atomicAdd(gv, v * v); *gc = 1.0; break;
      /* geomean finalize takes pow(product, 1/count): true counts */
      case VMGPU_AGGR_GEOMEAN: vm_atomic_mul_f64(gv, v); atomicAdd(gc, 1.0); break;
      default: break;
    }
  }
}

/* 16-byte (t, v) record of the pair-interleaved LDS slab */
struct __align__(16) vm_tv {
  int64_t t;
  double v;
};

/* Fused branch-free rate/deriv_fast evaluator (rollupDerivFast,
 * rollup.go:1954-1989 + the rfa construction of doInternal:779-810 reduced
 * to the fields rate reads): six independent LDS loads + selects.
 * SENT: ts/vals point into the pipe kernel's sentinel-padded slab and
 * 0 <= i <= j <= count, so the three record indices i-1, i, j-1 lie in
 * [-1, count] and need no clamp.  Whenever one of them lands on a sentinel
 * record the selects below already discard what was read there:
 *   i == 0      record i-1 is a front sentinel; has_prev is false (i > 0)
 *   i == count  record i is a back sentinel; has_prev is false (i < count)
 *               and j == count forces n == 0, so the result is NaN
 *   j == 0      record j-1 is a front sentinel; i == 0 forces n == 0 and
 *               has_prev false, so the result is NaN
 * (the clamped form read some in-range record in these cases and discarded
 * it the same way).
 * dt32 (wave-uniform): the series spans less than 2^31 ms, so every dt whose
 * slope is used — a difference of two of its timestamps, j-1 >= i-1 — is in
 * [0, 2^31): the low words give it exactly and vm_div1e3_small() equals the
 * true division.  Discarded slopes may be garbage on either path. */
template <int STR = 1, bool SENT = false>
static VM_DEV double eval_rate_fused(const KPlan& p, const SeriesWindow& sw,
                                     const int64_t* ts, const double* vals,
                                     int count, int i, int j, int64_t t_start,
                                     bool dt32 = false) {
  int im1, ii, jm1;
  if constexpr (SENT) {
    im1 = i - 1;
    ii = i;
    jm1 = j - 1;
  } else {
    im1 = i - 1 < 0 ? 0 : i - 1;
    ii = i < count - 1 ? i : (count - 1 < 0 ? 0 : count - 1);
    jm1 = j - 1 < 0 ? 0 : j - 1;
  }
  double v_prevc, v_first, v_end;
  int64_t t_prevc, t_first, t_end_s;
  if constexpr (STR == 2) {
    /* one b128 LDS read per boundary role instead of two scattered b64s */
    const vm_tv* tv = (const vm_tv*)ts;
    vm_tv a = tv[im1], b = tv[ii], c = tv[jm1];
    t_prevc = a.t;
    v_prevc = a.v;
    t_first = b.t;
    v_first = b.v;
    t_end_s = c.t;
    v_end = c.v;
  } else {
    v_prevc = vals[im1 * STR];
    t_prevc = ts[im1 * STR];
    v_first = vals[ii * STR];
    t_first = ts[ii * STR];
    v_end = vals[jm1 * STR];
    t_end_s = ts[jm1 * STR];
  }
  int n = j - i;
  /* a NaN previous sample counts as "no previous value", as in the
   * reference, whose prevValue uses NaN for exactly that */
  bool has_prev = (i < count) && (i > 0) &&
                  (t_prevc > t_start - sw.max_prev_interval) &&
                  !vm_isnan(v_prevc);
  double pv = has_prev ? v_prevc : v_first;
  int64_t ptm = has_prev ? t_prevc : t_first;
  /* unsigned subtraction: a discarded slot may pair a sentinel timestamp
   * with a sample's, which would overflow a signed difference */
  const int64_t dt64 = (int64_t)((uint64_t)t_end_s - (uint64_t)ptm);
  double secs;
  if (dt32) {
    int32_t dt = (int32_t)((uint32_t)t_end_s - (uint32_t)ptm);
    secs = vm_div1e3_small((double)dt);
  } else {
    secs = (double)dt64 / 1e3;
  }
  double slope = (v_end - pv) / secs;
  /* has_prev ? (n == 0 ? 0 : slope) : (n <= 1 ? NaN : slope), folded into
   * one predicate and one alternative (both alternatives have a zero low
   * word, so the select is on the high word only) */
  bool use_slope = (has_prev & (n != 0)) | (n > 1);
  double alt = has_prev ? 0.0 : vm_dnan();
  return use_slope ? slope : alt;
}

template <int FUNC_CT>
static VM_DEV uint64_t eval_grid_point_ij(const KPlan& p, const SeriesWindow& sw,
                                          const int64_t* ts, const double* vals,
                                          int count, int g, uint32_t s,
                                          const KIO& io, int i, int j) {
  int64_t t_end = p.start + (int64_t)g * p.step;
  int64_t t_start = t_end - sw.window;
  VmRfa r;
  r.window = sw.window;
  r.arg = p.arg;
  r.arg2 = p.arg2;
  r.prev_value = vm_dnan();
  r.prev_timestamp = t_start - sw.max_prev_interval;
  if (i < count && i > 0 && ts[i - 1] > r.prev_timestamp) {
    r.prev_value = vals[i - 1];
    r.prev_timestamp = ts[i - 1];
  }
  r.values = vals + i;
  r.timestamps = ts + i;
  r.n = j - i;
  r.real_prev_value = vm_dnan();
  if (i > 0) {
    int64_t curr = (r.n > 0) ? ts[i] : t_start;
    if (p.lookback_delta == 0 || (curr - ts[i - 1]) < p.lookback_delta)
      r.real_prev_value = vals[i - 1];
  }
  r.real_next_value = (j < count) ? vals[j] : vm_dnan();
  r.curr_timestamp = t_end;
  double v = vm_eval_rollup_fn(FUNC_CT >= 0 ? FUNC_CT : p.func, &r);
  (void)t_start;
  vm_emit_value(p, io, s, g, v);
  return (p.sspc > 0) ? (uint64_t)p.sspc : (uint64_t)(j - i);
}

template <int FUNC_CT>
static VM_DEV uint64_t eval_grid_point(const KPlan& p, const SeriesWindow& sw,
                                       const int64_t* ts, const double* vals,
                                       int count, int g, uint32_t s,
                                       const KIO& io) {
  int64_t t_end = p.start + (int64_t)g * p.step;
  int64_t t_start = t_end - sw.window;
  int i = vm_upper_bound(ts, count, t_start);
  int j = vm_upper_bound(ts, count, t_end);
  return eval_grid_point_ij<FUNC_CT>(p, sw, ts, vals, count, g, s, io, i, j);
}

/* ------------------------------------------------------------------ */
/* kernel 1: one wave per series (n <= CHUNK_WAVE)                    */
/* ------------------------------------------------------------------ */

template <int FUNC_CT, bool PREF = false>
__global__ __launch_bounds__(BLOCK_THREADS) void rollup_wave_kernel(KPlan p, KIO io) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave_in_block = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const size_t jbuf_bytes = vm_jbuf_bytes(p.jbuf_mode, p.jbuf_elems);
  const size_t wave_bytes = vm_wave_slab_bytes(p.chunk_wave, false) + jbuf_bytes;
  int64_t* lts = (int64_t*)(smem + (size_t)wave_in_block * wave_bytes);
  double* lvs = (double*)(smem + (size_t)wave_in_block * wave_bytes +
                          (size_t)p.chunk_wave * 8);
  double* lscratch = (double*)(smem + (size_t)wave_in_block * wave_bytes +
                               (size_t)p.chunk_wave * 16);
  char* jbuf_region = smem + (size_t)wave_in_block * wave_bytes +
                      (size_t)p.chunk_wave * 16 + 256;
  /* mode-1 layout (u16 j-cache); in mode 2 the same base is re-carved by
   * the scatter path below */
  uint16_t* jbuf = (uint16_t*)jbuf_region;
  uint64_t scanned = 0;
  const uint32_t wave_id = blockIdx.x * WAVES_PER_BLOCK + wave_in_block;
  const uint32_t wave_stride = gridDim.x * WAVES_PER_BLOCK;

  /* strided (XCD-spread) series assignment */
  for (uint32_t ws = wave_id; ws < io.n_sel; ws += wave_stride) {
    uint32_t s = io.series_sel ? io.series_sel[ws] : ws;
    uint64_t lo = io.offsets[s];
    int64_t n = (int64_t)(io.offsets[s + 1] - lo);

    int count = -1;
    if (p.rcr)
      count = load_rcr_fused_wave(io.ts + lo, io.vals + lo, n, lts, lvs,
                                  p.drop_stale != 0, p.max_staleness, lane);
    if (count < 0) {
      /* no rcr, or stale NaNs present: compact first, then scan */
      count = load_compact_wave(io.ts + lo, io.vals + lo, n, lts, lvs,
                                p.drop_stale != 0, lane);
      wave_lds_sync();
      if (p.rcr) rcr_scan_wave(lts, lvs, count, p.max_staleness, lane);
    }
    wave_lds_sync();
    /* compile-time gated: the inlined preFunc body costs ~10% on the hot
     * rate path when merely PRESENT (VGPR 32 -> 44), so it lives in its
     * own instantiation */
    if constexpr (PREF) {
      if (p.pre_func) pre_func_wave(lts, lvs, count, p.pre_func, lane);
    }

    int64_t si = p.step;
#ifndef VMGPU_ABL_NO_SCRAPE
    if (p.start < p.end) {
      if (io.series_si && count == (int)n) {
        int64_t c = io.series_si[s];
        si = c > 0 ? c : p.step;
      } else {
        si = scrape_interval_wave(lts, count, p.step, lane, lscratch);
      }
    }
#endif
    SeriesWindow sw = series_window(p, si);

    if (lane == 0) scanned += (uint64_t)count;
    /* window seek: a per-series linear time->index map gives each lane a
     * density-interpolated starting guess; vm_ub_hint's bounded walk
     * resolves it (binary-search fallback keeps irregular series exact). */
    double idx_per_ms = 0.0;
    int64_t ts0 = 0;
    if (count > 1) {
      ts0 = lts[0];
      int64_t span_ms = lts[count - 1] - ts0;
      idx_per_ms = span_ms > 0 ? (double)(count - 1) / (double)span_ms : 0.0;
    }
    if constexpr (FUNC_CT == VMF_RATE || FUNC_CT == VMF_DERIV_FAST) {
      /* Both fast paths exploit i(g) = j(g-dg) when the window is a step
       * multiple (the standard rate(m[5m]) @ 15s grid): the window START
       * boundary of point g is the window END boundary of point g-dg. */
      int dg64 = (sw.window > 0 && p.step > 0 && sw.window % p.step == 0)
                     ? (int)(sw.window / p.step) : 0;
      if (p.jbuf_mode == 2 && dg64 > 0 && count <= 65534 &&
          p.n_grid + dg64 <= p.jbuf_elems) {
        /* sample-scatter boundary map (J-only): each sample computes the
         * grid range where it is the last sample <= t_end (one boundary
         * per sample — t_hi(k) = t_lo(k+1)) and scatters index+1 into J
         * over the extended range [-dg, n_grid), replacing BOTH per-point
         * seeks; eval gathers values by index as before.  Exactly ub()
         * semantics: J[g] = #samples <= t_end(g).  (A fatter variant also
         * caching (ts, value) rows in LDS measured SLOWER — the extra
         * 4.6 KB/wave of LDS cost 3 waves/SIMD of occupancy.) */
        uint16_t* Jb = (uint16_t*)jbuf_region;
        const int ext = p.n_grid + dg64;
        for (int e = lane; e < ext; e += WAVE) Jb[e] = 0;
        wave_lds_sync();
        const double inv_step = 1.0 / (double)p.step;
        for (int base = 0; base < count; base += WAVE) {
          int k = base + lane;
          bool active = k < count;
          int64_t t_k = active ? lts[k] : 0;
          int64_t t_n = (active && k + 1 < count) ? lts[k + 1] : 0;
          /* g_lo = ceil((t_k - start)/step): float estimate, exact int fixup */
          int g_lo = (int)floor((double)(t_k - p.start) * inv_step) - 1;
          g_lo += (p.start + (int64_t)g_lo * p.step < t_k);
          g_lo += (p.start + (int64_t)g_lo * p.step < t_k);
          g_lo += (p.start + (int64_t)g_lo * p.step < t_k);
          int g_hi;
          if (k + 1 < count) {
            g_hi = (int)floor((double)(t_n - p.start) * inv_step) - 1;
            g_hi += (p.start + (int64_t)g_hi * p.step < t_n);
            g_hi += (p.start + (int64_t)g_hi * p.step < t_n);
            g_hi += (p.start + (int64_t)g_hi * p.step < t_n);
          } else {
            g_hi = p.n_grid;
          }
          if (g_lo < -dg64) g_lo = -dg64;
          if (g_hi > p.n_grid) g_hi = p.n_grid;
          if (active) {
            for (int g = g_lo; g < g_hi; g++) Jb[g + dg64] = (uint16_t)(k + 1);
          }
        }
        wave_lds_sync();
        for (int g0 = 0; g0 < p.n_grid; g0 += 4 * WAVE) {
#pragma unroll
          for (int u = 0; u < 4; u++) {
            int g = g0 + u * WAVE + lane;
            if (g < p.n_grid) {
              int64_t t_end = p.start + (int64_t)g * p.step;
              int64_t t_start = t_end - sw.window;
              int j = Jb[g + dg64];
              int i = Jb[g];                     /* = J[(g-dg)+dg] */
              vm_emit_value(p, io, s, g,
                            eval_rate_fused(p, sw, lts, lvs, count, i, j, t_start));
              scanned += 2;
            }
          }
        }
        wave_lds_sync();
        continue;
      }
      if (p.jbuf_mode >= 1 &&
          (size_t)p.n_grid * 2 <= vm_jbuf_bytes(p.jbuf_mode, p.jbuf_elems) &&
          dg64 > 0 && count <= 65535) {
        for (int g = lane; g < p.n_grid; g += WAVE) {
          int64_t t_end = p.start + (int64_t)g * p.step;
          int gj = (int)((double)(t_end - ts0) * idx_per_ms) + 1;
          jbuf[g] = (uint16_t)vm_ub_hint_fast(lts, count, t_end, gj);
        }
        wave_lds_sync();
        for (int g0 = 0; g0 < p.n_grid; g0 += 4 * WAVE) {
#pragma unroll
          for (int u = 0; u < 4; u++) {
            int g = g0 + u * WAVE + lane;
            if (g < p.n_grid) {
              int64_t t_end = p.start + (int64_t)g * p.step;
              int64_t t_start = t_end - sw.window;
              int j = jbuf[g];
              int i;
              if (g >= dg64) {
                i = jbuf[g - dg64];
              } else {
                int gi = (int)((double)(t_start - ts0) * idx_per_ms) + 1;
                i = vm_ub_hint_fast(lts, count, t_start, gi);
              }
              vm_emit_value(p, io, s, g,
                            eval_rate_fused(p, sw, lts, lvs, count, i, j, t_start));
              scanned += 2;
            }
          }
        }
        wave_lds_sync();
        continue;
      }
    }
    for (int g0 = 0; g0 < p.n_grid; g0 += 4 * WAVE) {
      /* four grid points per lane per outer iteration: independent seek and
       * eval chains that the scheduler interleaves (the phases are LDS-
       * latency chains, not bandwidth-bound) */
#pragma unroll
      for (int u = 0; u < 4; u++) {
        int g = g0 + u * WAVE + lane;
        if (g < p.n_grid) {
          int64_t t_end = p.start + (int64_t)g * p.step;
          int64_t t_start = t_end - sw.window;
          int gi = (int)((double)(t_start - ts0) * idx_per_ms) + 1;
          int gj = (int)((double)(t_end - ts0) * idx_per_ms) + 1;
          int i, j;
          if constexpr (FUNC_CT == VMF_RATE || FUNC_CT == VMF_DERIV_FAST) {
            i = vm_ub_hint_fast(lts, count, t_start, gi);
            j = vm_ub_hint_fast(lts, count, t_end, gj);
          } else {
            i = vm_ub_hint(lts, count, t_start, gi);
            j = vm_ub_hint(lts, count, t_end, gj);
          }
          if constexpr (FUNC_CT == VMF_RATE || FUNC_CT == VMF_DERIV_FAST) {
            vm_emit_value(p, io, s, g,
                          eval_rate_fused(p, sw, lts, lvs, count, i, j, t_start));
            scanned += 2; /* samplesScannedPerCall for rate/deriv_fast */
          } else {
            scanned += eval_grid_point_ij<FUNC_CT>(p, sw, lts, lvs, count, g, s, io, i, j);
          }
        }
      }
    }
    wave_lds_sync();
  }
  /* reduce samplesScanned: wave shuffle + one atomic per wave */
  for (int d = 32; d > 0; d >>= 1) scanned += __shfl_down((unsigned long long)scanned, d);
  if (lane == 0 && scanned) atomicAdd(io.samples_scanned, (unsigned long long)scanned);
}

#include "pipe_kernel.h"

/* ------------------------------------------------------------------ */
/* kernel 2: one 256-thread block per series (n <= CHUNK_BLOCK)       */
/* ------------------------------------------------------------------ */

template <int FUNC_CT>
__global__ __launch_bounds__(BLOCK_THREADS) void rollup_block_kernel(KPlan p, KIO io) {
  /* ALL LDS carved from one dynamic region (no static __shared__ in front —
   * guide §6 G17: statics shift the 16-B-aligned dynamic base).
   * layout: [0,8) count (int) + si (packed), [16, 16+CB*8) ts, then vals. */
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t CB = p.chunk_block;
  int* sh_count = (int*)smem;
  int64_t* sh_si = (int64_t*)(smem + 8);
  unsigned long long* sh_sum = (unsigned long long*)(smem + 16);
  int64_t* lts = (int64_t*)(smem + 32);
  double* lvs = (double*)(smem + 32 + (size_t)CB * 8);
  double* lscratch = (double*)(smem + 32 + (size_t)CB * 16);
  int has_jbuf = 0;
  (void)vm_block_lds_bytes(CB, p.jbuf_mode, p.n_grid, &has_jbuf);
  uint16_t* jbuf = (uint16_t*)(smem + 32 + (size_t)CB * 16 + 256);
  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  uint64_t scanned = 0;

  for (uint32_t bs = blockIdx.x; bs < io.n_sel; bs += gridDim.x) {
    uint32_t s = io.series_sel[bs];
    uint64_t lo = io.offsets[s];
    int64_t n = (int64_t)(io.offsets[s + 1] - lo);

    {
      /* block-wide copy + one-pass stale detection; the wave-0 ballot
       * compaction (in place, forward) only runs when a stale NaN is
       * actually present */
      int* sh_stale = (int*)(sh_sum);  /* reuse the 8-byte scratch word */
      if (tid == 0) *sh_stale = 0;
      __syncthreads();
      int loc = 0;
      for (int64_t k = tid; k < n; k += BLOCK_THREADS) {
        int64_t t = io.ts[lo + k];
        double v = io.vals[lo + k];
        lts[k] = t;
        lvs[k] = v;
        if (p.drop_stale && vm_is_stale_nan(v)) loc = 1;
      }
      if (loc) atomicExch(sh_stale, 1);
      __syncthreads();
      if (*sh_stale) {
        if (wave == 0) {
          int c = load_compact_wave(lts, lvs, n, lts, lvs, true, lane);
          if (lane == 0) *sh_count = c;
        }
      } else if (tid == 0) {
        *sh_count = (int)n;
      }
    }
    __syncthreads();
    int count = *sh_count;
    /* the counter-reset scan only touches VALUES and the j-cache fill only
     * reads TIMESTAMPS: wave 0 scans (pair rounds — half the serial chain)
     * while waves 1-3 fill the rate j-cache concurrently */
    if constexpr (FUNC_CT == VMF_RATE || FUNC_CT == VMF_DERIV_FAST) {
      if (has_jbuf && count > 1 && count <= 65535 && wave != 0) {
        int64_t ts0f = lts[0];
        int64_t span_ms = lts[count - 1] - ts0f;
        double ipm = span_ms > 0 ? (double)(count - 1) / (double)span_ms : 0.0;
        for (int g = (wave - 1) * WAVE + lane; g < p.n_grid;
             g += (BLOCK_THREADS - WAVE)) {
          int64_t t_end = p.start + (int64_t)g * p.step;
          int gj = (int)((double)(t_end - ts0f) * ipm) + 1;
          jbuf[g] = (uint16_t)vm_ub_hint_fast(lts, count, t_end, gj);
        }
      }
    }
    if (p.rcr && wave == 0)
      rcr_scan_col_pairs<1>(lts, lvs, count, p.max_staleness, lane);
    __syncthreads();
    if (p.pre_func && wave == 0)
      pre_func_wave(lts, lvs, count, p.pre_func, lane);
    __syncthreads();
    if (wave == 0) {
      int64_t si = p.step;
      if (p.start < p.end) {
        if (io.series_si && count == (int)n) {
          int64_t c = io.series_si[s];
          si = c > 0 ? c : p.step;
        } else {
          si = scrape_interval_wave(lts, count, p.step, lane, lscratch);
        }
      }
      if (lane == 0) *sh_si = si;
    }
    __syncthreads();
    SeriesWindow sw = series_window(p, *sh_si);

    if (tid == 0) scanned += (uint64_t)count;
    if constexpr (FUNC_CT == VMF_RATE || FUNC_CT == VMF_DERIV_FAST) {
      /* shared-boundary j-cache (see the wave kernel): one seek per point,
       * i(g) = j(g - window/step) when the window is a step multiple */
      int dg64 = (sw.window > 0 && p.step > 0 && sw.window % p.step == 0)
                     ? (int)(sw.window / p.step) : 0;
      if (has_jbuf && dg64 > 0 && count <= 65535) {
        double idx_per_ms = 0.0;
        int64_t ts0 = 0;
        if (count > 1) {
          ts0 = lts[0];
          int64_t span_ms = lts[count - 1] - ts0;
          idx_per_ms = span_ms > 0 ? (double)(count - 1) / (double)span_ms : 0.0;
        }
        /* count > 1 mirrors the concurrent prefill's gate exactly: the
         * j-cache was already built by waves 1-3 during the scan */
        if (count <= 1) {
          for (int g = tid; g < p.n_grid; g += BLOCK_THREADS) {
            int64_t t_end = p.start + (int64_t)g * p.step;
            int gj = (int)((double)(t_end - ts0) * idx_per_ms) + 1;
            jbuf[g] = (uint16_t)vm_ub_hint_fast(lts, count, t_end, gj);
          }
        }
        __syncthreads();
        for (int g = tid; g < p.n_grid; g += BLOCK_THREADS) {
          int64_t t_end = p.start + (int64_t)g * p.step;
          int64_t t_start = t_end - sw.window;
          int j = jbuf[g];
          int i;
          if (g >= dg64) {
            i = jbuf[g - dg64];
          } else {
            int gi = (int)((double)(t_start - ts0) * idx_per_ms) + 1;
            i = vm_ub_hint_fast(lts, count, t_start, gi);
          }
          vm_emit_value(p, io, s, g,
                        eval_rate_fused(p, sw, lts, lvs, count, i, j, t_start));
          scanned += 2;
        }
        __syncthreads();
        continue;
      }
    }
    for (int g0 = 0; g0 < p.n_grid; g0 += BLOCK_THREADS) {
      int g = g0 + tid;
      if (g < p.n_grid) scanned += eval_grid_point<FUNC_CT>(p, sw, lts, lvs, count, g, s, io);
    }
    __syncthreads();
  }
  for (int d = 32; d > 0; d >>= 1) scanned += __shfl_down((unsigned long long)scanned, d);
  if (tid == 0) *sh_sum = 0;
  __syncthreads();
  if (lane == 0 && scanned) atomicAdd(sh_sum, (unsigned long long)scanned);
  __syncthreads();
  if (tid == 0 && *sh_sum) atomicAdd(io.samples_scanned, *sh_sum);
}

/* ------------------------------------------------------------------ */
/* kernel 3: huge series via global scratch                           */
/* ------------------------------------------------------------------ */

template <int FUNC_CT>
__global__ __launch_bounds__(BLOCK_THREADS) void rollup_huge_kernel(KPlan p, KIO io) {
  __shared__ int sh_count;
  __shared__ int sh_has_stale;
  __shared__ int64_t sh_si;
  __shared__ double sh_scratch[32];
  const int tid = threadIdx.x;
  const int lane = tid % WAVE;
  const int wave = tid / WAVE;
  uint64_t scanned = 0;

  for (uint32_t bs = blockIdx.x; bs < io.n_sel; bs += gridDim.x) {
    uint32_t s = io.series_sel[bs];
    uint64_t lo = io.offsets[s];
    int64_t n = (int64_t)(io.offsets[s + 1] - lo);
    int64_t* dts = io.scr_ts + io.scr_offsets[bs];
    double* dvs = io.scr_vals + io.scr_offsets[bs];

    const int64_t* uts;
    const double* uvs;
    if (p.drop_stale || p.rcr || p.pre_func) {
      /* block-wide copy to the global scratch + stale detection in one
       * pass (the old wave-0-only copy serialized ~n*16 B per series on
       * one wave); stale compaction (rare) falls back to an IN-PLACE
       * wave-0 forward compaction — within each tile the wave's loads all
       * precede its stores and destinations never pass sources. */
      if (tid == 0) sh_has_stale = 0;
      __syncthreads();
      int loc = 0;
      for (int64_t k = tid; k < n; k += BLOCK_THREADS) {
        int64_t t = io.ts[lo + k];
        double v = io.vals[lo + k];
        dts[k] = t;
        dvs[k] = v;
        if (p.drop_stale && vm_is_stale_nan(v)) loc = 1;
      }
      if (loc) atomicExch(&sh_has_stale, 1);
      __syncthreads();
      if (wave == 0) {
        int c = (int)n;
        if (sh_has_stale)
          c = load_compact_wave(dts, dvs, n, dts, dvs, true, lane);
        if (p.rcr) rcr_scan_col_pairs<1>(dts, dvs, c, p.max_staleness, lane);
        if (p.pre_func) pre_func_wave(dts, dvs, c, p.pre_func, lane);
        if (lane == 0) sh_count = c;
      }
      __syncthreads();
      /* wave 0's global-scratch stores must be visible to the whole block:
       * same-CU reads, but L1 is per-CU so plain loads after syncthreads are
       * coherent within the block's CU. */
      uts = dts;
      uvs = dvs;
    } else {
      if (tid == 0) sh_count = (int)n;
      __syncthreads();
      uts = io.ts + lo;
      uvs = io.vals + lo;
    }
    int count = sh_count;
    if (wave == 0) {
      int64_t si = p.step;
      if (p.start < p.end) {
        if (io.series_si && count == (int)n) {
          int64_t c = io.series_si[s];
          si = c > 0 ? c : p.step;
        } else {
          /* scrape interval needs the tail of the (possibly compacted) column */
          si = scrape_interval_wave(uts, count, p.step, lane, sh_scratch);
        }
      }
      if (lane == 0) sh_si = si;
    }
    __syncthreads();
    SeriesWindow sw = series_window(p, sh_si);

    if (tid == 0) scanned += (uint64_t)count;
    /* density-interpolated seek hints (same scheme as the wave kernel):
     * a full binary search over a 10^4-sample column costs ~15 dependent
     * global loads per boundary; the hint + bounded walk resolves in ~1 */
    double idx_per_ms = 0.0;
    int64_t ts0 = 0;
    if (count > 1) {
      ts0 = uts[0];
      int64_t span_ms = uts[count - 1] - ts0;
      idx_per_ms = span_ms > 0 ? (double)(count - 1) / (double)span_ms : 0.0;
    }
    for (int g0 = 0; g0 < p.n_grid; g0 += BLOCK_THREADS) {
      int g = g0 + tid;
      if (g < p.n_grid) {
        int64_t t_end = p.start + (int64_t)g * p.step;
        int64_t t_start = t_end - sw.window;
        int gi = (int)((double)(t_start - ts0) * idx_per_ms) + 1;
        int gj = (int)((double)(t_end - ts0) * idx_per_ms) + 1;
        int i = vm_ub_hint(uts, count, t_start, gi);
        int j = vm_ub_hint(uts, count, t_end, gj);
        if constexpr (FUNC_CT == VMF_RATE || FUNC_CT == VMF_DERIV_FAST) {
          vm_emit_value(p, io, s, g,
                        eval_rate_fused(p, sw, uts, uvs, count, i, j, t_start));
          scanned += 2;
        } else {
          scanned += eval_grid_point_ij<FUNC_CT>(p, sw, uts, uvs, count, g, s, io, i, j);
        }
      }
    }
    __syncthreads();
  }
  for (int d = 32; d > 0; d >>= 1) scanned += __shfl_down((unsigned long long)scanned, d);
  __shared__ unsigned long long block_sum;
  if (tid == 0) block_sum = 0;
  __syncthreads();
  if (lane == 0 && scanned) atomicAdd(&block_sum, (unsigned long long)scanned);
  __syncthreads();
  if (tid == 0 && block_sum) atomicAdd(io.samples_scanned, block_sum);
}

/* ------------------------------------------------------------------ */
/* aggregate identity init + finalize                                 */
/* ------------------------------------------------------------------ */

__global__ void aggr_init_kernel(double* values, double* counts, uint64_t n, int32_t aggr) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  double ident = 0.0;
  if (aggr == VMGPU_AGGR_MIN) ident = vm_dinf();
  else if (aggr == VMGPU_AGGR_MAX) ident = -vm_dinf();
  else if (aggr == VMGPU_AGGR_GEOMEAN) ident = 1.0;
  for (; i < n; i += stride) {
    values[i] = ident;
    counts[i] = 0.0;
  }
}

__global__ void aggr_finalize_kernel(double* values, double* counts, uint64_t n, int32_t aggr) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    double c = counts[i];
    switch (aggr) {
      case VMGPU_AGGR_SUM:
      case VMGPU_AGGR_MIN:
      case VMGPU_AGGR_MAX:
      case VMGPU_AGGR_SUM2:
        if (c == 0) values[i] = vm_dnan();
        break;
      case VMGPU_AGGR_AVG:
        values[i] = (c == 0) ? vm_dnan() : values[i] / c;
        break;
      case VMGPU_AGGR_COUNT:
        if (values[i] == 0) values[i] = vm_dnan();
        break;
      case VMGPU_AGGR_GROUP:
        values[i] = (values[i] == 0) ? vm_dnan() : 1.0;
        break;
      case VMGPU_AGGR_GEOMEAN:
        values[i] = (c == 0) ? vm_dnan() : pow(values[i], 1.0 / c);
        break;
      default:
        break;
    }
  }
}

/* ------------------------------------------------------------------ */
/* launch dispatch: compile-time specialization for hot funcs         */
/* ------------------------------------------------------------------ */

/* Grid of the pipe kernel.  Every wave walks the series list with a
 * grid-wide stride, so any grid from one block to one block per four series
 * computes the same thing; what the grid decides is how long each wave's
 * chain of series is.  Measured on the flagship batch (1M series, 250,000
 * blocks needed, 1280 resident; profiles/pipe_prefetch.md section 3):
 *   - exactly the resident count (one block per slot, 195 series a wave) is
 *     the SLOWEST whole-residency grid, 1.58 ms: the launch ends with the
 *     slowest CU and nothing rebalances;
 *   - more, shorter blocks let the dispatcher rebalance: 1.45 ms at 4096,
 *     1.39 ms at 8192, 1.37 ms at 16384 (grouped: 1.80 / 1.71 / 1.89);
 *   - a grid between one and two residencies (1920) is slower than either,
 *     and chains of fewer than about ten series (32768 blocks) are far
 *     slower, 2.06 ms: each block pays an un-prefetched first series.
 * Hence: whole residencies, as many as leave each wave PIPE_MIN_CHAIN
 * series, at most PIPE_MAX_BLOCKS blocks.  The resident count is queried
 * once per instantiation and LDS size.
 *
 * VMGPU_PIPE_BLOCKS=<n> overrides the grid within [1, blocks needed]; it is
 * read at every launch, so tests can put many series on one wave and one
 * library can be measured at several grids.  Anything that is not a plain
 * integer is ignored. */
#define PIPE_MIN_CHAIN 16
#define PIPE_MAX_BLOCKS 8192

template <int FUNC_CT, bool GROUPED>
static uint32_t pipe_grid_blocks(uint32_t need, size_t lds) {
  static std::mutex mu;
  static std::map<size_t, uint32_t> resident_by_lds;
  uint32_t resident = 0;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = resident_by_lds.find(lds);
    if (it != resident_by_lds.end()) {
      resident = it->second;
    } else {
      int per_cu = 0, dev = 0;
      hipDeviceProp_t prop;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
              &per_cu, rollup_pipe_kernel<FUNC_CT, GROUPED>, BLOCK_THREADS,
              lds) == hipSuccess &&
          hipGetDevice(&dev) == hipSuccess &&
          hipGetDeviceProperties(&prop, dev) == hipSuccess && per_cu > 0 &&
          prop.multiProcessorCount > 0)
        resident = (uint32_t)per_cu * (uint32_t)prop.multiProcessorCount;
      else
        resident = MAX_WAVE_BLOCKS; /* no answer: the grid used before */
      resident_by_lds[lds] = resident;
    }
  }
  const uint32_t rounds = std::max<uint32_t>(
      1, need / std::max<uint32_t>(1, resident * PIPE_MIN_CHAIN));
  uint32_t blocks = (uint32_t)std::min<uint64_t>(
      std::min<uint64_t>((uint64_t)resident * rounds, PIPE_MAX_BLOCKS), need);
  blocks = std::max<uint32_t>(blocks, 1);
  if (const char* e = getenv("VMGPU_PIPE_BLOCKS")) {
    const long long cap = std::max<uint32_t>(need, 1);
    char* end = nullptr;
    long long v = strtoll(e, &end, 10);
    if (end != e && *end == '\0')
      blocks = (uint32_t)std::min<long long>(std::max<long long>(v, 1), cap);
  }
  return blocks;
}

template <int FUNC_CT>
static void launch_rollup_t(int which, uint32_t blocks, size_t lds,
                            const KPlan& p, const KIO& w, hipStream_t stream) {
  if (which == 0) {
    /* preFunc plans take the PREF instantiation (compile-time gated, see
     * the kernel) */
    if (p.pre_func != 0)
      hipLaunchKernelGGL((rollup_wave_kernel<FUNC_CT, true>), dim3(blocks),
                         dim3(BLOCK_THREADS), lds, stream, p, w);
    else
      hipLaunchKernelGGL((rollup_wave_kernel<FUNC_CT, false>), dim3(blocks),
                         dim3(BLOCK_THREADS), lds, stream, p, w);
  } else if (which == 1) {
    hipLaunchKernelGGL(rollup_block_kernel<FUNC_CT>, dim3(blocks),
                       dim3(BLOCK_THREADS), lds, stream, p, w);
  } else if (which == 3) {
    /* software-pipelined register-staged wave variant (series <= 256
     * samples); instantiated only for the hot specializations it is
     * measured on — everything else falls back to the wave kernel */
    if constexpr (FUNC_CT == VMF_RATE || FUNC_CT == VMF_DERIV_FAST) {
      /* `blocks` is the unclamped ceil(n_wave / WAVES_PER_BLOCK) here */
      if (p.aggr != VMGPU_AGGR_NONE && w.group_ids)
        hipLaunchKernelGGL((rollup_pipe_kernel<FUNC_CT, true>),
                           dim3(pipe_grid_blocks<FUNC_CT, true>(blocks, lds)),
                           dim3(BLOCK_THREADS), lds, stream, p, w);
      else
        hipLaunchKernelGGL((rollup_pipe_kernel<FUNC_CT, false>),
                           dim3(pipe_grid_blocks<FUNC_CT, false>(blocks, lds)),
                           dim3(BLOCK_THREADS), lds, stream, p, w);
    } else {
      launch_rollup_t<FUNC_CT>(0, std::min<uint32_t>(blocks, MAX_WAVE_BLOCKS),
                               lds, p, w, stream);
    }
  } else {
    hipLaunchKernelGGL(rollup_huge_kernel<FUNC_CT>, dim3(blocks),
                       dim3(BLOCK_THREADS), lds, stream, p, w);
  }
}

static hipStream_t launch_stream();

static void launch_rollup(int which, uint32_t blocks, size_t lds,
                          const KPlan& p, const KIO& w) {
  hipStream_t s = launch_stream();
  switch (p.func) {
    case VMF_RATE: launch_rollup_t<VMF_RATE>(which, blocks, lds, p, w, s); break;
    case VMF_INCREASE: launch_rollup_t<VMF_INCREASE>(which, blocks, lds, p, w, s); break;
    case VMF_INCREASE_PURE: launch_rollup_t<VMF_INCREASE_PURE>(which, blocks, lds, p, w, s); break;
    case VMF_DELTA: launch_rollup_t<VMF_DELTA>(which, blocks, lds, p, w, s); break;
    case VMF_AVG: launch_rollup_t<VMF_AVG>(which, blocks, lds, p, w, s); break;
    case VMF_MIN: launch_rollup_t<VMF_MIN>(which, blocks, lds, p, w, s); break;
    case VMF_MAX: launch_rollup_t<VMF_MAX>(which, blocks, lds, p, w, s); break;
    case VMF_SUM: launch_rollup_t<VMF_SUM>(which, blocks, lds, p, w, s); break;
    case VMF_COUNT: launch_rollup_t<VMF_COUNT>(which, blocks, lds, p, w, s); break;
    case VMF_LAST: launch_rollup_t<VMF_LAST>(which, blocks, lds, p, w, s); break;
    case VMF_DEFAULT_ROLLUP: launch_rollup_t<VMF_DEFAULT_ROLLUP>(which, blocks, lds, p, w, s); break;
    case VMF_QUANTILE: launch_rollup_t<VMF_QUANTILE>(which, blocks, lds, p, w, s); break;
    case VMF_DERIV_FAST: launch_rollup_t<VMF_DERIV_FAST>(which, blocks, lds, p, w, s); break;
    case VMF_FIRST: launch_rollup_t<VMF_FIRST>(which, blocks, lds, p, w, s); break;
    default: launch_rollup_t<-1>(which, blocks, lds, p, w, s); break;
  }
}

/* ------------------------------------------------------------------ */
/* host side                                                          */
/* ------------------------------------------------------------------ */

namespace {

struct Batch {
  int64_t* d_ts = nullptr;
  double* d_vals = nullptr;
  uint64_t* d_offsets = nullptr;
  int32_t* d_group_ids = nullptr;
  uint32_t n_series = 0;
  uint32_t n_groups = 0;
  uint64_t n_samples = 0;
  /* series partition by length */
  int64_t* d_si = nullptr;   /* per-series scrape-interval index */
  uint32_t* d_wave_list = nullptr;
  uint32_t* d_block_list = nullptr;
  uint32_t* d_huge_list = nullptr;
  uint32_t n_wave = 0, n_block = 0, n_huge = 0;
  uint32_t max_wave_len = 0;
  uint32_t max_block_len = 0;
  bool wave_is_identity = false; /* all series small: skip the list */
  uint64_t* d_huge_scr_offsets = nullptr;
  uint64_t huge_scratch_elems = 0;
  int64_t* d_scr_ts = nullptr;
  double* d_scr_vals = nullptr;
  /* outputs of the last exec */
  double* d_out = nullptr;
  size_t out_elems = 0;
  double* d_counts = nullptr;
  size_t count_elems = 0;
  unsigned long long* d_scanned = nullptr;
  /* shape of the last exec's output */
  uint32_t last_rows = 0;
  int32_t last_grid = 0;
  /* grouped batches are physically relayouted so each group's series are
   * contiguous in HBM (locality for the grouped-run accumulation);
   * perm[i] = original series id of physical row i (empty = identity) */
  std::vector<uint32_t> perm;
  /* histogram_over_time result + scratch (hot.hip), independent of d_out */
  vm_hot_state hot;
  /* count_values_over_time result + scratch (cvot.hip) */
  vm_cvot_state cvot;
};

struct Ctx {
  std::mutex mu;
  bool inited = false;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  double last_kernel_ms = 0.0;
  std::map<uint64_t, Batch> batches;
  uint64_t next_handle = 1;
};

Ctx g_ctx;
}  // namespace

static hipStream_t launch_stream() { return g_ctx.stream; }

/* stream-ordered pool allocation (devalloc.h) */
hipError_t vm_dev_malloc_raw(void** p, size_t n) {
  return hipMallocAsync(p, n, g_ctx.stream);
}
hipError_t vm_dev_free_raw(void* p) {
  if (!p) return hipSuccess;
  return hipFreeAsync(p, g_ctx.stream);
}

hipStream_t vm_ctx_stream(void) { return g_ctx.stream; }

/* batch_access.h */
std::mutex& vm_ctx_mutex(void) { return g_ctx.mu; }
bool vm_ctx_inited(void) { return g_ctx.inited; }
int vm_batch_cols_get(uint64_t handle, vm_batch_cols* out) {
  auto it = g_ctx.batches.find(handle);
  if (it == g_ctx.batches.end()) return 1;
  Batch& b = it->second;
  out->d_ts = b.d_ts;
  out->d_vals = b.d_vals;
  out->d_offsets = b.d_offsets;
  out->n_series = b.n_series;
  out->n_samples = b.n_samples;
  out->perm = b.perm.empty() ? nullptr : b.perm.data();
  out->hot = &b.hot;
  out->cvot = &b.cvot;
  out->d_out = b.d_out;
  out->last_rows = b.last_rows;
  out->last_grid = b.last_grid;
  return 0;
}
void vm_ctx_events(hipEvent_t* ev_start, hipEvent_t* ev_stop) {
  *ev_start = g_ctx.ev_start;
  *ev_stop = g_ctx.ev_stop;
}
void vm_ctx_set_last_kernel_ms(double ms) { g_ctx.last_kernel_ms = ms; }

namespace {

/* copy series perm[i] of the source CSR into dense row i of the new CSR */
__global__ __launch_bounds__(BLOCK_THREADS) void relayout_kernel(
    const int64_t* src_ts, const double* src_vals, const uint64_t* src_off,
    const uint32_t* perm, const uint64_t* dst_off, uint32_t n_series,
    int64_t* dst_ts, double* dst_vals) {
  const int lane = threadIdx.x % WAVE;
  const int wv = threadIdx.x / WAVE;
  uint32_t wid = blockIdx.x * (BLOCK_THREADS / WAVE) + wv;
  uint32_t stride = gridDim.x * (BLOCK_THREADS / WAVE);
  for (uint32_t i = wid; i < n_series; i += stride) {
    uint32_t s = perm[i];
    uint64_t slo = src_off[s];
    uint64_t dlo = dst_off[i];
    uint64_t n = src_off[s + 1] - slo;
    for (uint64_t k = lane; k < n; k += WAVE) {
      dst_ts[dlo + k] = src_ts[slo + k];
      dst_vals[dlo + k] = src_vals[slo + k];
    }
  }
}

/* Physically reorder a grouped batch so each group's series are contiguous
 * (stable by (group, series)).  b.d_ts/d_vals must hold the ORIGINAL CSR
 * (offsets_orig); on success they point at the relayouted CSR, b.perm maps
 * physical row -> original series, new_offsets holds the physical CSR, and
 * b.d_group_ids is uploaded in physical order.  Identity permutations skip
 * all work.  Returns 0 or an error code. */
static int relayout_by_group(Batch& b, const int32_t* group_ids,
                             const uint64_t* offsets_orig, uint32_t n_series,
                             std::vector<uint64_t>& new_offsets,
                             char* errbuf, size_t errbuf_len) {
  std::vector<uint32_t> perm(n_series);
  for (uint32_t s = 0; s < n_series; s++) perm[s] = s;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t c) {
    return group_ids[a] < group_ids[c];
  });
  bool identity = true;
  for (uint32_t s = 0; s < n_series && identity; s++)
    identity = (perm[s] == s);
  new_offsets.resize(n_series + 1);
  new_offsets[0] = 0;
  for (uint32_t i = 0; i < n_series; i++)
    new_offsets[i + 1] = new_offsets[i] +
                         (offsets_orig[perm[i] + 1] - offsets_orig[perm[i]]);
  if (identity) {
    for (uint32_t i = 0; i <= n_series; i++) new_offsets[i] = offsets_orig[i];
    return 0;
  }
  uint64_t total = offsets_orig[n_series];
  VmPoolBuf<int64_t> d_ts2;
  VmPoolBuf<double> d_vals2;
  VmPoolBuf<uint64_t> d_soff, d_doff;
  VmPoolBuf<uint32_t> d_perm;
  VM_HIP_TRY(d_ts2.alloc(total * 8 + 16), "alloc relayout ts");
  VM_HIP_TRY(d_vals2.alloc(total * 8 + 16), "alloc relayout vals");
  VM_HIP_TRY(d_soff.alloc((size_t)(n_series + 1) * 8), "alloc relayout soff");
  VM_HIP_TRY(d_doff.alloc((size_t)(n_series + 1) * 8), "alloc relayout doff");
  VM_HIP_TRY(d_perm.alloc((size_t)n_series * 4), "alloc relayout perm");
  hipStream_t st = g_ctx.stream;
  VM_HIP_TRY(hipMemcpyAsync(d_soff.p, offsets_orig, (size_t)(n_series + 1) * 8,
                            hipMemcpyHostToDevice, st), "ul soff");
  VM_HIP_TRY(hipMemcpyAsync(d_doff.p, new_offsets.data(), (size_t)(n_series + 1) * 8,
                            hipMemcpyHostToDevice, st), "ul doff");
  VM_HIP_TRY(hipMemcpyAsync(d_perm.p, perm.data(), (size_t)n_series * 4,
                            hipMemcpyHostToDevice, st), "ul perm");
  uint32_t blocks = std::min<uint32_t>(
      (n_series + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 4096);
  hipLaunchKernelGGL(relayout_kernel, dim3(blocks), dim3(BLOCK_THREADS), 0, st,
                     b.d_ts, b.d_vals, d_soff.p, d_perm.p, d_doff.p, n_series,
                     d_ts2.p, d_vals2.p);
  VM_HIP_TRY(hipStreamSynchronize(st), "sync relayout");
  hipError_t kerr = hipGetLastError();
  if (kerr != hipSuccess)
    return vm_hip_err(errbuf, errbuf_len, "relayout kernel", kerr);
  (void)vm_dev_free(b.d_ts);
  (void)vm_dev_free(b.d_vals);
  b.d_ts = d_ts2.release();
  b.d_vals = d_vals2.release();
  b.perm = std::move(perm);
  return 0;
}

int build_si_index(Batch& b, char* errbuf, size_t errbuf_len) {
  VM_HIP_TRY(vm_dev_malloc(&b.d_si, (size_t)b.n_series * 8), "alloc si index");
  uint32_t blocks = std::min<uint32_t>(
      (b.n_series + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 4096);
  hipLaunchKernelGGL(si_prep_kernel, dim3(blocks), dim3(BLOCK_THREADS), 0,
                     g_ctx.stream, b.d_ts, b.d_offsets, b.n_series, b.d_si);
  VM_HIP_TRY(hipStreamSynchronize(g_ctx.stream), "sync si index");
  hipError_t kerr = hipGetLastError();
  if (kerr != hipSuccess)
    return vm_hip_err(errbuf, errbuf_len, "si index kernel", kerr);
  return 0;
}

void free_batch(Batch& b) {
  (void)vm_dev_free(b.d_ts);
  (void)vm_dev_free(b.d_vals);
  (void)vm_dev_free(b.d_offsets);
  (void)vm_dev_free(b.d_group_ids);
  (void)vm_dev_free(b.d_si);
  (void)vm_dev_free(b.d_wave_list);
  (void)vm_dev_free(b.d_block_list);
  (void)vm_dev_free(b.d_huge_list);
  (void)vm_dev_free(b.d_huge_scr_offsets);
  (void)vm_dev_free(b.d_scr_ts);
  (void)vm_dev_free(b.d_scr_vals);
  (void)vm_dev_free(b.d_out);
  (void)vm_dev_free(b.d_counts);
  (void)vm_dev_free(b.d_scanned);
  vm_hot_state_free(&b.hot);
  vm_cvot_state_free(&b.cvot);
  b = Batch();
}

/* Everything a batch needs beyond its columns.  b comes in with d_ts /
 * d_vals on the device in the caller's series order, n_series, n_groups and
 * n_samples set; offsets_orig[n_series + 1] is that CSR on the host.  A
 * failure leaves b half built: build_batch cleans up. */
int build_batch_parts(Batch& b, const uint64_t* offsets_orig,
                      const int32_t* group_ids,
                      char* errbuf, size_t errbuf_len) {
  const uint32_t n_series = b.n_series;
  /* grouped batches: physically relayout so each group's series are
   * contiguous in HBM (see relayout_by_group).  eff_* describe the
   * PHYSICAL CSR used by the kernels; offsets_orig stays as the caller
   * has it. */
  std::vector<uint64_t> phys_offsets;
  std::vector<int32_t> phys_gids;
  const uint64_t* eff_offsets = offsets_orig;
  const int32_t* eff_gids = group_ids;
  if (group_ids && b.n_groups > 0) {
    int rrc = relayout_by_group(b, group_ids, offsets_orig, n_series,
                                phys_offsets, errbuf, errbuf_len);
    if (rrc != 0) return rrc;
    eff_offsets = phys_offsets.data();
    if (!b.perm.empty()) {
      phys_gids.resize(n_series);
      for (uint32_t i = 0; i < n_series; i++)
        phys_gids[i] = group_ids[b.perm[i]];
      eff_gids = phys_gids.data();
    }
  }

  /* partition series by length (host pass over the physical offsets);
   * vmgpu_rollup_exec sizes the wave and block kernels' LDS from the two
   * maxima */
  std::vector<uint32_t> wave_list, block_list, huge_list;
  std::vector<uint64_t> huge_scr_off;
  uint64_t huge_total = 0;
  for (uint32_t s = 0; s < n_series; s++) {
    uint64_t n = eff_offsets[s + 1] - eff_offsets[s];
    if (n <= CHUNK_WAVE) {
      wave_list.push_back(s);
      if ((uint32_t)n > b.max_wave_len) b.max_wave_len = (uint32_t)n;
    } else if (n <= CHUNK_BLOCK) {
      block_list.push_back(s);
      if ((uint32_t)n > b.max_block_len) b.max_block_len = (uint32_t)n;
    } else {
      huge_list.push_back(s);
      huge_scr_off.push_back(huge_total);
      huge_total += n;
    }
  }
  b.n_wave = (uint32_t)wave_list.size();
  b.n_block = (uint32_t)block_list.size();
  b.n_huge = (uint32_t)huge_list.size();
  b.wave_is_identity = (b.n_wave == n_series);
  b.huge_scratch_elems = huge_total;

  VM_HIP_TRY(vm_dev_malloc(&b.d_offsets, (n_series + 1) * sizeof(uint64_t)), "alloc offsets");
  VM_HIP_TRY(hipMemcpy(b.d_offsets, eff_offsets, (n_series + 1) * sizeof(uint64_t), hipMemcpyHostToDevice), "upload offsets");
  if (group_ids) {
    VM_HIP_TRY(vm_dev_malloc(&b.d_group_ids, n_series * sizeof(int32_t)), "alloc gids");
    VM_HIP_TRY(hipMemcpy(b.d_group_ids, eff_gids, n_series * sizeof(int32_t), hipMemcpyHostToDevice), "upload gids");
  }
  if (!b.wave_is_identity && b.n_wave) {
    VM_HIP_TRY(vm_dev_malloc(&b.d_wave_list, b.n_wave * 4), "alloc wave list");
    VM_HIP_TRY(hipMemcpy(b.d_wave_list, wave_list.data(), b.n_wave * 4, hipMemcpyHostToDevice), "upload wave list");
  }
  if (b.n_block) {
    VM_HIP_TRY(vm_dev_malloc(&b.d_block_list, b.n_block * 4), "alloc block list");
    VM_HIP_TRY(hipMemcpy(b.d_block_list, block_list.data(), b.n_block * 4, hipMemcpyHostToDevice), "upload block list");
  }
  if (b.n_huge) {
    VM_HIP_TRY(vm_dev_malloc(&b.d_huge_list, b.n_huge * 4), "alloc huge list");
    VM_HIP_TRY(hipMemcpy(b.d_huge_list, huge_list.data(), b.n_huge * 4, hipMemcpyHostToDevice), "upload huge list");
    VM_HIP_TRY(vm_dev_malloc(&b.d_huge_scr_offsets, b.n_huge * 8), "alloc huge offsets");
    VM_HIP_TRY(hipMemcpy(b.d_huge_scr_offsets, huge_scr_off.data(), b.n_huge * 8, hipMemcpyHostToDevice), "upload huge offsets");
    VM_HIP_TRY(vm_dev_malloc(&b.d_scr_ts, huge_total * sizeof(int64_t)), "alloc scratch ts");
    VM_HIP_TRY(vm_dev_malloc(&b.d_scr_vals, huge_total * sizeof(double)), "alloc scratch vals");
  }
  VM_HIP_TRY(vm_dev_malloc(&b.d_scanned, sizeof(unsigned long long)), "alloc scanned");
  return build_si_index(b, errbuf, errbuf_len);
}

/* The one builder both create paths end in: completes b (see
 * build_batch_parts) and registers it under a new handle.  On any failure
 * the whole half-built batch is freed, the caller's columns included. */
int build_batch(Batch& b, const uint64_t* offsets_orig,
                const int32_t* group_ids, uint64_t* out_handle,
                char* errbuf, size_t errbuf_len) {
  int rc = build_batch_parts(b, offsets_orig, group_ids, errbuf, errbuf_len);
  if (rc != 0) {
    free_batch(b);
    return rc;
  }
  uint64_t h = g_ctx.next_handle++;
  g_ctx.batches[h] = b;
  *out_handle = h;
  return 0;
}

}  // namespace

extern "C" {

int vmgpu_init(const int* device_ids, int n_devices) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  if (g_ctx.inited) return 0;
  if (n_devices != 1) return 1; /* one process per GPU (RCCL scaling model) */
  int dev = device_ids ? device_ids[0] : 0;
  if (hipSetDevice(dev) != hipSuccess) return 2;
  if (hipStreamCreate(&g_ctx.stream) != hipSuccess) return 3;
  {
    /* retain freed device memory in the pool: repeat queries re-use the
     * same multi-GB carve instead of re-mapping it */
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && pool) {
      uint64_t thr = ~0ULL;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
    }
  }
  if (hipEventCreate(&g_ctx.ev_start) != hipSuccess) return 4;
  if (hipEventCreate(&g_ctx.ev_stop) != hipSuccess) return 5;
  g_ctx.device = dev;
  g_ctx.inited = true;
  return 0;
}

int vmgpu_shutdown(void) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  if (!g_ctx.inited) return 0;
  for (auto& kv : g_ctx.batches) free_batch(kv.second);
  g_ctx.batches.clear();
  vm_hot_shutdown();
  vm_aggrhist_shutdown();
  vm_aggrcv_shutdown();
  vm_aggrtopk_shutdown();
  (void)hipEventDestroy(g_ctx.ev_start);
  (void)hipEventDestroy(g_ctx.ev_stop);
  (void)hipStreamDestroy(g_ctx.stream);
  g_ctx.stream = nullptr;
  g_ctx.inited = false;
  return 0;
}

int vmgpu_batch_create(const int64_t* ts, const double* vals,
                       const uint64_t* offsets, uint32_t n_series,
                       const int32_t* group_ids, uint32_t n_groups,
                       uint64_t* out_handle,
                       char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  if (!g_ctx.inited) return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  if (!ts || !vals || !offsets || !out_handle || n_series == 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad args");
  const uint64_t n_samples = offsets[n_series];
  /* +16 B slack: the pipe kernel's clamped tail PAIR load may touch one
   * element past the last series */
  VmPoolBuf<int64_t> d_ts;
  VmPoolBuf<double> d_vals;
  VM_HIP_TRY(d_ts.alloc(n_samples * sizeof(int64_t) + 16), "alloc ts");
  VM_HIP_TRY(d_vals.alloc(n_samples * sizeof(double) + 16), "alloc vals");
  VM_HIP_TRY(hipMemcpy(d_ts.p, ts, n_samples * sizeof(int64_t), hipMemcpyHostToDevice), "upload ts");
  VM_HIP_TRY(hipMemcpy(d_vals.p, vals, n_samples * sizeof(double), hipMemcpyHostToDevice), "upload vals");

  Batch b;
  b.n_series = n_series;
  b.n_groups = n_groups;
  b.n_samples = n_samples;
  b.d_ts = d_ts.release();
  b.d_vals = d_vals.release();
  return build_batch(b, offsets, group_ids, out_handle, errbuf, errbuf_len);
}

/* decode.hip seam: decode blocks, merge+dedup, compact — device-resident */
int vmdec_decode_merge_device(
    const uint8_t* payload, uint64_t payload_len,
    const vmgpu_block_desc* blocks, uint32_t n_blocks, uint64_t total_rows,
    const uint32_t* series_block_start, uint32_t n_series,
    int64_t dedup_interval, hipStream_t st,
    int64_t** out_d_ts, double** out_d_vals, uint64_t* h_final_offsets,
    char* errbuf, size_t errbuf_len);

/* Cold-cache fetch path fused on device (SURVEY.md §8f(1)+(2) motivation):
 * compressed-block payload in, resident rollup batch out — the decoded
 * columns never cross PCIe.  out_offsets[n_series+1] reports the merged
 * CSR so the host can interpret per-series results. */
int vmgpu_batch_create_from_blocks(
    const uint8_t* payload, uint64_t payload_len,
    const vmgpu_block_desc* blocks, uint32_t n_blocks, uint64_t total_rows,
    const uint32_t* series_block_start, uint32_t n_series,
    int64_t dedup_interval, const int32_t* group_ids, uint32_t n_groups,
    uint64_t* out_handle, uint64_t* out_offsets,
    char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  if (!g_ctx.inited) return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  if (!out_handle || !out_offsets || n_series == 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad args");
  int64_t* d_ts = nullptr;
  double* d_vals = nullptr;
  int rc = vmdec_decode_merge_device(payload, payload_len, blocks, n_blocks,
                                     total_rows, series_block_start, n_series,
                                     dedup_interval, g_ctx.stream,
                                     &d_ts, &d_vals, out_offsets,
                                     errbuf, errbuf_len);
  if (rc != 0) return rc;

  Batch b;
  b.n_series = n_series;
  b.n_groups = n_groups;
  b.n_samples = out_offsets[n_series];
  b.d_ts = d_ts;
  b.d_vals = d_vals;
  /* out_offsets reported to the caller stay in ORIGINAL series order */
  return build_batch(b, out_offsets, group_ids, out_handle, errbuf, errbuf_len);
}

/* Native descriptor build from a packed block stream (vmgpu.h): the C
 * parse that the reference does in Go when unpackWorker walks its
 * []sortedBlock (netstorage.go:423-614).  The stream buffer itself is the
 * device payload — data offsets point into it, nothing is re-copied on the
 * host. */
int vmgpu_batch_create_packed(
    const uint8_t* packed, uint64_t packed_len, uint64_t n_blocks,
    const uint32_t* series_block_start, uint32_t n_series,
    int64_t dedup_interval, const int32_t* group_ids, uint32_t n_groups,
    uint64_t* out_handle, uint64_t* out_offsets,
    char* errbuf, size_t errbuf_len) {
  if (!packed || !series_block_start || !out_handle || !out_offsets ||
      n_series == 0 || n_blocks == 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad args");
  std::vector<vmgpu_block_desc> descs(n_blocks);
  uint64_t off = 0;
  uint64_t total_rows = 0;
  for (uint64_t i = 0; i < n_blocks; i++) {
    if (off + sizeof(vmgpu_packed_block_hdr) > packed_len)
      return vm_set_err(errbuf, errbuf_len, "vmgpu: packed stream truncated");
    vmgpu_packed_block_hdr h;
    memcpy(&h, packed + off, sizeof(h)); /* stream need not be aligned */
    off += sizeof(h);
    vmgpu_block_desc& d = descs[i];
    d.ts_data_off = off;
    d.ts_data_len = h.ts_data_len;
    off += h.ts_data_len;
    d.val_data_off = off;
    d.val_data_len = h.val_data_len;
    off += h.val_data_len;
    if (off > packed_len)
      return vm_set_err(errbuf, errbuf_len, "vmgpu: packed stream truncated");
    if (h.rows == 0 || h.rows > 8192)
      return vm_set_err(errbuf, errbuf_len, "vmgpu: bad packed rows");
    d.out_off = total_rows;
    d.min_timestamp = h.min_timestamp;
    d.max_timestamp = h.max_timestamp;
    d.first_value = h.first_value;
    d.scale = h.scale;
    d.e10 = (h.scale == 0)
                ? 1.0
                : pow(10.0, (double)(h.scale < 0 ? -h.scale : h.scale));
    d.rows = h.rows;
    d.ts_mt = h.ts_mt;
    d.val_mt = h.val_mt;
    d.precision_bits = h.precision_bits;
    d._pad = 0;
    total_rows += h.rows;
  }
  return vmgpu_batch_create_from_blocks(
      packed, packed_len, descs.data(), (uint32_t)n_blocks, total_rows,
      series_block_start, n_series, dedup_interval, group_ids, n_groups,
      out_handle, out_offsets, errbuf, errbuf_len);
}

/* Pinned host memory for PCIe-rate payload/result staging (the cgo
 * production layer would hold these in a pool, like netstorage's
 * result buffer pools). */
int vmgpu_host_alloc(uint64_t nbytes, void** out_ptr) {
  if (!out_ptr || nbytes == 0) return 1;
  *out_ptr = nullptr;
  return hipHostMalloc(out_ptr, nbytes, hipHostMallocDefault) == hipSuccess
             ? 0 : 2;
}

int vmgpu_host_free(void* ptr) {
  return hipHostFree(ptr) == hipSuccess ? 0 : 1;
}

/* Physical-row -> original-series mapping of a (relayouted) grouped batch:
 * out_perm[n_series].  Identity batches fill 0..n-1.  Callers need this to
 * place per-series outputs of vmgpu_rollup_exec back in request order. */
int vmgpu_batch_perm(uint64_t handle, uint32_t* out_perm) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  auto it = g_ctx.batches.find(handle);
  if (it == g_ctx.batches.end() || !out_perm) return 1;
  const Batch& b = it->second;
  if (b.perm.empty()) {
    for (uint32_t i = 0; i < b.n_series; i++) out_perm[i] = i;
  } else {
    for (uint32_t i = 0; i < b.n_series; i++) out_perm[i] = b.perm[i];
  }
  return 0;
}

int vmgpu_batch_destroy(uint64_t handle) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  auto it = g_ctx.batches.find(handle);
  if (it == g_ctx.batches.end()) return 1;
  free_batch(it->second);
  g_ctx.batches.erase(it);
  return 0;
}

int vmgpu_rollup_exec(const vmgpu_plan* plan, uint64_t handle,
                      double* out, double* out_counts,
                      uint64_t* out_samples_scanned,
                      char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  if (!g_ctx.inited) return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  auto it = g_ctx.batches.find(handle);
  if (it == g_ctx.batches.end()) return vm_set_err(errbuf, errbuf_len, "vmgpu: bad handle");
  Batch& b = it->second;
  if (plan->step <= 0 || plan->start > plan->end)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad grid");
  int64_t n_grid64 = 1 + (plan->end - plan->start) / plan->step;
  if (n_grid64 > (int64_t)1 << 30)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: grid too large");
  int32_t n_grid = (int32_t)n_grid64;
  bool grouped = plan->aggr != VMGPU_AGGR_NONE;
  if (grouped && (!b.d_group_ids || b.n_groups == 0))
    return vm_set_err(errbuf, errbuf_len, "vmgpu: aggr plan needs group_ids");

  size_t out_elems = grouped ? (size_t)b.n_groups * n_grid
                             : (size_t)b.n_series * n_grid;
  size_t count_elems = grouped ? out_elems : 0;
  if (b.out_elems < out_elems) {
    (void)vm_dev_free(b.d_out);
    b.d_out = nullptr;
    VM_HIP_TRY(vm_dev_malloc(&b.d_out, out_elems * sizeof(double)), "alloc out");
    b.out_elems = out_elems;
  }
  if (count_elems && b.count_elems < count_elems) {
    (void)vm_dev_free(b.d_counts);
    b.d_counts = nullptr;
    VM_HIP_TRY(vm_dev_malloc(&b.d_counts, count_elems * sizeof(double)), "alloc counts");
    b.count_elems = count_elems;
  }
  VM_HIP_TRY(hipMemsetAsync(b.d_scanned, 0, 8, g_ctx.stream), "zero scanned");

  KPlan p;
  p.start = plan->start;
  p.end = plan->end;
  p.step = plan->step;
  p.window = plan->window;
  p.lookback_delta = plan->lookback_delta;
  p.min_staleness = plan->min_staleness_interval;
  p.max_staleness = plan->max_staleness_interval;
  p.n_grid = n_grid;
  p.func = plan->func;
  p.aggr = plan->aggr;
  p.sspc = plan->samples_scanned_per_call;
  p.may_adjust = plan->may_adjust_window;
  p.is_default = plan->is_default_rollup;
  p.rcr = plan->remove_counter_resets;
  p.drop_stale = plan->drop_stale_nans;
  p.pre_func = plan->pre_func;
  p.chunk_wave = (int32_t)std::min<uint32_t>(
      CHUNK_WAVE, std::max<uint32_t>(64, (b.max_wave_len + 63) & ~63u));
  p.chunk_block = (int32_t)std::min<uint32_t>(
      CHUNK_BLOCK, std::max<uint32_t>(64, (b.max_block_len + 63) & ~63u));
  /* rate boundary caches (see the wave kernel): the u16 j-cache
   * (shared-boundary path) is the measured default — both scatter
   * variants benched SLOWER at config 2 (full Et/Ev/J: 3.27 ms from LDS
   * occupancy loss; J-only scatter: 2.77 ms from the boundary-fixup +
   * divergent write cost) vs 2.51 ms for the j-cache.  Mode 2 remains
   * selectable for grids too large for the u16 cache. */
  /* The pipelined kernel fills a u16 j-cache by probing and reads any jbuf
   * of at least n_grid entries that way, whichever mode sized it; mode 2
   * as a sample-scatter map is the wave kernel's alone. */
  bool use_pipe = false;
  if ((plan->func == VMF_RATE || plan->func == VMF_DERIV_FAST) && b.n_wave &&
      b.max_wave_len <= (uint32_t)(PIPE_PCHUNKS * 2 * WAVE) &&
      plan->pre_func == 0 &&
      plan->window > 0 && plan->step > 0 && plan->window % plan->step == 0 &&
      n_grid > 1) {
    static int pipe_disabled = -1;
    if (pipe_disabled < 0) {
      const char* e = getenv("VMGPU_DISABLE_PIPE");
      pipe_disabled = (e && e[0] == '1') ? 1 : 0;
    }
    use_pipe = !pipe_disabled;
  }
  p.jbuf_elems = 0;
  p.jbuf_mode = 0;
  if ((plan->func == VMF_RATE || plan->func == VMF_DERIV_FAST) && n_grid > 1) {
    /* per-wave slab incl. the pipe kernel's sentinel records when that
     * kernel is the candidate (it stays the candidate only if a jbuf fits) */
    size_t base = (size_t)WAVES_PER_BLOCK *
                  vm_wave_slab_bytes(p.chunk_wave, use_pipe);
    int64_t dgp = (plan->window > 0 && plan->step > 0 &&
                   plan->window % plan->step == 0)
                      ? plan->window / plan->step : 0;
    if (n_grid <= 4096 &&
        base + WAVES_PER_BLOCK * vm_jbuf_bytes(1, n_grid) <= 64 * 1024) {
      p.jbuf_mode = 1;
      p.jbuf_elems = n_grid;
    } else if (dgp > 0 && n_grid + dgp <= 32000) {
      int32_t elems = (int32_t)(n_grid + dgp);
      if (base + WAVES_PER_BLOCK * vm_jbuf_bytes(2, elems) <= 64 * 1024) {
        p.jbuf_mode = 2;
        p.jbuf_elems = elems;
      }
    }
  }
  /* the pipe kernel carries only the j-cache rate path */
  if (p.jbuf_mode == 0) use_pipe = false;
  p.arg = plan->arg;
  p.arg2 = plan->arg2;

  KIO io;
  io.ts = b.d_ts;
  io.vals = b.d_vals;
  io.offsets = b.d_offsets;
  io.group_ids = b.d_group_ids;
  io.series_si = b.d_si;
  io.out = b.d_out;
  io.out_counts = b.d_counts;
  io.samples_scanned = b.d_scanned;
  io.scr_ts = b.d_scr_ts;
  io.scr_vals = b.d_scr_vals;
  io.scr_offsets = b.d_huge_scr_offsets;

  if (grouped) {
    uint64_t n = out_elems;
    int blocks = (int)std::min<uint64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(aggr_init_kernel, dim3(blocks), dim3(256), 0, g_ctx.stream,
                       b.d_out, b.d_counts, n, plan->aggr);
  }

  VM_HIP_TRY(hipEventRecord(g_ctx.ev_start, g_ctx.stream), "event start");

  /* compile-time specializations for the hot functions (see launch_rollup) */
  if (b.n_wave) {
    KIO w = io;
    w.series_sel = b.wave_is_identity ? nullptr : b.d_wave_list;
    w.n_sel = b.n_wave;
    uint32_t need = (b.n_wave + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    uint32_t blocks = std::min<uint32_t>(need, MAX_WAVE_BLOCKS);
    size_t lds = (size_t)WAVES_PER_BLOCK *
                 (vm_wave_slab_bytes(p.chunk_wave, use_pipe) +
                  vm_jbuf_bytes(p.jbuf_mode, p.jbuf_elems));
    /* software-pipelined register-staged variant for short series (the
     * config-2 flagship shape); VMGPU_DISABLE_PIPE=1 A/Bs the wave kernel.
     * The pipe launch sizes its own grid from the blocks needed
     * (pipe_grid_blocks); VMGPU_PIPE_BLOCKS=<n> overrides that grid, read
     * at every exec. */
    launch_rollup(use_pipe ? 3 : 0, use_pipe ? need : blocks, lds, p, w);
  }
  if (b.n_block) {
    KIO w = io;
    w.series_sel = b.d_block_list;
    w.n_sel = b.n_block;
    uint32_t blocks = std::min<uint32_t>(b.n_block, 2048);
    size_t lds = vm_block_lds_bytes(p.chunk_block, p.jbuf_mode, p.n_grid,
                                    nullptr);
    launch_rollup(1, blocks, lds, p, w);
  }
  if (b.n_huge) {
    KIO w = io;
    w.series_sel = b.d_huge_list;
    w.n_sel = b.n_huge;
    uint32_t blocks = std::min<uint32_t>(b.n_huge, 2048);
    launch_rollup(2, blocks, 0, p, w);
  }

  VM_HIP_TRY(hipEventRecord(g_ctx.ev_stop, g_ctx.stream), "event stop");

  if (grouped && !plan->skip_finalize) {
    uint64_t n = out_elems;
    int blocks = (int)std::min<uint64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(aggr_finalize_kernel, dim3(blocks), dim3(256), 0, g_ctx.stream,
                       b.d_out, b.d_counts, n, plan->aggr);
  }

  if (out) {
    VM_HIP_TRY(hipMemcpyAsync(out, b.d_out, out_elems * sizeof(double),
                           hipMemcpyDeviceToHost, g_ctx.stream), "download out");
  }
  if (out_counts && count_elems) {
    VM_HIP_TRY(hipMemcpyAsync(out_counts, b.d_counts, count_elems * sizeof(double),
                           hipMemcpyDeviceToHost, g_ctx.stream), "download counts");
  }
  unsigned long long scanned_h = 0;
  VM_HIP_TRY(hipMemcpyAsync(&scanned_h, b.d_scanned, 8, hipMemcpyDeviceToHost, g_ctx.stream),
          "download scanned");
  VM_HIP_TRY(hipStreamSynchronize(g_ctx.stream), "sync");
  hipError_t kerr = hipGetLastError();
  if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "kernel", kerr);

  float ms = 0;
  VM_HIP_TRY(hipEventElapsedTime(&ms, g_ctx.ev_start, g_ctx.ev_stop), "event elapsed");
  g_ctx.last_kernel_ms = (double)ms;

  if (out_samples_scanned) *out_samples_scanned = (uint64_t)scanned_h;
  b.last_rows = grouped ? b.n_groups : b.n_series;
  b.last_grid = n_grid;
  return 0;
}

int vmgpu_batch_fetch_out(uint64_t handle, double* dst, size_t n_elems,
                          double* dst_counts, size_t n_count_elems) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  auto it = g_ctx.batches.find(handle);
  if (it == g_ctx.batches.end()) return 1;
  Batch& b = it->second;
  if (dst && n_elems) {
    if (n_elems > b.out_elems) return 2;
    if (hipMemcpy(dst, b.d_out, n_elems * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return 3;
  }
  if (dst_counts && n_count_elems) {
    if (n_count_elems > b.count_elems) return 4;
    if (hipMemcpy(dst_counts, b.d_counts, n_count_elems * sizeof(double),
                  hipMemcpyDeviceToHost) != hipSuccess)
      return 5;
  }
  return 0;
}

void vmgpu_aggr_finalize_host(int32_t aggr, double* values, double* counts,
                              uint64_t n_elems) {
  const double dnan = __builtin_nan("");
  for (uint64_t i = 0; i < n_elems; i++) {
    double c = counts ? counts[i] : 0.0;
    switch (aggr) {
      case VMGPU_AGGR_SUM:
      case VMGPU_AGGR_MIN:
      case VMGPU_AGGR_MAX:
      case VMGPU_AGGR_SUM2:
        if (c == 0) values[i] = dnan;
        break;
      case VMGPU_AGGR_AVG:
        values[i] = (c == 0) ? dnan : values[i] / c;
        break;
      case VMGPU_AGGR_COUNT:
        if (values[i] == 0) values[i] = dnan;
        break;
      case VMGPU_AGGR_GROUP:
        values[i] = (values[i] == 0) ? dnan : 1.0;
        break;
      case VMGPU_AGGR_GEOMEAN:
        values[i] = (c == 0) ? dnan : pow(values[i], 1.0 / c);
        break;
      default:
        break;
    }
  }
}

int vmgpu_rollup_eval(const vmgpu_plan* plan,
                      const int64_t* ts, const double* vals,
                      const uint64_t* offsets, uint32_t n_series,
                      const int32_t* group_ids, uint32_t n_groups,
                      double* out, double* out_counts,
                      uint64_t* out_samples_scanned,
                      char* errbuf, size_t errbuf_len) {
  uint64_t h = 0;
  int rc = vmgpu_batch_create(ts, vals, offsets, n_series, group_ids, n_groups,
                              &h, errbuf, errbuf_len);
  if (rc) return rc;
  rc = vmgpu_rollup_exec(plan, h, out, out_counts, out_samples_scanned,
                         errbuf, errbuf_len);
  vmgpu_batch_destroy(h);
  return rc;
}

int vmgpu_last_kernel_ms(double* out_ms) {
  std::lock_guard<std::mutex> lock(g_ctx.mu);
  if (!g_ctx.inited) return 1;
  *out_ms = g_ctx.last_kernel_ms;
  return 0;
}

int vmgpu_device_info(char* name, size_t name_len, double* hbm_gib, int* cu_count) {
  hipDeviceProp_t prop;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 1;
  if (name && name_len) snprintf(name, name_len, "%s", prop.name);
  if (hbm_gib) *hbm_gib = (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0);
  if (cu_count) *cu_count = prop.multiProcessorCount;
  return 0;
}

}  /* extern "C" */
