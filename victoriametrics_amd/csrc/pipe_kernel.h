/* pipe_kernel.h — rollup_pipe_kernel, its pair scan and its staging helpers.
 * Not a stand-alone header: vmgpu.hip includes it between the wave and the
 * block kernel, behind the shared device helpers it uses. */

/* ------------------------------------------------------------------ */
/* kernel 1b: software-pipelined register-staged wave kernel          */
/*                                                                    */
/* The wave kernel above is instruction-ISSUE/latency bound, not HBM  */
/* bound (profiles/round1_final.md §5: FETCH/WRITE ≈ algorithmic but  */
/* ACTIVE_INST_ANY ≈ 30% at 7 waves/SIMD).  This variant restructures */
/* the per-series phases so the memory system never drains:           */
/*   - the series' columns are loaded straight into REGISTERS as      */
/*     pairs: lane l holds samples (2l, 2l+1) of each 128-sample      */
/*     chunk, one b128 load per column per chunk, PIPE_PCHUNKS chunks */
/*     in flight at once,                                             */
/*   - the removeCounterResets scan consumes those registers while    */
/*     writing the corrected pair-interleaved slab to LDS (no LDS     */
/*     re-read pass),                                                 */
/*   - the NEXT series' loads are issued as soon as the registers die,*/
/*     overlapping scrape/seek/eval/emit of the current series; they  */
/*     are inline asm, so the compiler inserts no wait for them, and  */
/*     the one hand-placed wait sits at the top of the next iteration,*/
/*   - the per-series descriptors are scalar loads issued two series  */
/*     ahead (pipe_desc_read),                                        */
/*   - every phase barrier is lgkm-only (wave_ds_sync), so the        */
/*     prefetched loads stay outstanding across the whole evaluation  */
/*     and the back edge.                                             */
/* Results are bit-identical to the wave kernel: same scan, same      */
/* j-cache seeks, same evaluators.                                    */
/* ------------------------------------------------------------------ */

#define PIPE_PCHUNKS 2 /* pair chunks: 2 x 128 samples = 256 cap */

/* Pair-rounds removeCounterResets over an LDS/global COLUMN (stride STR
 * in int64 units): the rcr_scan_pairs logic with per-round pair loads
 * instead of register sources — 128 samples per round instead of 64, so
 * the serial-round chain halves.  Bit-exact with rcr_scan_wave (same
 * element-order event walk, same segmented-max clamp). */
template <int STR = 1>
static __device__ void rcr_scan_col_pairs(int64_t* d_ts, double* d_vals,
                                          int count, int64_t msi, int lane) {
  double corr = 0.0;
  double prev_raw = 0.0;
  int64_t prev_ts = 0;
  double prev_fin = 0.0;
  for (int base = 0; base < count; base += 2 * WAVE) {
    int k0 = base + 2 * lane;
    int k1 = k0 + 1;
    bool a0 = k0 < count;
    bool a1 = k1 < count;
    double v0 = a0 ? d_vals[k0 * STR] : 0.0;
    double v1 = a1 ? d_vals[k1 * STR] : 0.0;
    int64_t t0 = a0 ? d_ts[k0 * STR] : 0;
    int64_t t1 = a1 ? d_ts[k1 * STR] : 0;
    int rem = count - base;
    if (rem > 2 * WAVE) rem = 2 * WAVE;
    int lastl = (rem - 1) >> 1;
    bool last_is_e1 = ((rem - 1) & 1) != 0;
    double pv0 = __shfl_up(v1, 1);
    int64_t pt0 = __shfl_up(t1, 1);
    if (lane == 0) { pv0 = prev_raw; pt0 = prev_ts; }
    bool isfirst0 = (k0 == 0);
    double d0 = v0 - pv0;
    double d1 = v1 - v0;
    double inc0 = 0.0, inc1 = 0.0;
    if (!isfirst0 && d0 < 0) inc0 = ((-d0 * 8) < pv0) ? (pv0 - v0) : pv0;
    if (d1 < 0) inc1 = ((-d1 * 8) < v0) ? (v0 - v1) : v0;
    bool gap0 = (!isfirst0 && msi > 0 && (t0 - pt0) > msi);
    bool gap1 = (msi > 0 && (t1 - t0) > msi);
    bool evt0 = a0 && (gap0 || inc0 != 0.0);
    bool evt1 = a1 && (gap1 || inc1 != 0.0);
    uint64_t em = __ballot(evt0 || evt1);
    uint64_t dm = __ballot((a0 && !isfirst0 && d0 < 0) || (a1 && d1 < 0));
    if (em == 0 && dm == 0 &&
        (base == 0 || __shfl(v0, 0) + corr >= prev_fin)) {
      if (corr != 0.0) {
        if (a0) d_vals[k0 * STR] = v0 + corr;
        if (a1) d_vals[k1 * STR] = v1 + corr;
      }
      double lv = last_is_e1 ? v1 : v0;
      int64_t lt = last_is_e1 ? t1 : t0;
      prev_raw = __shfl(lv, lastl);
      prev_ts = __shfl(lt, lastl);
      prev_fin = prev_raw + corr;
      continue;
    }
    double cc = corr;
    double mc0 = corr, mc1 = corr;
    uint64_t w = em;
    while (w) {
      int b = __ffsll((unsigned long long)w) - 1;
      w &= w - 1;
      double i0b = __shfl(inc0, b);
      double i1b = __shfl(inc1, b);
      int fl = __shfl((int)gap0 | ((int)gap1 << 1) | ((int)evt0 << 2) |
                          ((int)evt1 << 3), b);
      if (fl & 4) {
        double cn = (fl & 1) ? 0.0 : (cc + i0b);
        if (lane >= b) { mc0 = cn; mc1 = cn; }
        cc = cn;
      }
      if (fl & 8) {
        double cn = (fl & 2) ? 0.0 : (cc + i1b);
        if (lane > b) mc0 = cn;
        if (lane >= b) mc1 = cn;
        cc = cn;
      }
    }
    double fin0 = v0 + mc0;
    double fin1 = v1 + mc1;
    /* a NaN element keeps its value and restarts the running max, as the
     * reference's `values[i] < values[i-1]` test does on either side of it */
    bool f0 = isfirst0 || gap0 || vm_isnan(fin0);
    bool f1 = gap1 || vm_isnan(fin1);
    double x0 = fin0, x1 = fin1;
    /* clamp shortcut (vm_clamp_violates): one neighbour shuffle + ballot;
     * elements past the series end sit above every active one and feed
     * nothing that is stored or carried, so they are left out */
    double pf0 = __shfl_up(fin1, 1);
    if (lane == 0) pf0 = prev_fin;
    const bool clamp_needed =
        __ballot((a0 && !f0 && vm_clamp_violates(fin0, pf0)) ||
                 (a1 && !f1 && vm_clamp_violates(fin1, fin0))) != 0;
    if (clamp_needed) {
      if (lane == 0 && !f0) x0 = fmax(x0, prev_fin);
      double pm = f1 ? x1 : fmax(x0, x1);
      int pf = (f0 || f1) ? 1 : 0;
      for (int dlt = 1; dlt < WAVE; dlt <<= 1) {
        double pmo = __shfl_up(pm, dlt);
        int pfo = __shfl_up(pf, dlt);
        if (lane >= dlt) {
          if (!pf) pm = fmax(pm, pmo);
          pf |= pfo;
        }
      }
      double inc_m = __shfl_up(pm, 1);
      if (lane > 0 && !f0) x0 = fmax(x0, inc_m);
      if (!f1) x1 = fmax(x1, x0);
    }
    if (a0) d_vals[k0 * STR] = x0;
    if (a1) d_vals[k1 * STR] = x1;
    corr = cc;
    {
      double lvr = last_is_e1 ? v1 : v0;
      int64_t ltr = last_is_e1 ? t1 : t0;
      double lxf = last_is_e1 ? x1 : x0;
      prev_raw = __shfl(lvr, lastl);
      prev_ts = __shfl(ltr, lastl);
      prev_fin = __shfl(lxf, lastl);
    }
  }
}

/* Pair-register removeCounterResets: lane l holds samples (2l, 2l+1) of
 * each 128-sample chunk (ONE b128 global load per column per chunk).
 * Exactly the rcr_scan_wave semantics (rollup.go:921-958): the running
 * correction visits the (rare) event ELEMENTS in index order bitwise, and
 * the monotonic clamp is the same segmented prefix max, evaluated as
 * in-lane pair combines + the cross-lane scan (fmax is exactly
 * associative).  Writes the pair-interleaved LDS slab; returns n, or -1
 * when a stale NaN must be compacted out (caller falls back to the global
 * compact path). */
static VM_DEV int rcr_scan_pairs(const int64_t* t0a, const int64_t* t1a,
                                 const double* v0a, const double* v1a,
                                 int64_t n, int64_t* d_ts, double* d_vals,
                                 bool drop_stale, int64_t msi, int lane) {
  double corr = 0.0;
  double prev_raw = 0.0;
  int64_t prev_ts = 0;
  double prev_fin = 0.0;
#pragma unroll
  for (int c = 0; c < PIPE_PCHUNKS; c++) {
    int64_t base = (int64_t)c * 2 * WAVE;
    if (base >= n) continue;
    int64_t k0 = base + 2 * lane;
    int64_t k1 = k0 + 1;
    bool a0 = k0 < n;
    bool a1 = k1 < n;
    double v0 = a0 ? v0a[c] : 0.0;
    double v1 = a1 ? v1a[c] : 0.0;
    int64_t t0 = a0 ? t0a[c] : 0;
    int64_t t1 = a1 ? t1a[c] : 0;
    if (drop_stale &&
        __ballot((a0 && vm_is_stale_nan(v0)) ||
                 (a1 && vm_is_stale_nan(v1))) != 0)
      return -1;
    if (a0) d_ts[k0 * 2] = t0;
    if (a1) d_ts[k1 * 2] = t1;
    int rem = (int)(n - base);
    if (rem > 2 * WAVE) rem = 2 * WAVE;
    int lastl = (rem - 1) >> 1;
    bool last_is_e1 = ((rem - 1) & 1) != 0;
    /* previous element: elem0's is the neighbor lane's elem1; elem1's is
     * the in-lane elem0 (no cross-lane op) */
    double pv0 = __shfl_up(v1, 1);
    int64_t pt0 = __shfl_up(t1, 1);
    if (lane == 0) { pv0 = prev_raw; pt0 = prev_ts; }
    bool isfirst0 = (k0 == 0);
    double d0 = v0 - pv0;
    double d1 = v1 - v0;
    double inc0 = 0.0, inc1 = 0.0;
    if (!isfirst0 && d0 < 0) inc0 = ((-d0 * 8) < pv0) ? (pv0 - v0) : pv0;
    if (d1 < 0) inc1 = ((-d1 * 8) < v0) ? (v0 - v1) : v0;
    bool gap0 = (!isfirst0 && msi > 0 && (t0 - pt0) > msi);
    bool gap1 = (msi > 0 && (t1 - t0) > msi);
    bool evt0 = a0 && (gap0 || inc0 != 0.0);
    bool evt1 = a1 && (gap1 || inc1 != 0.0);
    uint64_t em = __ballot(evt0 || evt1);
    uint64_t dm = __ballot((a0 && !isfirst0 && d0 < 0) || (a1 && d1 < 0));
    if (em == 0 && dm == 0 &&
        (base == 0 || __shfl(v0, 0) + corr >= prev_fin)) {
      if (a0) d_vals[k0 * 2] = v0 + corr;
      if (a1) d_vals[k1 * 2] = v1 + corr;
      double lv = last_is_e1 ? v1 : v0;
      int64_t lt = last_is_e1 ? t1 : t0;
      prev_raw = __shfl(lv, lastl);
      prev_ts = __shfl(lt, lastl);
      prev_fin = prev_raw + corr;
      continue;
    }
    /* correction walk in exact element order (elem0 of lane b, then its
     * elem1) — identical serial sum to the reference */
    double cc = corr;
    double mc0 = corr, mc1 = corr;
    uint64_t w = em;
    while (w) {
      int b = __ffsll((unsigned long long)w) - 1;
      w &= w - 1;
      double i0b = __shfl(inc0, b);
      double i1b = __shfl(inc1, b);
      int fl = __shfl((int)gap0 | ((int)gap1 << 1) | ((int)evt0 << 2) |
                          ((int)evt1 << 3), b);
      if (fl & 4) { /* event at element 0 of lane b: applies to k >= 2b */
        double cn = (fl & 1) ? 0.0 : (cc + i0b);
        if (lane >= b) { mc0 = cn; mc1 = cn; }
        cc = cn;
      }
      if (fl & 8) { /* event at element 1 of lane b: applies to k >= 2b+1 */
        double cn = (fl & 2) ? 0.0 : (cc + i1b);
        if (lane > b) mc0 = cn;
        if (lane >= b) mc1 = cn;
        cc = cn;
      }
    }
    double fin0 = v0 + mc0;
    double fin1 = v1 + mc1;
    /* monotonic clamp = segmented prefix max; boundary elements (series
     * start / staleness gaps) keep their value and start a new segment */
    /* a NaN element keeps its value and restarts the running max, as the
     * reference's `values[i] < values[i-1]` test does on either side of it */
    bool f0 = isfirst0 || gap0 || vm_isnan(fin0);
    bool f1 = gap1 || vm_isnan(fin1);
    double x0 = fin0, x1 = fin1;
    /* clamp shortcut (vm_clamp_violates): one neighbour shuffle + ballot;
     * elements past the series end sit above every active one and feed
     * nothing that is stored or carried, so they are left out */
    double pf0 = __shfl_up(fin1, 1);
    if (lane == 0) pf0 = prev_fin;
    const bool clamp_needed =
        __ballot((a0 && !f0 && vm_clamp_violates(fin0, pf0)) ||
                 (a1 && !f1 && vm_clamp_violates(fin1, fin0))) != 0;
    if (clamp_needed) {
      if (lane == 0 && !f0) x0 = fmax(x0, prev_fin);
      double pm = f1 ? x1 : fmax(x0, x1);
      int pf = (f0 || f1) ? 1 : 0;
      for (int dlt = 1; dlt < WAVE; dlt <<= 1) {
        double pmo = __shfl_up(pm, dlt);
        int pfo = __shfl_up(pf, dlt);
        if (lane >= dlt) {
          if (!pf) pm = fmax(pm, pmo);
          pf |= pfo;
        }
      }
      double inc_m = __shfl_up(pm, 1); /* exclusive incoming (lane 0 unused) */
      if (lane > 0 && !f0) x0 = fmax(x0, inc_m);
      if (!f1) x1 = fmax(x1, x0);
    }
    if (a0) d_vals[k0 * 2] = x0;
    if (a1) d_vals[k1 * 2] = x1;
    corr = cc;
    {
      double lvr = last_is_e1 ? v1 : v0;
      int64_t ltr = last_is_e1 ? t1 : t0;
      double lxf = last_is_e1 ? x1 : x0;
      prev_raw = __shfl(lvr, lastl);
      prev_ts = __shfl(ltr, lastl);
      prev_fin = __shfl(lxf, lastl);
    }
  }
  return (int)n;
}

/* Per-series descriptor of the pipe kernel's series loop: the series index,
 * its sample range and its precomputed scrape interval.  All wave-uniform. */
struct PipeDesc {
  uint32_t s;
  uint64_t lo, hi; /* samples [lo, hi); the count is taken at the point of
                      use so that nothing waits for the loads when issued */
  int64_t si_raw;
  int32_t grp;     /* grouped instantiation only; -1 = no group */
  __device__ int64_t n() const { return (int64_t)(hi - lo); }
};

/* The selection list, the offsets, the scrape intervals and the group ids
 * are never written while a rollup kernel runs, so they may be read through
 * the constant address space: the compiler then emits scalar loads even after
 * the kernel's first store (it cannot prove that the output rows do not
 * alias a plain global pointer, and falls back to vector loads with a
 * vmcnt wait).  Callers pass wave-uniform indices only. */
#define VM_PIPE_RO __attribute__((address_space(4)))

static VM_DEV uint32_t pipe_sel(const KIO& io, uint32_t w) {
  if (!io.series_sel) return w;
  return __builtin_amdgcn_readfirstlane(
      ((const VM_PIPE_RO uint32_t*)io.series_sel)[w]);
}

template <bool GROUPED>
static VM_DEV void pipe_desc_read(const KIO& io, uint32_t s, PipeDesc& d) {
  const VM_PIPE_RO uint64_t* off = (const VM_PIPE_RO uint64_t*)io.offsets;
  d.s = s;
  d.lo = off[s];
  d.hi = off[s + 1];
  d.si_raw = io.series_si ? ((const VM_PIPE_RO int64_t*)io.series_si)[s] : 0;
  d.grp = -1;
  if constexpr (GROUPED) {
    if (io.group_ids) d.grp = ((const VM_PIPE_RO int32_t*)io.group_ids)[s];
  }
}

/* The staged loads of one series: one b128 per column per 128-sample chunk,
 * lane l taking samples (2l, 2l+1), the index clamped to the last pair (the
 * batch columns carry 16 B slack for that).  Issued only for a non-empty
 * series at an even sample offset.
 *
 * The four loads are inline asm, so the compiler neither counts
 * them nor waits for them; pipe_stage_wait below is the only wait, and
 * nothing may read qt/qv between the two (audit the ISA after an edit for a
 * v_mov or a spill of those registers: the destinations count as written
 * when the statement ends, not when the data lands).  Early-clobber
 * outputs: a destination must not share registers with the lane offsets the
 * later loads of the same statement still read.  The leading s_nop covers a
 * base pointer written by a VALU (v_readfirstlane) just before. */
typedef int64_t vm_i64v2 __attribute__((ext_vector_type(2)));
typedef double vm_f64v2 __attribute__((ext_vector_type(2)));

static VM_DEV void pipe_stage_issue(vm_i64v2 (&qt)[PIPE_PCHUNKS],
                                    vm_f64v2 (&qv)[PIPE_PCHUNKS],
                                    const int64_t* gts, const double* gvs,
                                    int64_t n, int lane) {
  static_assert(PIPE_PCHUNKS == 2, "pipe_stage_issue names two chunks");
  const int64_t nm2 = (n - 1) & ~(int64_t)1;
  int64_t k0 = 2 * lane;
  int64_t k1 = 2 * WAVE + 2 * lane;
  if (k0 > nm2) k0 = nm2;
  if (k1 > nm2) k1 = nm2;
  const uint32_t o0 = (uint32_t)k0 * 8u;
  const uint32_t o1 = (uint32_t)k1 * 8u;
  const int64_t* bts = (const int64_t*)vm_uniform_i64((int64_t)gts);
  const double* bvs = (const double*)vm_uniform_i64((int64_t)gvs);
  asm volatile(
      "s_nop 4\n\t"
      "global_load_dwordx4 %0, %4, %6\n\t"
      "global_load_dwordx4 %1, %4, %7\n\t"
      "global_load_dwordx4 %2, %5, %6\n\t"
      "global_load_dwordx4 %3, %5, %7"
      : "=&v"(qt[0]), "=&v"(qv[0]), "=&v"(qt[1]), "=&v"(qv[1])
      : "v"(o0), "v"(o1), "s"(bts), "s"(bvs)
      : "memory");
}

/* Retires the staged loads before their first consumer.  vmcnt(0): the row
 * stores of the previous series retire with them (a counted wait that left
 * those stores in flight measured no faster, profiles/pipe_prefetch.md).
 * The empty statement makes the registers opaque so that no consumer is
 * scheduled above the wait. */
static VM_DEV void pipe_stage_wait(vm_i64v2 (&qt)[PIPE_PCHUNKS],
                                   vm_f64v2 (&qv)[PIPE_PCHUNKS]) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" : "+v"(qt[0]), "+v"(qv[0]), "+v"(qt[1]), "+v"(qv[1])
               :: "memory");
}

/* One grid point of the jbuf paths, whose series all take the 31-bit dt
 * path: the rate over the sentinel-padded pair slab.  The VMGPU_PIPE_ABL_NO_EVAL
 * phase probe emits the window's last sample instead. */
static VM_DEV double pipe_eval_point(const KPlan& p, const SeriesWindow& sw,
                                     const int64_t* lts, const double* lvs,
                                     int count, int i, int j, int64_t t_start) {
#ifdef VMGPU_PIPE_ABL_NO_EVAL
  return (j > 0 && j <= count) ? lvs[(j - 1) * 2] : 0.0;
#else
  return eval_rate_fused<2, true>(p, sw, lts, lvs, count, i, j, t_start, true);
#endif
}

/* VMGPU_PIPE_MINWAVES forces an occupancy floor (waves/SIMD) on the pipe
 * kernel for A/B builds. */
template <int FUNC_CT, bool GROUPED>
__global__
#ifdef VMGPU_PIPE_MINWAVES
__launch_bounds__(BLOCK_THREADS, VMGPU_PIPE_MINWAVES)
#else
__launch_bounds__(BLOCK_THREADS)
#endif
void rollup_pipe_kernel(KPlan p, KIO io) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave_in_block = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const size_t jbuf_bytes = vm_jbuf_bytes(p.jbuf_mode, p.jbuf_elems);
  const size_t slab_bytes = vm_wave_slab_bytes(p.chunk_wave, true);
  const size_t wave_bytes = slab_bytes + jbuf_bytes;
  /* PAIR-interleaved series slab: sample k = 16-byte {t, v} at offset 16k
   * (stride template parameter STR=2 on every accessor) — the eval
   * gathers fetch one b128 LDS read per boundary role instead of two
   * scattered b64 reads.
   * Sentinel padding: lts points at sample 0, which
   * sits VM_SENT_RECS records into the wave's region.  Records -2 and -1
   * hold t = INT64_MIN and are written once per wave; records count and
   * count+1 hold t = INT64_MAX and are rewritten for every series once its
   * count is final (they reach 32 B past slot chunk_wave-1 for a
   * full-length series).  v = 0 in all four.  The probe and the rate
   * evaluator index records -2 .. count+1 without clamps; everything else
   * (staging, compaction, scan, scrape interval) sees an ordinary slab
   * through the shifted base.  Per wave: [front 32 B][chunk_wave x 16 B]
   * [back 32 B][scratch 256 B][jbuf]. */
  char* wave_base = smem + (size_t)wave_in_block * wave_bytes + VM_SENT_RECS * 16;
  int64_t* lts = (int64_t*)wave_base;
  double* lvs = (double*)(wave_base + 8);
  double* lscratch = (double*)(smem + (size_t)wave_in_block * wave_bytes +
                               slab_bytes - 256);
  uint16_t* jbuf = (uint16_t*)(smem + (size_t)wave_in_block * wave_bytes +
                               slab_bytes);
  /* front sentinels: lanes 0-3 write the four 8-byte words of records -2
   * and -1 (made visible by the first phase barrier below) */
  if (lane < 2 * VM_SENT_RECS)
    lts[lane - 2 * VM_SENT_RECS] = (lane & 1) ? 0 : INT64_MIN;
  /* wave-uniform running total (only uniform values are added), so it
   * lives in scalar registers; lane 0 publishes it at the end */
  uint64_t scanned = 0;
  const uint32_t wave_id = blockIdx.x * WAVES_PER_BLOCK + wave_in_block;
  const uint32_t wave_stride = gridDim.x * WAVES_PER_BLOCK;

  /* pair staging registers: lane l holds samples (2l, 2l+1) of each
   * 128-sample chunk, loaded with ONE b128 per column per chunk.  qt/qv
   * are the load destinations and are carried round the loop; rt0..rv1
   * are their halves, valid from pipe_stage_wait to the end of staging. */
  vm_i64v2 qt[PIPE_PCHUNKS];
  vm_f64v2 qv[PIPE_PCHUNKS];
  int64_t rt0[PIPE_PCHUNKS], rt1[PIPE_PCHUNKS];
  double rv0[PIPE_PCHUNKS], rv1[PIPE_PCHUNKS];

  /* wave_id is wave-uniform by construction; readfirstlane makes that
   * provable, so every descriptor below lives in scalar registers.  The
   * loop is a three-deep software pipeline over this wave's series
   * k, k+1, k+2, ...:
   *   - descriptors are scalar loads issued two series ahead, right
   *     behind the data prefetch, the selection entry one step before the
   *     offsets that depend on it.  They are retired by the lgkmcnt(0) of
   *     the phase barrier that follows, never by a vmcnt wait.
   *   - the data of series k+1 is loaded into qt/qv as soon as the scan of
   *     series k has consumed them, and is waited for exactly once, at the
   *     top of iteration k+1 (pipe_stage_wait).  Nothing else on the
   *     hot path waits on vmcnt: no drain before the prefetch issue
   *     and none at the back edge. */
  uint32_t ws = __builtin_amdgcn_readfirstlane(wave_id);
  /* window / step in grid points.  The host launches this kernel only with a
   * plan window, which series_window() hands back unchanged for every series,
   * so the two 64-bit divisions are done once per wave here and not once per
   * series in the loop (the instruction account of
   * profiles/pipe_probe_time.md found them there). */
  const int dg_plan = __builtin_amdgcn_readfirstlane(
      (p.window > 0 && p.step > 0 && p.window % p.step == 0)
          ? (int)(p.window / p.step) : 0);
  PipeDesc cur = {0, 0, 0, 0, -1};
  PipeDesc nxt = {0, 0, 0, 0, -1};
  uint32_t s_nn = 0;
  /* 64-bit positions: ws + 3 * wave_stride may pass 2^32 */
  const uint64_t n_sel = io.n_sel;
  if (ws < n_sel) {
    pipe_desc_read<GROUPED>(io, pipe_sel(io, ws), cur);
    if ((uint64_t)ws + wave_stride < n_sel)
      pipe_desc_read<GROUPED>(io, pipe_sel(io, ws + wave_stride), nxt);
    if ((uint64_t)ws + 2ull * wave_stride < n_sel)
      s_nn = pipe_sel(io, ws + 2 * wave_stride);
    if (cur.n() > 0 && (cur.lo & 1) == 0)
      pipe_stage_issue(qt, qv, io.ts + cur.lo, io.vals + cur.lo, cur.n(),
                       lane);
  }
  while (ws < n_sel) {
    const uint32_t s = cur.s;
    const uint64_t lo = cur.lo;
    const int64_t n = cur.n();
    const int64_t si_raw = cur.si_raw;
    const uint32_t ws_n = ws + wave_stride;
    const bool has_next = (uint64_t)ws + wave_stride < n_sel;
    const bool has_nn = (uint64_t)ws + 2ull * wave_stride < n_sel;
    const bool has_nnn = (uint64_t)ws + 3ull * wave_stride < n_sel;
    pipe_stage_wait(qt, qv);
#pragma unroll
    for (int c = 0; c < PIPE_PCHUNKS; c++) {
      rt0[c] = qt[c].x;
      rt1[c] = qt[c].y;
      rv0[c] = qv[c].x;
      rv1[c] = qv[c].y;
    }
    /* stage the current series into LDS from registers (rcr fused);
     * odd-offset series (no 16-B-aligned pair loads) fall to the global
     * compact path below */
    int count = -1;
    const bool pair_ok = ((lo & 1) == 0);
#ifdef VMGPU_PIPE_ABL_NO_SCAN
    if (false) {
#else
    if (p.rcr && pair_ok) {
#endif
      count = rcr_scan_pairs(rt0, rt1, rv0, rv1, n, lts, lvs,
                             p.drop_stale != 0, p.max_staleness, lane);
    } else if (pair_ok) {
      bool stale = false;
      if (p.drop_stale) {
#pragma unroll
        for (int c = 0; c < PIPE_PCHUNKS; c++) {
          int64_t k = (int64_t)c * 2 * WAVE + 2 * lane;
          if (__ballot((k < n && vm_is_stale_nan(rv0[c])) ||
                       (k + 1 < n && vm_is_stale_nan(rv1[c]))) != 0)
            stale = true;
        }
      }
      if (!stale) {
#pragma unroll
        for (int c = 0; c < PIPE_PCHUNKS; c++) {
          int64_t k = (int64_t)c * 2 * WAVE + 2 * lane;
          if (k < n) { lts[k * 2] = rt0[c]; lvs[k * 2] = rv0[c]; }
          if (k + 1 < n) {
            lts[(k + 1) * 2] = rt1[c];
            lvs[(k + 1) * 2] = rv1[c];
          }
        }
        count = (int)n;
      }
    }
    /* the staging registers are dead now — prefetch the NEXT series into
     * them; these loads stay in flight across scrape/seek/eval/emit and
     * the back edge, up to pipe_stage_wait */
    if (has_next && nxt.n() > 0 && (nxt.lo & 1) == 0)
      pipe_stage_issue(qt, qv, io.ts + nxt.lo, io.vals + nxt.lo, nxt.n(),
                       lane);
    /* descriptors of the series after the next one, and the selection
     * entry of the one after that.  Here and not earlier: an outstanding
     * scalar load turns every counted lgkmcnt wait of the scan above into
     * lgkmcnt(0); the phase barrier below is lgkmcnt(0) anyway. */
    PipeDesc nn = {0, 0, 0, 0, -1};
    uint32_t s_nnn = 0;
    if (has_nn) pipe_desc_read<GROUPED>(io, s_nn, nn);
    if (has_nnn) s_nnn = pipe_sel(io, ws_n + 2 * wave_stride);
    if (count < 0) {
      /* stale NaNs present or odd-offset series (rare): from global */
      count = load_compact_wave<2>(io.ts + lo, io.vals + lo, n, lts, lvs,
                                   p.drop_stale != 0, lane);
      wave_ds_sync();
      if (p.rcr) rcr_scan_wave<2>(lts, lvs, count, p.max_staleness, lane);
    }
    /* back sentinels behind the now-final count (count <= chunk_wave, so
     * they stay inside the slab's back room) */
    if (lane < 2 * VM_SENT_RECS)
      lts[count * 2 + lane] = (lane & 1) ? 0 : INT64_MAX;
    wave_ds_sync();

#ifdef VMGPU_PIPE_ABL_STAGE
    /* stage-only ablation: keep the output write traffic, skip the rest */
    for (int g = lane; g < p.n_grid; g += WAVE) {
      int gc = g < count ? g : (count > 0 ? count - 1 : 0);
      io.out[(size_t)s * (size_t)p.n_grid + (size_t)g] =
          count ? lvs[gc * 2] : 0.0;
    }
    wave_ds_sync();
    if (!has_next) break;
    ws = ws_n;
    cur = nxt;
    nxt = nn;
    s_nn = s_nnn;
    continue;
#endif

    int64_t si = p.step;
#ifndef VMGPU_ABL_NO_SCRAPE
    if (p.start < p.end) {
      if (io.series_si && count == (int)n) {
        si = si_raw > 0 ? si_raw : p.step;
      } else {
        si = scrape_interval_wave_t<true, 2>(lts, count, p.step, lane, lscratch);
      }
    }
#endif
    SeriesWindow sw = series_window(p, si);
    scanned += (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(count);

    double idx_per_ms = 0.0;
    int64_t ts0 = 0;
    /* dt32_series: every dt of this series fits 31 bits (see
     * eval_rate_fused).  A scalar: the dt path is one branch per series —
     * the jbuf loops below are built for the 31-bit path only, and the rare
     * wider series (span of 2^31 ms, 24.8 days, or more) is evaluated by
     * the two-probe loop behind them with the i64 conversion and the true
     * division.  With count <= 1 no slope is ever used. */
    bool dt32_series = true;
    if (count > 1) {
      ts0 = lts[0];
      int64_t span_ms = lts[(count - 1) * 2] - ts0;
      idx_per_ms = span_ms > 0 ? (double)(count - 1) / (double)span_ms : 0.0;
      dt32_series = __builtin_amdgcn_readfirstlane(
                 (int)(span_ms >= 0 && span_ms < ((int64_t)1 << 31))) != 0;
    }
    /* hint advance per 64-point round: the hint
     * (te - ts0) * idx_per_ms is carried as an f64 accumulator.  It only
     * steers the probe — the result is verified against the slab and falls
     * back to the binary search otherwise — so its rounding is free. */
    /* ts0 and the density come out of LDS reads, so the compiler keeps them
     * (and everything derived from them) in vector registers although they
     * are wave-uniform; moving them to scalar registers frees those VGPRs */
    ts0 = vm_uniform_i64(ts0);
    idx_per_ms = __longlong_as_double(
        vm_uniform_i64(__double_as_longlong(idx_per_ms)));
    const double hint_step =
        (double)((int64_t)WAVE * p.step) * idx_per_ms;
    /* emit: GROUPED folds the aggregate switch in with the per-series
     * group row hoisted out of the point loop; the ungrouped build is a
     * plain coalesced row store (no per-point branch, no switch). */
    double* out_row = io.out + (size_t)s * (size_t)p.n_grid;
    double* grp_vrow = nullptr;
    double* grp_crow = nullptr;
    if constexpr (GROUPED) {
      const int grp = cur.grp;
      if (grp >= 0) {
        grp_vrow = io.out + (size_t)grp * (size_t)p.n_grid;
        grp_crow = io.out_counts + (size_t)grp * (size_t)p.n_grid;
      }
    }
    auto emit = [&](int g, double v) {
      if constexpr (GROUPED) {
        if (grp_vrow && !vm_isnan(v)) {
          double* gv = grp_vrow + g;
          double* gc = grp_crow + g;
          switch (p.aggr) {
            case VMGPU_AGGR_SUM: atomicAdd(gv, v); *gc = 1.0; break;
            case VMGPU_AGGR_AVG: atomicAdd(gv, v); atomicAdd(gc, 1.0); break;
            case VMGPU_AGGR_MIN: vm_atomic_min_f64(gv, v); *gc = 1.0; break;
            case VMGPU_AGGR_MAX: vm_atomic_max_f64(gv, v); *gc = 1.0; break;
            case VMGPU_AGGR_COUNT:
            case VMGPU_AGGR_GROUP: atomicAdd(gv, 1.0); *gc = 1.0; break;
            case VMGPU_AGGR_SUM2: atomicAdd(gv, v * v); *gc = 1.0; break;
            case VMGPU_AGGR_GEOMEAN:
              vm_atomic_mul_f64(gv, v); atomicAdd(gc, 1.0); break;
            default: break;
          }
        }
      } else {
        out_row[g] = v;
      }
    };
    const int64_t t_step_wave = (int64_t)WAVE * p.step;
    bool done = false;
    if constexpr (FUNC_CT == VMF_RATE || FUNC_CT == VMF_DERIV_FAST) {
      /* with a plan window, sw.window is that window for every series */
      int dg64 = p.window > 0 ? dg_plan
                 : ((sw.window > 0 && p.step > 0 && sw.window % p.step == 0)
                        ? (int)(sw.window / p.step) : 0);
      if (dt32_series && p.jbuf_mode >= 1 &&
          (size_t)p.n_grid * 2 <= vm_jbuf_bytes(p.jbuf_mode, p.jbuf_elems) &&
          dg64 > 0 && count <= 65535) {
        if (dg64 < WAVE) {
          /* FUSED seek+eval: with dg < 64 the window-START boundary
           * j(g - dg) lives in THIS wave's just-computed j registers (or
           * the previous round's) — one shuffle replaces the whole jbuf
           * write/sync/read round trip.  Head lanes of round 0 (window
           * start before the grid) probe for i directly. */
          int j_prev = 0;
          int g = lane;
          int64_t te = p.start + (int64_t)lane * p.step;
          double hacc = (double)(te - ts0) * idx_per_ms;
          for (int r = 0; r * WAVE < p.n_grid;
               r++, g += WAVE, te += t_step_wave) {
            bool act = g < p.n_grid;
            int gj = (int)hacc + 1;
            hacc += hint_step;
            int j_cur = act ? vm_ub_pipe(lts, count, te, gj) : count;
            int i;
            int i_same = __shfl(j_cur, lane - dg64);
            int i_prev = __shfl(j_prev, lane + WAVE - dg64);
            i = (lane >= dg64) ? i_same : i_prev;
            if (r == 0 && lane < dg64) {
              int64_t t_start = te - sw.window;
              int gi = (int)((double)(t_start - ts0) * idx_per_ms) + 1;
              i = vm_ub_pipe(lts, count, t_start, gi);
            }
            if (act) {
              emit(g, pipe_eval_point(p, sw, lts, lvs, count, i, j_cur,
                                      te - sw.window));
            }
            j_prev = j_cur;
          }
          done = true;
        }
        if (!done) {
        /* j-cache fill: full lane-blocks without bounds checks, one masked
         * tail; t_end is strength-reduced (+64*step per round) */
        {
          int gf = lane;
          int64_t te = p.start + (int64_t)lane * p.step;
          const int fill_full = (p.n_grid / WAVE) * WAVE;
          double hacc = (double)(te - ts0) * idx_per_ms;
          for (; gf < fill_full; gf += WAVE, te += t_step_wave) {
            int gj = (int)hacc + 1;
            hacc += hint_step;
            jbuf[gf] = (uint16_t)vm_ub_pipe(lts, count, te, gj);
          }
          if (gf < p.n_grid) {
            int gj = (int)hacc + 1;
            jbuf[gf] = (uint16_t)vm_ub_pipe(lts, count, te, gj);
          }
        }
        wave_ds_sync();
        /* the first dg points (window start before the grid) probe for i;
         * keeping them out of the main loop keeps the hot body free of the
         * probe's registers and branches */
        const int ghead = dg64 < p.n_grid ? dg64 : p.n_grid;
        for (int g = lane; g < ghead; g += WAVE) {
          int64_t t_end = p.start + (int64_t)g * p.step;
          int64_t t_start = t_end - sw.window;
          int j = jbuf[g];
          int gi = (int)((double)(t_start - ts0) * idx_per_ms) + 1;
          int i = vm_ub_pipe(lts, count, t_start, gi);
          emit(g, pipe_eval_point(p, sw, lts, lvs, count, i, j, t_start));
        }
        /* main eval: full lane-blocks (no per-point exec masking), then one
         * masked tail round */
        {
          int g = ghead + lane;
          int64_t te = p.start + (int64_t)(ghead + lane) * p.step;
          const int span = p.n_grid - ghead;
          const int main_end = ghead + (span / WAVE) * WAVE;
          for (; g < main_end; g += WAVE, te += t_step_wave) {
            int j = jbuf[g];
            int i = jbuf[g - dg64];
            emit(g, pipe_eval_point(p, sw, lts, lvs, count, i, j,
                                    te - sw.window));
          }
          if (g < p.n_grid) {
            int j = jbuf[g];
            int i = jbuf[g - dg64];
            emit(g, pipe_eval_point(p, sw, lts, lvs, count, i, j,
                                    te - sw.window));
          }
        }
        }
        done = true;
      }
    }
    if (!done) {
      /* cold: series too wide for the 31-bit dt path, and the correctness
       * fallback (per-series window not a step multiple — the host gates
       * the pipe launch on plan shapes where the jbuf path applies).  Two
       * probes per point, i64 dt and true division. */
      for (int g = lane; g < p.n_grid; g += WAVE) {
        int64_t t_end = p.start + (int64_t)g * p.step;
        int64_t t_start = t_end - sw.window;
        int gi = (int)((double)(t_start - ts0) * idx_per_ms) + 1;
        int gj = (int)((double)(t_end - ts0) * idx_per_ms) + 1;
        int i = vm_ub_pipe(lts, count, t_start, gi);
        int j = vm_ub_pipe(lts, count, t_end, gj);
        emit(g, eval_rate_fused<2, true>(p, sw, lts, lvs, count, i, j, t_start,
                                         false));
      }
    }
    /* samplesScanned: every grid point of this series contributes exactly
     * samplesScannedPerCall (= 2 for rate/deriv_fast) */
    scanned += 2ull * (unsigned long long)p.n_grid;
    wave_ds_sync();
    if (!has_next) break; /* ws_n may have wrapped */
    ws = ws_n;
    cur = nxt;
    nxt = nn;
    s_nn = s_nnn;
  }
  if (lane == 0 && scanned) atomicAdd(io.samples_scanned, (unsigned long long)scanned);
}
