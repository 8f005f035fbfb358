/* pipe_probe.h — the pipe kernel's boundary probe over the sentinel-padded
 * slab, written as a count.
 *
 * The slab holds 16-byte {t, v} records.  Records -2 and -1 hold a front
 * sentinel no seek lies below, records n and n + 1 a back sentinel every seek
 * lies below, and the n samples between them are sorted, so the whole run of
 * records -2 .. n+1 is non-decreasing in t.  Time is int64, two 8-byte words
 * per record, and the sentinels are INT64_MIN and INT64_MAX (MIN and MAX
 * below).
 *
 * vm_probe_count4 looks for the upper bound of `seek` (the first index whose
 * timestamp is > seek, in [0, n]) next to a hint g.  With g clamped to
 * [0, n] the four records g-2 .. g+1 all exist (g-2 >= -2, g+1 <= n+1), so
 * they are read unconditionally: one base, four constant offsets, no edge
 * terms and nothing that depends on an earlier read.  Let c be the number of
 * the four whose timestamp is <= seek.  If
 *
 *     ts[g-2] <= seek < ts[g+1]                                  (bracket)
 *
 * then, the records being sorted, every record up to g-2 is <= seek and
 * every record from g+1 on is > seek, the c records <= seek are exactly
 * g-2 .. g-3+c, and the upper bound is g - 2 + c.  The bracket fixes the
 * outer two terms of the count (ts[g-2] counts, ts[g+1] does not), so
 * 1 <= c <= 3 and the answer is one of g-1, g, g+1.
 *
 * The edges fall out of the sentinels:
 *   - g <= 1 reads front sentinels.  MIN <= seek holds for every seek, so
 *     they count as "<= seek" like real samples in front of the answer
 *     would; at g == 0 both count, c >= 2 and the answer is >= 0.
 *   - g >= n-1 reads back sentinels.  MAX <= seek fails for every seek below
 *     MAX, so they never count; at g == n that leaves c <= 2 and the answer
 *     is <= n.
 *   - seek == MAX can bracket only below a real record, never below a back
 *     sentinel (seek < MAX is false), so a hint near n misses and the binary
 *     search returns n.  A real sample at MIN or MAX keeps the run sorted and
 *     needs nothing special.
 *
 * A miss (-1) sends the lane to the binary search; the probe never returns a
 * wrong index and never reads outside records -2 .. n+1.
 *
 * Plain C++ for host and device: the kernel (vmgpu.hip) and the host check
 * (tests/pipe_probe_check.cpp) compile this very function.  TS is anything
 * indexable that yields int64_t: a plain pointer in the kernel, a
 * bounds-recording view in the host check.
 */
#ifndef VM_PIPE_PROBE_H
#define VM_PIPE_PROBE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VM_PROBE_FN static __host__ __device__ __forceinline__
#else
#define VM_PROBE_FN static inline
#endif

/* ts indexes 8-byte words relative to sample 0, two per record.  Returns the
 * upper bound of seek, or -1 when the four records around the hint do not
 * bracket it. */
template <class TS>
VM_PROBE_FN int vm_probe_count4(TS ts, int n, int64_t seek, int g) {
  g = g < 0 ? 0 : (g > n ? n : g);
  const int b = (g - 2) * 2;
  const int64_t t_m2 = ts[b];
  const int64_t t_m1 = ts[b + 2];
  const int64_t t_0 = ts[b + 4];
  const int64_t t_p1 = ts[b + 6];
  /* under the bracket the outer two records contribute a fixed 1 + 0 to the
   * count, so only the inner two are counted: four compares in all */
  const bool bracket = (t_m2 <= seek) & (t_p1 > seek);
  const int c = 1 + (int)(t_m1 <= seek) + (int)(t_0 <= seek);
  return bracket ? g - 2 + c : -1;
}

#endif /* VM_PIPE_PROBE_H */
