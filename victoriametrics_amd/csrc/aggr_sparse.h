/* What the sparse aggregates over a member CSR share: aggrhist.hip
 * (histogram()) and aggrcv.hip (count_values()) both cut every group into
 * chunks of members, hand (chunk, tile of 64 columns) work items to
 * wavefronts, count into a zeroed u32 matrix and convert it to f64 at the
 * end.  Only the row discovery differs.  aggrtopk.hip (grouped topk) takes
 * the chunk list, the work items and the CSR checks from here and counts
 * nothing.  The library is built without
 * relocatable device code, so the kernel here is instantiated per file. */
#ifndef VMGPU_AGGR_SPARSE_H
#define VMGPU_AGGR_SPARSE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cstdio>
#include <vector>

#include "hot_common.h"

struct AhChunk {
  uint64_t begin; /* first member, index into group_rows */
  uint32_t n;     /* 1..chunk_members */
  uint32_t group;
};

namespace {

/* counters -> f64 result; an absent count is 0.0 (histogram()) or NaN
 * (count_values()) */
template <bool ZERO_IS_NAN>
__global__ __launch_bounds__(256) void ah_u32_to_f64_kernel(
    const uint32_t* __restrict__ cnt, uint64_t n, double* __restrict__ out) {
  const double dnan = __longlong_as_double((long long)HOT_NAN_BITS);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t c = cnt[i];
    out[i] = (ZERO_IS_NAN && c == 0) ? dnan : (double)c;
  }
}

/* every group cut into chunks of at most chunk_members members */
inline void ah_build_chunks(const uint64_t* group_offsets, uint32_t n_groups,
                            uint32_t chunk_members,
                            std::vector<AhChunk>* chunks) {
  chunks->clear();
  for (uint32_t g = 0; g < n_groups; g++)
    for (uint64_t lo = group_offsets[g]; lo < group_offsets[g + 1];
         lo += chunk_members) {
      AhChunk c;
      c.begin = lo;
      c.n = (uint32_t)std::min<uint64_t>(chunk_members, group_offsets[g + 1] - lo);
      c.group = g;
      chunks->push_back(c);
    }
}

inline uint32_t ah_blocks(uint64_t work, uint32_t per_block) {
  return (uint32_t)std::min<uint64_t>((work + per_block - 1) / per_block,
                                      HOT_MAX_BLOCKS);
}

/* "vmgpu: <op>: <what>" into errbuf; returns 1 as vm_set_err does */
inline int ah_csr_err(char* errbuf, size_t errbuf_len, const char* op,
                      const char* what) {
  if (errbuf && errbuf_len) snprintf(errbuf, errbuf_len, "vmgpu: %s: %s", op, what);
  return 1;
}

/* Checks of the grid and the member CSR shared by the operators' entry
 * points; op names the operator in the message ("aggr histogram").  Nothing
 * is launched or allocated before they pass; each operator bounds its own
 * result size afterwards.  Returns 0 or 1. */
inline int ah_validate_csr(const char* op, uint32_t n_in_rows, int64_t n_grid,
                           const uint32_t* group_rows,
                           const uint64_t* group_offsets, uint32_t n_groups,
                           char* errbuf, size_t errbuf_len) {
  if (n_grid <= 0 || n_grid > (int64_t)1 << 30)
    return ah_csr_err(errbuf, errbuf_len, op, "bad grid");
  if (n_groups == 0) return 0;
  if (!group_offsets) return ah_csr_err(errbuf, errbuf_len, op, "bad args");
  if (group_offsets[0] != 0)
    return ah_csr_err(errbuf, errbuf_len, op, "group_offsets must start at 0");
  for (uint32_t g = 0; g < n_groups; g++)
    if (group_offsets[g + 1] < group_offsets[g])
      return ah_csr_err(errbuf, errbuf_len, op, "group_offsets must not decrease");
  const uint64_t n_members = group_offsets[n_groups];
  if (n_members > 0xFFFFFFFFull)
    return ah_csr_err(errbuf, errbuf_len, op, "more than 2^32 - 1 members");
  if (n_members && !group_rows)
    return ah_csr_err(errbuf, errbuf_len, op, "bad args");
  for (uint64_t k = 0; k < n_members; k++)
    if (group_rows[k] >= n_in_rows)
      return ah_csr_err(errbuf, errbuf_len, op, "group_rows entry out of range");
  return 0;
}

}  // namespace

#endif
