/* hstat.hip — the histogram transforms over le-bucket groups:
 * histogram_avg / stddev / stdvar (hstat_kernel), histogram_share
 * (hshare_kernel) and histogram_quantile (hq_kernel, transform.go:1028-1074
 * + fixBrokenBuckets 1140).  One thread per (group, grid point); the bucket
 * rows come from the host, [n_rows x n_grid] with group_offsets as CSR.
 * Runs on the context stream under the context lock.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>

#include "batch_access.h"
#include "host_common.h"
#include "rollup_device.h"
#include "../../include/vmgpu.h"

/* histogram_avg / histogram_stddev / histogram_stdvar
 * (transform.go:transformHistogramAvg/Stddev/Stdvar + avgForLeTimeseries /
 * stdvarForLeTimeseries): (le+lePrev)/2-weighted moments over the bucket
 * column, +/-Inf les skipped, NO fixBrokenBuckets (the reference reads raw
 * cumulative values here). mode: 0 avg, 1 stddev, 2 stdvar. */
__global__ void hstat_kernel(int32_t mode, const double* bv, const double* les,
                             const uint64_t* goff, int64_t n_groups,
                             int32_t n_grid, double* out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)n_groups * n_grid;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    int64_t grp = (int64_t)(i / n_grid);
    int32_t g = (int32_t)(i % n_grid);
    int64_t lo = (int64_t)goff[grp];
    int64_t n_les = (int64_t)(goff[grp + 1] - lo);
    double le_prev = 0, v_prev = 0, sum = 0, sum2 = 0, wt = 0;
    for (int64_t j = 0; j < n_les; j++) {
      double le = les[lo + j];
      if (isinf(le)) continue;
      double v = bv[(size_t)(lo + j) * n_grid + g];
      double n = (le + le_prev) / 2;
      double w = v - v_prev;
      sum += n * w;
      sum2 += n * n * w;
      wt += w;
      le_prev = le;
      v_prev = v;
    }
    double r;
    if (wt == 0) {
      r = vm_dnan();
    } else if (mode == 0) {
      r = sum / wt;
    } else {
      double avg = sum / wt;
      double sv = sum2 / wt - avg * avg;
      if (sv < 0) sv = 0;
      r = (mode == 1) ? sqrt(sv) : sv;
    }
    out[i] = r;
  }
}

/* histogram_share (transform.go:transformHistogramShare): the quantile
 * walk's dual — share of samples <= leReq[g], with lower/upper bounds.
 * fixBrokenBuckets applied on the fly as in hq_kernel. */
__global__ void hshare_kernel(const double* le_req, const double* bv,
                              const double* les, const uint64_t* goff,
                              int64_t n_groups, int32_t n_grid, double* out,
                              double* out_lo, double* out_hi) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)n_groups * n_grid;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    int64_t grp = (int64_t)(i / n_grid);
    int32_t g = (int32_t)(i % n_grid);
    int64_t lo = (int64_t)goff[grp];
    int64_t n_les = (int64_t)(goff[grp + 1] - lo);
    double req = le_req[g];
    double q = vm_dnan(), lb = vm_dnan(), ub = vm_dnan();
    if (!vm_isnan(req) && n_les > 0) {
      if (req < 0) {
        q = 0; lb = 0; ub = 0;
      } else if (isinf(req) && req > 0) {
        q = 1; lb = 1; ub = 1;
      } else {
        /* fixBrokenBuckets pass: running-max with NaN->prev */
        double v_last = 0;
        {
          double fix_prev = 0;
          for (int64_t j = 0; j < n_les; j++) {
            double v = bv[(size_t)(lo + j) * n_grid + g];
            if (j == 0) fix_prev = vm_isnan(v) ? 0 : v;
            else if (!(vm_isnan(v) || fix_prev > v)) fix_prev = v;
          }
          v_last = fix_prev;
        }
        double vp = 0, lep = 0;
        double fix_prev = 0;
        bool done = false;
        for (int64_t j = 0; j < n_les && !done; j++) {
          double raw = bv[(size_t)(lo + j) * n_grid + g];
          double v;
          if (j == 0) v = vm_isnan(raw) ? 0 : raw;
          else v = (vm_isnan(raw) || fix_prev > raw) ? fix_prev : raw;
          fix_prev = v;
          double le = les[lo + j];
          if (req >= le) {
            vp = v;
            lep = le;
            continue;
          }
          /* lePrev <= req < le */
          lb = vp / v_last;
          if (isinf(le) && le > 0) {
            q = lb;
            ub = 1;
          } else if (lep == req) {
            q = lb;
            ub = lb;
          } else {
            ub = v / v_last;
            q = lb + (v - vp) / v_last * (req - lep) / (le - lep);
          }
          done = true;
        }
        if (!done) { q = 1; lb = 1; ub = 1; }
      }
    }
    out[i] = q;
    if (out_lo) out_lo[i] = lb;
    if (out_hi) out_hi[i] = ub;
  }
}

__global__ void hq_kernel(double phi, const double* bv, const double* les,
                          const uint64_t* goff, int64_t n_groups, int32_t n_grid,
                          double* out, double* out_lo, double* out_hi) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)n_groups * n_grid;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    int64_t grp = (int64_t)(i / n_grid);
    int32_t g = (int32_t)(i % n_grid);
    int64_t lo = (int64_t)goff[grp];
    int64_t n_les = (int64_t)(goff[grp + 1] - lo);
    double q = vm_dnan(), lb = vm_dnan(), ub = vm_dnan();
    if (!vm_isnan(phi)) {
      double fix_prev = 0;
      double v_last = 0;
      for (int64_t j = 0; j < n_les; j++) {
        double v = bv[(size_t)(lo + j) * n_grid + g];
        if (j == 0) fix_prev = vm_isnan(v) ? 0 : v;
        else if (!(vm_isnan(v) || fix_prev > v)) fix_prev = v;
        v_last = fix_prev;
      }
      if (v_last != 0) {
        if (phi < 0) {
          q = -vm_dinf();
          lb = -vm_dinf();
          double v0 = bv[(size_t)lo * n_grid + g];
          ub = vm_isnan(v0) ? 0 : v0;
        } else if (phi > 1) {
          q = vm_dinf();
          lb = v_last;
          ub = vm_dinf();
        } else {
          double v_req = v_last * phi;
          double vp = 0, lep = 0;
          fix_prev = 0;
          bool done = false;
          for (int64_t j = 0; j < n_les && !done; j++) {
            double raw = bv[(size_t)(lo + j) * n_grid + g];
            double v;
            if (j == 0) v = vm_isnan(raw) ? 0 : raw;
            else v = (vm_isnan(raw) || fix_prev > raw) ? fix_prev : raw;
            fix_prev = v;
            double le = les[lo + j];
            if (v <= 0) {
              lep = le;
              continue;
            }
            if (v < v_req) {
              vp = v;
              lep = le;
              continue;
            }
            if (isinf(le)) break;
            if (v == vp) {
              q = lep;
              lb = lep;
              ub = v;
              done = true;
              break;
            }
            q = lep + (le - lep) * (v_req - vp) / (v - vp);
            lb = lep;
            ub = le;
            done = true;
          }
          if (!done) {
            double vv = vm_dnan();
            for (int64_t j = n_les - 1; j >= 0; j--) {
              if (!isinf(les[lo + j])) {
                vv = les[lo + j];
                break;
              }
            }
            q = vv;
            lb = vv;
            ub = vm_dinf();
          }
        }
      }
    }
    out[i] = q;
    if (out_lo) out_lo[i] = lb;
    if (out_hi) out_hi[i] = ub;
  }
}

namespace {

/* what all three entry points take from the host: the bucket rows, their
 * le values and the CSR of the groups */
struct HistInputs {
  VmPoolBuf<double> bv, les;
  VmPoolBuf<uint64_t> off;

  int upload(const double* bucket_values, const double* les_h,
             const uint64_t* group_offsets, uint32_t n_groups, int32_t n_grid,
             hipStream_t st, char* errbuf, size_t errbuf_len) {
    uint64_t n_rows = group_offsets[n_groups];
    VM_HIP_TRY(bv.alloc((size_t)n_rows * n_grid * 8), "alloc bv");
    VM_HIP_TRY(les.alloc((size_t)n_rows * 8), "alloc les");
    VM_HIP_TRY(off.alloc((size_t)(n_groups + 1) * 8), "alloc off");
    VM_HIP_TRY(hipMemcpyAsync(bv.p, bucket_values, (size_t)n_rows * n_grid * 8,
                              hipMemcpyHostToDevice, st), "ul bv");
    VM_HIP_TRY(hipMemcpyAsync(les.p, les_h, (size_t)n_rows * 8, hipMemcpyHostToDevice, st), "ul les");
    VM_HIP_TRY(hipMemcpyAsync(off.p, group_offsets, (size_t)(n_groups + 1) * 8,
                              hipMemcpyHostToDevice, st), "ul off");
    return 0;
  }
};

}  // namespace

extern "C" {

int vmgpu_histogram_stat(int32_t mode, const double* bucket_values,
                         const double* les, const uint64_t* group_offsets,
                         uint32_t n_groups, int32_t n_grid, double* out,
                         char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited()) return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  if (!bucket_values || !les || !group_offsets || !out || n_groups == 0 || n_grid <= 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad args");
  hipStream_t st = vm_ctx_stream();
  HistInputs in;
  VmPoolBuf<double> d_out;
  size_t out_elems = (size_t)n_groups * n_grid;
  int rc = in.upload(bucket_values, les, group_offsets, n_groups, n_grid, st,
                     errbuf, errbuf_len);
  if (rc != 0) return rc;
  VM_HIP_TRY(d_out.alloc(out_elems * 8), "alloc out");
  uint32_t blocks = (uint32_t)std::min<size_t>((out_elems + 255) / 256, 4096);
  hipLaunchKernelGGL(hstat_kernel, dim3(blocks), dim3(256), 0, st, mode, in.bv.p,
                     in.les.p, in.off.p, (int64_t)n_groups, n_grid, d_out.p);
  VM_HIP_TRY(hipMemcpyAsync(out, d_out.p, out_elems * 8, hipMemcpyDeviceToHost, st), "dl out");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync hstat");
  hipError_t kerr = hipGetLastError();
  if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "hstat kernel", kerr);
  return 0;
}

int vmgpu_histogram_share(const double* le_req, const double* bucket_values,
                          const double* les, const uint64_t* group_offsets,
                          uint32_t n_groups, int32_t n_grid, double* out,
                          double* out_lower, double* out_upper,
                          char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited()) return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  if (!le_req || !bucket_values || !les || !group_offsets || !out ||
      n_groups == 0 || n_grid <= 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad args");
  hipStream_t st = vm_ctx_stream();
  HistInputs in;
  VmPoolBuf<double> d_req, d_out, d_lo, d_hi;
  size_t out_elems = (size_t)n_groups * n_grid;
  VM_HIP_TRY(d_req.alloc((size_t)n_grid * 8), "alloc req");
  int rc = in.upload(bucket_values, les, group_offsets, n_groups, n_grid, st,
                     errbuf, errbuf_len);
  if (rc != 0) return rc;
  VM_HIP_TRY(d_out.alloc(out_elems * 8), "alloc out");
  if (out_lower) VM_HIP_TRY(d_lo.alloc(out_elems * 8), "alloc lo");
  if (out_upper) VM_HIP_TRY(d_hi.alloc(out_elems * 8), "alloc hi");
  VM_HIP_TRY(hipMemcpyAsync(d_req.p, le_req, (size_t)n_grid * 8,
                            hipMemcpyHostToDevice, st), "ul req");
  uint32_t blocks = (uint32_t)std::min<size_t>((out_elems + 255) / 256, 4096);
  hipLaunchKernelGGL(hshare_kernel, dim3(blocks), dim3(256), 0, st, d_req.p,
                     in.bv.p, in.les.p, in.off.p, (int64_t)n_groups, n_grid,
                     d_out.p, d_lo.p, d_hi.p);
  VM_HIP_TRY(hipMemcpyAsync(out, d_out.p, out_elems * 8, hipMemcpyDeviceToHost, st), "dl out");
  if (out_lower) VM_HIP_TRY(hipMemcpyAsync(out_lower, d_lo.p, out_elems * 8, hipMemcpyDeviceToHost, st), "dl lo");
  if (out_upper) VM_HIP_TRY(hipMemcpyAsync(out_upper, d_hi.p, out_elems * 8, hipMemcpyDeviceToHost, st), "dl hi");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync hshare");
  hipError_t kerr = hipGetLastError();
  if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "hshare kernel", kerr);
  return 0;
}

int vmgpu_histogram_quantile(double phi, const double* bucket_values,
                             const double* les, const uint64_t* group_offsets,
                             uint32_t n_groups, int32_t n_grid,
                             double* out, double* out_lower, double* out_upper,
                             char* errbuf, size_t errbuf_len) {
  std::lock_guard<std::mutex> lock(vm_ctx_mutex());
  if (!vm_ctx_inited()) return vm_set_err(errbuf, errbuf_len, "vmgpu: not initialized");
  if (!bucket_values || !les || !group_offsets || !out || n_groups == 0 || n_grid <= 0)
    return vm_set_err(errbuf, errbuf_len, "vmgpu: bad args");
  hipStream_t st = vm_ctx_stream();
  HistInputs in;
  VmPoolBuf<double> d_out, d_lo, d_hi;
  size_t out_elems = (size_t)n_groups * n_grid;
  int rc = in.upload(bucket_values, les, group_offsets, n_groups, n_grid, st,
                     errbuf, errbuf_len);
  if (rc != 0) return rc;
  VM_HIP_TRY(d_out.alloc(out_elems * 8), "alloc out");
  if (out_lower) VM_HIP_TRY(d_lo.alloc(out_elems * 8), "alloc lo");
  if (out_upper) VM_HIP_TRY(d_hi.alloc(out_elems * 8), "alloc hi");
  uint32_t blocks = (uint32_t)std::min<size_t>((out_elems + 255) / 256, 4096);
  hipLaunchKernelGGL(hq_kernel, dim3(blocks), dim3(256), 0, st, phi, in.bv.p,
                     in.les.p, in.off.p, (int64_t)n_groups, n_grid, d_out.p,
                     d_lo.p, d_hi.p);
  VM_HIP_TRY(hipMemcpyAsync(out, d_out.p, out_elems * 8, hipMemcpyDeviceToHost, st), "dl out");
  if (out_lower) VM_HIP_TRY(hipMemcpyAsync(out_lower, d_lo.p, out_elems * 8, hipMemcpyDeviceToHost, st), "dl lo");
  if (out_upper) VM_HIP_TRY(hipMemcpyAsync(out_upper, d_hi.p, out_elems * 8, hipMemcpyDeviceToHost, st), "dl hi");
  VM_HIP_TRY(hipStreamSynchronize(st), "sync hq");
  hipError_t kerr = hipGetLastError();
  if (kerr != hipSuccess) return vm_hip_err(errbuf, errbuf_len, "hq kernel", kerr);
  return 0;
}

}  /* extern "C" */
