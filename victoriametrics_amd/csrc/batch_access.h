/* Narrow internal window onto a resident batch for entry points that live
 * outside vmgpu.hip (hot.hip, cvot.hip, topk.hip, aggrhist.hip, aggrcv.hip,
 * aggrtopk.hip; hstat.hip takes only the context lock from here).  Batch
 * itself stays private.  Same spirit as
 * vm_ctx_stream (devalloc.h): the caller runs on the context stream and
 * holds the context lock for as long as it uses what it got here. */
#ifndef VMGPU_BATCH_ACCESS_H
#define VMGPU_BATCH_ACCESS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

/* histogram_over_time state of a batch: the resident result of the last
 * exec plus the pass-to-pass scratch.  Owned by the batch
 * (vmgpu_batch_destroy frees it through vm_hot_state_free).  All buffers
 * are grow-only across execs, so a repeated query allocates nothing. */
struct vm_hot_state {
  /* result */
  double* d_out = nullptr;          /* [n_rows x n_grid] */
  uint32_t* d_row_series = nullptr; /* [n_rows] PHYSICAL series row */
  uint16_t* d_row_code = nullptr;   /* [n_rows] vmrange code */
  size_t out_cap = 0, row_series_cap = 0, row_code_cap = 0; /* bytes */
  uint64_t n_rows = 0;
  int32_t n_grid = 0;
  bool valid = false;
  /* scratch */
  uint16_t* d_codes = nullptr;      /* [n_samples] */
  uint32_t* d_masks = nullptr;      /* [n_series x 16] */
  uint32_t* d_row_counts = nullptr; /* [n_series] */
  uint64_t* d_row_start = nullptr;  /* [n_series + 1] */
  unsigned long long* d_scanned = nullptr;
};

/* count_values_over_time state of a batch (cvot.hip), independent of the
 * histogram state: both results can be resident at once.  Same ownership
 * and grow-only rule (vm_cvot_state_free). */
struct vm_cvot_state {
  /* result */
  double* d_out = nullptr;          /* [n_rows x n_grid] */
  uint32_t* d_row_series = nullptr; /* [n_rows] PHYSICAL series row */
  double* d_row_value = nullptr;    /* [n_rows] the counted value */
  size_t out_cap = 0, row_series_cap = 0, row_value_cap = 0; /* bytes */
  uint64_t n_rows = 0;
  int32_t n_grid = 0;
  bool valid = false;
  /* scratch, sized by the batch */
  uint32_t* d_local_row = nullptr;  /* [n_samples] row of the sample within
                                     * its series, or CVOT_ROW_NONE */
  uint64_t* d_row_keys = nullptr;   /* [n_samples] series s keeps its sorted
                                     * distinct order keys at offsets[s]; a
                                     * series too long for LDS sorts here */
  uint32_t* d_row_counts = nullptr; /* [n_series] */
  uint64_t* d_row_start = nullptr;  /* [n_series + 1] */
  uint32_t* d_long_list = nullptr;  /* [n_series] series above the wave cap */
  unsigned long long* d_small = nullptr; /* [0] samples scanned,
                                          * [1] low word: long-list length */
};

struct vm_batch_cols {
  const int64_t* d_ts;
  const double* d_vals;
  const uint64_t* d_offsets; /* [n_series + 1], physical CSR */
  uint32_t n_series;
  uint64_t n_samples;
  const uint32_t* perm;      /* host; physical row -> original series id,
                              * NULL = identity */
  vm_hot_state* hot;
  vm_cvot_state* cvot;
  /* resident output of the last vmgpu_rollup_exec (topk.hip selects from it
   * and masks it in place): [last_rows x last_grid], NULL / 0 before one */
  double* d_out;
  uint32_t last_rows;
  int32_t last_grid;
};

std::mutex& vm_ctx_mutex(void);
bool vm_ctx_inited(void);
/* 0 on success, 1 for an unknown handle.  Caller holds vm_ctx_mutex(). */
int vm_batch_cols_get(uint64_t handle, vm_batch_cols* out);
/* the context's hipEvent pair and the slot vmgpu_last_kernel_ms reports */
void vm_ctx_events(hipEvent_t* ev_start, hipEvent_t* ev_stop);
void vm_ctx_set_last_kernel_ms(double ms);

/* hot.hip: release every buffer of a batch's histogram state */
void vm_hot_state_free(vm_hot_state* h);

/* cvot.hip: release every buffer of a batch's count_values state */
void vm_cvot_state_free(vm_cvot_state* h);

/* hot.hip: drop the uploaded threshold table (called from vmgpu_shutdown
 * with the context lock held) */
void vm_hot_shutdown(void);

/* aggrhist.hip: free the histogram() aggregate's result and scratch (called
 * from vmgpu_shutdown with the context lock held) */
void vm_aggrhist_shutdown(void);

/* aggrcv.hip: the same for the count_values() aggregate */
void vm_aggrcv_shutdown(void);

/* aggrtopk.hip: the same for the grouped topk / bottomk aggregate */
void vm_aggrtopk_shutdown(void);

#endif
