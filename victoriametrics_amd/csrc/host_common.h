/* What every host entry point of the library shares: the error-buffer
 * helpers with their return codes, the try macro, and the two owners of
 * device memory.  One definition each; no translation unit keeps its own. */
#ifndef VMGPU_HOST_COMMON_H
#define VMGPU_HOST_COMMON_H
#include <hip/hip_runtime.h>
#include <cstdio>

#include "devalloc.h"

/* bad argument / bad state: returns 1 */
inline int vm_set_err(char* errbuf, size_t len, const char* msg) {
  if (errbuf && len) snprintf(errbuf, len, "%s", msg);
  return 1;
}

/* a HIP call failed: returns 2 */
inline int vm_hip_err(char* errbuf, size_t len, const char* what, hipError_t e) {
  if (errbuf && len) snprintf(errbuf, len, "%s: %s", what, hipGetErrorString(e));
  return 2;
}

/* needs errbuf / errbuf_len in scope; everything the function owns must be
 * held by a destructor, since this returns from the middle of it */
#define VM_HIP_TRY(expr, what)                                              \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) return vm_hip_err(errbuf, errbuf_len, what, _e);  \
  } while (0)

/* plain hipMalloc / hipFree, for the entry points that run on stream 0 */
struct VmDevBuf {
  void* p = nullptr;
  ~VmDevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
};

/* pool-backed owner (devalloc.h) for code on the context stream: the free
 * is ordered on that stream, behind whatever the function queued there.
 * release() hands the pointer on and leaves the owner empty. */
template <class T>
struct VmPoolBuf {
  T* p = nullptr;
  VmPoolBuf() = default;
  VmPoolBuf(const VmPoolBuf&) = delete;
  VmPoolBuf& operator=(const VmPoolBuf&) = delete;
  ~VmPoolBuf() { (void)vm_dev_free(p); }
  hipError_t alloc(size_t bytes) { return vm_dev_malloc(&p, bytes); }
  T* release() {
    T* q = p;
    p = nullptr;
    return q;
  }
};

#endif
