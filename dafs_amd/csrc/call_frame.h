// dafs_amd/csrc/call_frame.h -- the frame of one library call that queues device work on the context's stream (the
// capi_*.cpp files only).  The rule it keeps: host buffers, then frame; drain, then free.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

#include "ctx.h"
#include "hip_util.h"

namespace dafs {

// Every return waits for the stream and only then frees the call's own device arrays.  Host buffers that queued copies
// touch must still outlive the frame: it is declared after them.
struct call_frame {
  hipStream_t st;
  std::vector<void*> owned;
  explicit call_frame(dafs_hip_ctx* c) : st(c->stream) {}
  call_frame(const call_frame&) = delete;
  call_frame& operator=(const call_frame&) = delete;
  ~call_frame() {
    (void)hipStreamSynchronize(st);
    for (void* p : owned) (void)hipFree(p);
  }
  // a device array of this call, not kept in the context; null when there is no memory
  void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hip_check(hipMalloc(&p, bytes))) return nullptr;
    owned.push_back(p);
    return p;
  }
  // The queued operations; true on failure, like hip_check.  No bytes to send and no place to receive them are no-ops.
  bool up(void* dev, const void* host, size_t bytes) { return bytes && hip_check(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st)); }
  bool down(void* host, const void* dev, size_t bytes) { return host && hip_check(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st)); }
  bool fill(void* dev, int value, size_t bytes) { return hip_check(hipMemsetAsync(dev, value, bytes, st)); }
  // the wait whose result the call returns
  int finish() { return hip_check(hipStreamSynchronize(st)) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK; }
};

}  // namespace dafs
