// The staging of a synchronous host entry point around its _device entry:
// on the given device a stream and a few buffers, inputs copied up, the
// result copied down after a synchronise.  The first HIP failure is reported
// through set_error and kept in rc(); every later step is then skipped.
#pragma once

#include <cstdint>

#include "hip_check.h"

namespace isim {

class HostStage {
 public:
  // remembers the current device and switches to `device`
  explicit HostStage(int device) {
    if (!ok(hipGetDevice(&prev_), "hipGetDevice") || !ok(hipSetDevice(device), "hipSetDevice")) return;
    switched_ = true;
    if (!ok(hipStreamCreate(&stream_), "hipStreamCreate")) stream_ = nullptr;
  }
  // frees the buffers, destroys the stream, restores the device
  ~HostStage() {
    for (uint32_t i = 0; i < n_; ++i) (void)hipFree(buf_[i]);
    if (stream_) (void)hipStreamDestroy(stream_);
    if (switched_) (void)hipSetDevice(prev_);
  }
  HostStage(const HostStage &) = delete;
  HostStage &operator=(const HostStage &) = delete;

  int rc() const { return rc_; }
  hipStream_t stream() const { return stream_; }

  // a device buffer (nullptr: bytes is 0, or a failure)
  void *alloc(uint64_t bytes) {
    void *p = nullptr;
    if (rc_ != ISIM_OK || bytes == 0) return nullptr;
    if (!ok(n_ < kMaxBufs ? hipMalloc(&p, bytes) : hipErrorOutOfMemory, "hipMalloc")) return nullptr;
    return buf_[n_++] = p;
  }
  // a device buffer holding `bytes` of h once the stream reaches this point
  void *upload(const void *h, uint64_t bytes) {
    void *p = alloc(bytes);
    if (p && !ok(hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, stream_), "hipMemcpyAsync")) return nullptr;
    return p;
  }
  // waits for the stream, then copies `bytes` of d to h; the entry point's return value
  int download(void *h, const void *d, uint64_t bytes) {
    if (rc_ == ISIM_OK && ok(hipStreamSynchronize(stream_), "hipStreamSynchronize") && bytes)
      ok(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost), "hipMemcpy");
    return rc_;
  }

 private:
  static constexpr uint32_t kMaxBufs = 6;
  bool ok(hipError_t e, const char *what) {
    if (e != hipSuccess) rc_ = set_error(ISIM_EHIP, std::string("host staging: ") + what + ": " + hipGetErrorString(e));
    return e == hipSuccess;
  }
  int rc_ = ISIM_OK;
  int prev_ = 0;
  bool switched_ = false;
  hipStream_t stream_ = nullptr;
  void *buf_[kMaxBufs] = {};
  uint32_t n_ = 0;
};

}  // namespace isim
