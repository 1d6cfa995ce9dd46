// Owners of what a handler keeps on a device: a buffer (DevBuf), an event
// and the DES item pool.  Move-only; each releases its handle in its
// destructor, so a struct of them frees itself and cannot be copied.
#pragma once

#include <cstddef>
#include <vector>

#include "hip_check.h"

namespace isim {

template <typename H, auto Drop>
class Owned {
 public:
  Owned() = default;
  ~Owned() { reset(); }
  Owned(Owned &&o) noexcept : h_(o.release()) {}
  Owned &operator=(Owned &&o) noexcept {
    if (this != &o) reset(o.release());
    return *this;
  }
  Owned(const Owned &) = delete;
  Owned &operator=(const Owned &) = delete;

  H get() const { return h_; }
  explicit operator bool() const { return h_ != H(); }
  H release() {
    H h = h_;
    h_ = H();
    return h;
  }
  void reset(H h = H()) {
    if (h_ != H()) Drop(h_);
    h_ = h;
  }

 private:
  H h_ = H();
};

inline void drop_buf(void *p) { (void)hipFree(p); }
inline void drop_event(hipEvent_t e) { (void)hipEventDestroy(e); }
// the device first drains the hipFreeAsync calls queued on user streams
inline void drop_pool(hipMemPool_t p) {
  (void)hipDeviceSynchronize();
  (void)hipMemPoolDestroy(p);
}

template <typename T>
using DevBuf = Owned<T *, drop_buf>;
using DevEvent = Owned<hipEvent_t, drop_event>;
using DevPool = Owned<hipMemPool_t, drop_pool>;

// dst: a new buffer of bytes + pad, never empty, left as it comes
template <typename T>
int alloc(DevBuf<T> &dst, size_t bytes, size_t pad = 0) {
  void *p = nullptr;
  ISIM_HIPCHK(hipMalloc(&p, bytes + pad ? bytes + pad : 1));
  dst.reset((T *)p);
  return ISIM_OK;
}

// dst: a new buffer holding `bytes` of src and then `pad` zero bytes (the
// kernels that prefetch past a table's end read those); src null with bytes
// 0: a zeroed buffer of `pad`
template <typename T>
int upload(DevBuf<T> &dst, const void *src, size_t bytes, size_t pad = 0) {
  if (const int rc = alloc(dst, bytes, pad)) return rc;
  if (bytes) ISIM_HIPCHK(hipMemcpy(dst.get(), src, bytes, hipMemcpyHostToDevice));
  if (pad) ISIM_HIPCHK(hipMemset((char *)dst.get() + bytes, 0, pad));
  return ISIM_OK;
}

template <typename T, typename V>
int upload(DevBuf<T> &dst, const std::vector<V> &v, size_t pad = 0) {
  return upload(dst, v.data(), v.size() * sizeof(V), pad);
}

}  // namespace isim
