// Bump allocator over one device allocation: every part starts on a 256-byte
// boundary and takes a whole number of 256-byte units, an empty part one unit
// (no two parts share an address).  A layout function written against it is
// the single statement of a workspace: run over a null base it only sizes
// (bytes()), run over the allocation it hands out the same offsets.
#pragma once
#include <cstdint>

namespace isim {

class Arena {
 public:
  explicit Arena(void *base = nullptr) : base_((char *)base) {}
  template <typename T>
  T *take(uint64_t count) {
    T *p = (T *)here();
    const uint64_t bytes = count * sizeof(T);
    off_ += ((bytes ? bytes : 1) + 255) & ~255ull;
    return p;
  }
  // where the next part will start (null when sizing)
  void *here() const { return base_ ? base_ + off_ : nullptr; }
  uint64_t bytes() const { return off_; }

 private:
  char *base_;
  uint64_t off_ = 0;
};

}  // namespace isim
