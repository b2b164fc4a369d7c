// atmrt_cached.h — internal, host only (nothing of HIP: tests/csrc/cached_host.cpp compiles it with g++ alone): the one rule by
// which a context keeps what it builds from a frame's inputs (atmrt_ctx.h has the products, DESIGN.md §3 the table).
//
// A product is a value kept with the key it was built from.  A build that fails leaves the product EMPTY (it may have overwritten
// the device buffer already), never the old value under the old key.  Every successful build has a serial of its own; a product
// computed from another one names that one's serial() in its key, as the terrain's consumers name TileStore::generation.
#pragma once

#include <cstdint>
#include <cstring>

namespace atmrt {

// A double enters a key as its bits: a NaN parameter does not rebuild for ever, and -0.0 is not 0.0.
inline uint64_t bits(double v) {
  uint64_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}

struct Nothing {}; // the value of a product that lives in a device buffer alone

template <class Key, class Value = Nothing>
class Cached {
 public:
  // 0: holds nothing.  Otherwise the number of successful builds so far: it never repeats, across drop() and failures too.
  uint64_t serial() const { return serial_; }
  const Value& value() const { return value_; }
  void drop() { serial_ = 0; }
  // Key equal and not forced: 0 without calling `build`.  Otherwise the product is dropped and build(value) -> int status runs: key and
  // serial are committed only if it returned 0, any other status is returned.  *built: a build succeeded.
  template <class Build>
  int refresh(const Key& key, Build&& build, bool force = false, bool* built = nullptr) {
    if (built) *built = false;
    if (serial_ && !force && key == key_) return 0;
    drop();
    const int rc = build(value_);
    if (rc) return rc;
    key_ = key;
    serial_ = ++builds_;
    if (built) *built = true;
    return 0;
  }

 private:
  Key key_{};
  Value value_{};
  uint64_t serial_ = 0, builds_ = 0;
};

} // namespace atmrt
