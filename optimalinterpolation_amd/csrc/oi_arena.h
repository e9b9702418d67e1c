// First-fit free list over the byte offsets [0, size) of one allocation, in
// 256-byte granules.  Host code only and no HIP: the engine's Arena
// (oi_engine.cpp) puts a device allocation behind the offsets, and
// tests/host/arena_check.cpp drives this header alone under ASan + UBSan
// against a granule bitmap.
//
// Rules:
//   * alloc(bytes) rounds up to the granule and returns the lowest offset whose
//     free block holds it, or SIZE_MAX;
//   * a zero-byte block never touches the list: alloc(0) succeeds whatever is
//     free (it names the lowest free offset, or size() in a full arena; nothing
//     may be stored there) and release(off, 0) does nothing;
//   * release(off, bytes) returns a block alloc handed out.  A block the list
//     cannot have handed out -- off = SIZE_MAX of a failed alloc, a range past
//     size(), a range that meets a free block (a second release) -- changes
//     nothing: it would alias live blocks later.
#pragma once
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <map>

class OiFreeList {
 public:
  static constexpr size_t GRANULE = 256;
  static size_t round_up(size_t bytes) { return (bytes + (GRANULE - 1)) & ~(GRANULE - 1); }

  void reset(size_t bytes) {
    size_ = bytes;
    free_.clear();
    if (bytes) free_[0] = bytes;
  }
  size_t size() const { return size_; }

  // returns offset or SIZE_MAX
  size_t alloc(size_t bytes) {
    if (bytes == 0) return free_.empty() ? size_ : free_.begin()->first;
    if (bytes > size_) return SIZE_MAX;  // (also keeps the rounding from wrapping)
    bytes = round_up(bytes);
    for (auto it = free_.begin(); it != free_.end(); ++it) {
      if (it->second >= bytes) {
        const size_t off = it->first, len = it->second;
        free_.erase(it);
        if (len > bytes) free_[off + bytes] = len - bytes;
        return off;
      }
    }
    return SIZE_MAX;
  }

  void release(size_t off, size_t bytes) {
    if (bytes == 0 || off >= size_ || bytes > size_ - off) return;
    bytes = round_up(bytes);
    if (bytes > size_ - off) return;
    auto nx = free_.lower_bound(off);  // the first free block at or behind off
    if (nx != free_.end() && nx->first - off < bytes) return;
    if (nx != free_.begin()) {
      auto pv = std::prev(nx);
      if (pv->first + pv->second > off) return;
      if (pv->first + pv->second == off) {  // grows the block in front
        pv->second += bytes;
        if (nx != free_.end() && pv->first + pv->second == nx->first) {
          pv->second += nx->second;
          free_.erase(nx);
        }
        return;
      }
    }
    if (nx != free_.end() && off + bytes == nx->first) {
      bytes += nx->second;
      free_.erase(nx);
    }
    free_[off] = bytes;
  }

  // the list as it stands (tests, oi_test_engine_arena)
  size_t free_bytes() const {
    size_t b = 0;
    for (const auto& kv : free_) b += kv.second;
    return b;
  }
  size_t largest_free() const {
    size_t b = 0;
    for (const auto& kv : free_) b = kv.second > b ? kv.second : b;
    return b;
  }
  const std::map<size_t, size_t>& blocks() const { return free_; }

 private:
  size_t size_ = 0;
  std::map<size_t, size_t> free_;  // offset -> length, disjoint, never adjacent
};
