// Host helpers of the stream blocks' launch and *_layout functions.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace t2 {

// workgroups for `work` items at per_block each: at least one, at most `most`
inline uint32_t blocks_for(uint32_t work, uint32_t per_block, uint32_t most) {
  return std::min(most, std::max<uint32_t>(1, (work + per_block - 1) / per_block));
}

// carves a scratch allocation into 256-byte-aligned arrays: take(ptr, count) sets ptr (null where base is null: a
// sizing pass) and moves on; at is the size so far
struct LayoutTaker {
  void *base;
  size_t at = 0;
  template <class E>
  void operator()(E *&ptr, size_t count) {
    at = (at + 255) & ~(size_t)255;
    ptr = base ? (E *)((char *)base + at) : nullptr;
    at += count * sizeof(E);
  }
};

}  // namespace t2
