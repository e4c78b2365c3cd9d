// ppfit_wsplan.hpp -- the workspace plan of a host entry point: the arrays of
// a chunk of items one after another in one device buffer.  Host arithmetic
// only (no HIP header), so tools/ws_plan_check.cpp builds it with the host
// compiler alone.
#pragma once

#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdint>

namespace ppf {

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// The caller declares the arrays of one item (subint, portrait, row, profile
// or unit) in order, each with its bytes per item, then lays them out for
// nitem items under a byte limit.  Every array starts at a multiple of 256
// bytes, so no two overlap whatever the sizes.
struct WsPlan {
  static constexpr int kMaxArrays = 12;
  int narray = 0;
  size_t per[kMaxArrays];  // bytes per item
  size_t off[kMaxArrays];  // offset in the buffer (lay_out)
  size_t per_item = 0;     // all arrays of one item
  int64_t chunk = 0;       // items per pass
  size_t total = 0;        // bytes of a chunk's arrays, a multiple of 256
  char* base = nullptr;    // the buffer, once it holds them

  // the next array; the value names it in off[], per[] and at()
  int array(size_t bytes_per_item) {
    assert(narray < kMaxArrays);
    per[narray] = bytes_per_item;
    per_item += bytes_per_item;
    return narray++;
  }

  // chunk = the items that fit under limit at per_item + slack bytes each (at
  // least one, at most nitem and, when cap > 0, cap), then the offsets
  void lay_out(int64_t nitem, int64_t limit, size_t slack, int64_t cap = 0) {
    chunk = std::min<int64_t>(nitem, limit / (int64_t)(per_item + slack));
    if (cap > 0) chunk = std::min(chunk, cap);
    chunk = std::max<int64_t>(1, chunk);
    total = 0;
    for (int a = 0; a < narray; ++a) {
      off[a] = total;
      total = align256(total + (size_t)chunk * per[a]);
    }
  }

  // array a's part for the chunk's items item ..
  template <typename P>
  P* at(int a, int64_t item = 0) const {
    return reinterpret_cast<P*>(base + off[a] + (size_t)item * per[a]);
  }
};

}  // namespace ppf
