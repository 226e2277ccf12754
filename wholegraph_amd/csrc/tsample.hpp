// wholegraph_amd — the rules of one temporal neighbour sample over a CSR graph (wholegraph_amd_ext.h section 2r), usable from
// host and device code: when a neighbour is eligible, the key it competes with under either strategy, and the order of two
// keys. kernels/tsample.hip calls these with readers of a WholeMemory tensor, tests/cpp/tsample_test.cpp with plain arrays.
//
// A key is two words, compared hi first: {draw, 0xFFFFFFFF - j} under strategy 0, which is the composite
// (uint64(r) << 32) | (0xFFFFFFFF - j) of section 2r word for word, and {orderable(ts), 0xFFFFFFFF - j} under strategy 1. The
// larger key wins, so in both the tie goes to the lowest j. j < 2^31, so lo of a neighbour's key is never 0: {0, 0} is below
// every key and stands for "none".
#pragma once
#include <cstdint>

#include "pcg.hpp"

namespace wm {

constexpr int kTsampleMaxFanout = 64;   // what the register-held selection takes (a group of lanes holds the running top M)

struct ts_key {
  uint64_t hi;
  uint32_t lo;
};

WM_HD bool ts_key_less(ts_key a, ts_key b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
WM_HD ts_key ts_key_max(ts_key a, ts_key b) { return ts_key_less(a, b) ? b : a; }
WM_HD ts_key ts_key_min(ts_key a, ts_key b) { return ts_key_less(a, b) ? a : b; }

// is the neighbour with timestamp ts eligible for a centre at time t: not later than t (earlier, when !inclusive) and, with a
// window (time_window >= 0), at most time_window before it. With ts <= t the unsigned difference is the exact distance of any
// two int64 values.
WM_HD bool ts_eligible(int64_t ts, int64_t t, int inclusive, int64_t time_window)
{
  if (inclusive != 0 ? ts > t : ts >= t) return false;
  return time_window < 0 || static_cast<uint64_t>(t) - static_cast<uint64_t>(ts) <= static_cast<uint64_t>(time_window);
}

// int64 -> uint64, order-preserving
WM_HD uint64_t ts_orderable(int64_t ts) { return static_cast<uint64_t>(ts) ^ (UINT64_C(1) << 63); }

// strategy 0: the first 32-bit output of stream(seed, i, j + 1) of section 2m, i the centre's position in the batch and j the
// neighbour's position in its row
WM_HD ts_key ts_uniform_key(uint64_t seed, uint64_t i, uint32_t j)
{
  pcg32 g = walk_stream(seed, i, static_cast<uint64_t>(j) + 1);
  return {static_cast<uint64_t>(g.next_u32()), 0xFFFFFFFFu - j};
}
// strategy 1: the latest timestamp
WM_HD ts_key ts_last_key(int64_t ts, uint32_t j) { return {ts_orderable(ts), 0xFFFFFFFFu - j}; }

WM_HD ts_key ts_key_of(int strategy, uint64_t seed, uint64_t i, uint32_t j, int64_t ts)
{
  return strategy == 0 ? ts_uniform_key(seed, i, j) : ts_last_key(ts, j);
}
WM_HD uint32_t ts_key_position(ts_key k) { return 0xFFFFFFFFu - k.lo; }

// what the entry point requires of the scalar arguments
WM_HD bool ts_scalars_ok(int max_sample_count, int strategy)
{
  return max_sample_count <= kTsampleMaxFanout && (strategy == 0 || strategy == 1);
}

// c_i of section 2r from the number of eligible neighbours
WM_HD int64_t ts_count(int64_t eligible, int max_sample_count)
{
  return max_sample_count <= 0 || eligible < max_sample_count ? eligible : max_sample_count;
}

}  // namespace wm
