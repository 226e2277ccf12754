// wholegraph_amd — the running top-G of a group of G lanes, shared by the units that select the largest keys of a row without
// LDS (graph.hip: sample_weighted_small_kernel, a 64-bit key; tsample.hip, tysample.hip and labor.hip: a two-word key; rwr.hip:
// a 64-bit key). The key type K has top_key_max, top_key_min and top_key_xor (the key of the lane j away): those of uint64_t and of
// tsample.hpp's ts_key are here.
// Lane i of the group holds the i-th largest key seen so far; a batch of G keys, one per lane, is sorted across the lanes
// (bitonic network of shuffles) and merged: top[i] = max(top[i], batch[G - 1 - i]) holds the G largest of both as a bitonic
// sequence, which log2 G compare-exchanges put back in descending order. All lanes of a group call this together.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../tsample.hpp"

namespace wm {

__device__ __forceinline__ uint64_t top_key_max(uint64_t a, uint64_t b) { return max(a, b); }
__device__ __forceinline__ uint64_t top_key_min(uint64_t a, uint64_t b) { return min(a, b); }
__device__ __forceinline__ uint64_t top_key_xor(uint64_t a, int j) { return __shfl_xor(static_cast<unsigned long long>(a), j, 64); }

// the two-word key of tsample.hpp (tsample.hip, tysample.hip)
__device__ __forceinline__ ts_key top_key_max(ts_key a, ts_key b) { return ts_key_max(a, b); }
__device__ __forceinline__ ts_key top_key_min(ts_key a, ts_key b) { return ts_key_min(a, b); }
__device__ __forceinline__ ts_key top_key_xor(ts_key a, int j)
{
  return {__shfl_xor(static_cast<unsigned long long>(a.hi), j, 64), __shfl_xor(a.lo, j, 64)};
}

template <int G, typename K>
__device__ __forceinline__ K top_merge(K top, K b, int gl)
{
#pragma unroll
  for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const K o           = top_key_xor(b, j);
      const bool keep_max = ((gl & k) == 0) == ((gl & j) == 0);   // descending where (gl & k) == 0; k == G: everywhere
      b                   = keep_max ? top_key_max(b, o) : top_key_min(b, o);
    }
  }
  const K r = top_key_xor(b, G - 1);   // the batch in ascending order
  top       = top_key_max(top, r);
#pragma unroll
  for (int j = G >> 1; j > 0; j >>= 1) {
    const K o = top_key_xor(top, j);
    top       = (gl & j) == 0 ? top_key_max(top, o) : top_key_min(top, o);
  }
  return top;
}

// The sibling that keeps BOTH halves (tysample.hip: a key of two fields, relation above draw, where the largest G of the 2G
// are not the answer and every element's place in the whole order is needed). In: top in descending order, b in any order.
// Out: top ++ b is the descending order of all 2G keys — top the G largest, b the G smallest, each descending. The max half is
// top_merge's; the min half of the same comparison is bitonic as well and takes the same log2 G compare-exchanges.
template <int G, typename K>
__device__ __forceinline__ void top_merge_both(K& top, K& b, int gl)
{
#pragma unroll
  for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const K o           = top_key_xor(b, j);
      const bool keep_max = ((gl & k) == 0) == ((gl & j) == 0);
      b                   = keep_max ? top_key_max(b, o) : top_key_min(b, o);
    }
  }
  const K r = top_key_xor(b, G - 1);   // the batch in ascending order
  b         = top_key_min(top, r);
  top       = top_key_max(top, r);
#pragma unroll
  for (int j = G >> 1; j > 0; j >>= 1) {
    const K o = top_key_xor(top, j), q = top_key_xor(b, j);
    top       = (gl & j) == 0 ? top_key_max(top, o) : top_key_min(top, o);
    b         = (gl & j) == 0 ? top_key_max(b, q) : top_key_min(b, q);
  }
}

// v of the G lanes of a group in ascending order, lane 0 the smallest (the winners' positions, which is the output order)
template <int G>
__device__ __forceinline__ uint32_t top_sort_ascending(uint32_t v, int gl)
{
#pragma unroll
  for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint32_t o    = __shfl_xor(v, j, 64);
      const bool keep_min = ((gl & k) == 0) == ((gl & j) == 0);   // ascending where (gl & k) == 0; k == G: everywhere
      v                   = keep_min ? min(v, o) : max(v, o);
    }
  }
  return v;
}

}  // namespace wm
