// wholegraph_amd — the running top-G of a group of G lanes, shared by the units that select the largest keys of a row without
// LDS (graph.hip: sample_weighted_small_kernel, a 64-bit key; tsample.hip: a two-word key). The key type K brings
// top_key_max, top_key_min and top_key_xor (the key of the lane j away) with it; those of uint64_t are here. Lane i of the
// group holds the i-th largest key seen so far; a batch of G keys, one per lane, is sorted across the lanes (bitonic network
// of shuffles) and merged: top[i] = max(top[i], batch[G - 1 - i]) holds the G largest of both as a bitonic sequence, which
// log2 G compare-exchanges put back in descending order. All lanes of a group call this together.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wm {

__device__ __forceinline__ uint64_t top_key_max(uint64_t a, uint64_t b) { return max(a, b); }
__device__ __forceinline__ uint64_t top_key_min(uint64_t a, uint64_t b) { return min(a, b); }
__device__ __forceinline__ uint64_t top_key_xor(uint64_t a, int j) { return __shfl_xor(static_cast<unsigned long long>(a), j, 64); }

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

}  // namespace wm
