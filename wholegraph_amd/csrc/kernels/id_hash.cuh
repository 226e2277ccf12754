// wholegraph_amd — the hash of a node id, shared by the open-addressing tables that are keyed by one (graph.hip:
// append_unique's table; isub.hip: the membership table of the induced subgraph). The low bits pick the slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wm {

__device__ __forceinline__ uint32_t au_hash(uint64_t k)
{
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 29;
  return static_cast<uint32_t>(k);
}

}  // namespace wm
