// wholegraph_amd — element reads through a global reference, shared by the units that walk a CSR graph held in WholeMemory
// (graph.hip: the samplers; walk.hip: random walks). A CONTINUOUS tensor, a plain device array and one rank's view are a
// base pointer (stride 0); a CHUNKED tensor is an array of per-rank pointers, cut at a fixed stride (same_chunk) or at
// rank_offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <wholememory/global_reference.h>

namespace wm {

struct gref_view {
  char* base;
  char* const* rank_ptrs;
  const size_t* rank_offsets;
  size_t chunk_stride;
  int world_size;
  int same_chunk;
};

inline gref_view make_view(const wholememory_gref_t& g)
{
  gref_view v{};
  v.chunk_stride = g.stride;
  v.world_size   = g.world_size;
  v.same_chunk   = g.same_chunk ? 1 : 0;
  if (g.stride == 0) {
    v.base = static_cast<char*>(g.pointer);
  } else {
    v.rank_ptrs    = static_cast<char* const*>(g.pointer);
    v.rank_offsets = g.rank_memory_offsets;
  }
  return v;
}

template <typename T>
__device__ __forceinline__ T gref_load(const gref_view& v, int64_t elem_index)
{
  const size_t off = static_cast<size_t>(elem_index) * sizeof(T);
  if (v.chunk_stride == 0) return *reinterpret_cast<const T*>(v.base + off);
  int rank;
  size_t start;
  if (v.same_chunk) {
    rank  = static_cast<int>(off / v.chunk_stride);
    start = static_cast<size_t>(rank) * v.chunk_stride;
  } else {
    rank = 0;
    for (int r = 1; r < v.world_size; r++)
      if (off >= v.rank_offsets[r]) rank = r;
    start = v.rank_offsets[rank];
  }
  return *reinterpret_cast<const T*>(v.rank_ptrs[rank] + (off - start));
}

}  // namespace wm
