// wholegraph_amd — how the ops of a sampled CSC block (kernels/agg*.hip, kernels/gat*.hip) lay out a device workspace: a
// list of regions, each starting on a 256-byte boundary, behind a start that the caller may hand over at any address. One
// function gives both the size to allocate and the offsets, so a size function and its carve cannot disagree.
// Standard library only (no backend, no device header): tests/cpp/csc_workspace_test.cpp checks it alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace wm {

inline size_t up256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
inline int64_t up4(int64_t v) { return (v + 3) / 4 * 4; }

template <size_t N>
struct ws_layout {
  size_t off[N];   // where region i starts, from the first 256-byte boundary at or behind the workspace's start
  size_t bytes;    // what to allocate: the regions, and the bytes an unaligned start loses in front of them
};

template <size_t N>
ws_layout<N> ws_plan(const int64_t (&sizes)[N])   // sizes in bytes; an empty region takes no room
{
  ws_layout<N> l;
  size_t w = 0;
  for (size_t i = 0; i < N; ++i) {
    l.off[i] = w;
    w        = up256(w + static_cast<size_t>(sizes[i]));
  }
  l.bytes = w + 256;
  return l;
}

// the region at `off` (ws_layout::off) of the workspace that starts at `workspace`
template <class T>
T* ws_at(void* workspace, size_t off)
{
  return reinterpret_cast<T*>(up256(reinterpret_cast<uintptr_t>(workspace)) + off);
}

// the agg_concat backward (all row types, the weighted and the relation-typed op): sorted_dst [n_edges] int32, run_of
// [n_src] int32, then the fp32 partial rows [n_tiles, partial_stride] of the chunks of `chunk_edges` edges
struct agg_bwd_layout {
  int64_t n_tiles, partial_stride;
  ws_layout<3> ws;
};

inline agg_bwd_layout agg_bwd_plan(int64_t n_edges, int64_t n_src, int64_t dim, int64_t chunk_edges)
{
  agg_bwd_layout l;
  l.n_tiles              = (n_edges + chunk_edges - 1) / chunk_edges;
  l.partial_stride       = up4(dim);
  const int64_t sizes[3] = {n_edges * 4, n_src * 4, l.n_tiles * l.partial_stride * 4};
  l.ws                   = ws_plan(sizes);
  return l;
}

}  // namespace wm
