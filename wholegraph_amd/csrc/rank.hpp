// wholegraph_amd — the limits and the tile of `rank_rows` (wholegraph_amd_ext.h section 2w), shared by the entry point
// (rank.cpp) and the kernels (kernels/rank.hip).
#pragma once
#include <cstdint>

namespace wm {

constexpr int kRankMeasures = 3;   // 0 dot, 1 l1, 2 l2

// the sweep's tile: a workgroup of 256 lanes scores kRankEntityTile table rows against kRankQueryTile queries, kRankSlice
// columns at a time. The table is read ceil(n_queries / kRankQueryTile) times.
constexpr int kRankEntityTile = 256;
constexpr int kRankQueryTile  = 64;
constexpr int kRankSlice      = 32;

// what the entry point requires of the sizes: a batch below 2^31 - 1 queries (as every batch of the library) and a row of
// at least one column
inline bool rank_sizes_ok(int64_t n_queries, int64_t dim) { return n_queries >= 0 && n_queries < (INT64_C(1) << 31) - 1 && dim >= 1; }

}  // namespace wm
