// wholegraph_amd — the limits and the tile of `rank_rows` and `topk_rows` (wholegraph_amd_ext.h sections 2w and 2x), shared by
// the entry points (rank.cpp) and the kernels (kernels/rank.hip, kernels/topk.hip, kernels/rank_tile.cuh).
#pragma once
#include <cstdint>

namespace wm {

constexpr int kRankMeasures = 3;   // 0 dot, 1 l1, 2 l2

// the sweep's tile: a workgroup of 256 lanes scores kRankEntityTile table rows against kRankQueryTile queries, kRankSlice
// columns at a time. The table is read ceil(n_queries / kRankQueryTile) times.
constexpr int kRankEntityTile = 256;
constexpr int kRankQueryTile  = 64;
constexpr int kRankSlice      = 32;

// `topk_rows` (section 2x, kernels/topk.hip): the most rows a call returns per query, which is also the length of a query's
// running top and of a split's partial result (one key per lane of a wave), and the most rows of a call's range (the row's
// position in the range is the low word of its key)
constexpr int kTopkMax           = 64;
constexpr int64_t kTopkMaxRange  = INT64_C(1) << 31;

// what the entry point requires of the sizes: a batch below 2^31 - 1 queries (as every batch of the library) and a row of
// at least one column
inline bool rank_sizes_ok(int64_t n_queries, int64_t dim) { return n_queries >= 0 && n_queries < (INT64_C(1) << 31) - 1 && dim >= 1; }

}  // namespace wm
