// wholegraph_amd — what the ops over a sampled CSC block share on the host (aggregate.cpp, gat.cpp): the checks of the
// block, the block fields of an args struct and the edge index of a backward.
#pragma once

#include "ops_internal.hpp"

namespace wm {

// col_ind_needed: the op's own rule for when col_ind is read; rows: what the op calls its source rows ("x", "h")
inline void check_block(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                        bool col_ind_needed, const char* rows)
{
  if (n_edges < 0 || n_dst < 0 || n_src < 0) throw invalid_input("negative size");
  if (n_dst > n_src) throw invalid_input(format_string("n_dst > n_src: the targets are the first rows of %s", rows));
  if (row_ptr == nullptr) throw invalid_input("row_ptr is null");
  if (col_ind_needed && col_ind == nullptr) throw invalid_input("col_ind is null");
  if (n_edges >= (int64_t(1) << 31) || n_src >= (int64_t(1) << 31)) throw invalid_input("more than 2^31 - 1 edges or rows");
}

// the block fields of wm_agg_args, wm_agg16_args, wm_aggw_args and wm_gather_agg_args (backend.hpp: equal names)
template <class Args>
Args block_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, int64_t dim,
                int aggr)
{
  Args a{};
  a.row_ptr = row_ptr;
  a.col_ind = col_ind;
  a.n_edges = n_dst == 0 ? 0 : n_edges;   // (no target, no edge of any target)
  a.n_dst   = n_dst;
  a.n_src   = n_src;
  a.dim     = dim;
  a.mean    = aggr == WHOLEMEMORY_EXT_AGGR_MEAN ? 1 : 0;
  return a;
}

// the edge index of a backward: a stable sort of col_ind (runs of one source, edge positions ascending in each run) into
// ix->order / starts / unique (int32) / n_unique_dev. A code left by an earlier sort fails the call (device_error clears it).
// dedup_ids joins any side stream of its own before it returns (no deferred join asked for), so its outputs are ready for
// the kernels queued behind it on `stream`
inline void sort_col_ind(sorted_ids* ix, const int32_t* col_ind, int64_t n_edges, int64_t n_src, void* stream)
{
  const auto* bk = backend();
  if (bk->device_error != nullptr && bk->device_error() != 0)
    throw hip_error("an earlier id sort reported a device-side timeout (see the ERROR line above)");
  ix->run_or_throw(col_ind, WHOLEMEMORY_DT_INT, n_edges, n_src, 0, stream);
}

}  // namespace wm
