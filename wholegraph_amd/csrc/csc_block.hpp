// wholegraph_amd — what the ops over a sampled CSC block share on the host (aggregate.cpp, gat.cpp): the checked block, the
// checks of row tensors and heads, and the two call sequences (a forward with a workspace; a backward with the edge index
// and a workspace). Every entry point judges its arguments first, then the backend's capability, then (where there is a
// table) the table's memory type: a malformed call is INVALID_INPUT under every backend.
#pragma once

#include "ops_internal.hpp"

namespace wm {

// the block of an op's args, checked. col_ind_needed: the op's own rule for when col_ind is read; rows: what the op calls
// its source rows ("x", "h"). targets_among_sources: the targets are the first n_dst of the source rows (every op but the
// edge dot product, whose targets have rows of their own and may outnumber the sources)
inline wm_csc_block checked_block(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst,
                                  int64_t n_src, bool col_ind_needed, const char* rows, bool targets_among_sources = true)
{
  if (n_edges < 0 || n_dst < 0 || n_src < 0) throw invalid_input("negative size");
  if (targets_among_sources && n_dst > n_src)
    throw invalid_input(format_string("n_dst > n_src: the targets are the first rows of %s", rows));
  if (n_dst >= (int64_t(1) << 31)) throw invalid_input("more than 2^31 - 1 targets");
  if (row_ptr == nullptr) throw invalid_input("row_ptr is null");
  if (col_ind_needed && col_ind == nullptr) throw invalid_input("col_ind is null");
  if (n_edges >= (int64_t(1) << 31) || n_src >= (int64_t(1) << 31)) throw invalid_input("more than 2^31 - 1 edges or rows");
  return {row_ptr, col_ind, n_dst == 0 ? 0 : n_edges, n_dst, n_src};   // (no target, no edge of any target)
}

// a row tensor: present when the op reads or writes it, its stride at least the `row` columns in use
inline void check_rows(const void* p, bool needed, int64_t stride, int64_t row, const char* what)
{
  if (needed && p == nullptr) throw invalid_input(format_string("%s is null", what));
  if (stride < row) throw invalid_input(format_string("%s stride smaller than its row", what));
}

// heads and dim of an attention op; returns heads * dim, which stays below the op's `limit`
inline int64_t checked_heads(int64_t heads, int64_t dim, int64_t limit)
{
  if (heads < 1) throw invalid_input("heads must be >= 1");
  if (dim < 1) throw invalid_input("dim must be >= 1");
  if (heads * dim >= limit) throw invalid_input("heads * dim too large");
  return heads * dim;
}

// out / grad_out of an attention op: [n_dst, heads * dim] with concat, else the mean over heads, [n_dst, dim]
inline void check_out_rows(const void* p, int64_t stride, int64_t n_dst, int concat, int64_t heads, int64_t dim,
                           const char* what)
{
  check_rows(p, n_dst > 0, stride, concat ? heads * dim : dim, what);
}

inline void check_env(const wholememory_env_func_t* p_env_fns)
{
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
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

// a forward with scratch: launch(workspace), the workspace of `ws_bytes` (none asked for when 0: nullptr)
template <class Launch>
void forward_with_workspace(size_t ws_bytes, wholememory_env_func_t* p_env_fns, Launch launch)
{
  temp_mem ws(p_env_fns);
  launch(ws_bytes > 0 ? ws.device(static_cast<int64_t>(ws_bytes), WHOLEMEMORY_DT_INT8) : nullptr);
}

// a backward: launch(ix, workspace). The edge index is built when `wants_index` (the op's own rule: which of its gradients
// walk the sources) and the block has source rows, and is all null otherwise; the workspace is of `ws_bytes`
template <class Launch>
void backward_over_index(const wm_csc_block& b, bool wants_index, size_t ws_bytes, wholememory_env_func_t* p_env_fns,
                         void* stream, Launch launch)
{
  sorted_ids ids(p_env_fns);
  temp_mem ws(p_env_fns);
  wm_edge_index ix{};
  if (wants_index && b.n_src > 0) {
    sort_col_ind(&ids, b.col_ind, b.n_edges, b.n_src, stream);
    ix = {ids.order, ids.starts, static_cast<const int32_t*>(ids.unique), ids.n_unique_dev};
  }
  launch(ix, ws.device(static_cast<int64_t>(ws_bytes), WHOLEMEMORY_DT_INT8));
}

}  // namespace wm
