// wholegraph_amd — host side of `rank_rows` (wholegraph_amd_ext.h, section 2w): validation in the order the header states,
// the scratch of the thresholds and the three launches of kernels/rank.hip (threshold, sweep, filter correction). The
// semantics, and the one order of every fp32 sum, are stated in the header.
#include <wholememory/wholegraph_amd_ext.h>
#include <wholememory/wholememory_tensor.h>

#include "csr_graph.hpp"
#include "rank.hpp"

namespace {

using namespace wm;

// a tensor of `dim` dimensions: nullptr and another rank are INVALID_INPUT
bool tensor_of(wholememory_tensor_t t, int dim, const char* what, wholememory_tensor_description_t* out)
{
  if (t == nullptr) {
    WM_ERROR("%s is null", what);
    return false;
  }
  *out = *wholememory_tensor_get_tensor_description(t);
  if (out->dim != dim) {
    WM_ERROR("%s must be a %d-D tensor, got %d dimensions", what, dim, out->dim);
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

wholememory_error_code_t wholememory_ext_rank_rows(wholememory_tensor_t table_tensor, wholememory_tensor_t query_tensor,
                                                   wholememory_tensor_t target_tensor, int measure, int64_t entity_begin,
                                                   int64_t entity_end, wholememory_tensor_t filter_row_ptr_tensor,
                                                   wholememory_tensor_t filter_ids_tensor, wholememory_tensor_t greater_tensor,
                                                   wholememory_tensor_t equal_tensor, wholememory_env_func_t* p_env_fns,
                                                   void* stream)
{
  WM_API_BEGIN
  // (a) what must be there, and ranks
  if (p_env_fns == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  wholememory_tensor_description_t table, query, target, greater, equal, frow{}, fids{};
  if (!tensor_of(table_tensor, 2, "table", &table) || !tensor_of(query_tensor, 2, "query", &query) ||
      !tensor_of(target_tensor, 1, "target", &target) || !tensor_of(greater_tensor, 1, "greater", &greater) ||
      !tensor_of(equal_tensor, 1, "equal", &equal))
    return WHOLEMEMORY_INVALID_INPUT;
  const bool filtered = filter_row_ptr_tensor != nullptr;
  if (filtered != (filter_ids_tensor != nullptr)) {
    WM_ERROR("filter_row_ptr and filter_ids come together or not at all");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (filtered && (!tensor_of(filter_row_ptr_tensor, 1, "filter_row_ptr", &frow) || !tensor_of(filter_ids_tensor, 1, "filter_ids", &fids)))
    return WHOLEMEMORY_INVALID_INPUT;
  // (b) sizes and scalars
  const int64_t N = table.sizes[0], F = table.sizes[1], B = query.sizes[0];
  if (!rank_sizes_ok(B, F)) {
    WM_ERROR("%ld queries of %ld columns: fewer than 2^31 - 1 queries, at least one column", static_cast<long>(B), static_cast<long>(F));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (table.strides[1] != 1 || query.strides[1] != 1 || table.strides[0] < F || query.sizes[1] < F || query.strides[0] < F) {
    WM_ERROR("rows must be contiguous, a table row stride and a query row (and its stride) at least %ld columns", static_cast<long>(F));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (target.sizes[0] != B || greater.sizes[0] < B || equal.sizes[0] < B || target.strides[0] != 1 || greater.strides[0] != 1 ||
      equal.strides[0] != 1) {
    WM_ERROR("target needs %ld entries, greater and equal at least as many, all unit-stride", static_cast<long>(B));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (entity_begin < 0 || entity_begin > entity_end || entity_end > N) {
    WM_ERROR("the range [%ld, %ld) must lie in [0, %ld]", static_cast<long>(entity_begin), static_cast<long>(entity_end), static_cast<long>(N));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (measure < 0 || measure >= kRankMeasures) {
    WM_ERROR("measure must be 0 (dot), 1 (l1) or 2 (l2), got %d", measure);
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (filtered && (frow.sizes[0] != B + 1 || frow.strides[0] != 1 || (fids.sizes[0] > 0 && fids.strides[0] != 1))) {
    WM_ERROR("filter_row_ptr needs %ld entries; both filter tensors unit-stride", static_cast<long>(B + 1));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  // (c) dtypes
  if (table.dtype != WHOLEMEMORY_DT_FLOAT || query.dtype != WHOLEMEMORY_DT_FLOAT) {
    WM_ERROR("table and query must be float32");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  if (!is_index_dtype(target.dtype) || greater.dtype != WHOLEMEMORY_DT_INT64 || equal.dtype != WHOLEMEMORY_DT_INT64) {
    WM_ERROR("target must be int32 or int64, greater and equal int64");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  if (filtered && (!is_index_dtype(frow.dtype) || fids.dtype != target.dtype)) {
    WM_ERROR("filter_row_ptr must be int32 or int64, filter_ids of target's dtype");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  // (d) placement
  const csr_placement where = placement_of({table_tensor});
  if (where == csr_placement::hierarchy) {
    WM_ERROR("Memory type not supported.");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (where == csr_placement::distributed) {
    WM_ERROR("rank_rows on a DISTRIBUTED table is not implemented: rank the local rows per rank (entity_begin, entity_end) and add the counts");
    return WHOLEMEMORY_NOT_IMPLEMENTED;
  }
  const auto* bk = backend();
  if (bk->rank_threshold == nullptr || bk->rank_sweep == nullptr || bk->rank_filter == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (B == 0) return WHOLEMEMORY_SUCCESS;

  wm_rank_args a{};
  WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(table_tensor, &a.gref));
  a.table_rows           = N;
  a.table_stride         = table.strides[0];
  a.table_storage_offset = table.storage_offset;
  a.dim                  = F;
  a.query                = static_cast<const float*>(wholememory_tensor_get_data_pointer(query_tensor));
  a.query_stride         = query.strides[0];
  a.n_queries            = B;
  a.target               = wholememory_tensor_get_data_pointer(target_tensor);
  a.id_dtype             = target.dtype;
  a.measure              = measure;
  a.entity_begin         = entity_begin;
  a.entity_end           = entity_end;
  a.greater              = static_cast<int64_t*>(wholememory_tensor_get_data_pointer(greater_tensor));
  a.equal                = static_cast<int64_t*>(wholememory_tensor_get_data_pointer(equal_tensor));
  if (a.query == nullptr || a.target == nullptr || a.greater == nullptr || a.equal == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  if (filtered) {
    a.filter_row_ptr       = wholememory_tensor_get_data_pointer(filter_row_ptr_tensor);
    a.filter_row_ptr_dtype = frow.dtype;
    a.filter_ids           = wholememory_tensor_get_data_pointer(filter_ids_tensor);
    a.n_filter             = fids.sizes[0];
    if (a.filter_row_ptr == nullptr || (a.n_filter > 0 && a.filter_ids == nullptr)) return WHOLEMEMORY_INVALID_INPUT;
  }
  temp_mem thr_mem(p_env_fns);
  a.thr = static_cast<float*>(thr_mem.device(B, WHOLEMEMORY_DT_FLOAT));
  if (a.thr == nullptr) return WHOLEMEMORY_OUT_OF_MEMORY;
  WM_BK(bk->rank_threshold(&a, stream));
  WM_BK(bk->rank_sweep(&a, stream));
  WM_BK(bk->rank_filter(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

}  // extern "C"
