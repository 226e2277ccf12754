// wholegraph_amd — host side of `rank_rows` and `topk_rows` (wholegraph_amd_ext.h, sections 2w and 2x): validation in the
// order the header states (the part over the table, the queries, the range and the filter block is one set of helpers), the
// scratch and the launches of kernels/rank.hip (threshold, sweep, filter correction) and kernels/topk.hip (sweep, merge). The
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


// what rank_rows and topk_rows share: the table, the queries, the range, the measure and the optional filter block, checked
// in the four stages of the header's error order. Each op answers a stage's own tensors next to the shared ones
struct rank_operand_descs {
  wholememory_tensor_description_t table, query, frow{}, fids{};
  bool filtered;
  int64_t N, F, B;
};

// (a) what must be there, and ranks
bool operands_present(wholememory_tensor_t table_tensor, wholememory_tensor_t query_tensor, wholememory_tensor_t filter_row_ptr_tensor,
                      wholememory_tensor_t filter_ids_tensor, wholememory_env_func_t* p_env_fns, rank_operand_descs* d)
{
  if (p_env_fns == nullptr) return false;
  if (!tensor_of(table_tensor, 2, "table", &d->table) || !tensor_of(query_tensor, 2, "query", &d->query)) return false;
  d->filtered = filter_row_ptr_tensor != nullptr;
  if (d->filtered != (filter_ids_tensor != nullptr)) {
    WM_ERROR("filter_row_ptr and filter_ids come together or not at all");
    return false;
  }
  if (d->filtered && (!tensor_of(filter_row_ptr_tensor, 1, "filter_row_ptr", &d->frow) || !tensor_of(filter_ids_tensor, 1, "filter_ids", &d->fids)))
    return false;
  d->N = d->table.sizes[0], d->F = d->table.sizes[1], d->B = d->query.sizes[0];
  return true;
}

// (b) sizes and scalars, in two halves around the op's own tensors
bool operand_rows_ok(const rank_operand_descs& d)
{
  const auto &table = d.table, &query = d.query;
  const int64_t F = d.F;
  if (!rank_sizes_ok(d.B, F)) {
    WM_ERROR("%ld queries of %ld columns: fewer than 2^31 - 1 queries, at least one column", static_cast<long>(d.B), static_cast<long>(F));
    return false;
  }
  if (table.strides[1] != 1 || query.strides[1] != 1 || table.strides[0] < F || query.sizes[1] < F || query.strides[0] < F) {
    WM_ERROR("rows must be contiguous, a table row stride and a query row (and its stride) at least %ld columns", static_cast<long>(F));
    return false;
  }
  return true;
}
bool operand_scalars_ok(const rank_operand_descs& d, int64_t entity_begin, int64_t entity_end, int measure)
{
  if (entity_begin < 0 || entity_begin > entity_end || entity_end > d.N) {
    WM_ERROR("the range [%ld, %ld) must lie in [0, %ld]", static_cast<long>(entity_begin), static_cast<long>(entity_end), static_cast<long>(d.N));
    return false;
  }
  if (measure < 0 || measure >= kRankMeasures) {
    WM_ERROR("measure must be 0 (dot), 1 (l1) or 2 (l2), got %d", measure);
    return false;
  }
  if (d.filtered && (d.frow.sizes[0] != d.B + 1 || d.frow.strides[0] != 1 || (d.fids.sizes[0] > 0 && d.fids.strides[0] != 1))) {
    WM_ERROR("filter_row_ptr needs %ld entries; both filter tensors unit-stride", static_cast<long>(d.B + 1));
    return false;
  }
  return true;
}

// (c) dtypes of the table and the queries
bool operand_dtypes_ok(const rank_operand_descs& d)
{
  if (d.table.dtype != WHOLEMEMORY_DT_FLOAT || d.query.dtype != WHOLEMEMORY_DT_FLOAT) {
    WM_ERROR("table and query must be float32");
    return false;
  }
  return true;
}

// (d) placement
wholememory_error_code_t table_placement(wholememory_tensor_t table_tensor, const char* op, const char* pieces)
{
  const csr_placement where = placement_of({table_tensor});
  if (where == csr_placement::hierarchy) {
    WM_ERROR("Memory type not supported.");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (where == csr_placement::distributed) {
    WM_ERROR("%s on a DISTRIBUTED table is not implemented: %s", op, pieces);
    return WHOLEMEMORY_NOT_IMPLEMENTED;
  }
  return WHOLEMEMORY_SUCCESS;
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
  rank_operand_descs d;
  wholememory_tensor_description_t target, greater, equal;
  if (!operands_present(table_tensor, query_tensor, filter_row_ptr_tensor, filter_ids_tensor, p_env_fns, &d) ||
      !tensor_of(target_tensor, 1, "target", &target) || !tensor_of(greater_tensor, 1, "greater", &greater) ||
      !tensor_of(equal_tensor, 1, "equal", &equal))
    return WHOLEMEMORY_INVALID_INPUT;
  const auto &table = d.table, &query = d.query, &frow = d.frow, &fids = d.fids;
  const bool filtered = d.filtered;
  // (b) sizes and scalars
  const int64_t N = d.N, F = d.F, B = d.B;
  if (!operand_rows_ok(d)) return WHOLEMEMORY_INVALID_INPUT;
  if (target.sizes[0] != B || greater.sizes[0] < B || equal.sizes[0] < B || target.strides[0] != 1 || greater.strides[0] != 1 ||
      equal.strides[0] != 1) {
    WM_ERROR("target needs %ld entries, greater and equal at least as many, all unit-stride", static_cast<long>(B));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (!operand_scalars_ok(d, entity_begin, entity_end, measure)) return WHOLEMEMORY_INVALID_INPUT;
  // (c) dtypes
  if (!operand_dtypes_ok(d)) return WHOLEMEMORY_LOGIC_ERROR;
  if (!is_index_dtype(target.dtype) || greater.dtype != WHOLEMEMORY_DT_INT64 || equal.dtype != WHOLEMEMORY_DT_INT64) {
    WM_ERROR("target must be int32 or int64, greater and equal int64");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  if (filtered && (!is_index_dtype(frow.dtype) || fids.dtype != target.dtype)) {
    WM_ERROR("filter_row_ptr must be int32 or int64, filter_ids of target's dtype");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  // (d) placement
  WHOLEMEMORY_RETURN_ON_FAIL(table_placement(table_tensor, "rank_rows", "rank the local rows per rank (entity_begin, entity_end) and add the counts"));
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

wholememory_error_code_t wholememory_ext_topk_rows(wholememory_tensor_t table_tensor, wholememory_tensor_t query_tensor, int k,
                                                   int measure, int64_t entity_begin, int64_t entity_end,
                                                   wholememory_tensor_t filter_row_ptr_tensor, wholememory_tensor_t filter_ids_tensor,
                                                   wholememory_tensor_t ids_tensor, wholememory_tensor_t scores_tensor,
                                                   wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  // (a) what must be there, and ranks
  rank_operand_descs d;
  wholememory_tensor_description_t ids, scores;
  if (!operands_present(table_tensor, query_tensor, filter_row_ptr_tensor, filter_ids_tensor, p_env_fns, &d) ||
      !tensor_of(ids_tensor, 2, "ids", &ids) || !tensor_of(scores_tensor, 2, "scores", &scores))
    return WHOLEMEMORY_INVALID_INPUT;
  // (b) sizes and scalars
  const int64_t B = d.B;
  if (!operand_rows_ok(d)) return WHOLEMEMORY_INVALID_INPUT;
  if (k < 1 || k > kTopkMax) {
    WM_ERROR("k must lie in 1 .. %d, got %d", kTopkMax, k);
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (ids.sizes[0] != B || ids.sizes[1] != k || scores.sizes[0] != B || scores.sizes[1] != k || ids.strides[1] != 1 ||
      scores.strides[1] != 1 || ids.strides[0] < k || scores.strides[0] < k) {
    WM_ERROR("ids and scores must be [%ld, %d] with contiguous rows", static_cast<long>(B), k);
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (!operand_scalars_ok(d, entity_begin, entity_end, measure)) return WHOLEMEMORY_INVALID_INPUT;
  if (entity_end - entity_begin > kTopkMaxRange) {
    WM_ERROR("a call covers at most 2^31 rows: sweep a larger range in pieces and merge");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  // (c) dtypes
  if (!operand_dtypes_ok(d)) return WHOLEMEMORY_LOGIC_ERROR;
  if (ids.dtype != WHOLEMEMORY_DT_INT64 || scores.dtype != WHOLEMEMORY_DT_FLOAT) {
    WM_ERROR("ids must be int64 and scores float32");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  if (d.filtered && (!is_index_dtype(d.frow.dtype) || !is_index_dtype(d.fids.dtype))) {
    WM_ERROR("filter_row_ptr and filter_ids must be int32 or int64");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  // (d) placement
  WHOLEMEMORY_RETURN_ON_FAIL(table_placement(table_tensor, "topk_rows", "take the top of the local rows per rank (entity_begin, entity_end) and merge"));
  const auto* bk = backend();
  if (bk->topk_workspace_bytes == nullptr || bk->topk_sweep == nullptr || bk->topk_merge == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (B == 0) return WHOLEMEMORY_SUCCESS;

  wm_topk_args a{};
  WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(table_tensor, &a.gref));
  a.table_rows           = d.N;
  a.table_stride         = d.table.strides[0];
  a.table_storage_offset = d.table.storage_offset;
  a.dim                  = d.F;
  a.query                = static_cast<const float*>(wholememory_tensor_get_data_pointer(query_tensor));
  a.query_stride         = d.query.strides[0];
  a.n_queries            = B;
  a.measure              = measure;
  a.entity_begin         = entity_begin;
  a.entity_end           = entity_end;
  a.k                    = k;
  a.ids                  = static_cast<int64_t*>(wholememory_tensor_get_data_pointer(ids_tensor));
  a.ids_stride           = ids.strides[0];
  a.scores               = static_cast<float*>(wholememory_tensor_get_data_pointer(scores_tensor));
  a.scores_stride        = scores.strides[0];
  if (a.query == nullptr || a.ids == nullptr || a.scores == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  if (d.filtered) {
    a.filter_row_ptr       = wholememory_tensor_get_data_pointer(filter_row_ptr_tensor);
    a.filter_row_ptr_dtype = d.frow.dtype;
    a.filter_ids           = wholememory_tensor_get_data_pointer(filter_ids_tensor);
    a.filter_ids_dtype     = d.fids.dtype;
    a.n_filter             = d.fids.sizes[0];
    if (a.filter_row_ptr == nullptr || (a.n_filter > 0 && a.filter_ids == nullptr)) return WHOLEMEMORY_INVALID_INPUT;
  }
  const size_t bytes = bk->topk_workspace_bytes(&a);
  if (bytes == 0) return WHOLEMEMORY_INVALID_INPUT;
  temp_mem workspace(p_env_fns);
  a.workspace = workspace.device(static_cast<int64_t>(bytes / sizeof(int64_t)), WHOLEMEMORY_DT_INT64);
  if (a.workspace == nullptr) return WHOLEMEMORY_OUT_OF_MEMORY;
  WM_BK(bk->topk_sweep(&a, stream));
  WM_BK(bk->topk_merge(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

}  // extern "C"
