// wholegraph_amd — what the ops over the WholeMemory CSR graph share on the host (graph_ops.cpp: the two samplers, the fused
// hop, the multi-hop chain, the random walks, the node2vec walks, negative sampling, the induced subgraph, the temporal sampler):
// the graph tensors of
// one call, checked, and the one place that turns them into the backend's wm_csr_graph. The checks are separate steps because
// every entry point keeps its own ORDER of answers (the samplers judge placement before dtypes before sizes, as the reference
// does; the walks, the negatives, the induced subgraph and the temporal sampler judge shapes and sizes before dtypes before
// placement: wholegraph_amd_ext.h sections 2m - 2o, 2q and 2r), and a call with two faults gets the answer of the step its entry
// makes first.
#pragma once

#include <initializer_list>

#include "ops_internal.hpp"

namespace wm {

// a 1-D tensor as an array: nullptr and not 1-D are INVALID_INPUT, a description that does not convert is LOGIC_ERROR
inline bool array_of(wholememory_tensor_t t, const char* what, wholememory_array_description_t* out, wholememory_error_code_t* err)
{
  if (t == nullptr) {
    *err = WHOLEMEMORY_INVALID_INPUT;
    return false;
  }
  auto desc = *wholememory_tensor_get_tensor_description(t);
  auto* td  = &desc;
  if (td->dim != 1) {
    WM_ERROR("%s should be 1D tensor.", what);
    *err = WHOLEMEMORY_INVALID_INPUT;
    return false;
  }
  if (!wholememory_convert_tensor_desc_to_array(out, td)) {
    WM_ERROR("%s convert to array failed.", what);
    *err = WHOLEMEMORY_LOGIC_ERROR;
    return false;
  }
  return true;
}

inline bool is_index_dtype(wholememory_dtype_t d) { return d == WHOLEMEMORY_DT_INT || d == WHOLEMEMORY_DT_INT64; }

inline wholememory_memory_type_t memory_type_of(wholememory_tensor_t t)
{
  if (!wholememory_tensor_has_handle(t)) return WHOLEMEMORY_MT_NONE;
  return wholememory_get_memory_type(wholememory_tensor_get_memory_handle(t));
}

// where the tensors of an op lie, the worst of them: mapped into this rank (CONTINUOUS, CHUNKED, a plain device array), or
// reachable through a gather only, or not at all
enum class csr_placement { mapped, distributed, hierarchy };
inline csr_placement placement_of(std::initializer_list<wholememory_tensor_t> tensors)
{
  csr_placement worst = csr_placement::mapped;
  for (wholememory_tensor_t t : tensors) {
    if (t == nullptr) continue;
    const auto mt = memory_type_of(t);
    if (mt == WHOLEMEMORY_MT_HIERARCHY) return csr_placement::hierarchy;
    if (mt == WHOLEMEMORY_MT_DISTRIBUTED) worst = csr_placement::distributed;
  }
  return worst;
}

enum class csr_tensors { row_col, weights, all, row_col_time };   // which of a graph's tensors a placement step judges

// The graph tensors of one call. Every step answers SUCCESS or what is wrong; the plain ops report it (the code the step
// names, with a message), the fused hop and the chain DECLINE it (`declines`: NOT_SUPPORTED, no message — the caller takes
// the two-op route, which reports). What array_of answers is reported either way.
struct checked_graph {
  wholememory_tensor_t row, col, weight;   // weight: nullptr when the call has no weights
  bool declines;
  // per-edge timestamps, set by name after the braces (`g.time = ...`) by the one entry that has them: nullptr otherwise
  wholememory_tensor_t time = nullptr;
  wholememory_array_description_t row_desc{}, col_desc{}, weight_desc{}, time_desc{};

#define WM_CSR_ANSWER(code, ...)                          \
  do {                                                    \
    if (declines) return WHOLEMEMORY_NOT_SUPPORTED;       \
    WM_ERROR(__VA_ARGS__);                                \
    return code;                                          \
  } while (0)

  // (a) the arrays are there, 1-D and convertible
  wholememory_error_code_t arrays()
  {
    wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
    if (!array_of(row, "wm_csr_row_ptr_tensor", &row_desc, &err)) return err;
    if (!array_of(col, "wm_csr_col_ptr_tensor", &col_desc, &err)) return err;
    return WHOLEMEMORY_SUCCESS;
  }
  wholememory_error_code_t weight_array()
  {
    wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
    return array_of(weight, "wm_csr_weight_ptr_tensor", &weight_desc, &err) ? WHOLEMEMORY_SUCCESS : err;
  }

  wholememory_error_code_t time_array()
  {
    wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
    return array_of(time, "wm_csr_edge_time_tensor", &time_desc, &err) ? WHOLEMEMORY_SUCCESS : err;
  }

  // (b)
  wholememory_error_code_t one_time_per_edge() const
  {
    if (time_desc.size != col_desc.size)
      WM_CSR_ANSWER(WHOLEMEMORY_INVALID_INPUT, "wm_csr_edge_time_tensor must have one timestamp per edge (%ld vs %ld)",
                    static_cast<long>(time_desc.size), static_cast<long>(col_desc.size));
    return WHOLEMEMORY_SUCCESS;
  }
  wholememory_error_code_t one_weight_per_edge() const
  {
    if (weight_desc.size != col_desc.size)
      WM_CSR_ANSWER(WHOLEMEMORY_INVALID_INPUT, "wm_csr_weight_ptr_tensor must have one weight per edge (%ld vs %ld)",
                    static_cast<long>(weight_desc.size), static_cast<long>(col_desc.size));
    return WHOLEMEMORY_SUCCESS;
  }

  // (c) the dtype rules of ..._func.cuh:304-314 and the dispatch table of ..._impl_mapped.cu (logic_error there). `ids`: the
  // caller's node ids ("center nodes", "start nodes", ...), which index csr_row_ptr as the columns do
  wholememory_error_code_t row_dtype() const
  {
    if (row_desc.dtype != WHOLEMEMORY_DT_INT64)
      WM_CSR_ANSWER(WHOLEMEMORY_LOGIC_ERROR, "wm_csr_row_ptr_tensor must be int64, got %d", static_cast<int>(row_desc.dtype));
    return WHOLEMEMORY_SUCCESS;
  }
  wholememory_error_code_t col_and_id_dtype(wholememory_dtype_t id_dtype, const char* ids) const
  {
    if (!is_index_dtype(col_desc.dtype) || !is_index_dtype(id_dtype))
      WM_CSR_ANSWER(WHOLEMEMORY_LOGIC_ERROR, "%s and csr_col_ptr must be int32 or int64", ids);
    return WHOLEMEMORY_SUCCESS;
  }
  wholememory_error_code_t weight_dtype() const
  {
    if (weight_desc.dtype != WHOLEMEMORY_DT_FLOAT && weight_desc.dtype != WHOLEMEMORY_DT_DOUBLE)
      WM_CSR_ANSWER(WHOLEMEMORY_LOGIC_ERROR, "wm_csr_weight_ptr_tensor must be float or double");
    return WHOLEMEMORY_SUCCESS;
  }

  wholememory_error_code_t time_dtype() const
  {
    if (time_desc.dtype != WHOLEMEMORY_DT_INT64)
      WM_CSR_ANSWER(WHOLEMEMORY_LOGIC_ERROR, "wm_csr_edge_time_tensor must be int64, got %d", static_cast<int>(time_desc.dtype));
    return WHOLEMEMORY_SUCCESS;
  }

  // (d) HIERARCHY is INVALID_INPUT. DISTRIBUTED is the caller's where it has a gather route (*via_gather says whether to
  // take it), else NOT_IMPLEMENTED with the caller's sentence
  wholememory_error_code_t placement(csr_tensors which, const char* no_route, bool* via_gather = nullptr) const
  {
    const csr_placement p = which == csr_tensors::row_col        ? placement_of({row, col})
                            : which == csr_tensors::weights      ? placement_of({weight})
                            : which == csr_tensors::row_col_time ? placement_of({row, col, time})
                                                                 : placement_of({row, col, weight});
    if (p == csr_placement::hierarchy) WM_CSR_ANSWER(WHOLEMEMORY_INVALID_INPUT, "Memory type not supported.");
    if (via_gather != nullptr) {
      *via_gather = p == csr_placement::distributed;
    } else if (p == csr_placement::distributed) {
      WM_CSR_ANSWER(WHOLEMEMORY_NOT_IMPLEMENTED, "%s", no_route);
    }
    return WHOLEMEMORY_SUCCESS;
  }
#undef WM_CSR_ANSWER

  // (e) the graph as the backend takes it. The arrays of a DISTRIBUTED graph cannot be mapped: their grefs stay empty and the
  // op reaches them through wholememory_gather
  wholememory_error_code_t fill(wm_csr_graph* g) const
  {
    if (placement_of({row, col}) == csr_placement::mapped) {
      WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(row, &g->row_gref));
      WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(col, &g->col_gref));
    }
    g->row_storage_offset = row_desc.storage_offset;
    g->col_storage_offset = col_desc.storage_offset;
    g->col_dtype          = col_desc.dtype;
    g->n_nodes            = row_desc.size - 1;
    g->n_edges            = col_desc.size;
    if (weight != nullptr) {
      WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(weight, &g->weight_gref));
      g->weight_storage_offset = weight_desc.storage_offset;
      g->weight_dtype          = weight_desc.dtype;
    }
    if (time != nullptr) {
      WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(time, &g->time_gref));
      g->time_storage_offset = time_desc.storage_offset;
    }
    return WHOLEMEMORY_SUCCESS;
  }
};

}  // namespace wm
