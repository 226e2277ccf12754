// wholegraph_amd — host side of the relation-typed edge score of a sampled CSC block (wholegraph_amd_ext.h, section 2u):
// validation, the two edge indices of the backward (the library's id sort over col_ind for the per-source rows and over
// edge_type for the relation table, each built only when its gradient is asked for), scratch and the launches of
// kernels/kge.hip. The semantics, and the one order of every fp32 sum, are stated in the header.
#include <wholememory/wholegraph_amd_ext.h>

#include "csc_block.hpp"

namespace {

using namespace wm;

constexpr int64_t kMaxRowKge = (int64_t(1) << 31) / 4;   // dim stays below this, as for (2p)

// what the forward and the backward share: the block, whose targets have rows of their own (the waiver of (2p)), the types,
// the three row tensors and the model
wm_kge_args make_kge_args(const int32_t* row_ptr, const int32_t* col_ind, const int32_t* edge_type, int64_t n_edges,
                          int64_t n_dst, int64_t n_src, int64_t num_relations, const float* x_src, int64_t x_src_stride,
                          const float* x_dst, int64_t x_dst_stride, const float* rel, int64_t rel_stride, int64_t dim,
                          int model, int head_src)
{
  wm_kge_args a{};
  static_cast<wm_csc_block&>(a) =
    checked_block(row_ptr, col_ind, n_edges, n_dst, n_src, n_edges > 0 && n_dst > 0, "x_src", false);
  if (a.n_edges > 0 && edge_type == nullptr) throw invalid_input("edge_type is null");
  if (num_relations < 1 || num_relations >= (int64_t(1) << 31)) throw invalid_input("num_relations must be in [1, 2^31)");
  if (dim < 1 || dim >= kMaxRowKge) throw invalid_input("dim must be in [1, 2^29)");
  if (model < WM_KGE_DISTMULT || model > WM_KGE_ROTATE) throw invalid_input("unknown model");
  if ((model == WM_KGE_COMPLEX || model == WM_KGE_ROTATE) && dim % 2 != 0)
    throw invalid_input("the complex models read a row as [re | im]: dim must be even");
  check_rows(x_src, n_src > 0, x_src_stride, dim, "x_src");
  check_rows(x_dst, n_dst > 0, x_dst_stride, dim, "x_dst");
  check_rows(rel, true, rel_stride, dim, "rel");
  a.edge_type     = edge_type;
  a.dim           = dim;
  a.num_relations = num_relations;
  a.model         = model;
  a.head_src      = head_src ? 1 : 0;
  a.x_src         = x_src;
  a.x_src_stride  = x_src_stride;
  a.x_dst         = x_dst;
  a.x_dst_stride  = x_dst_stride;
  a.rel           = rel;
  a.rel_stride    = rel_stride;
  return a;
}

void check_optional_rows(const void* p, int64_t stride, int64_t row, const char* what)
{
  if (p != nullptr) check_rows(p, false, stride, row, what);
}

}  // namespace

extern "C" {

wholememory_error_code_t wholememory_ext_csc_kge_score_forward(
  const int32_t* row_ptr, const int32_t* col_ind, const int32_t* edge_type, int64_t n_edges, int64_t n_dst, int64_t n_src,
  int64_t num_relations, const float* x_src, int64_t x_src_stride, const float* x_dst, int64_t x_dst_stride, const float* rel,
  int64_t rel_stride, int64_t dim, int model, int head_src, float* score, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  wm_kge_args a = make_kge_args(row_ptr, col_ind, edge_type, n_edges, n_dst, n_src, num_relations, x_src, x_src_stride, x_dst,
                                x_dst_stride, rel, rel_stride, dim, model, head_src);
  if (a.n_edges > 0 && score == nullptr) throw invalid_input("score is null");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->kge_forward == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.score = score;
  WM_BK(bk->kge_forward(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_kge_score_backward(
  const int32_t* row_ptr, const int32_t* col_ind, const int32_t* edge_type, int64_t n_edges, int64_t n_dst, int64_t n_src,
  int64_t num_relations, const float* x_src, int64_t x_src_stride, const float* x_dst, int64_t x_dst_stride, const float* rel,
  int64_t rel_stride, int64_t dim, int model, int head_src, const float* score, const float* grad_score, float* grad_src,
  int64_t grad_src_stride, float* grad_dst, int64_t grad_dst_stride, float* grad_rel, int64_t grad_rel_stride,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  wm_kge_args a = make_kge_args(row_ptr, col_ind, edge_type, n_edges, n_dst, n_src, num_relations, x_src, x_src_stride, x_dst,
                                x_dst_stride, rel, rel_stride, dim, model, head_src);
  if (a.n_edges > 0 && grad_score == nullptr) throw invalid_input("grad_score is null");
  if (a.n_edges > 0 && score == nullptr && (model == WM_KGE_TRANSE_L2 || model == WM_KGE_ROTATE))
    throw invalid_input("score is null: the l2 models read the forward's score");
  if (grad_src == nullptr && grad_dst == nullptr && grad_rel == nullptr) throw invalid_input("no gradient asked for");
  check_optional_rows(grad_src, grad_src_stride, dim, "grad_src");
  check_optional_rows(grad_dst, grad_dst_stride, dim, "grad_dst");
  check_optional_rows(grad_rel, grad_rel_stride, dim, "grad_rel");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->kge_backward == nullptr || bk->kge_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.score           = const_cast<float*>(score);   // (written by the forward only)
  a.grad            = grad_score;
  a.grad_src        = grad_src;
  a.grad_src_stride = grad_src_stride;
  a.grad_dst        = grad_dst;
  a.grad_dst_stride = grad_dst_stride;
  a.grad_rel        = grad_rel;
  a.grad_rel_stride = grad_rel_stride;
  // the second index, over edge_type: the sort leaves a type outside [0, num_relations) out of every run, so no row of
  // grad_rel reads it. It lives around backward_over_index, which builds the first (read for grad_src only)
  sorted_ids rel_ids(p_env_fns);
  wm_edge_index rel_ix{};
  if (grad_rel != nullptr) {
    sort_col_ind(&rel_ids, a.edge_type, a.n_edges, num_relations, stream);
    rel_ix = {rel_ids.order, rel_ids.starts, static_cast<const int32_t*>(rel_ids.unique), rel_ids.n_unique_dev};
  }
  backward_over_index(a, grad_src != nullptr, bk->kge_backward_workspace_bytes(&a), p_env_fns, stream,
                      [&](const wm_edge_index& ix, void* ws) { WM_BK(bk->kge_backward(&a, ix, rel_ix, ws, stream)); });
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

}  // extern "C"
