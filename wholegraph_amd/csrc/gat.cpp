// wholegraph_amd — host side of the multi-head graph attention of a sampled CSC block (wholegraph_amd_ext.h, section 2c,
// section 2f: the same op with an edge term in the logit, section 2g: GATv2, and section 2k: scaled dot-product attention):
// validation, scratch, the edge index of the backward (the library's id sort over col_ind) and the launches of
// kernels/gat.hip / kernels/gat_edge.hip / kernels/gatv2.hip / kernels/tconv.hip. The semantics, and the one order of every
// fp32 sum, are stated in the header.
#include <wholememory/wholegraph_amd_ext.h>

#include <cmath>

#include "csc_block.hpp"

namespace {

using namespace wm;

void check_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                const float* h, int64_t h_stride, const float* att, int64_t heads, int64_t dim, const float* alpha,
                const float* scores)
{
  auto bad = [](const char* what) { throw invalid_input(what); };
  check_block(row_ptr, col_ind, n_edges, n_dst, n_src, n_edges > 0 && n_dst > 0, "h");
  if (heads < 1) bad("heads must be >= 1");
  if (dim < 1) bad("dim must be >= 1");
  if (n_src > 0 && h == nullptr) bad("h is null");
  if (att == nullptr) bad("att is null");
  if (n_edges > 0 && n_dst > 0 && alpha == nullptr) bad("alpha is null");
  if (n_src > 0 && scores == nullptr) bad("scores is null");
  if (h_stride < heads * dim) bad("h stride smaller than its row");
  if (heads * dim >= (int64_t(1) << 31)) bad("heads * dim too large");
}

wm_gat_args make_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                      const float* h, int64_t h_stride, const float* att, int64_t heads, int64_t dim, float slope,
                      int concat, const float* alpha, const float* scores)
{
  wm_gat_args a{};
  a.row_ptr  = row_ptr;
  a.col_ind  = col_ind;
  a.n_edges  = n_dst == 0 ? 0 : n_edges;   // (no target, no edge of any target)
  a.n_dst    = n_dst;
  a.n_src    = n_src;
  a.heads    = heads;
  a.dim      = dim;
  a.slope    = slope;
  a.concat   = concat ? 1 : 0;
  a.h        = h;
  a.h_stride = h_stride;
  a.att      = att;
  a.alpha    = const_cast<float*>(alpha);    // (written by the forward only)
  a.scores   = const_cast<float*>(scores);   // (written by the forward only)
  return a;
}

// what (2g) shares between its forward and backward: the checks of (2c), minus the scores, plus h_dst
wm_gatv2_args make_v2_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                           const float* h_src, int64_t h_src_stride, const float* h_dst, int64_t h_dst_stride,
                           const float* att, int64_t heads, int64_t dim, float slope, int concat, const float* alpha)
{
  auto bad = [](const char* what) { throw invalid_input(what); };
  check_block(row_ptr, col_ind, n_edges, n_dst, n_src, n_edges > 0 && n_dst > 0, "h_src");
  if (heads < 1) bad("heads must be >= 1");
  if (dim < 1) bad("dim must be >= 1");
  if (n_src > 0 && h_src == nullptr) bad("h_src is null");
  if (n_dst > 0 && h_dst == nullptr) bad("h_dst is null");
  if (att == nullptr) bad("att is null");
  if (n_edges > 0 && n_dst > 0 && alpha == nullptr) bad("alpha is null");
  if (h_src_stride < heads * dim) bad("h_src stride smaller than its row");
  if (h_dst_stride < heads * dim) bad("h_dst stride smaller than its row");
  if (heads * dim >= (int64_t(1) << 31)) bad("heads * dim too large");
  wm_gatv2_args a{};
  a.row_ptr      = row_ptr;
  a.col_ind      = col_ind;
  a.n_edges      = n_dst == 0 ? 0 : n_edges;   // (no target, no edge of any target)
  a.n_dst        = n_dst;
  a.n_src        = n_src;
  a.heads        = heads;
  a.dim          = dim;
  a.slope        = slope;
  a.concat       = concat ? 1 : 0;
  a.h_src        = h_src;
  a.h_src_stride = h_src_stride;
  a.h_dst        = h_dst;
  a.h_dst_stride = h_dst_stride;
  a.att          = att;
  a.alpha        = const_cast<float*>(alpha);   // (written by the forward only)
  return a;
}

// what (2k) shares between its forward and backward: the checks of (2g) with key / query / value in place of h_src / h_dst
// / att, and the scale, both of whose operations the host rounds correctly
wm_tconv_args make_tconv_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                              const float* key, int64_t key_stride, const float* query, int64_t query_stride,
                              const float* value, int64_t value_stride, int64_t heads, int64_t dim, int norm_by_dim,
                              int concat, const float* alpha)
{
  auto bad = [](const char* what) { throw invalid_input(what); };
  check_block(row_ptr, col_ind, n_edges, n_dst, n_src, n_edges > 0 && n_dst > 0, "key");
  if (heads < 1) bad("heads must be >= 1");
  if (dim < 1) bad("dim must be >= 1");
  if (n_src > 0 && key == nullptr) bad("key is null");
  if (n_src > 0 && value == nullptr) bad("value is null");
  if (n_dst > 0 && query == nullptr) bad("query is null");
  if (n_edges > 0 && n_dst > 0 && alpha == nullptr) bad("alpha is null");
  if (key_stride < heads * dim) bad("key stride smaller than its row");
  if (query_stride < heads * dim) bad("query stride smaller than its row");
  if (value_stride < heads * dim) bad("value stride smaller than its row");
  if (heads * dim >= (int64_t(1) << 30)) bad("heads * dim too large");
  wm_tconv_args a{};
  a.row_ptr      = row_ptr;
  a.col_ind      = col_ind;
  a.n_edges      = n_dst == 0 ? 0 : n_edges;   // (no target, no edge of any target)
  a.n_dst        = n_dst;
  a.n_src        = n_src;
  a.heads        = heads;
  a.dim          = dim;
  a.norm_by_dim  = norm_by_dim ? 1 : 0;
  a.scale        = 1.0f / sqrtf(static_cast<float>(dim));
  a.concat       = concat ? 1 : 0;
  a.key          = key;
  a.key_stride   = key_stride;
  a.query        = query;
  a.query_stride = query_stride;
  a.value        = value;
  a.value_stride = value_stride;
  a.alpha        = const_cast<float*>(alpha);   // (written by the forward only)
  return a;
}

}  // namespace

extern "C" {

wholememory_error_code_t wholememory_ext_csc_gat_forward(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges,
                                                         int64_t n_dst, int64_t n_src, const float* h, int64_t h_stride,
                                                         const float* att, int64_t heads, int64_t dim, float negative_slope,
                                                         int concat, float* out, int64_t out_stride, float* alpha,
                                                         float* scores, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk = backend();
  if (bk->gat_forward == nullptr || bk->gat_forward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  check_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, alpha, scores);
  if (n_dst > 0 && out == nullptr) throw invalid_input("out is null");
  if (out_stride < (concat ? heads * dim : dim)) throw invalid_input("out stride smaller than its row");
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
  wm_gat_args a = make_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, negative_slope, concat,
                            alpha, scores);
  a.out         = out;
  a.out_stride  = out_stride;
  temp_mem ws(p_env_fns);
  const size_t wb = bk->gat_forward_workspace_bytes(&a);
  void* d_ws      = wb > 0 ? ws.device(static_cast<int64_t>(wb), WHOLEMEMORY_DT_INT8) : nullptr;
  WM_BK(bk->gat_forward(&a, d_ws, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_gat_backward(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges,
                                                          int64_t n_dst, int64_t n_src, const float* h, int64_t h_stride,
                                                          const float* att, int64_t heads, int64_t dim,
                                                          float negative_slope, int concat, const float* alpha,
                                                          const float* scores, const float* grad_out,
                                                          int64_t grad_out_stride, float* grad_h, int64_t grad_h_stride,
                                                          float* grad_att, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk = backend();
  if (bk->gat_backward == nullptr || bk->gat_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  check_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, alpha, scores);
  if (n_dst > 0 && grad_out == nullptr) throw invalid_input("grad_out is null");
  if (grad_out_stride < (concat ? heads * dim : dim)) throw invalid_input("grad_out stride smaller than its row");
  if (n_src > 0 && grad_h == nullptr) throw invalid_input("grad_h is null");
  if (grad_h_stride < heads * dim) throw invalid_input("grad_h stride smaller than its row");
  if (grad_att == nullptr) throw invalid_input("grad_att is null");
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
  wm_gat_args a   = make_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, negative_slope, concat,
                              alpha, scores);
  a.grad          = grad_out;
  a.grad_stride   = grad_out_stride;
  a.grad_h        = grad_h;
  a.grad_h_stride = grad_h_stride;
  a.grad_att      = grad_att;
  sorted_ids ix(p_env_fns);   // the edge index; a block without source rows has none: null pointers
  temp_mem gat_ws(p_env_fns);
  if (n_src > 0) sort_col_ind(&ix, col_ind, a.n_edges, n_src, stream);
  void* d_gws = gat_ws.device(static_cast<int64_t>(bk->gat_backward_workspace_bytes(&a)), WHOLEMEMORY_DT_INT8);
  WM_BK(bk->gat_backward(&a, ix.order, ix.starts, static_cast<const int32_t*>(ix.unique), ix.n_unique_dev, d_gws, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_gat_edge_forward(
  const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, const float* h,
  int64_t h_stride, const float* att, const float* edge_feat, int64_t ef_stride, int64_t heads, int64_t dim,
  float negative_slope, int concat, float* out, int64_t out_stride, float* alpha, float* scores, float* edge_scores,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk = backend();
  if (bk->gat_edge_forward == nullptr || bk->gat_forward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  check_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, alpha, scores);
  if (n_edges > 0 && n_dst > 0 && edge_feat == nullptr) throw invalid_input("edge_feat is null");
  if (n_edges > 0 && n_dst > 0 && edge_scores == nullptr) throw invalid_input("edge_scores is null");
  if (ef_stride < heads * dim) throw invalid_input("edge_feat stride smaller than its row");
  if (n_dst > 0 && out == nullptr) throw invalid_input("out is null");
  if (out_stride < (concat ? heads * dim : dim)) throw invalid_input("out stride smaller than its row");
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
  wm_gat_edge_args a{};
  a.g = make_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, negative_slope, concat, alpha,
                  scores);
  a.g.out        = out;
  a.g.out_stride = out_stride;
  a.edge_feat    = edge_feat;
  a.ef_stride    = ef_stride;
  a.edge_scores  = edge_scores;
  temp_mem ws(p_env_fns);
  const size_t wb = bk->gat_forward_workspace_bytes(&a.g);
  void* d_ws      = wb > 0 ? ws.device(static_cast<int64_t>(wb), WHOLEMEMORY_DT_INT8) : nullptr;
  WM_BK(bk->gat_edge_forward(&a, d_ws, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_gat_edge_backward(
  const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, const float* h,
  int64_t h_stride, const float* att, const float* edge_feat, int64_t ef_stride, int64_t heads, int64_t dim,
  float negative_slope, int concat, const float* alpha, const float* scores, const float* edge_scores,
  const float* grad_out, int64_t grad_out_stride, float* grad_h, int64_t grad_h_stride, float* grad_att,
  float* grad_edge_feat, int64_t grad_ef_stride, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk = backend();
  if (bk->gat_edge_backward == nullptr || bk->gat_edge_backward_workspace_bytes == nullptr)
    return WHOLEMEMORY_NOT_SUPPORTED;
  check_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, alpha, scores);
  if (n_edges > 0 && n_dst > 0 && edge_feat == nullptr) throw invalid_input("edge_feat is null");
  if (n_edges > 0 && n_dst > 0 && edge_scores == nullptr) throw invalid_input("edge_scores is null");
  if (n_edges > 0 && n_dst > 0 && grad_edge_feat == nullptr) throw invalid_input("grad_edge_feat is null");
  if (ef_stride < heads * dim) throw invalid_input("edge_feat stride smaller than its row");
  if (grad_ef_stride < heads * dim) throw invalid_input("grad_edge_feat stride smaller than its row");
  if (n_dst > 0 && grad_out == nullptr) throw invalid_input("grad_out is null");
  if (grad_out_stride < (concat ? heads * dim : dim)) throw invalid_input("grad_out stride smaller than its row");
  if (n_src > 0 && grad_h == nullptr) throw invalid_input("grad_h is null");
  if (grad_h_stride < heads * dim) throw invalid_input("grad_h stride smaller than its row");
  if (grad_att == nullptr) throw invalid_input("grad_att is null");
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
  wm_gat_edge_args a{};
  a.g = make_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, negative_slope, concat, alpha,
                  scores);
  a.g.grad          = grad_out;
  a.g.grad_stride   = grad_out_stride;
  a.g.grad_h        = grad_h;
  a.g.grad_h_stride = grad_h_stride;
  a.g.grad_att      = grad_att;
  a.edge_feat       = edge_feat;
  a.ef_stride       = ef_stride;
  a.edge_scores     = const_cast<float*>(edge_scores);   // (written by the forward only)
  a.grad_edge_feat  = grad_edge_feat;
  a.grad_ef_stride  = grad_ef_stride;
  sorted_ids ix(p_env_fns);   // the edge index; a block without source rows has none: null pointers
  temp_mem gat_ws(p_env_fns);
  if (n_src > 0) sort_col_ind(&ix, col_ind, a.g.n_edges, n_src, stream);
  void* d_gws = gat_ws.device(static_cast<int64_t>(bk->gat_edge_backward_workspace_bytes(&a)), WHOLEMEMORY_DT_INT8);
  WM_BK(bk->gat_edge_backward(&a, ix.order, ix.starts, static_cast<const int32_t*>(ix.unique), ix.n_unique_dev, d_gws, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_gatv2_forward(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges,
                                                           int64_t n_dst, int64_t n_src, const float* h_src,
                                                           int64_t h_src_stride, const float* h_dst, int64_t h_dst_stride,
                                                           const float* att, int64_t heads, int64_t dim,
                                                           float negative_slope, int concat, float* out, int64_t out_stride,
                                                           float* alpha, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk = backend();
  wm_gatv2_args a = make_v2_args(row_ptr, col_ind, n_edges, n_dst, n_src, h_src, h_src_stride, h_dst, h_dst_stride, att,
                                 heads, dim, negative_slope, concat, alpha);
  if (n_dst > 0 && out == nullptr) throw invalid_input("out is null");
  if (out_stride < (concat ? heads * dim : dim)) throw invalid_input("out stride smaller than its row");
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
  // (after the checks: a malformed call is INVALID_INPUT under every backend)
  if (bk->gatv2_forward == nullptr || bk->gatv2_forward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.out        = out;
  a.out_stride = out_stride;
  temp_mem ws(p_env_fns);
  const size_t wb = bk->gatv2_forward_workspace_bytes(&a);
  void* d_ws      = wb > 0 ? ws.device(static_cast<int64_t>(wb), WHOLEMEMORY_DT_INT8) : nullptr;
  WM_BK(bk->gatv2_forward(&a, d_ws, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_gatv2_backward(
  const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, const float* h_src,
  int64_t h_src_stride, const float* h_dst, int64_t h_dst_stride, const float* att, int64_t heads, int64_t dim,
  float negative_slope, int concat, const float* alpha, const float* grad_out, int64_t grad_out_stride, float* grad_h_src,
  int64_t grad_h_src_stride, float* grad_h_dst, int64_t grad_h_dst_stride, float* grad_att,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk = backend();
  wm_gatv2_args a = make_v2_args(row_ptr, col_ind, n_edges, n_dst, n_src, h_src, h_src_stride, h_dst, h_dst_stride, att,
                                 heads, dim, negative_slope, concat, alpha);
  if (n_dst > 0 && grad_out == nullptr) throw invalid_input("grad_out is null");
  if (grad_out_stride < (concat ? heads * dim : dim)) throw invalid_input("grad_out stride smaller than its row");
  if (grad_h_src == nullptr && grad_h_dst == nullptr && grad_att == nullptr) throw invalid_input("no gradient asked for");
  if (grad_h_src != nullptr && grad_h_src_stride < heads * dim) throw invalid_input("grad_h_src stride smaller than its row");
  if (grad_h_dst != nullptr && grad_h_dst_stride < heads * dim) throw invalid_input("grad_h_dst stride smaller than its row");
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
  if (bk->gatv2_backward == nullptr || bk->gatv2_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.grad              = grad_out;
  a.grad_stride       = grad_out_stride;
  a.grad_h_src        = grad_h_src;
  a.grad_h_src_stride = grad_h_src_stride;
  a.grad_h_dst        = grad_h_dst;
  a.grad_h_dst_stride = grad_h_dst_stride;
  a.grad_att          = grad_att;
  sorted_ids ix(p_env_fns);   // the edge index of grad_h_src; without that gradient, or without source rows: null pointers
  temp_mem gat_ws(p_env_fns);
  if (grad_h_src != nullptr && n_src > 0) sort_col_ind(&ix, col_ind, a.n_edges, n_src, stream);
  void* d_gws = gat_ws.device(static_cast<int64_t>(bk->gatv2_backward_workspace_bytes(&a)), WHOLEMEMORY_DT_INT8);
  WM_BK(bk->gatv2_backward(&a, ix.order, ix.starts, static_cast<const int32_t*>(ix.unique), ix.n_unique_dev, d_gws, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_mha_simple_forward(
  const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, const float* key,
  int64_t key_stride, const float* query, int64_t query_stride, const float* value, int64_t value_stride, int64_t heads,
  int64_t dim, int norm_by_dim, int concat, float* out, int64_t out_stride, float* alpha, wholememory_env_func_t* p_env_fns,
  void* stream)
{
  WM_API_BEGIN
  const auto* bk  = backend();
  wm_tconv_args a = make_tconv_args(row_ptr, col_ind, n_edges, n_dst, n_src, key, key_stride, query, query_stride, value,
                                    value_stride, heads, dim, norm_by_dim, concat, alpha);
  if (n_dst > 0 && out == nullptr) throw invalid_input("out is null");
  if (out_stride < (concat ? heads * dim : dim)) throw invalid_input("out stride smaller than its row");
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
  // (after the checks: a malformed call is INVALID_INPUT under every backend)
  if (bk->tconv_forward == nullptr || bk->tconv_forward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.out        = out;
  a.out_stride = out_stride;
  temp_mem ws(p_env_fns);
  const size_t wb = bk->tconv_forward_workspace_bytes(&a);
  void* d_ws      = wb > 0 ? ws.device(static_cast<int64_t>(wb), WHOLEMEMORY_DT_INT8) : nullptr;
  WM_BK(bk->tconv_forward(&a, d_ws, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_mha_simple_backward(
  const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, const float* key,
  int64_t key_stride, const float* query, int64_t query_stride, const float* value, int64_t value_stride, int64_t heads,
  int64_t dim, int norm_by_dim, int concat, const float* alpha, const float* grad_out, int64_t grad_out_stride,
  float* grad_key, int64_t grad_key_stride, float* grad_query, int64_t grad_query_stride, float* grad_value,
  int64_t grad_value_stride, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk  = backend();
  wm_tconv_args a = make_tconv_args(row_ptr, col_ind, n_edges, n_dst, n_src, key, key_stride, query, query_stride, value,
                                    value_stride, heads, dim, norm_by_dim, concat, alpha);
  if (n_dst > 0 && grad_out == nullptr) throw invalid_input("grad_out is null");
  if (grad_out_stride < (concat ? heads * dim : dim)) throw invalid_input("grad_out stride smaller than its row");
  if (grad_key == nullptr && grad_query == nullptr && grad_value == nullptr) throw invalid_input("no gradient asked for");
  if (grad_key != nullptr && grad_key_stride < heads * dim) throw invalid_input("grad_key stride smaller than its row");
  if (grad_query != nullptr && grad_query_stride < heads * dim) throw invalid_input("grad_query stride smaller than its row");
  if (grad_value != nullptr && grad_value_stride < heads * dim) throw invalid_input("grad_value stride smaller than its row");
  if (p_env_fns == nullptr) throw invalid_input("p_env_fns is null");
  if (bk->tconv_backward == nullptr || bk->tconv_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.grad              = grad_out;
  a.grad_stride       = grad_out_stride;
  a.grad_key          = grad_key;
  a.grad_key_stride   = grad_key_stride;
  a.grad_query        = grad_query;
  a.grad_query_stride = grad_query_stride;
  a.grad_value        = grad_value;
  a.grad_value_stride = grad_value_stride;
  // the edge index of grad_key and grad_value; without both, or without source rows: null pointers
  sorted_ids ix(p_env_fns);
  temp_mem tconv_ws(p_env_fns);
  if ((grad_key != nullptr || grad_value != nullptr) && n_src > 0) sort_col_ind(&ix, col_ind, a.n_edges, n_src, stream);
  void* d_ws = tconv_ws.device(static_cast<int64_t>(bk->tconv_backward_workspace_bytes(&a)), WHOLEMEMORY_DT_INT8);
  WM_BK(bk->tconv_backward(&a, ix.order, ix.starts, static_cast<const int32_t*>(ix.unique), ix.n_unique_dev, d_ws, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

int64_t wholememory_ext_csc_gat_node_chunk(void) { return wm::kGatNodeChunk; }

}  // extern "C"
