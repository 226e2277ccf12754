// wholegraph_amd — host side of the multi-head graph attention of a sampled CSC block (wholegraph_amd_ext.h, section 2c,
// section 2f: the same op with an edge term in the logit, section 2g: GATv2, and section 2k: scaled dot-product attention)
// and of the edge dot product (section 2p), the logit of (2k) on its own: validation, scratch, the edge index of the backward
// (the library's id sort over col_ind) and the launches of kernels/gat.hip / kernels/gat_edge.hip / kernels/gatv2.hip /
// kernels/tconv.hip / kernels/edot.hip. The semantics, and the one order of every fp32 sum, are stated in the header.
#include <wholememory/wholegraph_amd_ext.h>

#include <cmath>

#include "csc_block.hpp"

namespace {

using namespace wm;

constexpr int64_t kMaxRow = int64_t(1) << 31, kMaxRowTconv = int64_t(1) << 30;   // heads * dim stays below these
constexpr int64_t kMaxRowEdot = (int64_t(1) << 31) / 4;                             // dim of (2p) stays below this

// what the args of every attention op hold alike, checked: the block (col_ind and alpha are read when a target has an
// edge), heads, dim (heads * dim below `max_row`) and concat. rows: what the op calls its source rows
template <class Args>
Args attention_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                    const char* rows, int64_t heads, int64_t dim, int64_t max_row, int concat, const float* alpha)
{
  Args a{};
  static_cast<wm_csc_block&>(a) = checked_block(row_ptr, col_ind, n_edges, n_dst, n_src, n_edges > 0 && n_dst > 0, rows);
  checked_heads(heads, dim, max_row);
  if (a.n_edges > 0 && alpha == nullptr) throw invalid_input("alpha is null");
  a.heads  = heads;
  a.dim    = dim;
  a.concat = concat ? 1 : 0;
  a.alpha  = const_cast<float*>(alpha);   // (written by the forward only)
  return a;
}

// a gradient that may be left out: only its stride is judged, and only when it is asked for
void check_optional_rows(const void* p, int64_t stride, int64_t row, const char* what)
{
  if (p != nullptr) check_rows(p, false, stride, row, what);
}

// what (2c) and (2f) share between forward and backward: h, att and the scores
wm_gat_args make_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                      const float* h, int64_t h_stride, const float* att, int64_t heads, int64_t dim, float slope,
                      int concat, const float* alpha, const float* scores)
{
  auto a = attention_args<wm_gat_args>(row_ptr, col_ind, n_edges, n_dst, n_src, "h", heads, dim, kMaxRow, concat, alpha);
  check_rows(h, n_src > 0, h_stride, heads * dim, "h");
  if (att == nullptr) throw invalid_input("att is null");
  if (n_src > 0 && scores == nullptr) throw invalid_input("scores is null");
  a.slope    = slope;
  a.h        = h;
  a.h_stride = h_stride;
  a.att      = att;
  a.scores   = const_cast<float*>(scores);   // (written by the forward only)
  return a;
}

// what (2f) adds to make_args in forward and backward: the rows and the scores of the edges
wm_gat_edge_args make_edge_args(const wm_gat_args& g, const float* edge_feat, int64_t ef_stride, const float* edge_scores)
{
  check_rows(edge_feat, g.n_edges > 0, ef_stride, g.heads * g.dim, "edge_feat");
  if (g.n_edges > 0 && edge_scores == nullptr) throw invalid_input("edge_scores is null");
  wm_gat_edge_args a{};
  a.g           = g;
  a.edge_feat   = edge_feat;
  a.ef_stride   = ef_stride;
  a.edge_scores = const_cast<float*>(edge_scores);   // (written by the forward only)
  return a;
}

// what (2g) shares between its forward and backward: h_src, h_dst and att
wm_gatv2_args make_v2_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                           const float* h_src, int64_t h_src_stride, const float* h_dst, int64_t h_dst_stride,
                           const float* att, int64_t heads, int64_t dim, float slope, int concat, const float* alpha)
{
  auto a = attention_args<wm_gatv2_args>(row_ptr, col_ind, n_edges, n_dst, n_src, "h_src", heads, dim, kMaxRow, concat, alpha);
  check_rows(h_src, n_src > 0, h_src_stride, heads * dim, "h_src");
  check_rows(h_dst, n_dst > 0, h_dst_stride, heads * dim, "h_dst");
  if (att == nullptr) throw invalid_input("att is null");
  a.slope        = slope;
  a.h_src        = h_src;
  a.h_src_stride = h_src_stride;
  a.h_dst        = h_dst;
  a.h_dst_stride = h_dst_stride;
  a.att          = att;
  return a;
}

// what (2k) shares between its forward and backward: key, query and value, and the scale, both of whose operations the
// host rounds correctly
wm_tconv_args make_tconv_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                              const float* key, int64_t key_stride, const float* query, int64_t query_stride,
                              const float* value, int64_t value_stride, int64_t heads, int64_t dim, int norm_by_dim,
                              int concat, const float* alpha)
{
  auto a = attention_args<wm_tconv_args>(row_ptr, col_ind, n_edges, n_dst, n_src, "key", heads, dim, kMaxRowTconv, concat,
                                         alpha);
  check_rows(key, n_src > 0, key_stride, heads * dim, "key");
  check_rows(value, n_src > 0, value_stride, heads * dim, "value");
  check_rows(query, n_dst > 0, query_stride, heads * dim, "query");
  a.norm_by_dim  = norm_by_dim ? 1 : 0;
  a.scale        = 1.0f / sqrtf(static_cast<float>(dim));
  a.key          = key;
  a.key_stride   = key_stride;
  a.query        = query;
  a.query_stride = query_stride;
  a.value        = value;
  a.value_stride = value_stride;
  return a;
}

// what (2p) shares between its forward and backward: the block, whose targets have rows of their own, x_src and x_dst
wm_edot_args make_edot_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                            const float* x_src, int64_t x_src_stride, const float* x_dst, int64_t x_dst_stride, int64_t dim)
{
  wm_edot_args a{};
  static_cast<wm_csc_block&>(a) =
    checked_block(row_ptr, col_ind, n_edges, n_dst, n_src, n_edges > 0 && n_dst > 0, "x_src", false);
  if (dim < 1 || dim >= kMaxRowEdot) throw invalid_input("dim must be in [1, 2^29)");
  check_rows(x_src, n_src > 0, x_src_stride, dim, "x_src");
  check_rows(x_dst, n_dst > 0, x_dst_stride, dim, "x_dst");
  a.dim          = dim;
  a.x_src        = x_src;
  a.x_src_stride = x_src_stride;
  a.x_dst        = x_dst;
  a.x_dst_stride = x_dst_stride;
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
  wm_gat_args a = make_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, negative_slope, concat,
                            alpha, scores);
  check_out_rows(out, out_stride, n_dst, concat, heads, dim, "out");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->gat_forward == nullptr || bk->gat_forward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.out        = out;
  a.out_stride = out_stride;
  forward_with_workspace(bk->gat_forward_workspace_bytes(&a), p_env_fns,
                         [&](void* ws) { WM_BK(bk->gat_forward(&a, ws, stream)); });
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
  wm_gat_args a = make_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim, negative_slope, concat,
                            alpha, scores);
  check_out_rows(grad_out, grad_out_stride, n_dst, concat, heads, dim, "grad_out");
  check_rows(grad_h, n_src > 0, grad_h_stride, heads * dim, "grad_h");
  if (grad_att == nullptr) throw invalid_input("grad_att is null");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->gat_backward == nullptr || bk->gat_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.grad          = grad_out;
  a.grad_stride   = grad_out_stride;
  a.grad_h        = grad_h;
  a.grad_h_stride = grad_h_stride;
  a.grad_att      = grad_att;
  backward_over_index(a, true, bk->gat_backward_workspace_bytes(&a), p_env_fns, stream,
                      [&](const wm_edge_index& ix, void* ws) { WM_BK(bk->gat_backward(&a, ix, ws, stream)); });
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
  wm_gat_edge_args a = make_edge_args(make_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim,
                                                negative_slope, concat, alpha, scores),
                                      edge_feat, ef_stride, edge_scores);
  check_out_rows(out, out_stride, n_dst, concat, heads, dim, "out");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->gat_edge_forward == nullptr || bk->gat_forward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.g.out        = out;
  a.g.out_stride = out_stride;
  forward_with_workspace(bk->gat_forward_workspace_bytes(&a.g), p_env_fns,
                         [&](void* ws) { WM_BK(bk->gat_edge_forward(&a, ws, stream)); });
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
  wm_gat_edge_args a = make_edge_args(make_args(row_ptr, col_ind, n_edges, n_dst, n_src, h, h_stride, att, heads, dim,
                                                negative_slope, concat, alpha, scores),
                                      edge_feat, ef_stride, edge_scores);
  check_rows(grad_edge_feat, a.g.n_edges > 0, grad_ef_stride, heads * dim, "grad_edge_feat");
  check_out_rows(grad_out, grad_out_stride, n_dst, concat, heads, dim, "grad_out");
  check_rows(grad_h, n_src > 0, grad_h_stride, heads * dim, "grad_h");
  if (grad_att == nullptr) throw invalid_input("grad_att is null");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->gat_edge_backward == nullptr || bk->gat_edge_backward_workspace_bytes == nullptr)
    return WHOLEMEMORY_NOT_SUPPORTED;
  a.g.grad          = grad_out;
  a.g.grad_stride   = grad_out_stride;
  a.g.grad_h        = grad_h;
  a.g.grad_h_stride = grad_h_stride;
  a.g.grad_att      = grad_att;
  a.grad_edge_feat  = grad_edge_feat;
  a.grad_ef_stride  = grad_ef_stride;
  backward_over_index(a.g, true, bk->gat_edge_backward_workspace_bytes(&a), p_env_fns, stream,
                      [&](const wm_edge_index& ix, void* ws) { WM_BK(bk->gat_edge_backward(&a, ix, ws, stream)); });
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
  wm_gatv2_args a = make_v2_args(row_ptr, col_ind, n_edges, n_dst, n_src, h_src, h_src_stride, h_dst, h_dst_stride, att,
                                 heads, dim, negative_slope, concat, alpha);
  check_out_rows(out, out_stride, n_dst, concat, heads, dim, "out");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->gatv2_forward == nullptr || bk->gatv2_forward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.out        = out;
  a.out_stride = out_stride;
  forward_with_workspace(bk->gatv2_forward_workspace_bytes(&a), p_env_fns,
                         [&](void* ws) { WM_BK(bk->gatv2_forward(&a, ws, stream)); });
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
  wm_gatv2_args a = make_v2_args(row_ptr, col_ind, n_edges, n_dst, n_src, h_src, h_src_stride, h_dst, h_dst_stride, att,
                                 heads, dim, negative_slope, concat, alpha);
  check_out_rows(grad_out, grad_out_stride, n_dst, concat, heads, dim, "grad_out");
  if (grad_h_src == nullptr && grad_h_dst == nullptr && grad_att == nullptr) throw invalid_input("no gradient asked for");
  check_optional_rows(grad_h_src, grad_h_src_stride, heads * dim, "grad_h_src");
  check_optional_rows(grad_h_dst, grad_h_dst_stride, heads * dim, "grad_h_dst");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->gatv2_backward == nullptr || bk->gatv2_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.grad              = grad_out;
  a.grad_stride       = grad_out_stride;
  a.grad_h_src        = grad_h_src;
  a.grad_h_src_stride = grad_h_src_stride;
  a.grad_h_dst        = grad_h_dst;
  a.grad_h_dst_stride = grad_h_dst_stride;
  a.grad_att          = grad_att;
  // (the edge index is read for grad_h_src only)
  backward_over_index(a, grad_h_src != nullptr, bk->gatv2_backward_workspace_bytes(&a), p_env_fns, stream,
                      [&](const wm_edge_index& ix, void* ws) { WM_BK(bk->gatv2_backward(&a, ix, ws, stream)); });
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
  wm_tconv_args a = make_tconv_args(row_ptr, col_ind, n_edges, n_dst, n_src, key, key_stride, query, query_stride, value,
                                    value_stride, heads, dim, norm_by_dim, concat, alpha);
  check_out_rows(out, out_stride, n_dst, concat, heads, dim, "out");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->tconv_forward == nullptr || bk->tconv_forward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.out        = out;
  a.out_stride = out_stride;
  forward_with_workspace(bk->tconv_forward_workspace_bytes(&a), p_env_fns,
                         [&](void* ws) { WM_BK(bk->tconv_forward(&a, ws, stream)); });
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
  wm_tconv_args a = make_tconv_args(row_ptr, col_ind, n_edges, n_dst, n_src, key, key_stride, query, query_stride, value,
                                    value_stride, heads, dim, norm_by_dim, concat, alpha);
  check_out_rows(grad_out, grad_out_stride, n_dst, concat, heads, dim, "grad_out");
  if (grad_key == nullptr && grad_query == nullptr && grad_value == nullptr) throw invalid_input("no gradient asked for");
  check_optional_rows(grad_key, grad_key_stride, heads * dim, "grad_key");
  check_optional_rows(grad_query, grad_query_stride, heads * dim, "grad_query");
  check_optional_rows(grad_value, grad_value_stride, heads * dim, "grad_value");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->tconv_backward == nullptr || bk->tconv_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.grad              = grad_out;
  a.grad_stride       = grad_out_stride;
  a.grad_key          = grad_key;
  a.grad_key_stride   = grad_key_stride;
  a.grad_query        = grad_query;
  a.grad_query_stride = grad_query_stride;
  a.grad_value        = grad_value;
  a.grad_value_stride = grad_value_stride;
  // (the edge index is read for grad_key and grad_value only)
  backward_over_index(a, grad_key != nullptr || grad_value != nullptr, bk->tconv_backward_workspace_bytes(&a), p_env_fns,
                      stream, [&](const wm_edge_index& ix, void* ws) { WM_BK(bk->tconv_backward(&a, ix, ws, stream)); });
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_edge_dot_forward(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges,
                                                              int64_t n_dst, int64_t n_src, const float* x_src,
                                                              int64_t x_src_stride, const float* x_dst, int64_t x_dst_stride,
                                                              int64_t dim, float* score, wholememory_env_func_t* p_env_fns,
                                                              void* stream)
{
  WM_API_BEGIN
  wm_edot_args a = make_edot_args(row_ptr, col_ind, n_edges, n_dst, n_src, x_src, x_src_stride, x_dst, x_dst_stride, dim);
  if (a.n_edges > 0 && score == nullptr) throw invalid_input("score is null");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->edot_forward == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.score = score;
  WM_BK(bk->edot_forward(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_edge_dot_backward(const int32_t* row_ptr, const int32_t* col_ind,
                                                               int64_t n_edges, int64_t n_dst, int64_t n_src,
                                                               const float* x_src, int64_t x_src_stride, const float* x_dst,
                                                               int64_t x_dst_stride, int64_t dim, const float* grad_score,
                                                               float* grad_src, int64_t grad_src_stride, float* grad_dst,
                                                               int64_t grad_dst_stride, wholememory_env_func_t* p_env_fns,
                                                               void* stream)
{
  WM_API_BEGIN
  wm_edot_args a = make_edot_args(row_ptr, col_ind, n_edges, n_dst, n_src, x_src, x_src_stride, x_dst, x_dst_stride, dim);
  if (a.n_edges > 0 && grad_score == nullptr) throw invalid_input("grad_score is null");
  if (grad_src == nullptr && grad_dst == nullptr) throw invalid_input("no gradient asked for");
  check_optional_rows(grad_src, grad_src_stride, dim, "grad_src");
  check_optional_rows(grad_dst, grad_dst_stride, dim, "grad_dst");
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->edot_backward == nullptr || bk->edot_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.grad            = grad_score;
  a.grad_src        = grad_src;
  a.grad_src_stride = grad_src_stride;
  a.grad_dst        = grad_dst;
  a.grad_dst_stride = grad_dst_stride;
  // (the edge index is read for grad_src only)
  backward_over_index(a, grad_src != nullptr, bk->edot_backward_workspace_bytes(&a), p_env_fns, stream,
                      [&](const wm_edge_index& ix, void* ws) { WM_BK(bk->edot_backward(&a, ix, ws, stream)); });
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

int64_t wholememory_ext_csc_gat_node_chunk(void) { return wm::kGatNodeChunk; }

}  // extern "C"
