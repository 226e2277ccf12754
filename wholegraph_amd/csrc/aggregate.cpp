// wholegraph_amd — host side of the neighbour aggregation of a sampled CSC block (wholegraph_amd_ext.h, section 2b):
// validation, the edge index of the backward (the library's id sort over col_ind) and the launches of kernels/agg.hip
// (fp32 rows), kernels/agg_half.hip (fp16 / bf16 rows, the _typed entry points) and kernels/agg_weighted.hip (a weight per
// edge, section 2d, the _weighted entry points) and kernels/agg_gather.hip (rows read from a WholeMemory table by global id,
// section 2e) and kernels/agg_quant.hip (the same from an 8-bit row-quantized table, section 2j) and kernels/agg_rel.hip (a
// type per edge and a slot per relation, section 2h, the _rel_ entry points) and kernels/pna.hip (sum, mean, min, max and std
// out of one read of the neighbour rows, section 2l, the _pna_ entry points). The semantics, and the one order of every fp32 sum, are stated in the header.
#include <atomic>

#include <wholememory/wholegraph_amd_ext.h>
#include <wholememory/wholememory_tensor.h>

#include "csc_block.hpp"

namespace {

using namespace wm;

// what the agg_concat entry points check alike, and the args they fill alike: the block, dim and aggr; the rows that are
// read (`in`, [in_rows, in_cols]) and the rows that are written (`out`, [out_rows, out_cols])
template <class Args>
Args checked_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                  const void* in, int64_t in_stride, int64_t in_cols, int64_t dim, int aggr, const void* out,
                  int64_t out_stride, int64_t out_cols, int64_t in_rows, int64_t out_rows)
{
  Args a{};
  static_cast<wm_csc_block&>(a) = checked_block(row_ptr, col_ind, n_edges, n_dst, n_src, n_edges > 0, "x");
  if (dim < 1) throw invalid_input("dim must be >= 1");
  if (aggr != WHOLEMEMORY_EXT_AGGR_SUM && aggr != WHOLEMEMORY_EXT_AGGR_MEAN) throw invalid_input("aggr must be SUM or MEAN");
  check_rows(in, in_rows > 0, in_stride, in_cols, "input");
  check_rows(out, out_rows > 0, out_stride, out_cols, "output");
  a.dim  = dim;
  a.mean = aggr == WHOLEMEMORY_EXT_AGGR_MEAN ? 1 : 0;
  return a;
}

// the backward of the agg_concat family: nothing to do without source rows, else the edge index, the workspace of
// agg_backward_workspace_bytes and `entry` (the backend's *_backward named `name`)
template <class Args>
void agg_backward(const char* name, int (*entry)(const Args*, const wm_edge_index&, void*, void*), const Args& a,
                  wholememory_env_func_t* p_env_fns, void* stream)
{
  if (a.n_src == 0) return;
  backward_over_index(a, true, backend()->agg_backward_workspace_bytes(a.n_edges, a.n_src, a.dim), p_env_fns, stream,
                      [&](const wm_edge_index& ix, void* ws) {
                        const int rc = entry(&a, ix, ws, stream);
                        if (rc != 0) throw hip_error(format_string("%s failed with code %d", name, rc));
                      });
}

// the memory types whose rows the fused gathers read with plain loads
bool table_is_mapped(wholememory_tensor_t table)
{
  if (!wholememory_tensor_has_handle(table)) return true;
  const auto mt = wholememory_get_memory_type(wholememory_tensor_get_memory_handle(table));
  if (mt != WHOLEMEMORY_MT_CONTINUOUS && mt != WHOLEMEMORY_MT_CHUNKED) return false;
  return !mapped_via_exchange(table, mt);   // (served by a collective, not by loads)
}

bool rows16(wholememory_dtype_t dtype) { return dtype == WHOLEMEMORY_DT_HALF || dtype == WHOLEMEMORY_DT_BF16; }

std::atomic<int64_t> g_gather_agg_calls{0};   // fused forwards that reached the backend
std::atomic<int64_t> g_qagg_calls{0};         // the same over a quantized table (section 2j)

// what the two _rel_ entry points check alike, ahead of checked_args
void check_rel(const int32_t* edge_type, int64_t n_edges, int64_t num_relations, int aggr, const float* edge_scale)
{
  if (num_relations < 1) throw invalid_input("num_relations must be >= 1");
  if (num_relations >= (int64_t(1) << 31) - 1) throw invalid_input("num_relations must be below 2^31 - 1");
  if (n_edges < 0) throw invalid_input("negative size");
  if (n_edges > 0 && edge_type == nullptr) throw invalid_input("edge_type is null");
  if (aggr == WHOLEMEMORY_EXT_AGGR_MEAN && n_edges > 0 && edge_scale == nullptr)
    throw invalid_input("edge_scale is null (MEAN writes it in the forward and reads it in the backward)");
}

}  // namespace

extern "C" {

wholememory_error_code_t wholememory_ext_csc_aggregate_forward(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges,
                                                               int64_t n_dst, int64_t n_src, const float* x, int64_t x_stride,
                                                               int64_t dim, int aggr, float* out, int64_t out_stride,
                                                               wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  (void)p_env_fns;   // (the forward needs no scratch)
  auto a = checked_args<wm_agg_args>(row_ptr, col_ind, n_edges, n_dst, n_src, x, x_stride, dim, dim, aggr, out, out_stride,
                                     2 * dim, n_src, n_dst);
  const auto* bk = backend();
  if (bk->agg_forward == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.in            = x;
  a.in_stride     = x_stride;
  a.out           = out;
  a.out_stride    = out_stride;
  WM_BK(bk->agg_forward(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_aggregate_backward(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges,
                                                                int64_t n_dst, int64_t n_src, const float* grad_out,
                                                                int64_t grad_out_stride, int64_t dim, int aggr, float* grad_x,
                                                                int64_t grad_x_stride, wholememory_env_func_t* p_env_fns,
                                                                void* stream)
{
  WM_API_BEGIN
  auto a = checked_args<wm_agg_args>(row_ptr, col_ind, n_edges, n_dst, n_src, grad_out, grad_out_stride, 2 * dim, dim, aggr,
                                     grad_x, grad_x_stride, dim, n_dst, n_src);
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->agg_backward == nullptr || bk->agg_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.grad        = grad_out;
  a.grad_stride = grad_out_stride;
  a.out         = grad_x;
  a.out_stride  = grad_x_stride;
  agg_backward("agg_backward", bk->agg_backward, a, p_env_fns, stream);
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_aggregate_forward_typed(const int32_t* row_ptr, const int32_t* col_ind,
                                                                     int64_t n_edges, int64_t n_dst, int64_t n_src,
                                                                     const void* x, int64_t x_stride, int64_t dim, int aggr,
                                                                     void* out, int64_t out_stride, wholememory_dtype_t dtype,
                                                                     wholememory_env_func_t* p_env_fns, void* stream)
{
  if (dtype == WHOLEMEMORY_DT_FLOAT)
    return wholememory_ext_csc_aggregate_forward(row_ptr, col_ind, n_edges, n_dst, n_src, static_cast<const float*>(x),
                                                 x_stride, dim, aggr, static_cast<float*>(out), out_stride, p_env_fns, stream);
  WM_API_BEGIN
  (void)p_env_fns;
  if (!rows16(dtype)) throw invalid_input("dtype must be FLOAT, HALF or BF16");
  auto a = checked_args<wm_agg16_args>(row_ptr, col_ind, n_edges, n_dst, n_src, x, x_stride, dim, dim, aggr, out, out_stride,
                                       2 * dim, n_src, n_dst);
  const auto* bk = backend();
  if (bk->agg16_forward == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.dtype         = dtype;
  a.in            = x;
  a.in_stride     = x_stride;
  a.out           = out;
  a.out_stride    = out_stride;
  WM_BK(bk->agg16_forward(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_aggregate_backward_typed(const int32_t* row_ptr, const int32_t* col_ind,
                                                                      int64_t n_edges, int64_t n_dst, int64_t n_src,
                                                                      const void* grad_out, int64_t grad_out_stride,
                                                                      int64_t dim, int aggr, void* grad_x,
                                                                      int64_t grad_x_stride, wholememory_dtype_t dtype,
                                                                      wholememory_env_func_t* p_env_fns, void* stream)
{
  if (dtype == WHOLEMEMORY_DT_FLOAT)
    return wholememory_ext_csc_aggregate_backward(row_ptr, col_ind, n_edges, n_dst, n_src,
                                                  static_cast<const float*>(grad_out), grad_out_stride, dim, aggr,
                                                  static_cast<float*>(grad_x), grad_x_stride, p_env_fns, stream);
  WM_API_BEGIN
  if (!rows16(dtype)) throw invalid_input("dtype must be FLOAT, HALF or BF16");
  auto a = checked_args<wm_agg16_args>(row_ptr, col_ind, n_edges, n_dst, n_src, grad_out, grad_out_stride, 2 * dim, dim, aggr,
                                       grad_x, grad_x_stride, dim, n_dst, n_src);
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->agg16_backward == nullptr || bk->agg_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.dtype         = dtype;
  a.grad          = grad_out;
  a.grad_stride   = grad_out_stride;
  a.out           = grad_x;
  a.out_stride    = grad_x_stride;
  agg_backward("agg16_backward", bk->agg16_backward, a, p_env_fns, stream);
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_aggregate_weighted_forward(const int32_t* row_ptr, const int32_t* col_ind,
                                                                        const float* w, int64_t n_edges, int64_t n_dst,
                                                                        int64_t n_src, const float* x, int64_t x_stride,
                                                                        int64_t dim, int aggr, float* out, int64_t out_stride,
                                                                        wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  (void)p_env_fns;   // (the forward needs no scratch)
  auto a = checked_args<wm_aggw_args>(row_ptr, col_ind, n_edges, n_dst, n_src, x, x_stride, dim, dim, aggr, out, out_stride,
                                      2 * dim, n_src, n_dst);
  if (n_edges > 0 && w == nullptr) throw invalid_input("w is null");
  const auto* bk = backend();
  if (bk->aggw_forward == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.w            = w;
  a.in           = x;
  a.in_stride    = x_stride;
  a.out          = out;
  a.out_stride   = out_stride;
  WM_BK(bk->aggw_forward(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_aggregate_weighted_backward(
  const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, const float* x,
  int64_t x_stride, const float* w, const float* grad_out, int64_t grad_out_stride, int64_t dim, int aggr, float* grad_x,
  int64_t grad_x_stride, float* grad_w, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  // (grad_x may be null: its rows and stride are checked only when it is asked for)
  auto a = checked_args<wm_aggw_args>(row_ptr, col_ind, n_edges, n_dst, n_src, grad_out, grad_out_stride, 2 * dim, dim, aggr,
                                      grad_x, grad_x != nullptr ? grad_x_stride : dim, dim, n_dst,
                                      grad_x != nullptr ? n_src : 0);
  if (grad_x == nullptr && grad_w == nullptr) throw invalid_input("grad_x and grad_w are both null");
  if (n_edges > 0 && w == nullptr) throw invalid_input("w is null");
  if (grad_w != nullptr) check_rows(x, n_src > 0, x_stride, dim, "x");   // the gradient of the weights reads the rows of x
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->aggw_backward == nullptr || bk->agg_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.w            = w;
  a.in           = x;
  a.in_stride    = x_stride;
  a.grad         = grad_out;
  a.grad_stride  = grad_out_stride;
  a.out          = grad_x;
  a.out_stride   = grad_x_stride;
  a.grad_w       = grad_w;
  if (grad_x != nullptr && n_src > 0) {
    agg_backward("aggw_backward", bk->aggw_backward, a, p_env_fns, stream);
  } else if (grad_w != nullptr) {   // (no gradient walks the sources: no index, no workspace)
    a.out = nullptr;
    WM_BK(bk->aggw_backward(&a, wm_edge_index{}, nullptr, stream));
  }
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

int64_t wholememory_ext_csc_aggregate_chunk_edges(void) { return wm::kAggChunkEdges; }

wholememory_error_code_t wholememory_ext_csc_gather_aggregate_forward(wholememory_tensor_t table, const void* node_ids,
                                                                      int node_id_dtype, const int32_t* row_ptr,
                                                                      const int32_t* col_ind, int64_t n_edges, int64_t n_dst,
                                                                      int64_t n_src, int aggr, float* out, int64_t out_stride,
                                                                      wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  (void)p_env_fns;   // (the forward needs no scratch)
  if (table == nullptr) throw invalid_input("table is null");
  const wholememory_tensor_description_t td = *wholememory_tensor_get_tensor_description(table);
  if (td.dim != 2) throw invalid_input("the table must be a 2-D tensor");
  if (td.dtype != WHOLEMEMORY_DT_FLOAT && !rows16(td.dtype)) throw invalid_input("table dtype must be FLOAT, HALF or BF16");
  if (td.strides[1] != 1) throw invalid_input("the table's rows must be contiguous");
  if (node_id_dtype != WHOLEMEMORY_DT_INT && node_id_dtype != WHOLEMEMORY_DT_INT64)
    throw invalid_input("node_id_dtype must be INT or INT64");
  const int64_t dim = td.sizes[1];
  // (the virtual x: n_src rows of `dim` elements behind node_ids)
  auto a = checked_args<wm_gather_agg_args>(row_ptr, col_ind, n_edges, n_dst, n_src, node_ids, dim, dim, dim, aggr, out,
                                            out_stride, 2 * dim, n_src, n_dst);
  if (n_src > 0 && td.sizes[0] < 1) throw invalid_input("node ids into a table without rows");
  const auto* bk = backend();
  if (bk->gather_agg_forward == nullptr || !table_is_mapped(table)) return WHOLEMEMORY_NOT_SUPPORTED;
  WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(table, &a.gref));
  a.table_dtype          = td.dtype;
  a.table_rows           = td.sizes[0];
  a.table_stride         = td.strides[0];
  a.table_storage_offset = td.storage_offset;
  a.node_ids             = node_ids;
  a.node_id_dtype        = static_cast<wholememory_dtype_t>(node_id_dtype);
  a.out                  = out;
  a.out_stride           = out_stride;
  WM_BK(bk->gather_agg_forward(&a, stream));
  g_gather_agg_calls.fetch_add(1, std::memory_order_relaxed);
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

int64_t wholememory_ext_gather_aggregate_calls(void) { return g_gather_agg_calls.load(std::memory_order_relaxed); }

wholememory_error_code_t wholememory_ext_csc_gather_dequantize_aggregate_forward(
  wholememory_tensor_t table, int64_t dim, const void* node_ids, int node_id_dtype, const int32_t* row_ptr,
  const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, int aggr, float* out, int64_t out_stride,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  (void)p_env_fns;   // (the forward needs no scratch)
  if (table == nullptr) throw invalid_input("table is null");
  const wholememory_tensor_description_t td = *wholememory_tensor_get_tensor_description(table);
  if (td.dim != 2) throw invalid_input("the table must be a 2-D tensor");
  if (td.dtype != WHOLEMEMORY_DT_INT8) throw invalid_input("a quantized table must be INT8");
  if (td.strides[1] != 1) throw invalid_input("the table's rows must be contiguous");
  if (dim < 1) throw invalid_input("dim must be >= 1");
  const int64_t row_bytes = (dim + 3) / 4 * 4 + 8;
  if (td.sizes[1] < row_bytes)
    throw invalid_input(format_string("the table's rows hold %ld bytes, dim %ld needs %ld", static_cast<long>(td.sizes[1]),
                                      static_cast<long>(dim), static_cast<long>(row_bytes)));
  if (td.strides[0] < row_bytes || td.strides[0] % 4 != 0)
    throw invalid_input("the table's row stride must be >= the row's bytes and a multiple of 4");
  if (td.storage_offset % 4 != 0) throw invalid_input("the table's storage offset must be a multiple of 4 bytes");
  if (node_id_dtype != WHOLEMEMORY_DT_INT && node_id_dtype != WHOLEMEMORY_DT_INT64)
    throw invalid_input("node_id_dtype must be INT or INT64");
  // (the virtual x: n_src rows of `dim` values behind node_ids)
  auto a = checked_args<wm_qagg_args>(row_ptr, col_ind, n_edges, n_dst, n_src, node_ids, dim, dim, dim, aggr, out, out_stride,
                                      2 * dim, n_src, n_dst);
  if (n_src > 0 && td.sizes[0] < 1) throw invalid_input("node ids into a table without rows");
  const auto* bk = backend();
  if (bk->qagg_forward == nullptr || !table_is_mapped(table)) return WHOLEMEMORY_NOT_SUPPORTED;
  WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(table, &a.gref));
  a.table_rows           = td.sizes[0];
  a.table_stride         = td.strides[0];
  a.table_storage_offset = td.storage_offset;
  a.node_ids             = node_ids;
  a.node_id_dtype        = static_cast<wholememory_dtype_t>(node_id_dtype);
  a.out                  = out;
  a.out_stride           = out_stride;
  WM_BK(bk->qagg_forward(&a, stream));
  g_qagg_calls.fetch_add(1, std::memory_order_relaxed);
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

int64_t wholememory_ext_gather_dequantize_aggregate_calls(void) { return g_qagg_calls.load(std::memory_order_relaxed); }

wholememory_error_code_t wholememory_ext_csc_rel_aggregate_forward(const int32_t* row_ptr, const int32_t* col_ind,
                                                                   const int32_t* edge_type, int64_t n_edges, int64_t n_dst,
                                                                   int64_t n_src, int64_t num_relations, const float* x,
                                                                   int64_t x_stride, int64_t dim, int aggr, float* out,
                                                                   int64_t out_stride, float* edge_scale,
                                                                   wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  check_rel(edge_type, n_edges, num_relations, aggr, edge_scale);
  auto a = checked_args<wm_relagg_args>(row_ptr, col_ind, n_edges, n_dst, n_src, x, x_stride, dim, dim, aggr, out, out_stride,
                                        (num_relations + 1) * dim, n_src, n_dst);
  check_env(p_env_fns);   // (as the backward; the forward needs no scratch)
  const auto* bk = backend();
  if (bk->relagg_forward == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.edge_type     = edge_type;
  a.num_relations = num_relations;
  a.edge_scale    = a.mean ? edge_scale : nullptr;
  a.in            = x;
  a.in_stride     = x_stride;
  a.out           = out;
  a.out_stride    = out_stride;
  WM_BK(bk->relagg_forward(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_rel_aggregate_backward(const int32_t* row_ptr, const int32_t* col_ind,
                                                                    const int32_t* edge_type, int64_t n_edges, int64_t n_dst,
                                                                    int64_t n_src, int64_t num_relations,
                                                                    const float* edge_scale, const float* grad_out,
                                                                    int64_t grad_out_stride, int64_t dim, int aggr,
                                                                    float* grad_x, int64_t grad_x_stride,
                                                                    wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  check_rel(edge_type, n_edges, num_relations, aggr, edge_scale);
  auto a = checked_args<wm_relagg_args>(row_ptr, col_ind, n_edges, n_dst, n_src, grad_out, grad_out_stride,
                                        (num_relations + 1) * dim, dim, aggr, grad_x, grad_x_stride, dim, n_dst, n_src);
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->relagg_backward == nullptr || bk->agg_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.edge_type     = edge_type;
  a.num_relations = num_relations;
  a.edge_scale    = a.mean ? const_cast<float*>(edge_scale) : nullptr;   // (read only by the backward)
  a.grad          = grad_out;
  a.grad_stride   = grad_out_stride;
  a.out           = grad_x;
  a.out_stride    = grad_x_stride;
  agg_backward("relagg_backward", bk->relagg_backward, a, p_env_fns, stream);
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

}  // extern "C"

namespace {

// what the two _pna_ entry points check alike; `rows` / `rows_stride` / `rows_n`: the [n_dst, (A + 1) * dim] side (out, or
// grad_out), `other` / `other_stride` / `other_n`: the [n_src, dim] side (x, or grad_x)
wm_pna_args pna_args(const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src,
                     int64_t dim, int mask, const void* rows, int64_t rows_stride, const void* other, int64_t other_stride)
{
  wm_pna_args a{};
  static_cast<wm_csc_block&>(a) = checked_block(row_ptr, col_ind, n_edges, n_dst, n_src, n_edges > 0, "x");
  if (dim < 1) throw invalid_input("dim must be >= 1");
  if (mask < 1 || mask > WM_PNA_ALL) throw invalid_input("aggregators: a non-empty mask of the five WHOLEMEMORY_EXT_PNA_ bits");
  int slots = 1;
  for (int bit = 1; bit <= WM_PNA_STD; bit <<= 1) slots += (mask & bit) ? 1 : 0;
  check_rows(rows, n_dst > 0, rows_stride, slots * dim, "the targets' rows ((aggregators + 1) * dim columns)");
  check_rows(other, n_src > 0, other_stride, dim, "the sources' rows");
  a.dim  = dim;
  a.mask = mask;
  return a;
}

}  // namespace

extern "C" {

wholememory_error_code_t wholememory_ext_csc_pna_aggregate_forward(const int32_t* row_ptr, const int32_t* col_ind,
                                                                   int64_t n_edges, int64_t n_dst, int64_t n_src,
                                                                   const float* x, int64_t x_stride, int64_t dim,
                                                                   int aggregators, float eps, float* out,
                                                                   int64_t out_stride, int32_t* arg_min, int32_t* arg_max,
                                                                   float* std_mean, float* std_coef,
                                                                   wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  (void)p_env_fns;   // (the forward needs no scratch)
  auto a = pna_args(row_ptr, col_ind, n_edges, n_dst, n_src, dim, aggregators, out, out_stride, x, x_stride);
  if (!(eps >= 0.0f)) throw invalid_input("eps must be >= 0");
  const auto* bk = backend();
  if (bk->pna_forward == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.eps        = eps;
  a.in         = x;
  a.in_stride  = x_stride;
  a.out        = out;
  a.out_stride = out_stride;
  a.arg_min    = (aggregators & WM_PNA_MIN) ? arg_min : nullptr;
  a.arg_max    = (aggregators & WM_PNA_MAX) ? arg_max : nullptr;
  a.std_mean   = (aggregators & WM_PNA_STD) ? std_mean : nullptr;
  a.std_coef   = (aggregators & WM_PNA_STD) ? std_coef : nullptr;
  WM_BK(bk->pna_forward(&a, stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_csc_pna_aggregate_backward(
  const int32_t* row_ptr, const int32_t* col_ind, int64_t n_edges, int64_t n_dst, int64_t n_src, const float* x,
  int64_t x_stride, int64_t dim, int aggregators, const int32_t* arg_min, const int32_t* arg_max, const float* std_mean,
  const float* std_coef, const float* grad_out, int64_t grad_out_stride, float* grad_x, int64_t grad_x_stride,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  auto a = pna_args(row_ptr, col_ind, n_edges, n_dst, n_src, dim, aggregators, grad_out, grad_out_stride, grad_x,
                    grad_x_stride);
  if (n_dst > 0) {   // what the forward saved for the selected aggregators
    if ((aggregators & WM_PNA_MIN) && arg_min == nullptr) throw invalid_input("min is selected and arg_min is null");
    if ((aggregators & WM_PNA_MAX) && arg_max == nullptr) throw invalid_input("max is selected and arg_max is null");
    if ((aggregators & WM_PNA_STD) && (std_mean == nullptr || std_coef == nullptr))
      throw invalid_input("std is selected and std_mean or std_coef is null");
  }
  if (aggregators & WM_PNA_STD) check_rows(x, n_src > 0, x_stride, dim, "x (read for std)");   // the gradient of std reads x
  check_env(p_env_fns);
  const auto* bk = backend();
  if (bk->pna_backward == nullptr || bk->pna_backward_workspace_bytes == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  a.in          = x;
  a.in_stride   = x_stride;
  // (read only by the backward, and only for the selected aggregators)
  a.arg_min     = (aggregators & WM_PNA_MIN) ? const_cast<int32_t*>(arg_min) : nullptr;
  a.arg_max     = (aggregators & WM_PNA_MAX) ? const_cast<int32_t*>(arg_max) : nullptr;
  a.std_mean    = (aggregators & WM_PNA_STD) ? const_cast<float*>(std_mean) : nullptr;
  a.std_coef    = (aggregators & WM_PNA_STD) ? const_cast<float*>(std_coef) : nullptr;
  a.grad        = grad_out;
  a.grad_stride = grad_out_stride;
  a.out         = grad_x;
  a.out_stride  = grad_x_stride;
  if (n_src == 0) return WHOLEMEMORY_SUCCESS;
  backward_over_index(a, true, bk->pna_backward_workspace_bytes(a.n_edges, n_src, dim), p_env_fns, stream,
                      [&](const wm_edge_index& ix, void* ws) { WM_BK(bk->pna_backward(&a, ix, ws, stream)); });
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

}  // extern "C"
