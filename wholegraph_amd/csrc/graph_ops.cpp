// wholegraph_amd — host side of neighbour sampling and the small graph utilities (the C ABI of
// include/wholememory/wholegraph_op.h and graph_op.h). Kernels: kernels/graph.hip.
//
// Reference call stacks: wholegraph_csr_unweighted_sample_without_replacement
//   cpp/src/wholegraph_ops/unweighted_sample_without_replacement.cpp:24-190 (validation, dispatch on memory type)
//   -> ..._impl_mapped.cu -> ..._func.cuh:283-470 (count, scan, D2H of the total, output allocation, sample kernel);
// graph_append_unique cpp/src/graph_ops/append_unique.cpp:23-83 -> append_unique_func.cuh:300-353;
// csr_add_self_loop cpp/src/graph_ops/csr_add_self_loop.cpp:22-80.
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include <wholememory/graph_op.h>
#include <wholememory/wholegraph_op.h>
#include <wholememory/wholememory_op.h>

#include "csr_graph.hpp"
#include "knobs.hpp"
#include "neg_sample.hpp"
#include "ops_internal.hpp"
#include "pcg.hpp"
#include "tsample.hpp"
#include "walk_n2v.hpp"

namespace {

using namespace wm;

// one variable-size result handed to the caller's allocator (reference output_memory_handle.hpp:23-93)
void* output_alloc(wholememory_env_func_t* env, void* memory_context, int64_t count, wholememory_dtype_t dtype)
{
  wholememory_tensor_description_t d;
  wholememory_initialize_tensor_desc(&d);
  d.dim            = 1;
  d.sizes[0]       = count;
  d.strides[0]     = 1;
  d.dtype          = dtype;
  d.storage_offset = 0;
  return env->output_fns.malloc_fn(&d, WHOLEMEMORY_MA_DEVICE, memory_context, env->output_fns.global_context);
}

// a caller-side device array wrapped as a wholememory_tensor_t for the duration of one call
struct local_tensor {
  wholememory_tensor_t handle = nullptr;
  local_tensor(void* ptr, int64_t count, wholememory_dtype_t dtype)
  {
    wholememory_tensor_description_t d;
    wholememory_initialize_tensor_desc(&d);
    d.dim            = 1;
    d.sizes[0]       = count;
    d.strides[0]     = 1;
    d.dtype          = dtype;
    d.storage_offset = 0;
    if (wholememory_make_tensor_from_pointer(&handle, ptr, &d) != WHOLEMEMORY_SUCCESS) throw std::bad_alloc();
  }
  ~local_tensor()
  {
    if (handle != nullptr) wholememory_destroy_tensor(handle);
  }
  local_tensor(const local_tensor&)            = delete;
  local_tensor& operator=(const local_tensor&) = delete;
};

const wm_device_backend* graph_backend()
{
  const auto* bk = backend();
  if (bk->sample_unweighted == nullptr || bk->sample_weighted == nullptr || bk->append_unique_phase1 == nullptr) return nullptr;
  return bk;
}

constexpr int kMaxWeightedFanout = 8192;   // what the weighted sampler takes

// counts[0 .. n_center): what the sampler will emit per centre (row bounds from a.row_pairs when the graph is DISTRIBUTED)
int sample_counts(const wm_device_backend* bk, const wm_sample_args& a, const int* n_dev, int* counts, void* stream)
{
  return bk->sample_counts(a.row_pairs != nullptr ? nullptr : &a.row_gref, a.row_storage_offset, a.row_pairs, a.centers,
                           a.center_dtype, a.n_center, n_dev, a.max_sample_count, counts, stream);
}

// shared body of the two samplers; wm_csr_weight_ptr_tensor == nullptr selects the unweighted one
wholememory_error_code_t sample_without_replacement(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, bool weighted, wholememory_tensor_t center_nodes_tensor,
  int max_sample_count, wholememory_tensor_t output_sample_offset_tensor, void* output_dest_memory_context,
  void* output_center_localid_memory_context, void* output_edge_gid_memory_context, unsigned long long random_seed,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  const auto* bk = graph_backend();
  if (bk == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (p_env_fns == nullptr || output_dest_memory_context == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  checked_graph g{wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, false};
  wholememory_array_description_t center_desc, offset_desc;
  WHOLEMEMORY_RETURN_ON_FAIL(g.arrays());
  if (!array_of(center_nodes_tensor, "center_nodes_tensor", &center_desc, &err)) return err;
  if (!array_of(output_sample_offset_tensor, "output_sample_offset_tensor", &offset_desc, &err)) return err;
  // DISTRIBUTED CSR (reference ..._impl_nccl.cu / ..._nccl_func.cuh:196-390): the arrays are not addressable from this
  // rank, so row bounds and sampled columns travel through wholememory_gather (collective over the CSR's communicator)
  bool via_gather = false;
  WHOLEMEMORY_RETURN_ON_FAIL(g.placement(csr_tensors::row_col, nullptr, &via_gather));
  if (via_gather && weighted) {
    WM_ERROR("weighted sampling on DISTRIBUTED CSR tensors is not implemented (the reference has no such path either)");
    return WHOLEMEMORY_NOT_IMPLEMENTED;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.row_dtype());
  if (offset_desc.dtype != WHOLEMEMORY_DT_INT) {
    WM_ERROR("output_sample_offset_tensor must be int32, got %d", static_cast<int>(offset_desc.dtype));
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.col_and_id_dtype(center_desc.dtype, "center nodes"));
  const int64_t n = center_desc.size;
  if (n >= (INT64_C(1) << 31) - 1) return WHOLEMEMORY_INVALID_INPUT;
  if (offset_desc.size < n + 1) {
    WM_ERROR("output_sample_offset_tensor needs %ld entries, has %ld", static_cast<long>(n + 1),
             static_cast<long>(offset_desc.size));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (weighted) {
    WHOLEMEMORY_RETURN_ON_FAIL(g.weight_array());
    WHOLEMEMORY_RETURN_ON_FAIL(g.placement(
      csr_tensors::weights, "WEIGHTED sampling with a DISTRIBUTED weight tensor is not implemented (the reference has no such "
                            "path either; unweighted sampling on a DISTRIBUTED CSR is: see via_gather above)"));
    WHOLEMEMORY_RETURN_ON_FAIL(g.weight_dtype());
    WHOLEMEMORY_RETURN_ON_FAIL(g.one_weight_per_edge());
    if (max_sample_count > kMaxWeightedFanout) {
      // reference: key generation + cub segmented sort for > 256 samples (func.cuh:470-560); the in-LDS selection
      // built here covers 1..8192 (a candidate list of 2 M keys must fit the 160 KiB of LDS)
      WM_ERROR("weighted sampling with max_sample_count > 8192 is not implemented in this build");
      return WHOLEMEMORY_NOT_IMPLEMENTED;
    }
  }
  wm_sample_args a{};
  WHOLEMEMORY_RETURN_ON_FAIL(g.fill(&a));
  a.centers            = wholememory_tensor_get_data_pointer(center_nodes_tensor);
  a.center_dtype       = center_desc.dtype;
  a.n_center           = static_cast<int>(n);
  a.max_sample_count   = max_sample_count;
  a.random_seed        = random_seed;
  int* offsets         = static_cast<int*>(wholememory_tensor_get_data_pointer(output_sample_offset_tensor));
  a.sample_offsets     = offsets;

  // per-center counts -> exclusive scan into the caller's offset tensor -> total on the host
  temp_mem counts_mem(p_env_fns), scan_mem(p_env_fns);
  int* counts           = static_cast<int*>(counts_mem.device(n + 1, WHOLEMEMORY_DT_INT));
  const size_t scan_ws  = bk->scan_i32_workspace_bytes(n + 1);
  void* scan_ws_ptr     = scan_mem.device(static_cast<int64_t>(scan_ws), WHOLEMEMORY_DT_INT8);
  temp_mem pair_ids_mem(p_env_fns), pairs_mem(p_env_fns), egid_mem(p_env_fns);
  if (via_gather) {
    // (row_ptr[c], row_ptr[c + 1]) of every center node in one gather
    int64_t* pair_ids = static_cast<int64_t*>(pair_ids_mem.device(2 * n, WHOLEMEMORY_DT_INT64));
    int64_t* pairs    = static_cast<int64_t*>(pairs_mem.device(2 * n, WHOLEMEMORY_DT_INT64));
    WM_BK(bk->sample_pair_ids(a.centers, a.center_dtype, a.n_center, pair_ids, stream));
    local_tensor ids_t(pair_ids, 2 * n, WHOLEMEMORY_DT_INT64), pairs_t(pairs, 2 * n, WHOLEMEMORY_DT_INT64);
    WHOLEMEMORY_RETURN_ON_FAIL(wholememory_gather(wm_csr_row_ptr_tensor, ids_t.handle, pairs_t.handle, p_env_fns, stream, -1));
    a.row_pairs = pairs;
  }
  WM_BK(sample_counts(bk, a, nullptr, counts, stream));
  WM_BK(bk->exclusive_scan_i32(counts, offsets, n + 1, scan_ws_ptr, scan_ws, stream));
  int total = 0;
  WM_BK(bk->memcpy_async(&total, offsets + n, sizeof(int), stream));
  WM_BK(bk->stream_sync(stream));

  a.out_ids = output_alloc(p_env_fns, output_dest_memory_context, total, a.col_dtype);
  if (output_center_localid_memory_context != nullptr)
    a.out_center_lid = static_cast<int*>(output_alloc(p_env_fns, output_center_localid_memory_context, total, WHOLEMEMORY_DT_INT));
  if (output_edge_gid_memory_context != nullptr)
    a.out_edge_gid = static_cast<int64_t*>(output_alloc(p_env_fns, output_edge_gid_memory_context, total, WHOLEMEMORY_DT_INT64));
  if (total > 0 && a.out_ids == nullptr) return WHOLEMEMORY_OUT_OF_MEMORY;
  if (via_gather) {
    // positions first (edge ids), then the columns by one more gather; every rank takes part even with nothing to sample
    void* out_ids = a.out_ids;
    a.out_ids     = nullptr;
    if (a.out_edge_gid == nullptr) a.out_edge_gid = static_cast<int64_t*>(egid_mem.device(total, WHOLEMEMORY_DT_INT64));
    if (total > 0) WM_BK(bk->sample_unweighted(&a, stream));
    local_tensor egid_t(a.out_edge_gid, total, WHOLEMEMORY_DT_INT64), out_t(out_ids, total, a.col_dtype);
    WHOLEMEMORY_RETURN_ON_FAIL(wholememory_gather(wm_csr_col_ptr_tensor, egid_t.handle, out_t.handle, p_env_fns, stream, -1));
  } else if (total > 0) {
    WM_BK(weighted ? bk->sample_weighted(&a, stream) : bk->sample_unweighted(&a, stream));
  }
  // The reference returns with the samples complete (:385,:404), and so does this by default. A host framework whose env
  // allocator is ordered on `stream`, like every consumer of the outputs, may declare that
  // (wholememory_ext_set_async_completion): the call then returns with the kernels queued — one host round trip per call
  // (the count) instead of two. The DISTRIBUTED route keeps the drain: its gathers are
  // collectives and peers read this rank's buffers.
  if (via_gather || !async_completion_enabled() || debug_sync_enabled()) WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
}

}  // namespace

extern "C" {

wholememory_error_code_t wholegraph_csr_unweighted_sample_without_replacement(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t center_nodes_tensor, int max_sample_count, wholememory_tensor_t output_sample_offset_tensor,
  void* output_dest_memory_context, void* output_center_localid_memory_context, void* output_edge_gid_memory_context,
  unsigned long long random_seed, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  return sample_without_replacement(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, nullptr, false, center_nodes_tensor,
                                    max_sample_count, output_sample_offset_tensor, output_dest_memory_context,
                                    output_center_localid_memory_context, output_edge_gid_memory_context, random_seed,
                                    p_env_fns, stream);
  WM_API_END
}

wholememory_error_code_t wholegraph_csr_weighted_sample_without_replacement(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t center_nodes_tensor, int max_sample_count,
  wholememory_tensor_t output_sample_offset_tensor, void* output_dest_memory_context,
  void* output_center_localid_memory_context, void* output_edge_gid_memory_context, unsigned long long random_seed,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  return sample_without_replacement(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, true,
                                    center_nodes_tensor, max_sample_count, output_sample_offset_tensor,
                                    output_dest_memory_context, output_center_localid_memory_context,
                                    output_edge_gid_memory_context, random_seed, p_env_fns, stream);
  WM_API_END
}

// Random walks (extension, wholegraph_amd_ext.h sections 2m and 2n; kernels/walk.hip, kernels/walk_n2v.hip): n walks of
// walk_length steps as ONE launch on `stream`. The outputs are the caller's, their sizes known beforehand: nothing is
// allocated, nothing read back, the call does not synchronise, and every answer but SUCCESS is given before any device work.
namespace {

// an output that is the dense [n, width] block, given as a 2-D tensor of that shape or as a 1-D one of n * width entries
bool dense_block(wholememory_tensor_t t, int64_t n, int64_t width)
{
  const auto d = *wholememory_tensor_get_tensor_description(t);
  if (d.dim == 1) return d.sizes[0] == n * width && (d.strides[0] == 1 || d.sizes[0] <= 1);
  return d.dim == 2 && d.sizes[0] == n && d.sizes[1] == width && d.strides[1] == 1 && (d.strides[0] == width || n <= 1);
}

// the walks' own tensors, next to the graph: check() answers what section 2m lists, in its order, and touches no device;
// fill() fills the backend's argument block
struct walk_call {
  checked_graph g;
  wholememory_tensor_t start_nodes_tensor;
  int walk_length;
  wholememory_tensor_t output_walks_tensor, output_edge_ids_tensor;
  wholememory_array_description_t start_desc;

  wholememory_error_code_t check();
  wholememory_error_code_t fill(unsigned long long random_seed, wm_walk_args& a) const;
};

wholememory_error_code_t walk_call::check()
{
  if (output_walks_tensor == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  WHOLEMEMORY_RETURN_ON_FAIL(g.arrays());
  if (!array_of(start_nodes_tensor, "start_nodes_tensor", &start_desc, &err)) return err;
  if (walk_length < 1) {
    WM_ERROR("walk_length must be at least 1, got %d", walk_length);
    return WHOLEMEMORY_INVALID_INPUT;
  }
  const int64_t n = start_desc.size, L = walk_length;
  if (n < 0 || g.row_desc.size < 1 || n > ((INT64_C(1) << 31) - 1) / (L + 1)) {
    WM_ERROR("%ld walks of %d steps: the outputs must hold fewer than 2^31 entries", static_cast<long>(n), walk_length);
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (!dense_block(output_walks_tensor, n, L + 1) ||
      (output_edge_ids_tensor != nullptr && !dense_block(output_edge_ids_tensor, n, L))) {
    WM_ERROR("output_walks_tensor must be [%ld, %ld] and output_edge_ids_tensor [%ld, %ld], dense", static_cast<long>(n),
             static_cast<long>(L + 1), static_cast<long>(n), static_cast<long>(L));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  const bool weighted = g.weight != nullptr;
  if (weighted) {
    WHOLEMEMORY_RETURN_ON_FAIL(g.weight_array());
    WHOLEMEMORY_RETURN_ON_FAIL(g.one_weight_per_edge());
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.row_dtype());
  WHOLEMEMORY_RETURN_ON_FAIL(g.col_and_id_dtype(start_desc.dtype, "start nodes"));
  if (wholememory_tensor_get_tensor_description(output_walks_tensor)->dtype != g.col_desc.dtype) {
    WM_ERROR("output_walks_tensor must have the dtype of wm_csr_col_ptr_tensor");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  if (output_edge_ids_tensor != nullptr &&
      wholememory_tensor_get_tensor_description(output_edge_ids_tensor)->dtype != WHOLEMEMORY_DT_INT64) {
    WM_ERROR("output_edge_ids_tensor must be int64");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  if (weighted) WHOLEMEMORY_RETURN_ON_FAIL(g.weight_dtype());
  return g.placement(csr_tensors::all,
                     "random walks on DISTRIBUTED tensors are not implemented: every step would be a collective gather");
}

wholememory_error_code_t walk_call::fill(unsigned long long random_seed, wm_walk_args& a) const
{
  a = wm_walk_args{};
  WHOLEMEMORY_RETURN_ON_FAIL(g.fill(&a));
  a.starts       = wholememory_tensor_get_data_pointer(start_nodes_tensor);
  a.start_dtype  = start_desc.dtype;
  a.n            = start_desc.size;
  a.walk_length  = walk_length;
  a.random_seed  = random_seed;
  a.out_walks    = wholememory_tensor_get_data_pointer(output_walks_tensor);
  a.out_edge_ids = output_edge_ids_tensor != nullptr
                     ? static_cast<int64_t*>(wholememory_tensor_get_data_pointer(output_edge_ids_tensor))
                     : nullptr;
  if (a.starts == nullptr || a.out_walks == nullptr || (output_edge_ids_tensor != nullptr && a.out_edge_ids == nullptr))
    return WHOLEMEMORY_INVALID_INPUT;
  return WHOLEMEMORY_SUCCESS;
}

}  // namespace

wholememory_error_code_t wholememory_ext_csr_random_walk(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t start_nodes_tensor, int walk_length,
  unsigned long long random_seed, wholememory_tensor_t output_walks_tensor, wholememory_tensor_t output_edge_ids_tensor,
  void* stream)
{
  WM_API_BEGIN
  walk_call c{{wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, false}, start_nodes_tensor, walk_length,
              output_walks_tensor, output_edge_ids_tensor};
  WHOLEMEMORY_RETURN_ON_FAIL(c.check());
  const auto* bk = backend();
  if (bk->walk_uniform == nullptr || bk->walk_weighted == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (c.start_desc.size == 0) return WHOLEMEMORY_SUCCESS;
  wm_walk_args a;
  WHOLEMEMORY_RETURN_ON_FAIL(c.fill(random_seed, a));
  WM_BK(wm_csr_weight_ptr_tensor != nullptr ? bk->walk_weighted(&a, stream) : bk->walk_uniform(&a, stream));
  if (debug_sync_enabled()) WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

// node2vec (p, q) walks (section 2n): the tensors of section 2m, checked by the same code, and the step rule's own arguments
wholememory_error_code_t wholememory_ext_csr_node2vec_walk(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t start_nodes_tensor, int walk_length,
  float p, float q, int col_sorted, unsigned long long random_seed, wholememory_tensor_t output_walks_tensor,
  wholememory_tensor_t output_edge_ids_tensor, void* stream)
{
  WM_API_BEGIN
  walk_call c{{wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, false}, start_nodes_tensor, walk_length,
              output_walks_tensor, output_edge_ids_tensor};
  WHOLEMEMORY_RETURN_ON_FAIL(c.check());
  if (!wm::n2v_pq_ok(p, q)) {
    WM_ERROR("p and q and their fp32 reciprocals must be finite and > 0, got p = %g, q = %g", static_cast<double>(p),
             static_cast<double>(q));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  const auto* bk = backend();
  if (bk->walk_node2vec == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (c.start_desc.size == 0) return WHOLEMEMORY_SUCCESS;
  wm_n2v_args a;
  WHOLEMEMORY_RETURN_ON_FAIL(c.fill(random_seed, a.walk));
  a.inv_p      = 1.0f / p;
  a.inv_q      = 1.0f / q;
  a.col_sorted = col_sorted;
  WM_BK(bk->walk_node2vec(&a, stream));
  if (debug_sync_enabled()) WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

// Negative sampling (extension, wholegraph_amd_ext.h section 2o; kernels/neg_sample.hip): num_negatives nodes per source that
// are not the source and not in its row, as ONE launch on `stream`. The output is the caller's: nothing is allocated, nothing
// read back, the call does not synchronise, and every answer but SUCCESS is given before any device work.
wholememory_error_code_t wholememory_ext_csr_negative_sample(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor, wholememory_tensor_t src_nodes_tensor,
  int num_negatives, int mode, int exclude, int max_tries, int col_sorted, unsigned long long random_seed,
  wholememory_tensor_t output_negatives_tensor, void* stream)
{
  WM_API_BEGIN
  if (output_negatives_tensor == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  checked_graph g{wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, nullptr, false};
  wholememory_array_description_t src_desc;
  WHOLEMEMORY_RETURN_ON_FAIL(g.arrays());
  if (!array_of(src_nodes_tensor, "src_nodes_tensor", &src_desc, &err)) return err;
  if (!wm::neg_scalars_ok(num_negatives, mode, exclude, max_tries)) {
    WM_ERROR("num_negatives must be >= 1, mode 0 or 1, exclude in [0, 3] and max_tries in [1, 64], got %d, %d, %d, %d",
             num_negatives, mode, exclude, max_tries);
    return WHOLEMEMORY_INVALID_INPUT;
  }
  const int64_t n = src_desc.size, K = num_negatives;
  if (n < 0 || g.row_desc.size < 1 || n > ((INT64_C(1) << 31) - 1) / K) {
    WM_ERROR("%ld sources of %d negatives: the output must hold fewer than 2^31 entries", static_cast<long>(n), num_negatives);
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (!dense_block(output_negatives_tensor, n, K)) {
    WM_ERROR("output_negatives_tensor must be [%ld, %ld], dense", static_cast<long>(n), static_cast<long>(K));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.row_dtype());
  WHOLEMEMORY_RETURN_ON_FAIL(g.col_and_id_dtype(src_desc.dtype, "source nodes"));
  if (wholememory_tensor_get_tensor_description(output_negatives_tensor)->dtype != g.col_desc.dtype) {
    WM_ERROR("output_negatives_tensor must have the dtype of wm_csr_col_ptr_tensor");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.placement(
    csr_tensors::row_col,
    "negative sampling on DISTRIBUTED tensors is not implemented: every membership test would be a collective gather"));
  const auto* bk = backend();
  if (bk->negative_sample == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (n == 0) return WHOLEMEMORY_SUCCESS;
  wm_neg_args a{};
  WHOLEMEMORY_RETURN_ON_FAIL(g.fill(&a));
  a.src                = wholememory_tensor_get_data_pointer(src_nodes_tensor);
  a.src_dtype          = src_desc.dtype;
  a.n                  = n;
  a.num_negatives      = num_negatives;
  a.mode               = mode;
  a.exclude            = exclude;
  a.max_tries          = max_tries;
  a.col_sorted         = col_sorted;
  a.random_seed        = random_seed;
  a.out                = wholememory_tensor_get_data_pointer(output_negatives_tensor);
  if (a.src == nullptr || a.out == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  WM_BK(bk->negative_sample(&a, stream));
  if (debug_sync_enabled()) WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

// Node-induced subgraph (extension, wholegraph_amd_ext.h section 2q; kernels/isub.hip): the block of subgraph-wise training,
// every graph edge among `nodes`, as local CSR arrays. The sampler's shape: count per row, scan into the caller's offsets, ONE
// host round trip for the size, outputs from the caller's allocator, fill. Every answer about the arguments comes before any
// device work; the answer about the size (2^31 entries or more) comes after the count, with no output allocated.
wholememory_error_code_t wholememory_ext_csr_induced_subgraph(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor, wholememory_tensor_t nodes_tensor,
  wholememory_tensor_t output_offset_tensor, void* output_col_memory_context, void* output_edge_gid_memory_context,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  if (p_env_fns == nullptr || output_col_memory_context == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  checked_graph g{wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, nullptr, false};
  wholememory_array_description_t nodes_desc, offset_desc;
  WHOLEMEMORY_RETURN_ON_FAIL(g.arrays());
  if (!array_of(nodes_tensor, "nodes_tensor", &nodes_desc, &err)) return err;
  if (!array_of(output_offset_tensor, "output_offset_tensor", &offset_desc, &err)) return err;
  const int64_t n = nodes_desc.size;
  if (n < 0 || g.row_desc.size < 1 || n >= (INT64_C(1) << 31) - 1) {
    WM_ERROR("%ld nodes: the subgraph must have fewer than 2^31 - 1 rows", static_cast<long>(n));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (offset_desc.size < n + 1) {
    WM_ERROR("output_offset_tensor needs %ld entries, has %ld", static_cast<long>(n + 1), static_cast<long>(offset_desc.size));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.row_dtype());
  WHOLEMEMORY_RETURN_ON_FAIL(g.col_and_id_dtype(nodes_desc.dtype, "nodes"));
  if (offset_desc.dtype != WHOLEMEMORY_DT_INT) {
    WM_ERROR("output_offset_tensor must be int32, got %d", static_cast<int>(offset_desc.dtype));
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.placement(
    csr_tensors::row_col,
    "the induced subgraph of DISTRIBUTED tensors is not implemented: every membership probe would be a collective gather"));
  const auto* bk = backend();
  if (bk->isub_workspace_bytes == nullptr || bk->isub_build == nullptr || bk->isub_count == nullptr || bk->isub_fill == nullptr ||
      bk->exclusive_scan_i32 == nullptr)
    return WHOLEMEMORY_NOT_SUPPORTED;
  int* offsets = static_cast<int*>(wholememory_tensor_get_data_pointer(output_offset_tensor));
  if (offsets == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  const bool drain = !async_completion_enabled() || debug_sync_enabled();
  if (n == 0) {
    WM_BK(bk->memset_async(offsets, 0, sizeof(int), stream));
    (void)output_alloc(p_env_fns, output_col_memory_context, 0, WHOLEMEMORY_DT_INT);
    if (output_edge_gid_memory_context != nullptr) (void)output_alloc(p_env_fns, output_edge_gid_memory_context, 0, WHOLEMEMORY_DT_INT64);
    if (drain) WM_BK(bk->stream_sync(stream));
    return WHOLEMEMORY_SUCCESS;
  }
  wm_isub_args a{};
  WHOLEMEMORY_RETURN_ON_FAIL(g.fill(&a));
  a.nodes      = wholememory_tensor_get_data_pointer(nodes_tensor);
  a.node_dtype = nodes_desc.dtype;
  a.n          = n;
  a.offsets    = offsets;
  if (a.nodes == nullptr) return WHOLEMEMORY_INVALID_INPUT;

  temp_mem ws_mem(p_env_fns), counts_mem(p_env_fns), scan_mem(p_env_fns), host_mem(p_env_fns);
  size_t table_bytes    = 0;
  const size_t ws_bytes = bk->isub_workspace_bytes(n, &table_bytes);
  a.workspace           = ws_mem.device(static_cast<int64_t>(ws_bytes), WHOLEMEMORY_DT_INT8);
  a.counts              = static_cast<int*>(counts_mem.device(n + 1, WHOLEMEMORY_DT_INT));
  const size_t scan_ws  = bk->scan_i32_workspace_bytes(n + 1);
  void* scan_ws_ptr     = scan_mem.device(static_cast<int64_t>(scan_ws), WHOLEMEMORY_DT_INT8);
  a.total               = static_cast<int64_t*>(host_mem.pinned(1, WHOLEMEMORY_DT_INT64));   // written by the count's last kernel
  if (a.workspace == nullptr || a.counts == nullptr || scan_ws_ptr == nullptr || a.total == nullptr) return WHOLEMEMORY_OUT_OF_MEMORY;

  // table, rows counted, offsets, and the 64-bit total on the host: the one round trip of the call
  WM_BK(bk->fill_ff_async != nullptr ? bk->fill_ff_async(a.workspace, table_bytes, stream)
                                     : bk->memset_async(a.workspace, 0xFF, table_bytes, stream));
  WM_BK(bk->isub_build(&a, stream));
  WM_BK(bk->isub_count(&a, stream));
  WM_BK(bk->exclusive_scan_i32(a.counts, offsets, n + 1, scan_ws_ptr, scan_ws, stream));
  WM_BK(bk->stream_sync(stream));
  const int64_t m = *a.total;
  if (m < 0 || m >= (INT64_C(1) << 31)) {
    WM_ERROR("the induced subgraph of these %ld nodes has %ld entries: the outputs must hold fewer than 2^31", static_cast<long>(n),
             static_cast<long>(m));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  a.out_col = static_cast<int*>(output_alloc(p_env_fns, output_col_memory_context, m, WHOLEMEMORY_DT_INT));
  if (output_edge_gid_memory_context != nullptr)
    a.out_edge_gid = static_cast<int64_t*>(output_alloc(p_env_fns, output_edge_gid_memory_context, m, WHOLEMEMORY_DT_INT64));
  if (m > 0 && (a.out_col == nullptr || (output_edge_gid_memory_context != nullptr && a.out_edge_gid == nullptr)))
    return WHOLEMEMORY_OUT_OF_MEMORY;
  if (m > 0) WM_BK(bk->isub_fill(&a, stream));
  // as the sampler: complete on return, unless the host framework has declared its allocator ordered on `stream`
  if (drain) WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

// Temporal neighbour sampling (extension, wholegraph_amd_ext.h section 2r; kernels/tsample.hip): per centre, the neighbours whose
// edge time passes the rule against the centre's time, at most max_sample_count of them. The flow of the induced subgraph:
// count per centre, scan into the caller's offsets, ONE host round trip for the size, outputs from the caller's allocator,
// select. Every answer about the arguments comes before any device work; the answer about the size (2^31 entries or more,
// reachable with max_sample_count <= 0 only) comes after the count, with no output allocated.
wholememory_error_code_t wholememory_ext_csr_temporal_sample(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor, wholememory_tensor_t wm_csr_edge_time_tensor,
  wholememory_tensor_t center_nodes_tensor, wholememory_tensor_t center_times_tensor, int max_sample_count, int strategy,
  int inclusive, long long time_window, unsigned long long random_seed, wholememory_tensor_t output_offset_tensor,
  void* output_dest_memory_context, void* output_center_localid_memory_context, void* output_edge_gid_memory_context,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  if (p_env_fns == nullptr || output_dest_memory_context == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  checked_graph g{wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, nullptr, false};
  g.time = wm_csr_edge_time_tensor;
  wholememory_array_description_t center_desc, ctime_desc, offset_desc;
  WHOLEMEMORY_RETURN_ON_FAIL(g.arrays());
  WHOLEMEMORY_RETURN_ON_FAIL(g.time_array());
  if (!array_of(center_nodes_tensor, "center_nodes_tensor", &center_desc, &err)) return err;
  if (!array_of(center_times_tensor, "center_times_tensor", &ctime_desc, &err)) return err;
  if (!array_of(output_offset_tensor, "output_offset_tensor", &offset_desc, &err)) return err;
  if (!wm::ts_scalars_ok(max_sample_count, strategy)) {
    WM_ERROR("max_sample_count must be at most %d and strategy 0 (uniform) or 1 (last), got %d and %d", wm::kTsampleMaxFanout,
             max_sample_count, strategy);
    return WHOLEMEMORY_INVALID_INPUT;
  }
  const int64_t n = center_desc.size;
  if (g.row_desc.size < 1) {
    WM_ERROR("wm_csr_row_ptr_tensor has no entry: a graph of n_nodes nodes has n_nodes + 1");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (n < 0 || n >= (INT64_C(1) << 31) - 1) {
    WM_ERROR("%ld centres: a batch must have fewer than 2^31 - 1", static_cast<long>(n));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.one_time_per_edge());
  if (ctime_desc.size != n) {
    WM_ERROR("center_times_tensor must have one time per centre (%ld vs %ld)", static_cast<long>(ctime_desc.size), static_cast<long>(n));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (offset_desc.size < n + 1) {
    WM_ERROR("output_offset_tensor needs %ld entries, has %ld", static_cast<long>(n + 1), static_cast<long>(offset_desc.size));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.row_dtype());
  WHOLEMEMORY_RETURN_ON_FAIL(g.col_and_id_dtype(center_desc.dtype, "center nodes"));
  WHOLEMEMORY_RETURN_ON_FAIL(g.time_dtype());
  if (ctime_desc.dtype != WHOLEMEMORY_DT_INT64) {
    WM_ERROR("center_times_tensor must be int64, got %d", static_cast<int>(ctime_desc.dtype));
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  if (offset_desc.dtype != WHOLEMEMORY_DT_INT) {
    WM_ERROR("output_offset_tensor must be int32, got %d", static_cast<int>(offset_desc.dtype));
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  WHOLEMEMORY_RETURN_ON_FAIL(g.placement(
    csr_tensors::row_col_time,
    "temporal sampling on DISTRIBUTED tensors is not implemented here: Python composes the route from the all-neighbour sampler, "
    "a gather of the times and this op on the gathered rows (wholegraph_ops.temporal_sample_without_replacement)"));
  const auto* bk = backend();
  if (bk->tsample_workspace_bytes == nullptr || bk->tsample_count == nullptr || bk->tsample_select == nullptr ||
      bk->exclusive_scan_i32 == nullptr)
    return WHOLEMEMORY_NOT_SUPPORTED;
  int* offsets = static_cast<int*>(wholememory_tensor_get_data_pointer(output_offset_tensor));
  if (offsets == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  const bool drain = !async_completion_enabled() || debug_sync_enabled();
  if (n == 0) {
    WM_BK(bk->memset_async(offsets, 0, sizeof(int), stream));
    (void)output_alloc(p_env_fns, output_dest_memory_context, 0, g.col_desc.dtype);
    if (output_center_localid_memory_context != nullptr) (void)output_alloc(p_env_fns, output_center_localid_memory_context, 0, WHOLEMEMORY_DT_INT);
    if (output_edge_gid_memory_context != nullptr) (void)output_alloc(p_env_fns, output_edge_gid_memory_context, 0, WHOLEMEMORY_DT_INT64);
    if (drain) WM_BK(bk->stream_sync(stream));
    return WHOLEMEMORY_SUCCESS;
  }
  wm_tsample_args a{};
  WHOLEMEMORY_RETURN_ON_FAIL(g.fill(&a));
  a.centers          = wholememory_tensor_get_data_pointer(center_nodes_tensor);
  a.center_dtype     = center_desc.dtype;
  a.center_times     = static_cast<const int64_t*>(wholememory_tensor_get_data_pointer(center_times_tensor));
  a.n                = n;
  a.max_sample_count = max_sample_count;
  a.strategy         = strategy;
  a.inclusive        = inclusive;
  a.time_window      = time_window;
  a.random_seed      = random_seed;
  a.offsets          = offsets;
  if (a.centers == nullptr || a.center_times == nullptr) return WHOLEMEMORY_INVALID_INPUT;

  temp_mem ws_mem(p_env_fns), counts_mem(p_env_fns), scan_mem(p_env_fns), host_mem(p_env_fns);
  a.workspace          = ws_mem.device(static_cast<int64_t>(bk->tsample_workspace_bytes(n)), WHOLEMEMORY_DT_INT8);
  a.counts             = static_cast<int*>(counts_mem.device(n + 1, WHOLEMEMORY_DT_INT));
  const size_t scan_ws = bk->scan_i32_workspace_bytes(n + 1);
  void* scan_ws_ptr    = scan_mem.device(static_cast<int64_t>(scan_ws), WHOLEMEMORY_DT_INT8);
  a.total              = static_cast<int64_t*>(host_mem.pinned(1, WHOLEMEMORY_DT_INT64));   // written by the count's last kernel
  if (a.workspace == nullptr || a.counts == nullptr || scan_ws_ptr == nullptr || a.total == nullptr) return WHOLEMEMORY_OUT_OF_MEMORY;

  // centres counted, offsets, and the 64-bit total on the host: the one round trip of the call
  WM_BK(bk->tsample_count(&a, stream));
  WM_BK(bk->exclusive_scan_i32(a.counts, offsets, n + 1, scan_ws_ptr, scan_ws, stream));
  WM_BK(bk->stream_sync(stream));
  const int64_t m = *a.total;
  if (m < 0 || m >= (INT64_C(1) << 31)) {
    WM_ERROR("the temporal sample of these %ld centres has %ld entries: the outputs must hold fewer than 2^31", static_cast<long>(n),
             static_cast<long>(m));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  a.out_ids = output_alloc(p_env_fns, output_dest_memory_context, m, a.col_dtype);
  if (output_center_localid_memory_context != nullptr)
    a.out_center_lid = static_cast<int*>(output_alloc(p_env_fns, output_center_localid_memory_context, m, WHOLEMEMORY_DT_INT));
  if (output_edge_gid_memory_context != nullptr)
    a.out_edge_gid = static_cast<int64_t*>(output_alloc(p_env_fns, output_edge_gid_memory_context, m, WHOLEMEMORY_DT_INT64));
  if (m > 0 && (a.out_ids == nullptr || (output_center_localid_memory_context != nullptr && a.out_center_lid == nullptr) ||
                (output_edge_gid_memory_context != nullptr && a.out_edge_gid == nullptr)))
    return WHOLEMEMORY_OUT_OF_MEMORY;
  if (m > 0) WM_BK(bk->tsample_select(&a, stream));
  // as the sampler: complete on return, unless the host framework has declared its allocator ordered on `stream`
  if (drain) WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t generate_random_positive_int_cpu(int64_t random_seed, int64_t subsequence, wholememory_tensor_t output)
{
  WM_API_BEGIN
  if (output == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  const auto d = *wholememory_tensor_get_tensor_description(output);
  if (d.dim != 1) {
    WM_ERROR("output should be 1D tensor.");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (!is_index_dtype(d.dtype)) {
    WM_ERROR("output should be int64 or int32 tensor.");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  void* p = wholememory_tensor_get_data_pointer(output);
  pcg32 rng(static_cast<uint64_t>(random_seed), 0, static_cast<uint64_t>(subsequence));
  for (int64_t i = 0; i < d.sizes[0]; i++) {
    if (d.dtype == WHOLEMEMORY_DT_INT)
      static_cast<int32_t*>(p)[i] = rng.next_i32();
    else
      static_cast<int64_t*>(p)[i] = rng.next_i64();
  }
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t generate_exponential_distribution_negative_float_cpu(int64_t random_seed, int64_t subsequence,
                                                                              wholememory_tensor_t output)
{
  WM_API_BEGIN
  if (output == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  const auto d = *wholememory_tensor_get_tensor_description(output);
  if (d.dim != 1) {
    WM_ERROR("output should be 1D tensor.");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (d.dtype != WHOLEMEMORY_DT_FLOAT) {
    WM_ERROR("output should be float.");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  float* p = static_cast<float*>(wholememory_tensor_get_data_pointer(output));
  pcg32 rng(static_cast<uint64_t>(random_seed), 0, static_cast<uint64_t>(subsequence));
  // log2 of a uniform in (0,1) built from a mantissa in [0.5,1) and a geometric exponent = the number of leading zero
  // bits of a 64-bit stream (redrawn while it is all zeros): raft_random_gen.cu:83-105
  for (int64_t i = 0; i < d.sizes[0]; i++) {
    float u = rng.next_float();
    u       = static_cast<float>(-(0.5 + 0.5 * static_cast<double>(u)));
    uint64_t bits;
    int redraws = -1;
    do {
      bits = rng.next_u64();
      redraws++;
    } while (bits == 0);
    const int zeros = __builtin_clzll(bits) + redraws * 64;
    u               = static_cast<float>(static_cast<double>(u) * std::pow(2.0, -zeros));
    p[i]            = static_cast<float>(std::log1p(static_cast<double>(u)) / std::log(2.0));
  }
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t graph_append_unique(wholememory_tensor_t target_nodes_tensor,
                                             wholememory_tensor_t neighbor_nodes_tensor,
                                             void* output_unique_node_memory_context,
                                             wholememory_tensor_t output_neighbor_raw_to_unique_mapping_tensor,
                                             wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk = graph_backend();
  if (bk == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (p_env_fns == nullptr || output_unique_node_memory_context == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  wholememory_array_description_t target_desc, neighbor_desc;
  if (!array_of(target_nodes_tensor, "target_nodes_tensor", &target_desc, &err)) return err;
  if (!array_of(neighbor_nodes_tensor, "neighbor_nodes_tensor", &neighbor_desc, &err)) return err;
  if (target_desc.dtype != neighbor_desc.dtype) {  // append_unique.cpp:45-49
    WM_ERROR("target_nodes_dtype should be the same with neighbor_nodes_dtype");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  if (!is_index_dtype(target_desc.dtype)) {
    WM_ERROR("node ids must be int32 or int64");
    return WHOLEMEMORY_LOGIC_ERROR;
  }
  int* mapping = nullptr;
  if (output_neighbor_raw_to_unique_mapping_tensor != nullptr) {
    wholememory_array_description_t map_desc;
    if (!array_of(output_neighbor_raw_to_unique_mapping_tensor, "output_neighbor_raw_to_unique_mapping_tensor", &map_desc, &err))
      return err;
    if (map_desc.size != neighbor_desc.size) {  // append_unique.cpp:63-68
      WM_ERROR("output_neighbor_raw_to_unique_mapping size should be the same as neighbor_nodes");
      return WHOLEMEMORY_INVALID_INPUT;
    }
    if (map_desc.dtype != WHOLEMEMORY_DT_INT) {
      WM_ERROR("output_neighbor_raw_to_unique_mapping must be int32");
      return WHOLEMEMORY_LOGIC_ERROR;
    }
    mapping = static_cast<int*>(wholememory_tensor_get_data_pointer(output_neighbor_raw_to_unique_mapping_tensor));
  }
  if (target_desc.size + neighbor_desc.size >= (INT64_C(1) << 31) - 1) return WHOLEMEMORY_INVALID_INPUT;
  const int nt = static_cast<int>(target_desc.size), nn = static_cast<int>(neighbor_desc.size);
  const void* targets   = wholememory_tensor_get_data_pointer(target_nodes_tensor);
  const void* neighbors = wholememory_tensor_get_data_pointer(neighbor_nodes_tensor);
  if (nt + nn == 0) {
    (void)output_alloc(p_env_fns, output_unique_node_memory_context, 0, target_desc.dtype);
    return WHOLEMEMORY_SUCCESS;
  }
  temp_mem ws_mem(p_env_fns), host_mem(p_env_fns);
  void* ws  = ws_mem.device(static_cast<int64_t>(bk->append_unique_workspace_bytes(nt, nn, target_desc.dtype)), WHOLEMEMORY_DT_INT8);
  int* host = static_cast<int*>(host_mem.pinned(2, WHOLEMEMORY_DT_INT));   // written by the phase's last kernel
  WM_BK(bk->append_unique_phase1(targets, nt, neighbors, nn, nullptr, target_desc.dtype, ws, nullptr, host, nullptr, stream));
  WM_BK(bk->stream_sync(stream));
  const int new_count = host[1];
  void* out = output_alloc(p_env_fns, output_unique_node_memory_context, static_cast<int64_t>(nt) + new_count, target_desc.dtype);
  if (out == nullptr) return WHOLEMEMORY_OUT_OF_MEMORY;
  WM_BK(bk->append_unique_phase2(targets, nt, nn, nn, target_desc.dtype, ws, out, mapping, nullptr, nullptr, nullptr, stream));
  if (!async_completion_enabled() || debug_sync_enabled()) WM_BK(bk->stream_sync(stream));  // (reference append_unique_func.cuh:351)
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

namespace {
// offsets[0 .. n] of a hop: one launch (counts inside the scan, kernels/graph.hip: chain_scan_kernel) where the backend has
// it and takes the size, else count kernel + scan.
int hop_offsets(const wm_device_backend* bk, const wm_sample_args& a, const int* n_dev, int* counts, int* offsets, void* scan_ws,
                size_t scan_ws_bytes, void* stream, int ws_is_ones = 0)
{
  if (bk->sample_offsets != nullptr) {
    const int rc = bk->sample_offsets(&a.row_gref, a.row_storage_offset, a.centers, a.center_dtype, a.n_center, n_dev,
                                      a.max_sample_count, offsets, scan_ws, scan_ws_bytes, ws_is_ones, stream);
    if (rc != -3) return rc;
  }
  const int rc = sample_counts(bk, a, n_dev, counts, stream);
  if (rc != 0) return rc;
  return bk->exclusive_scan_i32(counts, offsets, static_cast<int64_t>(a.n_center) + 1, scan_ws, scan_ws_bytes, stream);
}

// the weight tensor of a weighted fused hop / chain: one float or double per edge, mapped into this rank, or the op declines
wholememory_error_code_t declined_weights(checked_graph& g)
{
  WHOLEMEMORY_RETURN_ON_FAIL(g.weight_array());
  WHOLEMEMORY_RETURN_ON_FAIL(g.placement(csr_tensors::weights, nullptr));
  WHOLEMEMORY_RETURN_ON_FAIL(g.weight_dtype());
  return g.one_weight_per_edge();
}

// an edge attribute the chain fetches on the device (kernels/graph.hip: edge_attr_gather_kernel): 1-D, 4- or 8-byte elements,
// one per edge, mapped into this rank. SUCCESS fills *out (when given); NOT_SUPPORTED = the caller gathers it itself
struct edge_attr {
  wholememory_gref_t gref;
  int64_t storage_offset;
  int elt_bytes;
};
wholememory_error_code_t ext_edge_attr(wholememory_tensor_t t, int64_t n_edges, edge_attr* out)
{
  if (t == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  auto td = *wholememory_tensor_get_tensor_description(t);
  wholememory_array_description_t desc;
  if (td.dim != 1 || !wholememory_convert_tensor_desc_to_array(&desc, &td)) return WHOLEMEMORY_NOT_SUPPORTED;
  const size_t elt = wholememory_dtype_get_element_size(desc.dtype);
  if (placement_of({t}) != csr_placement::mapped || (elt != 4 && elt != 8) || desc.size != n_edges) return WHOLEMEMORY_NOT_SUPPORTED;
  if (out != nullptr) {
    WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(t, &out->gref));
    out->storage_offset = desc.storage_offset;
    out->elt_bytes      = static_cast<int>(elt);
  }
  return WHOLEMEMORY_SUCCESS;
}
std::atomic<int64_t> g_edge_chain_calls{0};   // successful non-query wholememory_ext_multilayer_sample_edges calls
}  // namespace

// One hop of multi-layer sampling as ONE call (extension; the reference runs the sampler and append_unique as two ops with a
// host round trip each to size their outputs — wholegraph_ops/unweighted_sample_without_replacement + graph_ops/append_unique,
// driven by python/.../torch/graph_structure.py:140-196). Here the sampled ids go to scratch sized for the upper bound
// n_center * max_sample_count, append_unique reads the number in use on the device, and the host learns both counts —
// samples and new unique ids — with a single synchronise. Outputs are bit-identical to the two-op sequence:
//   output_sample_offset_tensor  int32 [n_center + 1]   (caller-allocated, as in the sampler)
//   unique                       frontier ++ new neighbour ids in first-occurrence order   (append_unique's output)
//   neighbor_pos                 int32 [n_samples]: position of every sampled neighbour in `unique`
//   center_lid                   int32 [n_samples]: position of its centre in the frontier
// Mapped CSR (CONTINUOUS / CHUNKED / plain) with column ids of the frontier's dtype only; anything else answers
// WHOLEMEMORY_NOT_SUPPORTED before touching the stream and the caller takes the two-op route.
// (weighted: the same hop with the weighted sampler, wholememory_ext_weighted_sample_append_unique; it also declines a weight
// tensor that is not mapped, not float / double or not one entry per edge, and a fan-out above 8192)
// (edge ids: with output_edge_gid_memory_context the sampler also writes the graph edge id of every sample — position in
// csr_col_ptr — to scratch of the same upper bound, copied to an exactly sized int64 [n_samples] output once the count is
// known; wholememory_ext_sample_append_unique_edges. Nothing else about the hop changes.)
static wholememory_error_code_t sample_append_unique_body(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, bool weighted, wholememory_tensor_t center_nodes_tensor, int max_sample_count,
  unsigned long long random_seed, wholememory_tensor_t output_sample_offset_tensor, void* output_unique_memory_context,
  void* output_neighbor_pos_memory_context, void* output_center_localid_memory_context, wholememory_env_func_t* p_env_fns,
  void* stream, void* output_edge_gid_memory_context = nullptr)
{
  const auto* bk = graph_backend();
  if (bk == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (p_env_fns == nullptr || output_unique_memory_context == nullptr || output_neighbor_pos_memory_context == nullptr ||
      output_center_localid_memory_context == nullptr)
    return WHOLEMEMORY_INVALID_INPUT;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  checked_graph g{wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, true};
  wholememory_array_description_t center_desc, offset_desc;
  WHOLEMEMORY_RETURN_ON_FAIL(g.arrays());
  if (!array_of(center_nodes_tensor, "center_nodes_tensor", &center_desc, &err)) return err;
  if (!array_of(output_sample_offset_tensor, "output_sample_offset_tensor", &offset_desc, &err)) return err;
  if (weighted && wm_csr_weight_ptr_tensor == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  WHOLEMEMORY_RETURN_ON_FAIL(g.placement(csr_tensors::row_col, nullptr));
  WHOLEMEMORY_RETURN_ON_FAIL(g.row_dtype());
  const int64_t n = center_desc.size;
  const int64_t room = n * static_cast<int64_t>(std::max(max_sample_count, 0));
  if (max_sample_count <= 0 || offset_desc.dtype != WHOLEMEMORY_DT_INT || !is_index_dtype(center_desc.dtype) ||
      g.col_desc.dtype != center_desc.dtype || offset_desc.size < n + 1 || n == 0 || n + room >= (INT64_C(1) << 31) - 1)
    return WHOLEMEMORY_NOT_SUPPORTED;
  if (weighted) {
    WHOLEMEMORY_RETURN_ON_FAIL(declined_weights(g));
    if (max_sample_count > kMaxWeightedFanout) return WHOLEMEMORY_NOT_SUPPORTED;
  }
  wm_sample_args a{};
  WHOLEMEMORY_RETURN_ON_FAIL(g.fill(&a));
  a.centers            = wholememory_tensor_get_data_pointer(center_nodes_tensor);
  a.center_dtype       = center_desc.dtype;
  a.n_center           = static_cast<int>(n);
  a.max_sample_count   = max_sample_count;
  a.random_seed        = random_seed;
  int* offsets         = static_cast<int*>(wholememory_tensor_get_data_pointer(output_sample_offset_tensor));
  a.sample_offsets     = offsets;

  const int nt = static_cast<int>(n), nn_room = static_cast<int>(room);
  temp_mem counts_mem(p_env_fns), scan_mem(p_env_fns), ids_mem(p_env_fns), lid_mem(p_env_fns), ws_mem(p_env_fns),
    host_mem(p_env_fns), egid_mem(p_env_fns);
  int* counts          = static_cast<int*>(counts_mem.device(n + 1, WHOLEMEMORY_DT_INT));
  const size_t scan_ws = bk->scan_i32_workspace_bytes(n + 1);
  void* scan_ws_ptr    = scan_mem.device(static_cast<int64_t>(scan_ws), WHOLEMEMORY_DT_INT8);
  void* ids            = ids_mem.device(room, a.col_dtype);
  int* lid             = static_cast<int*>(lid_mem.device(room, WHOLEMEMORY_DT_INT));
  int64_t* egid        = nullptr;
  if (output_edge_gid_memory_context != nullptr) egid = static_cast<int64_t*>(egid_mem.device(room, WHOLEMEMORY_DT_INT64));
  // the edge ids of the hop at their exact size, once the host knows it
  auto emit_edge_ids = [&](int total) -> wholememory_error_code_t {
    if (egid == nullptr) return WHOLEMEMORY_SUCCESS;
    void* out = output_alloc(p_env_fns, output_edge_gid_memory_context, total, WHOLEMEMORY_DT_INT64);
    if (total > 0 && out == nullptr) return WHOLEMEMORY_OUT_OF_MEMORY;
    if (total > 0) WM_BK(bk->memcpy_async(out, egid, static_cast<size_t>(total) * sizeof(int64_t), stream));
    return WHOLEMEMORY_SUCCESS;
  };
  void* ws = ws_mem.device(static_cast<int64_t>(bk->append_unique_workspace_bytes(nt, nn_room, center_desc.dtype)), WHOLEMEMORY_DT_INT8);
  // {samples, new unique ids}: left in pinned memory by the last kernel before the host looks (no copy commands)
  int* host = static_cast<int*>(host_mem.pinned(2, WHOLEMEMORY_DT_INT));

  WM_BK(hop_offsets(bk, a, nullptr, counts, offsets, scan_ws_ptr, scan_ws, stream));
  a.out_ids        = ids;
  a.out_center_lid = lid;
  a.out_edge_gid   = egid;
  WM_BK(weighted ? bk->sample_weighted(&a, stream) : bk->sample_unweighted(&a, stream));   // writes exactly offsets[n] entries of the scratch arrays
  int rc = bk->append_unique_phase1(a.centers, nt, ids, nn_room, offsets + n, center_desc.dtype, ws, nullptr, host, nullptr, stream);
  int total = 0, n_new = 0;
  if (rc == -3) {
    // a frontier too big for the route that works from a device-side count: learn the sample count first
    WM_BK(bk->memcpy_async(host, offsets + n, sizeof(int), stream));
    WM_BK(bk->stream_sync(stream));
    total = host[0];
    temp_mem ws2_mem(p_env_fns);
    void* ws2 = ws2_mem.device(static_cast<int64_t>(bk->append_unique_workspace_bytes(nt, total, center_desc.dtype)), WHOLEMEMORY_DT_INT8);
    WM_BK(bk->append_unique_phase1(a.centers, nt, ids, total, nullptr, center_desc.dtype, ws2, nullptr, host, nullptr, stream));
    WM_BK(bk->stream_sync(stream));
    n_new = host[1];
    void* uniq = output_alloc(p_env_fns, output_unique_memory_context, static_cast<int64_t>(nt) + n_new, center_desc.dtype);
    int* pos   = static_cast<int*>(output_alloc(p_env_fns, output_neighbor_pos_memory_context, total, WHOLEMEMORY_DT_INT));
    int* olid  = static_cast<int*>(output_alloc(p_env_fns, output_center_localid_memory_context, total, WHOLEMEMORY_DT_INT));
    if (uniq == nullptr || (total > 0 && (pos == nullptr || olid == nullptr))) return WHOLEMEMORY_OUT_OF_MEMORY;
    WM_BK(bk->append_unique_phase2(a.centers, nt, total, total, center_desc.dtype, ws2, uniq, pos, lid, olid, nullptr, stream));
    WHOLEMEMORY_RETURN_ON_FAIL(emit_edge_ids(total));
    WM_BK(bk->stream_sync(stream));   // ws2 goes out of scope here
    return WHOLEMEMORY_SUCCESS;
  }
  if (rc != 0) return rc == -1 ? WHOLEMEMORY_LOGIC_ERROR : WHOLEMEMORY_CUDA_ERROR;
  WM_BK(bk->stream_sync(stream));             // the only host round trip of the hop
  total = host[0], n_new = host[1];
  void* uniq = output_alloc(p_env_fns, output_unique_memory_context, static_cast<int64_t>(nt) + n_new, center_desc.dtype);
  int* pos   = static_cast<int*>(output_alloc(p_env_fns, output_neighbor_pos_memory_context, total, WHOLEMEMORY_DT_INT));
  int* olid  = static_cast<int*>(output_alloc(p_env_fns, output_center_localid_memory_context, total, WHOLEMEMORY_DT_INT));
  if (uniq == nullptr || (total > 0 && (pos == nullptr || olid == nullptr))) return WHOLEMEMORY_OUT_OF_MEMORY;
  WM_BK(bk->append_unique_phase2(a.centers, nt, nn_room, total, center_desc.dtype, ws, uniq, pos, lid, olid, nullptr, stream));
  WHOLEMEMORY_RETURN_ON_FAIL(emit_edge_ids(total));
  if (!async_completion_enabled() || debug_sync_enabled()) WM_BK(bk->stream_sync(stream));   // else: outputs and scratch are ordered on `stream`
  return WHOLEMEMORY_SUCCESS;
}

wholememory_error_code_t wholememory_ext_sample_append_unique(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t center_nodes_tensor, int max_sample_count, unsigned long long random_seed,
  wholememory_tensor_t output_sample_offset_tensor, void* output_unique_memory_context,
  void* output_neighbor_pos_memory_context, void* output_center_localid_memory_context, wholememory_env_func_t* p_env_fns,
  void* stream)
{
  WM_API_BEGIN
  return sample_append_unique_body(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, nullptr, false, center_nodes_tensor,
                                   max_sample_count, random_seed, output_sample_offset_tensor, output_unique_memory_context,
                                   output_neighbor_pos_memory_context, output_center_localid_memory_context, p_env_fns, stream);
  WM_API_END
}

wholememory_error_code_t wholememory_ext_weighted_sample_append_unique(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t center_nodes_tensor, int max_sample_count,
  unsigned long long random_seed, wholememory_tensor_t output_sample_offset_tensor, void* output_unique_memory_context,
  void* output_neighbor_pos_memory_context, void* output_center_localid_memory_context, wholememory_env_func_t* p_env_fns,
  void* stream)
{
  WM_API_BEGIN
  return sample_append_unique_body(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, true,
                                   center_nodes_tensor, max_sample_count, random_seed, output_sample_offset_tensor,
                                   output_unique_memory_context, output_neighbor_pos_memory_context,
                                   output_center_localid_memory_context, p_env_fns, stream);
  WM_API_END
}

wholememory_error_code_t wholememory_ext_sample_append_unique_edges(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t center_nodes_tensor, int max_sample_count,
  unsigned long long random_seed, wholememory_tensor_t output_sample_offset_tensor, void* output_unique_memory_context,
  void* output_neighbor_pos_memory_context, void* output_center_localid_memory_context, void* output_edge_gid_memory_context,
  wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  if (output_edge_gid_memory_context == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  return sample_append_unique_body(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor,
                                   wm_csr_weight_ptr_tensor != nullptr, center_nodes_tensor, max_sample_count, random_seed,
                                   output_sample_offset_tensor, output_unique_memory_context, output_neighbor_pos_memory_context,
                                   output_center_localid_memory_context, p_env_fns, stream, output_edge_gid_memory_context);
  WM_API_END
}

// The whole chain of hops of GraphStructure.multilayer_sample_without_replacement as ONE call with NO host round trip inside
// (extension; the reference pays two per hop, the fused hop above one): every array is sized by the CALLER for its upper
// bound — hop h has at most cap_c[h] centres (cap_c[0] = seeds, cap_c[h + 1] = cap_c[h] + cap_s[h]) and cap_s[h] = cap_c[h] x
// fan-out samples — the counts stay on the device from hop to hop (wm_sample_args::n_center_dev, wm_au_bounds), and the last
// kernel of every hop leaves {samples, new unique ids} in counts_host[2h], counts_host[2h + 1] (pinned memory). The caller
// synchronises the stream ONCE, reads the counts and trims:
//   sample_offsets[h]  int32 [cap_c[h] + 1]          first n_c[h] + 1 entries are the hop's csr_row_ptr
//   unique[h]          ids   [cap_c[h] + cap_s[h]]    first n_c[h] + new[h] entries = centres ++ new neighbours = hop h + 1's centres
//                                                      (last hop: the entries behind them are -1 up to the array's room, so the
//                                                      whole array can feed a gather before the host has read the counts)
//   neighbor_pos[h]    int32 [cap_s[h]]               first samples[h] entries
//   center_lid[h]      int32 [cap_s[h]]               first samples[h] entries
// with n_c[0] = seeds, n_c[h + 1] = n_c[h] + new[h]. Outputs equal those of `hops` fused-hop calls bit for bit (same kernels,
// same per-hop seeds). WHOLEMEMORY_NOT_SUPPORTED (nothing queued): CSR not mapped into this rank, dtypes differ, an empty seed
// array, a fan-out <= 0, or a hop whose upper bounds are too big for the hash-table route of append_unique.
// (weighted: every hop samples with the weighted sampler on the same weight tensor, wholememory_ext_multilayer_sample_weighted;
// declined as well for a weight tensor the fused hop declines and for a fan-out above 8192)
// (edge ids, wholememory_ext_multilayer_sample_edges: with `edges` the sampler of hop h also writes the graph edge id of every
// sample to edge_gid[h], int64 [cap_s[h]], first samples[h] entries defined; with n_attrs > 0 one more kernel behind hop h
// (edge_attr_gather_kernel) fills attr_out[h * n_attrs + k] = attr_tensors[k][edge_gid[h]] for those entries. It reads the
// hop's sample count on the device from sample_offsets[h][cap_c[h]], the word append_unique takes its neighbour count from.
// Kernels, their order, the counts and every other output are those of the chain without edge ids.)
static wholememory_error_code_t multilayer_sample_body(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, bool weighted, wholememory_tensor_t seed_nodes_tensor, int hops,
  const int* max_sample_counts, const unsigned long long* random_seeds, void* const* sample_offsets, void* const* unique,
  int* const* neighbor_pos, int* const* center_lid, int* counts_host, wholememory_env_func_t* p_env_fns, void* stream,
  bool edges = false, int64_t* const* edge_gid = nullptr, int n_attrs = 0, const wholememory_tensor_t* attr_tensors = nullptr,
  void* const* attr_out = nullptr)
{
  const auto* bk = graph_backend();
  if (bk == nullptr || bk->append_unique_takes_bounds == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (n_attrs > 0 && bk->edge_attr_gather == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  // sample_offsets == nullptr: a QUERY — would this chain be taken? (SUCCESS / NOT_SUPPORTED, nothing queued, no buffer needed:
  // the caller asks before it allocates the upper-bound buffers)
  const bool query = sample_offsets == nullptr;
  if (hops <= 0 || hops > 16 || max_sample_counts == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  if (!query && (p_env_fns == nullptr || random_seeds == nullptr || unique == nullptr || neighbor_pos == nullptr ||
                 center_lid == nullptr || counts_host == nullptr))
    return WHOLEMEMORY_INVALID_INPUT;
  if (!query && edges && (edge_gid == nullptr || (n_attrs > 0 && attr_out == nullptr))) return WHOLEMEMORY_INVALID_INPUT;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  checked_graph g{wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, true};
  wholememory_array_description_t seed_desc;
  WHOLEMEMORY_RETURN_ON_FAIL(g.arrays());
  if (!array_of(seed_nodes_tensor, "seed_nodes_tensor", &seed_desc, &err)) return err;
  if (weighted && wm_csr_weight_ptr_tensor == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  WHOLEMEMORY_RETURN_ON_FAIL(g.placement(csr_tensors::row_col, nullptr));
  WHOLEMEMORY_RETURN_ON_FAIL(g.row_dtype());
  if (!is_index_dtype(seed_desc.dtype) || g.col_desc.dtype != seed_desc.dtype || seed_desc.size == 0) return WHOLEMEMORY_NOT_SUPPORTED;
  if (weighted) WHOLEMEMORY_RETURN_ON_FAIL(declined_weights(g));
  std::vector<edge_attr> attrs(n_attrs);
  for (int k = 0; k < n_attrs; k++)
    WHOLEMEMORY_RETURN_ON_FAIL(ext_edge_attr(attr_tensors[k], g.col_desc.size, query ? nullptr : &attrs[k]));
  std::vector<int64_t> cap_c(hops + 1), cap_s(hops);
  cap_c[0] = seed_desc.size;
  for (int h = 0; h < hops; h++) {
    if (max_sample_counts[h] <= 0 || (weighted && max_sample_counts[h] > kMaxWeightedFanout)) return WHOLEMEMORY_NOT_SUPPORTED;
    cap_s[h]     = cap_c[h] * max_sample_counts[h];
    cap_c[h + 1] = cap_c[h] + cap_s[h];
    if (cap_c[h + 1] >= (INT64_C(1) << 31) - 1 ||
        !bk->append_unique_takes_bounds(static_cast<int>(cap_c[h]), static_cast<int>(cap_s[h]), seed_desc.dtype))
      return WHOLEMEMORY_NOT_SUPPORTED;
  }
  if (query) return WHOLEMEMORY_SUCCESS;
  wm_sample_args a{};
  WHOLEMEMORY_RETURN_ON_FAIL(g.fill(&a));
  a.center_dtype = seed_desc.dtype;

  // scratch of all hops at once (the kernels are queued back to back; nothing may be reused before the last one has run)
  temp_mem n_dev_mem(p_env_fns);
  int* n_dev = static_cast<int*>(n_dev_mem.device(hops, WHOLEMEMORY_DT_INT));   // centres of hop h + 1 = unique ids after hop h
  std::vector<std::unique_ptr<temp_mem>> keep;
  auto scratch = [&](int64_t count, wholememory_dtype_t dt) {
    keep.emplace_back(new temp_mem(p_env_fns));
    return keep.back()->device(count, dt);
  };
  // the offsets scans' workspaces of all hops in one block, initialised (0xFF: the scans' state) by ONE fill command
  std::vector<size_t> scan_bytes(hops), scan_at(hops);
  size_t scan_total = 0;
  for (int h = 0; h < hops; h++) {
    scan_bytes[h] = bk->scan_i32_workspace_bytes(cap_c[h] + 1);
    scan_at[h]    = scan_total;
    scan_total += scan_bytes[h];
  }
  char* scan_block = static_cast<char*>(scratch(static_cast<int64_t>(scan_total), WHOLEMEMORY_DT_INT8));
  if (bk->fill_ff_async != nullptr)
    WM_BK(bk->fill_ff_async(scan_block, scan_total, stream));
  else
    WM_BK(bk->memset_async(scan_block, 0xFF, scan_total, stream));
  for (int h = 0; h < hops; h++) {
    const int nc = static_cast<int>(cap_c[h]), ns = static_cast<int>(cap_s[h]);
    const int* centres_in_use = h == 0 ? nullptr : n_dev + (h - 1);
    a.centers          = h == 0 ? wholememory_tensor_get_data_pointer(seed_nodes_tensor) : unique[h - 1];
    a.n_center         = nc;
    a.n_center_dev     = centres_in_use;
    a.max_sample_count = max_sample_counts[h];
    a.random_seed      = random_seeds[h];
    int* offsets       = static_cast<int*>(sample_offsets[h]);
    a.sample_offsets   = offsets;
    int* counts        = static_cast<int*>(scratch(nc + 1, WHOLEMEMORY_DT_INT));
    const size_t scan_ws = scan_bytes[h];
    void* scan_ws_ptr  = scan_block + scan_at[h];
    void* ids          = scratch(ns, a.col_dtype);
    void* ws = scratch(static_cast<int64_t>(bk->append_unique_workspace_bytes(nc, ns, seed_desc.dtype)), WHOLEMEMORY_DT_INT8);
    WM_BK(hop_offsets(bk, a, centres_in_use, counts, offsets, scan_ws_ptr, scan_ws, stream, 1));   // offsets[nc] = samples of the hop
    a.out_ids        = ids;
    a.out_center_lid = center_lid[h];
    a.out_edge_gid   = edges ? edge_gid[h] : nullptr;
    // the sampling kernel empties the hop's hash table on the side (one fill command fewer per hop)
    a.fill_ff_ptr = nullptr, a.fill_ff_bytes = 0;
    const bool side_fill = bk->append_unique_table_region != nullptr &&
                           bk->append_unique_table_region(nc, ns, seed_desc.dtype, ws, &a.fill_ff_ptr, &a.fill_ff_bytes) == 0;
    if (!side_fill) a.fill_ff_ptr = nullptr, a.fill_ff_bytes = 0;
    WM_BK(weighted ? bk->sample_weighted(&a, stream) : bk->sample_unweighted(&a, stream));
    // (the hop's counts are published by phase 2's emitting kernel: one tiny launch fewer per hop)
    // (the outermost frontier is padded with -1 up to its room: a gather can be queued on the whole array before the host
    // has read the counts — negative ids are skipped, gather_scatter_func.cuh:296)
    wm_au_bounds b{centres_in_use, offsets + nc, n_dev + h, counts_host + 2 * h, side_fill ? 1 : 0, h == hops - 1 ? 1 : 0};
    int rc = bk->append_unique_phase1(a.centers, nc, ids, ns, offsets + nc, seed_desc.dtype, ws, nullptr, nullptr, &b, stream);
    if (rc != 0) return rc == -1 ? WHOLEMEMORY_LOGIC_ERROR : WHOLEMEMORY_CUDA_ERROR;
    WM_BK(bk->append_unique_phase2(a.centers, nc, ns, ns, seed_desc.dtype, ws, unique[h], neighbor_pos[h], nullptr, nullptr, &b, stream));
    // the attributes of the hop's sampled edges, WM_MAX_EDGE_ATTRS per launch, sized on the device by offsets[nc]
    for (int k0 = 0; k0 < n_attrs; k0 += WM_MAX_EDGE_ATTRS) {
      wm_edge_attr_args g{};
      g.edge_gid = edge_gid[h], g.n_dev = offsets + nc, g.n = ns;
      g.n_attrs  = std::min(n_attrs - k0, WM_MAX_EDGE_ATTRS);
      for (int k = 0; k < g.n_attrs; k++) {
        g.attr[k].gref = attrs[k0 + k].gref, g.attr[k].storage_offset = attrs[k0 + k].storage_offset;
        g.attr[k].elt_bytes = attrs[k0 + k].elt_bytes, g.attr[k].out = attr_out[static_cast<size_t>(h) * n_attrs + k0 + k];
      }
      rc = bk->edge_attr_gather(&g, stream);
      if (rc != 0) return rc == -1 ? WHOLEMEMORY_INVALID_INPUT : WHOLEMEMORY_CUDA_ERROR;
    }
  }
  // by default the call returns complete, like every op of the reference; a host framework that declared stream-ordered
  // allocators (wholememory_ext_set_async_completion) gets it back with everything queued and synchronises when it reads
  // counts_host
  if (!async_completion_enabled() || debug_sync_enabled()) WM_BK(bk->stream_sync(stream));
  if (edges) g_edge_chain_calls.fetch_add(1, std::memory_order_relaxed);
  return WHOLEMEMORY_SUCCESS;
}

wholememory_error_code_t wholememory_ext_multilayer_sample(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor, wholememory_tensor_t seed_nodes_tensor,
  int hops, const int* max_sample_counts, const unsigned long long* random_seeds, void* const* sample_offsets, void* const* unique,
  int* const* neighbor_pos, int* const* center_lid, int* counts_host, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  return multilayer_sample_body(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, nullptr, false, seed_nodes_tensor, hops,
                                max_sample_counts, random_seeds, sample_offsets, unique, neighbor_pos, center_lid, counts_host,
                                p_env_fns, stream);
  WM_API_END
}

wholememory_error_code_t wholememory_ext_multilayer_sample_weighted(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t seed_nodes_tensor, int hops, const int* max_sample_counts,
  const unsigned long long* random_seeds, void* const* sample_offsets, void* const* unique, int* const* neighbor_pos,
  int* const* center_lid, int* counts_host, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  return multilayer_sample_body(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, true, seed_nodes_tensor,
                                hops, max_sample_counts, random_seeds, sample_offsets, unique, neighbor_pos, center_lid,
                                counts_host, p_env_fns, stream);
  WM_API_END
}

wholememory_error_code_t wholememory_ext_multilayer_sample_edges(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t seed_nodes_tensor, int hops, const int* max_sample_counts,
  const unsigned long long* random_seeds, void* const* sample_offsets, void* const* unique, int* const* neighbor_pos,
  int* const* center_lid, int64_t* const* edge_gid, int n_attrs, const wholememory_tensor_t* attr_tensors, void* const* attr_out,
  int* counts_host, wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  // (before anything looks at the device or the backend)
  if (n_attrs < 0 || (n_attrs > 0 && attr_tensors == nullptr)) return WHOLEMEMORY_INVALID_INPUT;
  if (sample_offsets != nullptr && (edge_gid == nullptr || (n_attrs > 0 && attr_out == nullptr))) return WHOLEMEMORY_INVALID_INPUT;
  for (int k = 0; k < n_attrs; k++)
    if (attr_tensors[k] == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  return multilayer_sample_body(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor,
                                wm_csr_weight_ptr_tensor != nullptr, seed_nodes_tensor, hops, max_sample_counts, random_seeds,
                                sample_offsets, unique, neighbor_pos, center_lid, counts_host, p_env_fns, stream, true, edge_gid,
                                n_attrs, attr_tensors, attr_out);
  WM_API_END
}

int64_t wholememory_ext_edge_chain_calls(void) { return g_edge_chain_calls.load(std::memory_order_relaxed); }

wholememory_error_code_t csr_add_self_loop(wholememory_tensor_t csr_row_ptr_tensor, wholememory_tensor_t csr_col_ptr_tensor,
                                           wholememory_tensor_t output_csr_row_ptr_tensor,
                                           wholememory_tensor_t output_csr_col_ptr_tensor, void* stream)
{
  WM_API_BEGIN
  const auto* bk = graph_backend();
  if (bk == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  wholememory_error_code_t err = WHOLEMEMORY_SUCCESS;
  wholememory_array_description_t row_desc, col_desc, out_row_desc, out_col_desc;
  if (!array_of(csr_row_ptr_tensor, "csr_row_ptr_tensor", &row_desc, &err)) return err;
  if (!array_of(csr_col_ptr_tensor, "csr_col_ptr_tensor", &col_desc, &err)) return err;
  if (!array_of(output_csr_row_ptr_tensor, "output_csr_row_ptr_tensor", &out_row_desc, &err)) return err;
  if (!array_of(output_csr_col_ptr_tensor, "output_csr_col_ptr_tensor", &out_col_desc, &err)) return err;
  // int32 only: csr_add_self_loop.cpp:32-63
  if (row_desc.dtype != WHOLEMEMORY_DT_INT || col_desc.dtype != WHOLEMEMORY_DT_INT || out_row_desc.dtype != WHOLEMEMORY_DT_INT ||
      out_col_desc.dtype != WHOLEMEMORY_DT_INT) {
    WM_ERROR("csr_add_self_loop works on int32 CSR arrays");
    return WHOLEMEMORY_INVALID_INPUT;
  }
  // the reference launches without looking at the output sizes; writing past a short output is refused here
  if (row_desc.size < 1 || out_row_desc.size < row_desc.size || out_col_desc.size < col_desc.size + row_desc.size - 1) {
    WM_ERROR("csr_add_self_loop outputs need %ld row and %ld col entries", static_cast<long>(row_desc.size),
             static_cast<long>(col_desc.size + row_desc.size - 1));
    return WHOLEMEMORY_INVALID_INPUT;
  }
  WM_BK(bk->csr_add_self_loop(static_cast<const int*>(wholememory_tensor_get_data_pointer(csr_row_ptr_tensor)),
                              static_cast<const int*>(wholememory_tensor_get_data_pointer(csr_col_ptr_tensor)),
                              static_cast<int*>(wholememory_tensor_get_data_pointer(output_csr_row_ptr_tensor)),
                              static_cast<int*>(wholememory_tensor_get_data_pointer(output_csr_col_ptr_tensor)),
                              static_cast<int>(row_desc.size - 1), stream));
  WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

// Self-test of the env functions (reference wholememory_op.h:58-79, wholememory_test_op.cu:60-160): computes
// out[i, :] = T(float(i)) + input[:] into a scratch buffer obtained through p_env_fns->temporary_fns, then copies it to
// the fixed output tensor and to device / pinned / host outputs allocated through p_env_fns->output_fns for every
// non-null memory context.
wholememory_error_code_t wholememory_env_test_op(wholememory_tensor_t input_tensor, wholememory_tensor_t output_fixed_tensor,
                                                 void* output_variable_device_tensor_handle,
                                                 void* output_variable_pinned_tensor_handle,
                                                 void* output_variable_host_tensor_handle, int64_t output_variable_entry_count,
                                                 wholememory_env_func_t* p_env_fns, void* stream)
{
  WM_API_BEGIN
  const auto* bk = backend();
  if (bk->env_test_fill == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (input_tensor == nullptr || output_fixed_tensor == nullptr || p_env_fns == nullptr) return WHOLEMEMORY_INVALID_INPUT;
  auto in_desc  = *wholememory_tensor_get_tensor_description(input_tensor);
  auto out_desc = *wholememory_tensor_get_tensor_description(output_fixed_tensor);
  if (in_desc.dim != 1 || out_desc.dim != 2 || out_desc.sizes[0] != output_variable_entry_count ||
      out_desc.sizes[1] != in_desc.sizes[0] || in_desc.dtype != out_desc.dtype)
    return WHOLEMEMORY_INVALID_INPUT;  // the reference aborts on these (WHOLEMEMORY_CHECK_NOTHROW)
  const int64_t dim = in_desc.sizes[0], n = output_variable_entry_count;
  temp_mem scratch(p_env_fns);
  void* tmp = scratch.device(n * dim, in_desc.dtype);
  int rc    = bk->env_test_fill(wholememory_tensor_get_data_pointer(input_tensor), tmp, in_desc.dtype, dim, n, dim, stream);
  if (rc == -1) return WHOLEMEMORY_INVALID_INPUT;
  if (rc != 0) return WHOLEMEMORY_CUDA_ERROR;
  const size_t bytes = static_cast<size_t>(n) * dim * wholememory_dtype_get_element_size(in_desc.dtype);
  auto out_alloc = [&](void* ctx, wholememory_memory_allocation_type_t type) -> void* {
    if (ctx == nullptr) return nullptr;
    auto d = out_desc;
    d.strides[0] = dim, d.strides[1] = 1, d.storage_offset = 0;
    return p_env_fns->output_fns.malloc_fn(&d, type, ctx, p_env_fns->output_fns.global_context);
  };
  void* dsts[4] = {wholememory_tensor_get_data_pointer(output_fixed_tensor),
                   out_alloc(output_variable_device_tensor_handle, WHOLEMEMORY_MA_DEVICE),
                   out_alloc(output_variable_pinned_tensor_handle, WHOLEMEMORY_MA_PINNED),
                   out_alloc(output_variable_host_tensor_handle, WHOLEMEMORY_MA_HOST)};
  for (void* dst : dsts)
    if (dst != nullptr && bytes > 0) WM_BK(bk->memcpy_async(dst, tmp, bytes, stream));
  WM_BK(bk->stream_sync(stream));  // the scratch buffer returns to the caller's allocator
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

}  // extern "C"
