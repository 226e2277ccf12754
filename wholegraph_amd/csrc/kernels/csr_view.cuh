// wholegraph_amd — the CSR graph of a wm_csr_graph as the kernels read it, shared by the units that do (graph.hip: the
// samplers; walk.hip, walk_n2v.hip: the walks; neg_sample.hip; isub.hip; tsample.hip): the views of the arrays with their storage offsets, filled in
// one place, and the launchers' dispatch on the dtypes of the node ids and of csr_col_ptr.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "gref_view.cuh"

namespace wm {

struct csr_view {
  gref_view row_ptr, col_ptr;
  int64_t row_off, col_off;  // storage offsets (elements)
  int64_t n_nodes, n_edges;
};

struct csr_weights {
  gref_view weight_ptr;
  int64_t weight_off;  // storage offset (elements)
};

inline csr_view csr_view_of(const wm_csr_graph& g)
{
  return {make_view(g.row_gref), make_view(g.col_gref), g.row_storage_offset, g.col_storage_offset, g.n_nodes, g.n_edges};
}

// (an empty weight_gref gives an empty view: the kernels without weights never read it)
inline csr_weights csr_weights_of(const wm_csr_graph& g) { return {make_view(g.weight_gref), g.weight_storage_offset}; }

// does x occur in col_ind[s, e)? A group of G lanes scans the row together: all lanes of the group call this with the same
// (s, e), each trip a lane loads one of the next G entries and the group passes them round by shuffles, every lane comparing
// against its own x — in x's type (node2vec compares in ColT, the negative sampler an int64 candidate in int64)
template <typename ColT, int G, typename X>
__device__ __forceinline__ bool csr_group_scan(const csr_view& g, int64_t s, int64_t e, X x, int gl)
{
  bool found = false;
  for (int64_t r = s; r < e; r += G) {
    const int64_t pos = r + gl;
    const ColT y      = pos < e ? gref_load<ColT>(g.col_ptr, g.col_off + pos) : ColT(0);
    const int cnt     = e - r < G ? static_cast<int>(e - r) : G;
#pragma unroll
    for (int k = 0; k < G; k++) {
      const ColT yk = __shfl(y, k, G);
      found |= (k < cnt) & (static_cast<X>(yk) == x);
    }
  }
  return found;
}

struct csr_times {
  gref_view time_ptr;
  int64_t time_off;  // storage offset (elements)
};

// (an empty time_gref gives an empty view: only the temporal sampler reads it)
inline csr_times csr_times_of(const wm_csr_graph& g) { return {make_view(g.time_gref), g.time_storage_offset}; }

// f(IdT(), ColT()) with the integer types of the caller's node ids and of csr_col_ptr; -1 (nothing queued) for a dtype that
// is neither int32 nor int64
template <typename F>
int dispatch_id_col(wholememory_dtype_t id_dtype, wholememory_dtype_t col_dtype, F f)
{
  const bool id32 = id_dtype == WHOLEMEMORY_DT_INT, col32 = col_dtype == WHOLEMEMORY_DT_INT;
  if ((!id32 && id_dtype != WHOLEMEMORY_DT_INT64) || (!col32 && col_dtype != WHOLEMEMORY_DT_INT64)) return -1;
  if (id32 && col32) return f(int32_t(), int32_t());
  if (id32) return f(int32_t(), int64_t());
  if (col32) return f(int64_t(), int32_t());
  return f(int64_t(), int64_t());
}

// the weight level on top of it: f(IdT(), ColT(), WT()) with float or double weights, -1 for any other weight dtype
template <typename F>
int dispatch_id_col_weight(wholememory_dtype_t id_dtype, wholememory_dtype_t col_dtype, wholememory_dtype_t weight_dtype, F f)
{
  if (weight_dtype == WHOLEMEMORY_DT_FLOAT) return dispatch_id_col(id_dtype, col_dtype, [&](auto id, auto col) { return f(id, col, float()); });
  if (weight_dtype == WHOLEMEMORY_DT_DOUBLE) return dispatch_id_col(id_dtype, col_dtype, [&](auto id, auto col) { return f(id, col, double()); });
  return -1;
}

}  // namespace wm
