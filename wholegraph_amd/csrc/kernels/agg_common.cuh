// wholegraph_amd — device and launch helpers shared by the aggregation ops of a sampled CSC block (kernels/agg.hip, the
// GraphSAGE `agg_concat` op, and kernels/agg_half.hip, the same op on fp16 / bf16 rows; kernels/gat.hip, the GAT
// `mha_gat_n2n` op): fp32 pieces of a row, the clamped edge range of a
// target, the lookups of the deterministic per-source backward over the id sort, and the launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"

namespace wm {

// scratch of the agg_concat backward: the id sort's outputs and the op's workspace (agg_bwd_prepare carves it)
struct wm_agg_bwd_state {
  const int32_t* order;        // [n_edges] edge positions, sorted by source (stable)
  const int32_t* run_starts;   // [n_unique + 1]
  const int32_t* unique_ids;   // [n_unique] sources with edges, ascending
  const int64_t* n_unique;     // device scalar written by the sort
  int32_t* sorted_dst;         // [n_edges]
  int32_t* run_of;             // [n_src]
  float* partial;              // [n_tiles, partial_stride] fp32, whatever the type of the rows
  int64_t n_tiles, partial_stride;
};

// fills `b` from the id sort's outputs and `workspace` (hip_agg_backward_workspace_bytes) and queues agg_bwd_prep_kernel
// (kernels/agg.hip), which reads only the index part of `a`: row_ptr, n_dst, n_edges, n_src, dim. 0 or -2.
int agg_bwd_prepare(const wm_agg_args* a, const int32_t* order, const int32_t* run_starts, const int32_t* unique_ids,
                    const int64_t* n_unique_dev, void* workspace, wm_agg_bwd_state* b, void* stream);

namespace {

constexpr int kAggBlock = 256;
constexpr int kAggBatch = 8;   // neighbour rows in flight per lane
constexpr int64_t kAggMaxBlocks = 1 << 20;

template <int VEC>
struct fvec {
  float v[VEC];
};

template <int VEC>
__device__ __forceinline__ fvec<VEC> ldv(const float* p)
{
  fvec<VEC> r;
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = p[i];
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ void stv(float* p, const fvec<VEC>& a)
{
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = a.v[i];
  }
}

template <int VEC>
__device__ __forceinline__ fvec<VEC> splat(float s)
{
  fvec<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = s;
  return r;
}

template <int VEC>
__device__ __forceinline__ void add_to(fvec<VEC>& acc, const fvec<VEC>& b)
{
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc.v[i] = acc.v[i] + b.v[i];
}

template <int VEC>
__device__ __forceinline__ fvec<VEC> scaled(const fvec<VEC>& a, float s)
{
  fvec<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = a.v[i] * s;
  return r;
}

// edges of target d, clamped to [0, n_edges) so that an inconsistent row_ptr cannot send a load out of col_ind
__device__ __forceinline__ void edge_range(const int32_t* row_ptr, int64_t d, int64_t n_edges, int64_t& e0, int64_t& e1)
{
  int64_t a = row_ptr[d], b = row_ptr[d + 1];
  a  = a < 0 ? 0 : (a > n_edges ? n_edges : a);
  b  = b < a ? a : (b > n_edges ? n_edges : b);
  e0 = a, e1 = b;
}

// the lookups of the per-source backward (the id sort of col_ind: order, run_starts, unique_ids, n_unique):
// sorted_dst[i] = the target whose edge range holds position order[i]; run_of[unique[i]] = i
__device__ __forceinline__ void bwd_prep_at(int64_t i, const int32_t* row_ptr, int64_t n_dst, const int32_t* order,
                                            const int32_t* unique_ids, int64_t nu, int32_t* sorted_dst, int32_t* run_of)
{
  const int64_t pos = order[i];
  int64_t lo = 0, hi = n_dst;   // the last d in [0, n_dst) with row_ptr[d] <= pos
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (row_ptr[mid] <= pos) lo = mid;
    else hi = mid;
  }
  sorted_dst[i] = static_cast<int32_t>(lo);
  if (i < nu) run_of[unique_ids[i]] = static_cast<int32_t>(i);
}

// the chunk k >= 1 of a run that starts in tile t = [t*C, (t+1)*C) of the sorted positions, if any: [cs, ce)
__device__ __forceinline__ bool chunk_in_tile(int64_t t, const int32_t* run_starts, int64_t nu, int64_t& cs, int64_t& ce)
{
  constexpr int64_t C   = kAggChunkEdges;
  const int64_t covered = run_starts[nu];   // sorted positions that belong to runs (ids out of range sort behind them)
  const int64_t pos0    = t * C;
  if (pos0 >= covered) return false;
  int64_t lo = 0, hi = nu;   // the run that covers pos0: last u with run_starts[u] <= pos0
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (run_starts[mid] <= pos0) lo = mid;
    else hi = mid;
  }
  const int64_t s0 = run_starts[lo], s1 = run_starts[lo + 1];
  const int64_t k  = (pos0 - s0 + C - 1) / C;
  cs               = s0 + k * C;
  if (k < 1 || cs >= s1 || cs >= pos0 + C) return false;   // no chunk k >= 1 starts in this tile
  ce = cs + C < s1 ? cs + C : s1;
  return true;
}

int rc_last() { return hipGetLastError() == hipSuccess ? 0 : -2; }

int blocks_for(int64_t groups, int groups_per_block)
{
  int64_t n = (groups + groups_per_block - 1) / groups_per_block;
  if (n < 1) n = 1;
  return static_cast<int>(n < kAggMaxBlocks ? n : kAggMaxBlocks);
}

// 16-byte pieces when every row start is 16-byte aligned; group width from the number of pieces (or floats) of a row
bool use_vec4(int64_t dim, const void* a, int64_t a_stride, const void* b, int64_t b_stride)
{
  return dim % 4 == 0 && a_stride % 4 == 0 && b_stride % 4 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(b) % 16 == 0;
}
int lanes_for(int64_t pieces) { return pieces <= 16 ? 16 : (pieces <= 32 ? 32 : 64); }

#define WM_AGG_DISPATCH(VEC_, PIECES_, LAUNCH_)                          \
  do {                                                                   \
    const int lanes__ = lanes_for(PIECES_);                              \
    if (VEC_) {                                                          \
      if (lanes__ == 16) LAUNCH_(4, 16);                                 \
      else if (lanes__ == 32) LAUNCH_(4, 32);                            \
      else LAUNCH_(4, 64);                                               \
    } else {                                                             \
      if (lanes__ == 16) LAUNCH_(1, 16);                                 \
      else if (lanes__ == 32) LAUNCH_(1, 32);                            \
      else LAUNCH_(1, 64);                                               \
    }                                                                    \
  } while (0)

}  // namespace
}  // namespace wm
