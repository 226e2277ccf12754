// wholegraph_amd — neighbour aggregation of a sampled CSC block (the GraphSAGE `agg_concat` op) on gfx950.
//
// Forward (one group of LANES lanes per target row d, LANES = 16 / 32 / 64 from the row width):
//   out[d, 0:F]  = A(d): the fp32 sum of x[col_ind[e]] over e in [row_ptr[d], row_ptr[d+1]), left to right from the first
//                  term, times r(d) = fl(1 / deg(d)) for "mean"; +0.0 for a target without neighbours
//   out[d, F:2F] = x[d]
// The group loads the column ids of up to LANES edges with one coalesced load and hands them out with shuffles; the
// neighbour rows of a batch of kAggBatch edges are then loaded back to back (16-byte pieces when the rows allow it). That
// walk is agg_common.cuh's (for_target_pieces, for_edge_batches), as in every per-target kernel of the block ops; the
// kernel says what a lane fetches, what a slot loads and what it adds.
//
// Backward (grad_x[s] for every source row s; no atomics, one fixed order of every sum):
//   1 the existing id sort (dedup_ids, called by the host) sorts col_ind: runs of equal sources, positions ascending
//   2 agg_bwd_prep_kernel: sorted_dst[j] = target of edge order[j] (a search in row_ptr), run_of[unique[u]] = u
//   3 agg_bwd_chunk_kernel: a run of more than kAggChunkEdges edges is cut into chunks of that many edges from its start;
//     chunk k >= 1 is summed by a group of its own into a partial row. Tile t = [t*C, (t+1)*C) of the sorted positions
//     holds at most one such chunk start (only the run that covers position t*C can have one there), so the chunk's slot
//     is its tile.
//   4 agg_bwd_fold_kernel: one group per source row: chunk 0 of its run, then the partials of chunks 1, 2, ... in chunk
//     order, then the self term G[s, F:2F] for s < n_dst; rows without edges get the self term or +0.0.
// run_of[] is not initialised: a value is used only when 0 <= u < n_unique and unique[u] == s (a sparse-set check).
// Steps 1 and 2 do not depend on the op: agg_bwd_prepare (below) is shared with kernels/agg_half.hip, agg_weighted.hip and
// agg_rel.hip. The walk of steps 3 and 4 (tiles, the run of a source, the partials in chunk order, the self term) is
// agg_common.cuh's, shared with those files and with the attention ops; fold_edges, the per-edge term, is this op's own
// (its loop over the sorted positions is written out: agg_common.cuh's header has the reason).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "agg_common.cuh"

namespace wm {
namespace {

// -0.0 is the identity of IEEE addition: acc = -0.0 followed by acc + t_0 + t_1 + ... is the left-to-right sum that starts
// from the first term (also when that term is -0.0)

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void agg_forward_kernel(wm_agg_args p)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t F = p.dim;
  for_target_pieces<VEC, LANES>(p, F, [&](int64_t d, int64_t e0, int64_t e1, int64_t c, int64_t cl, bool act) {
    const int64_t deg = e1 - e0;
    const float r     = deg > 0 ? 1.0f / static_cast<float>(deg) : 0.0f;
    const float* self = p.in + d * p.in_stride;
    float* orow       = p.out + d * p.out_stride;
    fvec<VEC> acc     = splat<VEC>(-0.0f);
    int my            = 0;
    fvec<VEC> v[kAggBatch];
    for_edge_batches<LANES>(
        e0, e1, gl, [&](int64_t e, bool in) { my = in ? p.col_ind[e] : 0; },
        [&](int k, int from, int64_t) {
          const int src = __shfl(my, from, LANES);
          v[k]          = ldv<VEC>(p.in + static_cast<int64_t>(src) * p.in_stride + cl);
        },
        [&](int k, int64_t) { add_to(acc, v[k]); });
    if (act) {
      const fvec<VEC> a = deg == 0 ? splat<VEC>(0.0f) : (p.mean ? scaled(acc, r) : acc);
      stv(orow + c, a);
      stv(orow + F + c, ldv<VEC>(self + c));
    }
  });
}

// acc += t(e) for the edges at sorted positions [eb0, ee), in that order (LANES lanes, this lane's columns at cl)
template <int VEC, int LANES>
__device__ __forceinline__ void fold_edges(fvec<VEC>& acc, const wm_agg_args& p, const int32_t* sorted_dst, int64_t eb0,
                                           int64_t ee, int64_t cl, int gl)
{
  for (int64_t eb = eb0; eb < ee; eb += LANES) {   // (written out: on for_edge_batches agg_bwd_fold_kernel measured slower)
    const int nb = static_cast<int>(ee - eb < LANES ? ee - eb : LANES);
    int my_d     = 0;
    float my_r   = 1.0f;
    if (gl < nb) {
      my_d = sorted_dst[eb + gl];
      if (p.mean) my_r = 1.0f / static_cast<float>(p.row_ptr[my_d + 1] - p.row_ptr[my_d]);
    }
    for (int j = 0; j < nb; j += kAggBatch) {
      fvec<VEC> v[kAggBatch];
      float rs[kAggBatch];
#pragma unroll
      for (int k = 0; k < kAggBatch; ++k) {
        const int from = j + k < nb ? j + k : nb - 1;
        const int d    = __shfl(my_d, from, LANES);
        rs[k]          = __shfl(my_r, from, LANES);
        v[k]           = ldv<VEC>(p.grad + static_cast<int64_t>(d) * p.grad_stride + cl);
      }
#pragma unroll
      for (int k = 0; k < kAggBatch; ++k)
        if (j + k < nb) add_to(acc, p.mean ? scaled(v[k], rs[k]) : v[k]);
    }
  }
}

// sorted_dst[j] = the target whose edge range holds position order[j]; run_of[unique[u]] = u
__global__ __launch_bounds__(kAggBlock) void agg_bwd_prep_kernel(const int32_t* row_ptr, int64_t n_dst, int64_t n_edges,
                                                                 csc_bwd_index b)
{
  const int64_t nu = *b.n_unique;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_edges;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    bwd_prep_at(i, row_ptr, n_dst, b.order, b.unique_ids, nu, b.sorted_dst, b.run_of);
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void agg_bwd_chunk_kernel(wm_agg_args p, wm_agg_bwd_state b)
{
  const int gl = threadIdx.x % LANES;
  for_chunk_pieces<VEC, LANES>(b, p.dim, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    fvec<VEC> acc = splat<VEC>(-0.0f);
    fold_edges<VEC, LANES>(acc, p, b.sorted_dst, cs, ce, cl, gl);
    if (act) stv(b.partial + t * b.partial_stride + c, acc);
  });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void agg_bwd_fold_kernel(wm_agg_args p, wm_agg_bwd_state b)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t F       = p.dim;
  const int64_t nu      = *b.n_unique;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; s < p.n_src;
       s += static_cast<int64_t>(gridDim.x) * kGroups) {
    const src_run r = run_of_source(b, nu, s);
    const bool self = s < p.n_dst;
    for (int64_t cb = 0; cb < F; cb += LANES * VEC) {
      const int64_t c  = cb + gl * VEC;
      const bool act   = c < F;
      const int64_t cl = act ? c : 0;
      fvec<VEC> acc    = splat<VEC>(-0.0f);
      fold_edges<VEC, LANES>(acc, p, b.sorted_dst, r.s0, r.c0e, cl, gl);
      add_partials(acc, b, r, cl);
      const fvec<VEC> res = with_self_term(acc, r.has, self, p.grad, s * p.grad_stride + F + cl);
      if (act) stv(p.out + s * p.out_stride + c, res);
    }
  }
}

}  // namespace

int hip_agg_forward(const wm_agg_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_dst == 0 || a->dim == 0) return 0;
  const bool v4 = use_vec4(a->dim, a->in, a->in_stride, a->out, a->out_stride);
#define WM_AGG_FWD(V, L)                                                                                                  \
  hipLaunchKernelGGL((agg_forward_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a)
  WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_AGG_FWD);
#undef WM_AGG_FWD
  return rc_last();
}

size_t hip_agg_backward_workspace_bytes(int64_t n_edges, int64_t n_src, int64_t dim)
{
  return agg_bwd_plan(n_edges, n_src, dim, kAggChunkEdges).ws.bytes;
}

int agg_bwd_prepare(const wm_csc_block& blk, int64_t dim, const wm_edge_index& ix, void* workspace, csc_bwd_index* bp,
                    void* stream_v)
{
  hipStream_t stream     = static_cast<hipStream_t>(stream_v);
  const agg_bwd_layout l = agg_bwd_plan(blk.n_edges, blk.n_src, dim, kAggChunkEdges);
  csc_bwd_index& b       = *bp;
  set_sorted(b, ix);
  b.sorted_dst           = ws_at<int32_t>(workspace, l.ws.off[0]);
  b.run_of               = ws_at<int32_t>(workspace, l.ws.off[1]);
  b.partial              = ws_at<float>(workspace, l.ws.off[2]);
  b.n_tiles              = l.n_tiles;
  b.partial_stride       = l.partial_stride;
  if (blk.n_edges > 0) {
    const int blocks = blocks_for(blk.n_edges, kAggBlock);
    hipLaunchKernelGGL(agg_bwd_prep_kernel, dim3(blocks < 8192 ? blocks : 8192), dim3(kAggBlock), 0, stream, blk.row_ptr,
                       blk.n_dst, blk.n_edges, b);
    if (rc_last() != 0) return -2;
  }
  return 0;
}

int hip_agg_backward(const wm_agg_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_src == 0 || a->dim == 0) return 0;
  wm_agg_bwd_state b;
  if (agg_bwd_prepare(*a, a->dim, ix, workspace, &b, stream_v) != 0) return -2;
  const bool v4 = use_vec4(a->dim, a->grad, a->grad_stride, a->out, a->out_stride);
  if (b.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_AGG_CHUNK(V, L)                                                                                                   \
  hipLaunchKernelGGL((agg_bwd_chunk_kernel<V, L>), dim3(blocks_for(b.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
    WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_AGG_CHUNK);
#undef WM_AGG_CHUNK
    if (rc_last() != 0) return -2;
  }
#define WM_AGG_FOLD(V, L)                                                                                                   \
  hipLaunchKernelGGL((agg_bwd_fold_kernel<V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
  WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_AGG_FOLD);
#undef WM_AGG_FOLD
  return rc_last();
}

}  // namespace wm
