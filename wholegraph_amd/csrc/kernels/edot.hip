// wholegraph_amd — the dot product of the two endpoint rows of every edge of a sampled CSC block (the `edge_dot_n2n` op: the
// score of skip-gram training over walks and negatives, and the decoder of a link-prediction model) on gfx950. The
// semantics and the one order of every fp32 sum: wholegraph_amd_ext.h, section 2p. score[e] = x_dst[d] . x_src[col[e]] as a
// balanced tree of adjacent pairs over Fp (the smallest power of two >= F, padded with +0.0); no heads, no scale.
//
// Forward, edot_fwd_kernel<VEC, LANES>: one group of LANES lanes per target d. The tree has the two implementations of
// gat_common.cuh that give the same bits:
//   * VEC = 4 (F a power of two in [4, 256], both rows 16-byte aligned): a lane owns 4 adjacent columns, the target's piece
//     of x_dst stays in registers over the edge loop, the source rows are loaded a batch of kAggBatch back to back, the F / 4
//     lanes of the row combine with xor exchanges (head_tree) and the lane at column 0 stores score[e] (for_edge_batches of
//     agg_common.cuh; the kernel keeps its frame, which has no column loop);
//   * VEC = 1, everything else: a lane of the group takes every LANES-th edge of the target and pushes the Fp products
//     through pair_tree, as tconv_dot_kernel does per (target, head).
//
// Backward (no atomics; one fixed order of every sum):
//   1 edot_bwd_dst_kernel<VEC, LANES>, a lane group per target: grad_dst[d] = sum of g[e] * x_src[col[e]], left to right.
//   2 the library's id sort of col_ind (host) and the prep kernel of kernels/agg.hip (agg_bwd_prepare), then
//     edot_bwd_chunk_kernel / edot_bwd_fold_kernel<VEC, LANES>: grad_src out of the walk of agg_common.cuh; the term of
//     sorted position i is g[order[i]] * x_dst[sorted_dst[i]], per source the edges in sorted order, cut into chunks of
//     kAggChunkEdges exactly as the agg backward.
//   No tree is involved in either, so both take 16-byte pieces whenever F % 4 == 0 and their rows are aligned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "gat_common.cuh"

namespace wm {
namespace {

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void edot_fwd_kernel(wm_edot_args p)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t F       = p.dim;
  for (int64_t d = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; d < p.n_dst;
       d += static_cast<int64_t>(gridDim.x) * kGroups) {
    int64_t e0, e1;
    edge_range(p.row_ptr, d, p.n_edges, e0, e1);
    if constexpr (VEC == 4) {   // the row lies within the group: F / 4 <= LANES
      const int lh      = static_cast<int>(F / 4);
      const int64_t cl  = gl < lh ? gl * 4 : 0;
      const fvec<4> xd  = ldv<4>(p.x_dst + d * p.x_dst_stride + cl);
      int my            = 0;
      fvec<4> v[kAggBatch];
      for_edge_batches<LANES>(
          e0, e1, gl, [&](int64_t e, bool in) { my = in ? p.col_ind[e] : 0; },
          [&](int k, int from, int64_t) {
            const int src = __shfl(my, from, LANES);
            v[k]          = ldv<4>(p.x_src + static_cast<int64_t>(src) * p.x_src_stride + cl);
          },
          [&](int k, int64_t e) {
            fvec<4> q;
#pragma unroll
            for (int t = 0; t < 4; ++t) q.v[t] = xd.v[t] * v[k].v[t];
            const float s = head_tree<LANES>(q, lh);
            if (gl == 0) p.score[e] = s;
          });
    } else {
      const uint32_t Fp = pow2_at_least(F);
      const float* y    = p.x_dst + d * p.x_dst_stride;
      for (int64_t e = e0 + gl; e < e1; e += LANES) {
        const float* x = p.x_src + static_cast<int64_t>(p.col_ind[e]) * p.x_src_stride;
        pair_tree t;
        t.top = 0.0f;
        for (uint32_t f = 0; f < Fp; ++f) t.push(f < F ? y[f] * x[f] : 0.0f, f);
        p.score[e] = t.top;
      }
    }
  }
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void edot_bwd_dst_kernel(wm_edot_args p)
{
  const int gl = threadIdx.x % LANES;
  for_target_pieces<VEC, LANES>(p, p.dim, [&](int64_t d, int64_t e0, int64_t e1, int64_t c, int64_t cl, bool act) {
    fvec<VEC> acc = splat<VEC>(-0.0f);
    int my        = 0;
    float my_g    = 0.0f;
    fvec<VEC> v[kAggBatch];
    float g[kAggBatch];
    for_edge_batches<LANES>(
        e0, e1, gl,
        [&](int64_t e, bool in) {
          my = 0, my_g = 0.0f;
          if (in) my = p.col_ind[e], my_g = p.grad[e];
        },
        [&](int k, int from, int64_t) {
          const int src = __shfl(my, from, LANES);
          g[k]          = __shfl(my_g, from, LANES);
          v[k]          = ldv<VEC>(p.x_src + static_cast<int64_t>(src) * p.x_src_stride + cl);
        },
        [&](int k, int64_t) { add_to(acc, scaled(v[k], g[k])); });
    if (act) stv(p.grad_dst + d * p.grad_dst_stride + c, e1 > e0 ? acc : splat<VEC>(0.0f));
  });
}

// acc += g[order[i]] * x_dst[sorted_dst[i]] for the sorted positions i in [eb0, ee), in that order (this lane's columns at cl)
template <int VEC, int LANES>
__device__ __forceinline__ void fold_edot_edges(fvec<VEC>& acc, const wm_edot_args& p, const csc_bwd_index& b, int64_t eb0,
                                                int64_t ee, int64_t cl, int gl)
{
  int my_d   = 0;
  float my_g = 0.0f;
  fvec<VEC> v[kAggBatch];
  float g[kAggBatch];
  for_edge_batches<LANES>(
      eb0, ee, gl,
      [&](int64_t i, bool in) {
        my_d = 0, my_g = 0.0f;
        if (in) my_d = b.sorted_dst[i], my_g = p.grad[b.order[i]];
      },
      [&](int k, int from, int64_t) {
        const int dst = __shfl(my_d, from, LANES);
        g[k]          = __shfl(my_g, from, LANES);
        v[k]          = ldv<VEC>(p.x_dst + static_cast<int64_t>(dst) * p.x_dst_stride + cl);
      },
      [&](int k, int64_t) { add_to(acc, scaled(v[k], g[k])); });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void edot_bwd_chunk_kernel(wm_edot_args p, csc_bwd_index b)
{
  const int gl = threadIdx.x % LANES;
  for_chunk_pieces<VEC, LANES>(b, p.dim, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    fvec<VEC> acc = splat<VEC>(-0.0f);
    fold_edot_edges<VEC, LANES>(acc, p, b, cs, ce, cl, gl);
    if (act) stv(b.partial + t * b.partial_stride + c, acc);
  });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void edot_bwd_fold_kernel(wm_edot_args p, csc_bwd_index b)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t F       = p.dim;
  const int64_t nu      = *b.n_unique;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; s < p.n_src;
       s += static_cast<int64_t>(gridDim.x) * kGroups) {
    const src_run r = run_of_source(b, nu, s);
    for (int64_t cb = 0; cb < F; cb += LANES * VEC) {
      const int64_t c  = cb + gl * VEC;
      const bool act   = c < F;
      const int64_t cl = act ? c : 0;
      fvec<VEC> acc    = splat<VEC>(-0.0f);
      fold_edot_edges<VEC, LANES>(acc, p, b, r.s0, r.c0e, cl, gl);
      add_partials(acc, b, r, cl);
      if (act) stv(p.grad_src + s * p.grad_src_stride + c, r.has ? acc : splat<VEC>(0.0f));
    }
  }
}

// the lane-split tree: F a power of two in [4, 256] (the row is then an aligned power-of-two range of at most 64 lanes)
bool fwd_vec4(const wm_edot_args* a)
{
  const int64_t F = a->dim;
  return F >= 4 && F <= 256 && (F & (F - 1)) == 0 && row16(a->x_src, a->x_src_stride) && row16(a->x_dst, a->x_dst_stride);
}
bool bwd_dst_vec4(const wm_edot_args* a)
{
  return a->dim % 4 == 0 && row16(a->x_src, a->x_src_stride) && row16(a->grad_dst, a->grad_dst_stride);
}
bool bwd_src_vec4(const wm_edot_args* a)
{
  return a->dim % 4 == 0 && row16(a->x_dst, a->x_dst_stride) && row16(a->grad_src, a->grad_src_stride);
}

}  // namespace

int hip_edot_forward(const wm_edot_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_dst == 0 || a->n_edges == 0) return 0;
  const bool v4 = fwd_vec4(a);
#define WM_EDOT_FWD(V, L)                                                                                              \
  hipLaunchKernelGGL((edot_fwd_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, *a)
  WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_EDOT_FWD);
#undef WM_EDOT_FWD
  return rc_last();
}

// the workspace of the per-source walk: sorted_dst, run_of and the partial rows, as the agg backward's (ws_plan lays them
// out); without grad_src, regions of no size
size_t hip_edot_backward_workspace_bytes(const wm_edot_args* a)
{
  const bool src = a->grad_src != nullptr && a->n_src > 0;
  return agg_bwd_plan(src ? a->n_edges : 0, src ? a->n_src : 0, a->dim, kAggChunkEdges).ws.bytes;
}

int hip_edot_backward(const wm_edot_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->grad_dst != nullptr && a->n_dst > 0) {
    const bool v4 = bwd_dst_vec4(a);
#define WM_EDOT_DST(V, L)                                                                                                 \
  hipLaunchKernelGGL((edot_bwd_dst_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a)
    WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_EDOT_DST);
#undef WM_EDOT_DST
    if (rc_last() != 0) return -2;
  }
  if (a->grad_src != nullptr && a->n_src > 0) {
    csc_bwd_index b;
    if (agg_bwd_prepare(*a, a->dim, ix, workspace, &b, stream_v) != 0) return -2;
    const bool v4 = bwd_src_vec4(a);
    if (b.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_EDOT_CHUNK(V, L)                                                                                                   \
  hipLaunchKernelGGL((edot_bwd_chunk_kernel<V, L>), dim3(blocks_for(b.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
      WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_EDOT_CHUNK);
#undef WM_EDOT_CHUNK
      if (rc_last() != 0) return -2;
    }
#define WM_EDOT_FOLD(V, L)                                                                                                   \
  hipLaunchKernelGGL((edot_bwd_fold_kernel<V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
    WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_EDOT_FOLD);
#undef WM_EDOT_FOLD
    if (rc_last() != 0) return -2;
  }
  return 0;
}

}  // namespace wm
