// wholegraph_amd — edge-weighted neighbour aggregation of a sampled CSC block (`agg_concat_weighted`) on gfx950: the op of
// kernels/agg.hip with every neighbour row multiplied by a per-edge fp32 weight w[e], and gradients into the rows AND into
// the weights. Semantics and the one order of every sum: wholegraph_amd_ext.h, section (2d). Every product is rounded on its
// own before the add that follows it (-ffp-contract=off: no fused multiply-add).
//
// Forward (aggw_forward_kernel, the structure of agg_forward_kernel): a group of LANES lanes per target row; the column ids
//   and the weights of up to LANES edges are loaded coalesced and handed out with shuffles, the neighbour rows of a batch of
//   kAggBatch edges are loaded back to back, then multiplied and added in edge order (the walk of agg_common.cuh:
//   for_target_pieces, for_edge_batches; a lane fetches the column id and the weight of its position).
// Backward into x (aggw_bwd_chunk_kernel / aggw_bwd_fold_kernel): the per-source sums of kernels/agg.hip over the same id
//   sort, prep kernel and chunk tiles (agg_bwd_prepare) with the walk of agg_common.cuh; the term of sorted position j is
//   w[order[j]] * t(order[j]) (fold_edges_w).
// Backward into w (aggw_bwd_weight_kernel): a group of LANES lanes per kAggBatch consecutive edge positions (CSC order, so
//   the grad_out row of a target is reused from cache across its edges). Lane k < kAggBatch finds the target of edge k (a
//   search in row_ptr); both rows of every edge of the batch are loaded back to back as pieces. The dot product of an edge
//   is the balanced binary tree of (2d) over Fp = the next power of two >= dim columns: a lane's piece in registers, then
//   xor-butterflies at distance 1, 2, 4 ... over the group, which sums one aligned block of LANES * VEC columns; with more
//   than one block per row, lane k keeps the block sums of edge k on a binary-counter stack (block b is merged with the
//   stack levels of the trailing one bits of b), which is the same tree continued upwards. Columns in [dim, Fp) enter as
//   +0.0 (the stated padding), lanes past Fp as -0.0, the identity of IEEE addition, so the tree is the same for any group
//   size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "agg_common.cuh"

namespace wm {
namespace {

constexpr int kAggwStack = 20;   // levels of the block-sum stack: 2^20 blocks of at least 16 columns, more than any row here

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void aggw_forward_kernel(wm_aggw_args p)
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
    float my_w        = 0.0f;
    fvec<VEC> v[kAggBatch];
    float ws[kAggBatch];
    for_edge_batches<LANES>(
        e0, e1, gl, [&](int64_t e, bool in) { my = in ? p.col_ind[e] : 0, my_w = in ? p.w[e] : 0.0f; },
        [&](int k, int from, int64_t) {
          const int src = __shfl(my, from, LANES);
          ws[k]         = __shfl(my_w, from, LANES);
          v[k]          = ldv<VEC>(p.in + static_cast<int64_t>(src) * p.in_stride + cl);
        },
        [&](int k, int64_t) { add_to(acc, scaled(v[k], ws[k])); });
    if (act) {
      const fvec<VEC> a = deg == 0 ? splat<VEC>(0.0f) : (p.mean ? scaled(acc, r) : acc);
      stv(orow + c, a);
      stv(orow + F + c, ldv<VEC>(self + c));
    }
  });
}

// acc += w[order[j]] * t(order[j]) for the sorted positions j in [eb0, ee), in that order (this lane's columns at cl)
template <int VEC, int LANES>
__device__ __forceinline__ void fold_edges_w(fvec<VEC>& acc, const wm_aggw_args& p, const wm_agg_bwd_state& b, int64_t eb0,
                                             int64_t ee, int64_t cl, int gl)
{
  int my_d   = 0;
  float my_r = 1.0f, my_w = 0.0f;
  fvec<VEC> v[kAggBatch];
  float rs[kAggBatch], ws[kAggBatch];
  for_edge_batches<LANES>(
      eb0, ee, gl,
      [&](int64_t i, bool in) {
        my_d = 0, my_r = 1.0f, my_w = 0.0f;
        if (in) {
          my_d = b.sorted_dst[i];
          my_w = p.w[b.order[i]];
          if (p.mean) my_r = 1.0f / static_cast<float>(p.row_ptr[my_d + 1] - p.row_ptr[my_d]);
        }
      },
      [&](int k, int from, int64_t) {
        const int d = __shfl(my_d, from, LANES);
        rs[k]       = __shfl(my_r, from, LANES);
        ws[k]       = __shfl(my_w, from, LANES);
        v[k]        = ldv<VEC>(p.grad + static_cast<int64_t>(d) * p.grad_stride + cl);
      },
      [&](int k, int64_t) { add_to(acc, scaled(p.mean ? scaled(v[k], rs[k]) : v[k], ws[k])); });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void aggw_bwd_chunk_kernel(wm_aggw_args p, wm_agg_bwd_state b)
{
  const int gl = threadIdx.x % LANES;
  for_chunk_pieces<VEC, LANES>(b, p.dim, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    fvec<VEC> acc = splat<VEC>(-0.0f);
    fold_edges_w<VEC, LANES>(acc, p, b, cs, ce, cl, gl);
    if (act) stv(b.partial + t * b.partial_stride + c, acc);
  });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void aggw_bwd_fold_kernel(wm_aggw_args p, wm_agg_bwd_state b)
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
      fold_edges_w<VEC, LANES>(acc, p, b, r.s0, r.c0e, cl, gl);
      add_partials(acc, b, r, cl);
      const fvec<VEC> res = with_self_term(acc, r.has, self, p.grad, s * p.grad_stride + F + cl);
      if (act) stv(p.out + s * p.out_stride + c, res);
    }
  }
}

// the tree over one lane's piece: adjacent pairs, level by level
template <int VEC>
__device__ __forceinline__ float piece_tree(const fvec<VEC>& q)
{
  if constexpr (VEC == 4) {
    const float a = q.v[0] + q.v[1], b = q.v[2] + q.v[3];
    return a + b;
  } else {
    static_assert(VEC == 1, "pieces of 1 or 4 floats");
    return q.v[0];
  }
}

// grad_w[e] = tree sum over c of t(e)[c] * x[col_ind[e], c]; `fp` = the next power of two >= dim
template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void aggw_bwd_weight_kernel(wm_aggw_args p, int64_t fp)
{
  constexpr int kGroups    = kAggBlock / LANES;
  constexpr int64_t kBlock = LANES * VEC;   // columns the group sums per pass
  const int gl             = threadIdx.x % LANES;
  const int64_t F          = p.dim;
  const int64_t nblocks    = fp > kBlock ? fp / kBlock : 1;
  const int64_t ngroups    = (p.n_edges + kAggBatch - 1) / kAggBatch;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; g < ngroups;
       g += static_cast<int64_t>(gridDim.x) * kGroups) {
    const int64_t e0 = g * kAggBatch;
    const int nb     = static_cast<int>(p.n_edges - e0 < kAggBatch ? p.n_edges - e0 : kAggBatch);
    int my_src = 0, my_d = 0;
    float my_r = 1.0f;
    if (gl < nb) {
      const int64_t e = e0 + gl;
      my_src          = p.col_ind[e];
      int64_t lo = 0, hi = p.n_dst;   // the last d in [0, n_dst) with row_ptr[d] <= e
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (p.row_ptr[mid] <= e) lo = mid;
        else hi = mid;
      }
      my_d = static_cast<int>(lo);
      if (p.mean) my_r = 1.0f / static_cast<float>(p.row_ptr[lo + 1] - p.row_ptr[lo]);
    }
    int src[kAggBatch], dst[kAggBatch];
    float rs[kAggBatch];
#pragma unroll
    for (int k = 0; k < kAggBatch; ++k) {
      const int from = k < nb ? k : nb - 1;
      src[k]         = __shfl(my_src, from, LANES);
      dst[k]         = __shfl(my_d, from, LANES);
      rs[k]          = __shfl(my_r, from, LANES);
    }
    float st[kAggwStack];   // lane k: the block sums of edge k waiting for their sibling (level l: 2^l blocks)
#pragma unroll
    for (int l = 0; l < kAggwStack; ++l) st[l] = 0.0f;
    float total = 0.0f;
    for (int64_t blk = 0; blk < nblocks; ++blk) {
      const int64_t cb = blk * kBlock;
      const int64_t c  = cb + gl * VEC;
      float s[kAggBatch];
      if (cb < F) {   // (group-uniform)
        const bool act   = c < F;
        const int64_t cl = act ? c : 0;
        fvec<VEC> xv[kAggBatch], gv[kAggBatch];
#pragma unroll
        for (int k = 0; k < kAggBatch; ++k) {
          xv[k] = ldv<VEC>(p.in + static_cast<int64_t>(src[k]) * p.in_stride + cl);
          gv[k] = ldv<VEC>(p.grad + static_cast<int64_t>(dst[k]) * p.grad_stride + cl);
        }
        const float pad = c < fp ? 0.0f : -0.0f;
#pragma unroll
        for (int k = 0; k < kAggBatch; ++k) {
          fvec<VEC> q;
          const fvec<VEC> t = p.mean ? scaled(gv[k], rs[k]) : gv[k];
#pragma unroll
          for (int i = 0; i < VEC; ++i) q.v[i] = act ? t.v[i] * xv[k].v[i] : pad;
          float v = piece_tree<VEC>(q);
#pragma unroll
          for (int m = 1; m < LANES; m <<= 1) v = v + __shfl_xor(v, m, LANES);
          s[k] = v;
        }
      } else {
#pragma unroll
        for (int k = 0; k < kAggBatch; ++k) s[k] = 0.0f;   // a block of padding: +0.0 + +0.0 ...
      }
      float mine = 0.0f;
#pragma unroll
      for (int k = 0; k < kAggBatch; ++k)
        if (gl == k) mine = s[k];
      bool carry = true;   // push block `blk`: merge with the levels of its trailing one bits, park at the first zero bit
#pragma unroll
      for (int l = 0; l < kAggwStack; ++l) {
        if (carry) {
          if ((blk >> l) & 1) {
            mine = st[l] + mine;
          } else {
            st[l] = mine;
            carry = false;
          }
        }
      }
      total = mine;   // (after the last block: merged through every level)
    }
    if (gl < nb) p.grad_w[e0 + gl] = total;
  }
}

}  // namespace

int hip_aggw_forward(const wm_aggw_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_dst == 0 || a->dim == 0) return 0;
  const bool v4 = use_vec4(a->dim, a->in, a->in_stride, a->out, a->out_stride);
#define WM_AGGW_FWD(V, L)                                                                                                  \
  hipLaunchKernelGGL((aggw_forward_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a)
  WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_AGGW_FWD);
#undef WM_AGGW_FWD
  return rc_last();
}

int hip_aggw_backward(const wm_aggw_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->dim == 0) return 0;
  if (a->out != nullptr && a->n_src > 0) {   // grad_x: the per-source sums over the id sort
    wm_agg_bwd_state b;
    if (agg_bwd_prepare(*a, a->dim, ix, workspace, &b, stream_v) != 0) return -2;
    const bool v4 = use_vec4(a->dim, a->grad, a->grad_stride, a->out, a->out_stride);
    if (b.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_AGGW_CHUNK(V, L)                                                                                         \
  hipLaunchKernelGGL((aggw_bwd_chunk_kernel<V, L>), dim3(blocks_for(b.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
      WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_AGGW_CHUNK);
#undef WM_AGGW_CHUNK
      if (rc_last() != 0) return -2;
    }
#define WM_AGGW_FOLD(V, L)                                                                                        \
  hipLaunchKernelGGL((aggw_bwd_fold_kernel<V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
    WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_AGGW_FOLD);
#undef WM_AGGW_FOLD
    if (rc_last() != 0) return -2;
  }
  if (a->grad_w != nullptr && a->n_edges > 0) {   // grad_w: one dot product per edge, in CSC order
    const bool v4 = use_vec4(a->dim, a->grad, a->grad_stride, a->in, a->in_stride);
    int64_t fp    = 1;
    while (fp < a->dim) fp <<= 1;
    const int64_t groups = (a->n_edges + kAggBatch - 1) / kAggBatch;
#define WM_AGGW_WEIGHT(V, L)                                                                                      \
  hipLaunchKernelGGL((aggw_bwd_weight_kernel<V, L>), dim3(blocks_for(groups, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, fp)
    WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_AGGW_WEIGHT);
#undef WM_AGGW_WEIGHT
    if (rc_last() != 0) return -2;
  }
  return 0;
}

}  // namespace wm
