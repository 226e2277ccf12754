// wholegraph_amd — scaled dot-product multi-head attention over a sampled CSC block (the `mha_simple_n2n` op behind the
// TransformerConv layer) on gfx950. The semantics and the one order of every fp32 sum: wholegraph_amd_ext.h, section 2k. H
// heads of F columns; head k owns columns [k*F, (k+1)*F) of a row. t[e,k] = query[d] . key[col[e]] over the head's columns as
// a balanced tree of adjacent pairs over Fp (the smallest power of two >= F, padded with +0.0), l = t * scale (norm_by_dim)
// or t; the softmax of l over a target's edges weights the rows of `value`.
//
// The tree has the two implementations of gat_common.cuh that give the same bits:
//   * 16-byte instantiations (VEC = 4: F a power of two in [4, 256], every row 16-byte aligned): a lane owns 4 adjacent
//     columns and the F / 4 lanes of a head combine with xor exchanges (head_tree);
//   * everything else: tconv_dot_kernel, one thread per (target, head), pushes the Fp products through pair_tree, and the
//     element-wise instantiations (VEC = 1) of the row kernels read its result.
//
// Forward, tconv_fwd_kernel<VEC, LANES>: one group of LANES lanes per target d, the target's query piece in registers.
// Pass 1 (VEC = 4) reads the KEY rows, a batch of kAggBatch loaded back to back, and KEEPS the logits: the lane at the
// head's first column stores l into alpha[e, k] (the forward owns alpha until it writes it), the max m is taken on the way.
// Pass 2 reads the logits back for den = sum of expf(l - m), left to right; pass 3 reads the VALUE rows,
// alpha = expf(l - m) / den, o += alpha * row, and writes alpha over l. With VEC = 1 a head may span several column blocks
// of the group, so the logits live in the workspace instead of alpha. Passes 1 and 3, and both row passes of the per-target
// backward, are walks of agg_common.cuh (for_edge_batches inside for_target_pieces).
//
// Backward (no atomics; one fixed order of every sum):
//   1 tconv_bwd_dst_kernel<VEC, LANES>, a lane group per target (only when grad_query or grad_key is asked for): da by the
//     same tree over the VALUE rows (kept in scratch), c = sum of alpha * da; then a pass over the KEY rows:
//     ds = (alpha * (da - c)) * scale (or without the scale) to scratch — the scratch holds ds, not dl: that is what both
//     later sums multiply by — and grad_query[d] = sum of ds * key, left to right. Without grad_query the key rows are not
//     read.
//   2 the library's id sort of col_ind (host), tconv_bwd_prep_kernel, then tconv_bwd_chunk_kernel / tconv_bwd_fold_kernel:
//     grad_key and grad_value out of ONE walk (agg_common.cuh's) over a row of 2 * H * F columns. A lane's piece at column
//     c < H*F folds ds[e] * query[d(e)] (grad_key), a piece at c >= H*F folds alpha[e] * G_k[d(e)] (grad_value); per source
//     the edges in sorted order, cut into chunks of kAggChunkEdges exactly as the agg backward. order and sorted_dst are
//     loaded once for both. When only one of the two is asked for, the walk covers that half of the columns alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../backend.hpp"
#include "gat_common.cuh"

namespace wm {
namespace {

// backward scratch: the index of the per-source walk and the op's own regions of the workspace
struct tconv_bwd_state {
  csc_bwd_index ix;   // partial rows: 2 * heads * dim columns (the grad_key half, then the grad_value half)
  float* da;          // [n_edges, heads]
  float* ds;          // [n_edges, heads]
  int64_t c0, c1;     // the columns of the 2 * heads * dim the per-source walk covers
};

// one thread per (target d, head k). MODE 0: dst[e, k] = l[e, k]; MODE 1: dst[e, k] = da[e, k] = tree of G_k[d] * value
template <int MODE>
__global__ __launch_bounds__(kAggBlock) void tconv_dot_kernel(wm_tconv_args p, float* dst)
{
  const int64_t H = p.heads, F = p.dim, n = p.n_dst * H;
  const uint32_t Fp = pow2_at_least(F);
  const float r     = 1.0f / static_cast<float>(H);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t d = i / H, k = i - d * H;
    int64_t e0, e1;
    edge_range(p.row_ptr, d, p.n_edges, e0, e1);
    const float* y = MODE == 0 ? p.query + d * p.query_stride + k * F : p.grad + d * p.grad_stride + (p.concat ? k * F : 0);
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t j = p.col_ind[e];
      const float* x  = MODE == 0 ? p.key + j * p.key_stride + k * F : p.value + j * p.value_stride + k * F;
      pair_tree t;
      t.top = 0.0f;
      for (uint32_t f = 0; f < Fp; ++f) {
        float q = 0.0f;
        if (f < F) {
          if (MODE == 0) q = y[f] * x[f];
          else q = (p.concat ? y[f] : y[f] * r) * x[f];
        }
        t.push(q, f);
      }
      dst[e * H + k] = MODE == 0 && p.norm_by_dim ? t.top * p.scale : t.top;
    }
  }
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void tconv_fwd_kernel(wm_tconv_args p, float* o, int64_t o_stride, float* lbuf)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t H = p.heads, F = p.dim, HF = H * F;
  const int lh = static_cast<int>(F / 4);   // (VEC = 4) lanes of a head
  for_target_pieces<VEC, LANES>(p, HF, [&](int64_t d, int64_t e0, int64_t e1, int64_t c, int64_t cl, bool act) {
    const int64_t hk  = cl / F;   // (a piece never straddles two heads: VEC = 4 only when F % 4 == 0)
    const bool writer = act && c == hk * F;
    float m = -INFINITY, den = -0.0f;
    int my = 0;
    fvec<VEC> v[kAggBatch];
    float l[kAggBatch];
    const auto fetch = [&](int64_t e, bool in) { my = in ? p.col_ind[e] : 0; };
    if constexpr (VEC == 4) {   // pass 1: the logits, kept in lbuf (= alpha); a head lies within this column block
      const fvec<4> qd = ldv<4>(p.query + d * p.query_stride + cl);
      for_edge_batches<LANES>(
          e0, e1, gl, fetch,
          [&](int k, int from, int64_t) {
            const int src = __shfl(my, from, LANES);
            v[k]          = ldv<4>(p.key + static_cast<int64_t>(src) * p.key_stride + cl);
          },
          [&](int k, int64_t e) {
            fvec<4> q;
#pragma unroll
            for (int t = 0; t < 4; ++t) q.v[t] = qd.v[t] * v[k].v[t];
            float lg = head_tree<LANES>(q, lh);
            if (p.norm_by_dim) lg = lg * p.scale;
            m = fmaxf(m, lg);
            if (writer) lbuf[e * H + hk] = lg;
          });
      __threadfence_block();   // the head's other lanes read the logits back below
    } else {
#pragma unroll 4
      for (int64_t e = e0; e < e1; ++e) m = fmaxf(m, lbuf[e * H + hk]);
    }
#pragma unroll 4
    for (int64_t e = e0; e < e1; ++e) den = den + expf(lbuf[e * H + hk] - m);   // pass 2, left to right
    fvec<VEC> acc = splat<VEC>(-0.0f);
    for_edge_batches<LANES>(   // pass 3: the value rows
        e0, e1, gl, fetch,
        [&](int k, int from, int64_t e) {
          const int src = __shfl(my, from, LANES);
          v[k]          = ldv<VEC>(p.value + static_cast<int64_t>(src) * p.value_stride + cl);
          l[k]          = lbuf[e * H + hk];
        },
        [&](int k, int64_t e) {
          const float a = expf(l[k] - m) / den;
          add_to(acc, scaled(v[k], a));
          if (writer) p.alpha[e * H + hk] = a;
        });
    if (act) stv(o + d * o_stride + c, e1 > e0 ? acc : splat<VEC>(0.0f));
  });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void tconv_bwd_dst_kernel(wm_tconv_args p, tconv_bwd_state b)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t H = p.heads, F = p.dim, HF = H * F;
  const int lh  = static_cast<int>(F / 4);
  const float r = 1.0f / static_cast<float>(H);
  const bool gq = p.grad_query != nullptr;
  for_target_pieces<VEC, LANES>(p, HF, [&](int64_t d, int64_t e0, int64_t e1, int64_t c, int64_t cl, bool act) {
    const int64_t hk  = cl / F;
    const bool writer = act && c == hk * F;
    int my = 0;
    fvec<VEC> v[kAggBatch];
    float a[kAggBatch], x[kAggBatch];
    const auto fetch = [&](int64_t e, bool in) { my = in ? p.col_ind[e] : 0; };
    if constexpr (VEC == 4) {   // da by the tree, kept in b.da; a head lies within this column block
      fvec<4> gv = ldv<4>(p.grad + d * p.grad_stride + (p.concat ? cl : cl - hk * F));
      if (!p.concat) gv = scaled(gv, r);
      for_edge_batches<LANES>(
          e0, e1, gl, fetch,
          [&](int k, int from, int64_t) {
            const int src = __shfl(my, from, LANES);
            v[k]          = ldv<4>(p.value + static_cast<int64_t>(src) * p.value_stride + cl);
          },
          [&](int k, int64_t e) {
            fvec<4> q;
#pragma unroll
            for (int t = 0; t < 4; ++t) q.v[t] = gv.v[t] * v[k].v[t];
            const float da = head_tree<LANES>(q, lh);
            if (writer) b.da[e * H + hk] = da;
          });
      __threadfence_block();   // the head's other lanes read da back below
    }
    float cs = -0.0f;
#pragma unroll 4
    for (int64_t e = e0; e < e1; ++e) cs = cs + p.alpha[e * H + hk] * b.da[e * H + hk];
    fvec<VEC> gd = splat<VEC>(-0.0f);
    for_edge_batches<LANES>(   // ds, and grad_query from the key rows
        e0, e1, gl, fetch,
        [&](int k, int from, int64_t e) {
          const int src = __shfl(my, from, LANES);
          v[k]          = gq ? ldv<VEC>(p.key + static_cast<int64_t>(src) * p.key_stride + cl) : splat<VEC>(0.0f);
          a[k]          = p.alpha[e * H + hk];
          x[k]          = b.da[e * H + hk];
        },
        [&](int k, int64_t e) {
          const float dl = a[k] * (x[k] - cs);
          const float ds = p.norm_by_dim ? dl * p.scale : dl;
          add_to(gd, scaled(v[k], ds));
          if (writer) b.ds[e * H + hk] = ds;
        });
    if (act && gq) stv(p.grad_query + d * p.grad_query_stride + c, e1 > e0 ? gd : splat<VEC>(0.0f));
  });
}

__global__ __launch_bounds__(kAggBlock) void tconv_bwd_prep_kernel(wm_tconv_args p, tconv_bwd_state b)
{
  const int64_t nu = *b.ix.n_unique;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n_edges;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    bwd_prep_at(i, p.row_ptr, p.n_dst, b.ix.order, b.ix.unique_ids, nu, b.ix.sorted_dst, b.ix.run_of);
}

// what a lane's piece at column c2 of the 2 * H * F wide row reads per edge: a scalar sc[e, hk] and the row piece
// rows[dst(e) * stride + col], times r when `mean` (the grad_value half without concat)
struct tconv_piece {
  const float* sc;
  const float* rows;
  int64_t stride, col, hk;
  bool mean;
};

__device__ __forceinline__ tconv_piece piece_at(const wm_tconv_args& p, const tconv_bwd_state& b, int64_t c2)
{
  const int64_t F = p.dim, HF = p.heads * F;
  tconv_piece q;
  if (c2 < HF) {   // grad_key: ds * query[d]
    q.hk = c2 / F, q.sc = b.ds, q.rows = p.query, q.stride = p.query_stride, q.col = c2, q.mean = false;
  } else {         // grad_value: alpha * G_k[d]
    const int64_t cc = c2 - HF;
    q.hk = cc / F, q.sc = p.alpha, q.rows = p.grad, q.stride = p.grad_stride;
    q.col = p.concat ? cc : cc - q.hk * F, q.mean = !p.concat;
  }
  return q;
}

// acc += sc[e, hk] * row piece of dst(e) for the edges at sorted positions [eb0, ee), in that order
template <int VEC, int LANES>
__device__ __forceinline__ void fold_tconv_edges(fvec<VEC>& acc, const wm_tconv_args& p, const tconv_bwd_state& b,
                                                 const tconv_piece& q, int64_t eb0, int64_t ee, int gl)
{
  const int64_t H = p.heads;
  const float r   = 1.0f / static_cast<float>(H);
  int my_e = 0, my_d = 0;
  fvec<VEC> v[kAggBatch];
  float a[kAggBatch];
  for_edge_batches<LANES>(
      eb0, ee, gl,
      [&](int64_t i, bool in) {
        my_e = 0, my_d = 0;
        if (in) my_e = b.ix.order[i], my_d = b.ix.sorted_dst[i];
      },
      [&](int k, int from, int64_t) {
        const int64_t e = __shfl(my_e, from, LANES);
        const int dst   = __shfl(my_d, from, LANES);
        v[k]            = ldv<VEC>(q.rows + static_cast<int64_t>(dst) * q.stride + q.col);
        a[k]            = q.sc[e * H + q.hk];
      },
      [&](int k, int64_t) { add_to(acc, scaled(q.mean ? scaled(v[k], r) : v[k], a[k])); });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void tconv_bwd_chunk_kernel(wm_tconv_args p, tconv_bwd_state b)
{
  const int gl = threadIdx.x % LANES;
  for_chunk_pieces<VEC, LANES>(b.ix, b.c1 - b.c0, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    const tconv_piece q = piece_at(p, b, b.c0 + cl);
    fvec<VEC> acc       = splat<VEC>(-0.0f);
    fold_tconv_edges<VEC, LANES>(acc, p, b, q, cs, ce, gl);
    if (act) stv(b.ix.partial + t * b.ix.partial_stride + b.c0 + c, acc);
  });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void tconv_bwd_fold_kernel(wm_tconv_args p, tconv_bwd_state b)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t HF = p.heads * p.dim, width = b.c1 - b.c0;
  const int64_t nu = *b.ix.n_unique;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; s < p.n_src;
       s += static_cast<int64_t>(gridDim.x) * kGroups) {
    const src_run r = run_of_source(b.ix, nu, s);
    for (int64_t cb = 0; cb < width; cb += LANES * VEC) {
      const int64_t c   = cb + gl * VEC;
      const bool act    = c < width;
      const int64_t c2  = b.c0 + (act ? c : 0);   // column of the 2 * H * F
      const tconv_piece q = piece_at(p, b, c2);
      fvec<VEC> acc = splat<VEC>(-0.0f);
      fold_tconv_edges<VEC, LANES>(acc, p, b, q, r.s0, r.c0e, gl);
      add_partials(acc, b.ix, r, c2);
      if (!r.has) acc = splat<VEC>(0.0f);
      if (act) {
        if (c2 < HF) stv(p.grad_key + s * p.grad_key_stride + c2, acc);
        else stv(p.grad_value + s * p.grad_value_stride + (c2 - HF), acc);
      }
    }
  }
}

// the lane-split tree: F a power of two in [4, 256] (a head is then an aligned power-of-two range of at most 64 lanes)
bool tree_vec4(const wm_tconv_args* a)
{
  const int64_t F = a->dim;
  return F >= 4 && F <= 256 && (F & (F - 1)) == 0 && row16(a->key, a->key_stride) && row16(a->query, a->query_stride) &&
         row16(a->value, a->value_stride);
}
bool fwd_vec4(const wm_tconv_args* a)
{
  return tree_vec4(a) && (!a->concat || row16(a->out, a->out_stride));   // (the workspace rows of the head mean are aligned)
}
bool bwd_dst_vec4(const wm_tconv_args* a)
{
  return tree_vec4(a) && row16(a->grad, a->grad_stride) &&
         (a->grad_query == nullptr || row16(a->grad_query, a->grad_query_stride));
}
bool bwd_src_vec4(const wm_tconv_args* a)
{
  return a->dim % 4 == 0 && row16(a->query, a->query_stride) && row16(a->grad, a->grad_stride) &&
         (a->grad_key == nullptr || row16(a->grad_key, a->grad_key_stride)) &&
         (a->grad_value == nullptr || row16(a->grad_value, a->grad_value_stride));
}

struct tconv_bwd_layout {
  int64_t n_tiles, partial_stride;
  ws_layout<5> ws;   // sorted_dst, run_of, da, ds, partial
};

tconv_bwd_layout bwd_layout(const wm_tconv_args* a)
{
  tconv_bwd_layout l;
  const int64_t H = a->heads, HF = H * a->dim, E = a->n_edges;
  const bool src = a->grad_key != nullptr || a->grad_value != nullptr;
  const bool dst = a->grad_key != nullptr || a->grad_query != nullptr;
  l.n_tiles        = (E + kAggChunkEdges - 1) / kAggChunkEdges;
  l.partial_stride = up4(2 * HF);
  const int64_t sizes[5] = {src ? E * 4 : 0, src ? a->n_src * 4 : 0, dst ? E * H * 4 : 0, dst ? E * H * 4 : 0,
                            src ? l.n_tiles * l.partial_stride * 4 : 0};
  l.ws = ws_plan(sizes);
  return l;
}

// forward: the per-head rows before the mean over heads (without concat), the logits (element-wise instantiations)
ws_layout<2> fwd_layout(const wm_tconv_args* a)
{
  const int64_t sizes[2] = {a->concat ? 0 : a->n_dst * a->heads * a->dim * 4, fwd_vec4(a) ? 0 : a->n_edges * a->heads * 4};
  return ws_plan(sizes);
}

}  // namespace

size_t hip_tconv_forward_workspace_bytes(const wm_tconv_args* a)
{
  const bool rows = !a->concat && a->n_dst * a->heads * a->dim > 0, logits = !fwd_vec4(a) && a->n_edges * a->heads > 0;
  return rows || logits ? fwd_layout(a).bytes : 0;
}

int hip_tconv_forward(const wm_tconv_args* a, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const int64_t H = a->heads, F = a->dim, HF = H * F;
  if (a->n_dst == 0) return 0;
  const ws_layout<2> l = fwd_layout(a);
  float* o             = a->concat ? a->out : ws_at<float>(workspace, l.off[0]);
  const int64_t os     = a->concat ? a->out_stride : HF;
  const bool v4        = fwd_vec4(a);
  float* lbuf          = v4 ? a->alpha : ws_at<float>(workspace, l.off[1]);
  if (!v4 && a->n_edges > 0) {
    hipLaunchKernelGGL(tconv_dot_kernel<0>, dim3(blocks_for(a->n_dst * H, kAggBlock)), dim3(kAggBlock), 0, stream, *a, lbuf);
    if (rc_last() != 0) return -2;
  }
#define WM_TCONV_FWD(V, L)                                                                                                   \
  hipLaunchKernelGGL((tconv_fwd_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, *a, \
                     o, os, lbuf)
  WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_TCONV_FWD);
#undef WM_TCONV_FWD
  if (rc_last() != 0) return -2;
  if (!a->concat) {
    wm_gat_args g{};   // (the head mean reads the sizes and out only)
    g.n_dst      = a->n_dst;
    g.heads      = H;
    g.dim        = F;
    g.out        = a->out;
    g.out_stride = a->out_stride;
    if (gat_head_mean(&g, o, os, stream_v) != 0) return -2;
  }
  return 0;
}

size_t hip_tconv_backward_workspace_bytes(const wm_tconv_args* a) { return bwd_layout(a).ws.bytes; }

int hip_tconv_backward(const wm_tconv_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream       = static_cast<hipStream_t>(stream_v);
  const tconv_bwd_layout l = bwd_layout(a);
  const int64_t H = a->heads, HF = H * a->dim;
  tconv_bwd_state b;
  set_sorted(b.ix, ix);
  b.ix.sorted_dst     = ws_at<int32_t>(workspace, l.ws.off[0]);
  b.ix.run_of         = ws_at<int32_t>(workspace, l.ws.off[1]);
  b.da                = ws_at<float>(workspace, l.ws.off[2]);
  b.ds                = ws_at<float>(workspace, l.ws.off[3]);
  b.ix.partial        = ws_at<float>(workspace, l.ws.off[4]);
  b.ix.n_tiles        = l.n_tiles;
  b.ix.partial_stride = l.partial_stride;
  b.c0                = a->grad_key != nullptr ? 0 : HF;
  b.c1                = a->grad_value != nullptr ? 2 * HF : HF;
  if (a->n_dst > 0 && (a->grad_query != nullptr || a->grad_key != nullptr)) {
    const bool v4 = bwd_dst_vec4(a);
    if (!v4 && a->n_edges > 0) {
      hipLaunchKernelGGL(tconv_dot_kernel<1>, dim3(blocks_for(a->n_dst * H, kAggBlock)), dim3(kAggBlock), 0, stream, *a, b.da);
      if (rc_last() != 0) return -2;
    }
#define WM_TCONV_DST(V, L)                                                                                               \
  hipLaunchKernelGGL((tconv_bwd_dst_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
    WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_TCONV_DST);
#undef WM_TCONV_DST
    if (rc_last() != 0) return -2;
  }
  if (b.c1 > b.c0 && a->n_src > 0) {
    if (a->n_edges > 0) {
      const int blocks = blocks_for(a->n_edges, kAggBlock);
      hipLaunchKernelGGL(tconv_bwd_prep_kernel, dim3(blocks < 8192 ? blocks : 8192), dim3(kAggBlock), 0, stream, *a, b);
      if (rc_last() != 0) return -2;
    }
    const bool v4       = bwd_src_vec4(a);
    const int64_t width = b.c1 - b.c0;
    if (b.ix.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_TCONV_CHUNK(V, L)                                                                                   \
  hipLaunchKernelGGL((tconv_bwd_chunk_kernel<V, L>), dim3(blocks_for(b.ix.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
      WM_AGG_DISPATCH(v4, v4 ? width / 4 : width, WM_TCONV_CHUNK);
#undef WM_TCONV_CHUNK
      if (rc_last() != 0) return -2;
    }
#define WM_TCONV_FOLD(V, L)                                                                                  \
  hipLaunchKernelGGL((tconv_bwd_fold_kernel<V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
    WM_AGG_DISPATCH(v4, v4 ? width / 4 : width, WM_TCONV_FOLD);
#undef WM_TCONV_FOLD
    if (rc_last() != 0) return -2;
  }
  return 0;
}

}  // namespace wm
