// wholegraph_amd — GATv2 ("dynamic") multi-head graph attention over a sampled CSC block (the `mha_gat_v2_n2n` op) on
// gfx950. The semantics and the one order of every fp32 sum: wholegraph_amd_ext.h, section 2g. H heads of F columns; head k
// owns columns [k*F, (k+1)*F) of a row. u = h_src[col[e]] + h_dst[d], v = LeakyReLU(u), l[e,k] = att[k] . v as a balanced
// tree of adjacent pairs over Fp (the smallest power of two >= F, padded with +0.0).
//
// The tree has two implementations that give the same bits (pair_tree and head_tree of gat_common.cuh):
//   * 16-byte instantiations (VEC = 4: F a power of two in [4, 256], every row and att 16-byte aligned): a lane owns 4
//     adjacent columns, (q0 + q1) + (q2 + q3), and the F / 4 lanes of a head (an aligned power-of-two lane range of the
//     group) combine with xor exchanges at distance 1, 2, 4, ...: every lane of the head ends with the tree's root.
//   * everything else: gatv2_dot_kernel, one thread per (target, head), pushes the Fp terms through a binary-counter stack
//     held in registers (level i holds a finished subtree of 2^i terms waiting for its right sibling), and the element-wise
//     instantiations (VEC = 1) of the row kernels read its result.
//
// Forward, gatv2_fwd_kernel<VEC, LANES>: one group of LANES lanes per target d, the target's h_dst piece and the att piece
// in registers. Pass 1 (VEC = 4) reads the neighbour rows, a batch of kAggBatch loaded back to back, and KEEPS the logits:
// the lane at the head's first column stores l into alpha[e, k] (the forward owns alpha until it writes it), the max m is
// taken on the way. Pass 2 reads the logits back for den = sum of expf(l - m), left to right; pass 3 reads the rows a
// second time, alpha = expf(l - m) / den, o += alpha * row, and writes alpha over l. (The stated softmax needs m before
// any w; an online, rescaling softmax would change the bits.) With VEC = 1 a head may span several column blocks of the
// group, so the logits live in the workspace instead of alpha. Passes 1 and 3, and both row passes of the per-target
// backward, are walks of agg_common.cuh (for_edge_batches inside for_target_pieces): a kernel says what a slot loads and
// what it does with it.
//
// Backward (no atomics; one fixed order of every sum):
//   1 gatv2_bwd_dst_kernel<VEC, LANES>, a lane group per target: da by the same tree (kept in scratch), c = sum of
//     alpha * da; then a second pass over the rows: dl = alpha * (da - c) to scratch, grad_h_dst[d] = sum of dl * g and
//     A(d) = sum of dl * v, both left to right.
//   2 gatv2_att_chunk_kernel / gatv2_att_fold_kernel: grad_att = the A(d) summed in node chunks of kGatNodeChunk.
//   3 the library's id sort of col_ind (host), gatv2_bwd_prep_kernel, then gatv2_bwd_chunk_kernel / gatv2_bwd_fold_kernel:
//     per source j, the sum of (alpha * G_k[d]) + dl * g over its edges in sorted order, cut into chunks of kAggChunkEdges
//     exactly as the agg backward (the walk is agg_common.cuh's). Per edge they read G[d], h_dst[d], alpha[e] and dl[e];
//     the source's own row once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../backend.hpp"
#include "gat_common.cuh"

namespace wm {
namespace {

// backward scratch: the index of the per-source walk and the op's own regions of the workspace
struct gatv2_bwd_state {
  csc_bwd_index ix;
  float* da;                   // [n_edges, heads]
  float* dl;                   // [n_edges, heads]
  float* arow;                 // [n_dst, heads * dim]: A(d)
  float* att_partial;          // [n_node_chunks, heads * dim]
  int64_t n_node_chunks;
};

// one thread per (target d, head k). MODE 0: dst[e, k] = l[e, k]; MODE 1: dst[e, k] = da[e, k] = tree of G_k[d] * h_src
template <int MODE>
__global__ __launch_bounds__(kAggBlock) void gatv2_dot_kernel(wm_gatv2_args p, float* dst)
{
  const int64_t H = p.heads, F = p.dim, n = p.n_dst * H;
  const uint32_t Fp = pow2_at_least(F);
  const float r     = 1.0f / static_cast<float>(H);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t d = i / H, k = i - d * H;
    int64_t e0, e1;
    edge_range(p.row_ptr, d, p.n_edges, e0, e1);
    const float* y = MODE == 0 ? p.h_dst + d * p.h_dst_stride + k * F : p.grad + d * p.grad_stride + (p.concat ? k * F : 0);
    const float* a = p.att + k * F;
    for (int64_t e = e0; e < e1; ++e) {
      const float* x = p.h_src + static_cast<int64_t>(p.col_ind[e]) * p.h_src_stride + k * F;
      pair_tree t;
      t.top = 0.0f;
      for (uint32_t f = 0; f < Fp; ++f) {
        float q = 0.0f;
        if (f < F) {
          if (MODE == 0) q = a[f] * leaky(x[f] + y[f], p.slope);
          else q = (p.concat ? y[f] : y[f] * r) * x[f];
        }
        t.push(q, f);
      }
      dst[e * H + k] = t.top;
    }
  }
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void gatv2_fwd_kernel(wm_gatv2_args p, float* o, int64_t o_stride, float* lbuf)
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
      const fvec<4> hd = ldv<4>(p.h_dst + d * p.h_dst_stride + cl), av = ldv<4>(p.att + cl);
      for_edge_batches<LANES>(
          e0, e1, gl, fetch,
          [&](int k, int from, int64_t) {
            const int src = __shfl(my, from, LANES);
            v[k]          = ldv<4>(p.h_src + static_cast<int64_t>(src) * p.h_src_stride + cl);
          },
          [&](int k, int64_t e) {
            fvec<4> q;
#pragma unroll
            for (int t = 0; t < 4; ++t) q.v[t] = av.v[t] * leaky(v[k].v[t] + hd.v[t], p.slope);
            const float lg = head_tree<LANES>(q, lh);
            m              = fmaxf(m, lg);
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
    for_edge_batches<LANES>(   // pass 3: the rows again
        e0, e1, gl, fetch,
        [&](int k, int from, int64_t e) {
          const int src = __shfl(my, from, LANES);
          v[k]          = ldv<VEC>(p.h_src + static_cast<int64_t>(src) * p.h_src_stride + cl);
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
__global__ __launch_bounds__(kAggBlock) void gatv2_bwd_dst_kernel(wm_gatv2_args p, gatv2_bwd_state b)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t H = p.heads, F = p.dim, HF = H * F;
  const int lh  = static_cast<int>(F / 4);
  const float r = 1.0f / static_cast<float>(H);
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
            v[k]          = ldv<4>(p.h_src + static_cast<int64_t>(src) * p.h_src_stride + cl);
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
    const fvec<VEC> hd = ldv<VEC>(p.h_dst + d * p.h_dst_stride + cl), av = ldv<VEC>(p.att + cl);
    fvec<VEC> gd = splat<VEC>(-0.0f), ar = splat<VEC>(-0.0f);
    for_edge_batches<LANES>(
        e0, e1, gl, fetch,
        [&](int k, int from, int64_t e) {
          const int src = __shfl(my, from, LANES);
          v[k]          = ldv<VEC>(p.h_src + static_cast<int64_t>(src) * p.h_src_stride + cl);
          a[k]          = p.alpha[e * H + hk];
          x[k]          = b.da[e * H + hk];
        },
        [&](int k, int64_t e) {
          const float dl = a[k] * (x[k] - cs);
#pragma unroll
          for (int t = 0; t < VEC; ++t) {
            const float u = v[k].v[t] + hd.v[t];
            const float g = u > 0.0f ? av.v[t] : av.v[t] * p.slope;
            gd.v[t]       = gd.v[t] + dl * g;
            ar.v[t]       = ar.v[t] + dl * leaky(u, p.slope);
          }
          if (writer) b.dl[e * H + hk] = dl;
        });
    if (e1 == e0) gd = splat<VEC>(0.0f), ar = splat<VEC>(0.0f);
    if (act && p.grad_h_dst != nullptr) stv(p.grad_h_dst + d * p.grad_h_dst_stride + c, gd);
    if (act && p.grad_att != nullptr) stv(b.arow + d * HF + c, ar);
  });
}

// one thread per (node chunk q, column c): the chunk's sum of A(d)[c], left to right
__global__ __launch_bounds__(kAggBlock) void gatv2_att_chunk_kernel(wm_gatv2_args p, gatv2_bwd_state b)
{
  const int64_t HF = p.heads * p.dim, n = b.n_node_chunks * HF;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t q = i / HF, c = i - q * HF;
    const int64_t j0 = q * kGatNodeChunk, j1 = j0 + kGatNodeChunk < p.n_dst ? j0 + kGatNodeChunk : p.n_dst;
    float acc = -0.0f;
#pragma unroll 8
    for (int64_t j = j0; j < j1; ++j) acc = acc + b.arow[j * HF + c];
    b.att_partial[i] = acc;
  }
}

// grad_att[c]: the chunk sums in chunk order; +0.0 without targets
__global__ __launch_bounds__(kAggBlock) void gatv2_att_fold_kernel(wm_gatv2_args p, gatv2_bwd_state b)
{
  const int64_t HF = p.heads * p.dim;
  for (int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; c < HF;
       c += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float acc = -0.0f;
#pragma unroll 8
    for (int64_t q = 0; q < b.n_node_chunks; ++q) acc = acc + b.att_partial[q * HF + c];
    p.grad_att[c] = b.n_node_chunks > 0 ? acc : 0.0f;
  }
}

__global__ __launch_bounds__(kAggBlock) void gatv2_bwd_prep_kernel(wm_gatv2_args p, gatv2_bwd_state b)
{
  const int64_t nu = *b.ix.n_unique;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n_edges;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    bwd_prep_at(i, p.row_ptr, p.n_dst, b.ix.order, b.ix.unique_ids, nu, b.ix.sorted_dst, b.ix.run_of);
}

// acc += (alpha[e, hk] * G_k[dst(e)]) + dl[e, hk] * g for the edges at sorted positions [eb0, ee), in that order; hs is the
// source's own piece, av the piece of att
template <int VEC, int LANES>
__device__ __forceinline__ void fold_gatv2_edges(fvec<VEC>& acc, const wm_gatv2_args& p, const gatv2_bwd_state& b,
                                                 const fvec<VEC>& hs, const fvec<VEC>& av, int64_t eb0, int64_t ee,
                                                 int64_t gcol, int64_t cl, int64_t hk, int gl)
{
  const int64_t H = p.heads;
  const float r   = 1.0f / static_cast<float>(H);
  int my_e = 0, my_d = 0;
  fvec<VEC> gv[kAggBatch], hd[kAggBatch];
  float a[kAggBatch], x[kAggBatch];
  for_edge_batches<LANES>(
      eb0, ee, gl,
      [&](int64_t i, bool in) {
        my_e = 0, my_d = 0;
        if (in) my_e = b.ix.order[i], my_d = b.ix.sorted_dst[i];
      },
      [&](int k, int from, int64_t) {
        const int64_t e = __shfl(my_e, from, LANES);
        const int dst   = __shfl(my_d, from, LANES);
        gv[k]           = ldv<VEC>(p.grad + static_cast<int64_t>(dst) * p.grad_stride + gcol);
        hd[k]           = ldv<VEC>(p.h_dst + static_cast<int64_t>(dst) * p.h_dst_stride + cl);
        a[k]            = p.alpha[e * H + hk];
        x[k]            = b.dl[e * H + hk];
      },
      [&](int k, int64_t) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
          const float t1 = (p.concat ? gv[k].v[t] : gv[k].v[t] * r) * a[k];
          const float u  = hs.v[t] + hd[k].v[t];
          const float g  = u > 0.0f ? av.v[t] : av.v[t] * p.slope;
          acc.v[t]       = acc.v[t] + (t1 + x[k] * g);
        }
      });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void gatv2_bwd_chunk_kernel(wm_gatv2_args p, gatv2_bwd_state b)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t F = p.dim;
  for_chunk_pieces<VEC, LANES>(b.ix, p.heads * F, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    const int64_t s    = p.col_ind[b.ix.order[cs]];   // the source this chunk belongs to
    const int64_t hk   = cl / F;
    const fvec<VEC> hs = ldv<VEC>(p.h_src + s * p.h_src_stride + cl), av = ldv<VEC>(p.att + cl);
    fvec<VEC> acc = splat<VEC>(-0.0f);
    fold_gatv2_edges<VEC, LANES>(acc, p, b, hs, av, cs, ce, p.concat ? cl : cl - hk * F, cl, hk, gl);
    if (act) stv(b.ix.partial + t * b.ix.partial_stride + c, acc);
  });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void gatv2_bwd_fold_kernel(wm_gatv2_args p, gatv2_bwd_state b)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t F = p.dim, HF = p.heads * F;
  const int64_t nu = *b.ix.n_unique;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; s < p.n_src;
       s += static_cast<int64_t>(gridDim.x) * kGroups) {
    const src_run r = run_of_source(b.ix, nu, s);
    for (int64_t cb = 0; cb < HF; cb += LANES * VEC) {
      const int64_t c  = cb + gl * VEC;
      const bool act   = c < HF;
      const int64_t cl = act ? c : 0;
      const int64_t hk = cl / F;
      const fvec<VEC> hs = ldv<VEC>(p.h_src + s * p.h_src_stride + cl), av = ldv<VEC>(p.att + cl);
      fvec<VEC> acc = splat<VEC>(-0.0f);
      fold_gatv2_edges<VEC, LANES>(acc, p, b, hs, av, r.s0, r.c0e, p.concat ? cl : cl - hk * F, cl, hk, gl);
      add_partials(acc, b.ix, r, cl);
      if (!r.has) acc = splat<VEC>(0.0f);
      if (act) stv(p.grad_h_src + s * p.grad_h_src_stride + c, acc);
    }
  }
}

// the lane-split tree: F a power of two in [4, 256] (a head is then an aligned power-of-two range of at most 64 lanes)
bool tree_vec4(const wm_gatv2_args* a)
{
  const int64_t F = a->dim;
  return F >= 4 && F <= 256 && (F & (F - 1)) == 0 && aligned16(a->att) && row16(a->h_src, a->h_src_stride) &&
         row16(a->h_dst, a->h_dst_stride);
}
bool fwd_vec4(const wm_gatv2_args* a)
{
  return tree_vec4(a) && (!a->concat || row16(a->out, a->out_stride));   // (the workspace rows of the head mean are aligned)
}
bool bwd_dst_vec4(const wm_gatv2_args* a)
{
  return tree_vec4(a) && row16(a->grad, a->grad_stride) &&
         (a->grad_h_dst == nullptr || row16(a->grad_h_dst, a->grad_h_dst_stride));
}
bool bwd_src_vec4(const wm_gatv2_args* a)
{
  return a->dim % 4 == 0 && aligned16(a->att) && row16(a->h_src, a->h_src_stride) && row16(a->h_dst, a->h_dst_stride) &&
         row16(a->grad, a->grad_stride) && row16(a->grad_h_src, a->grad_h_src_stride);
}

struct gatv2_bwd_layout {
  int64_t n_tiles, partial_stride, n_node_chunks;
  ws_layout<7> ws;   // sorted_dst, run_of, da, dl, arow, att_partial, partial
};

gatv2_bwd_layout bwd_layout(const wm_gatv2_args* a)
{
  gatv2_bwd_layout l;
  const int64_t H = a->heads, HF = H * a->dim, E = a->n_edges;
  const bool src = a->grad_h_src != nullptr, att = a->grad_att != nullptr;
  l.n_tiles        = (E + kAggChunkEdges - 1) / kAggChunkEdges;
  l.partial_stride = up4(HF);
  l.n_node_chunks  = (a->n_dst + kGatNodeChunk - 1) / kGatNodeChunk;
  const int64_t sizes[7] = {src ? E * 4 : 0,
                            src ? a->n_src * 4 : 0,
                            E * H * 4,
                            E * H * 4,
                            att ? a->n_dst * HF * 4 : 0,
                            att ? l.n_node_chunks * HF * 4 : 0,
                            src ? l.n_tiles * l.partial_stride * 4 : 0};
  l.ws = ws_plan(sizes);
  return l;
}

// forward: the per-head rows before the mean over heads (without concat), the logits (element-wise instantiations)
ws_layout<2> fwd_layout(const wm_gatv2_args* a)
{
  const int64_t sizes[2] = {a->concat ? 0 : a->n_dst * a->heads * a->dim * 4, fwd_vec4(a) ? 0 : a->n_edges * a->heads * 4};
  return ws_plan(sizes);
}

}  // namespace

size_t hip_gatv2_forward_workspace_bytes(const wm_gatv2_args* a)
{
  const bool rows = !a->concat && a->n_dst * a->heads * a->dim > 0, logits = !fwd_vec4(a) && a->n_edges * a->heads > 0;
  return rows || logits ? fwd_layout(a).bytes : 0;
}

int hip_gatv2_forward(const wm_gatv2_args* a, void* workspace, void* stream_v)
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
    hipLaunchKernelGGL(gatv2_dot_kernel<0>, dim3(blocks_for(a->n_dst * H, kAggBlock)), dim3(kAggBlock), 0, stream, *a, lbuf);
    if (rc_last() != 0) return -2;
  }
#define WM_GATV2_FWD(V, L)                                                                                                   \
  hipLaunchKernelGGL((gatv2_fwd_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, *a, \
                     o, os, lbuf)
  WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_GATV2_FWD);
#undef WM_GATV2_FWD
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

size_t hip_gatv2_backward_workspace_bytes(const wm_gatv2_args* a) { return bwd_layout(a).ws.bytes; }

int hip_gatv2_backward(const wm_gatv2_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream       = static_cast<hipStream_t>(stream_v);
  const gatv2_bwd_layout l = bwd_layout(a);
  const int64_t H = a->heads, HF = H * a->dim;
  gatv2_bwd_state b;
  set_sorted(b.ix, ix);
  b.ix.sorted_dst     = ws_at<int32_t>(workspace, l.ws.off[0]);
  b.ix.run_of         = ws_at<int32_t>(workspace, l.ws.off[1]);
  b.da                = ws_at<float>(workspace, l.ws.off[2]);
  b.dl                = ws_at<float>(workspace, l.ws.off[3]);
  b.arow              = ws_at<float>(workspace, l.ws.off[4]);
  b.att_partial       = ws_at<float>(workspace, l.ws.off[5]);
  b.ix.partial        = ws_at<float>(workspace, l.ws.off[6]);
  b.ix.n_tiles        = l.n_tiles;
  b.ix.partial_stride = l.partial_stride;
  b.n_node_chunks     = l.n_node_chunks;
  if (a->n_dst > 0) {
    const bool v4 = bwd_dst_vec4(a);
    if (!v4 && a->n_edges > 0) {
      hipLaunchKernelGGL(gatv2_dot_kernel<1>, dim3(blocks_for(a->n_dst * H, kAggBlock)), dim3(kAggBlock), 0, stream, *a, b.da);
      if (rc_last() != 0) return -2;
    }
#define WM_GATV2_DST(V, L)                                                                                               \
  hipLaunchKernelGGL((gatv2_bwd_dst_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
    WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_GATV2_DST);
#undef WM_GATV2_DST
    if (rc_last() != 0) return -2;
  }
  if (a->grad_att != nullptr) {
    if (a->n_dst > 0) {
      hipLaunchKernelGGL(gatv2_att_chunk_kernel, dim3(blocks_for(b.n_node_chunks * HF, kAggBlock)), dim3(kAggBlock), 0, stream,
                         *a, b);
      if (rc_last() != 0) return -2;
    }
    hipLaunchKernelGGL(gatv2_att_fold_kernel, dim3(blocks_for(HF, kAggBlock)), dim3(kAggBlock), 0, stream, *a, b);
    if (rc_last() != 0) return -2;
  }
  if (a->grad_h_src != nullptr && a->n_src > 0) {
    if (a->n_edges > 0) {
      const int blocks = blocks_for(a->n_edges, kAggBlock);
      hipLaunchKernelGGL(gatv2_bwd_prep_kernel, dim3(blocks < 8192 ? blocks : 8192), dim3(kAggBlock), 0, stream, *a, b);
      if (rc_last() != 0) return -2;
    }
    const bool v4 = bwd_src_vec4(a);
    if (b.ix.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_GATV2_CHUNK(V, L)                                                                                   \
  hipLaunchKernelGGL((gatv2_bwd_chunk_kernel<V, L>), dim3(blocks_for(b.ix.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
      WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_GATV2_CHUNK);
#undef WM_GATV2_CHUNK
      if (rc_last() != 0) return -2;
    }
#define WM_GATV2_FOLD(V, L)                                                                                  \
  hipLaunchKernelGGL((gatv2_bwd_fold_kernel<V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
    WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_GATV2_FOLD);
#undef WM_GATV2_FOLD
    if (rc_last() != 0) return -2;
  }
  return 0;
}

}  // namespace wm
