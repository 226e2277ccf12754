// wholegraph_amd — multi-head graph attention over a sampled CSC block (the GAT `mha_gat_n2n` op) on gfx950.
// The semantics and the one order of every fp32 sum: wholegraph_amd_ext.h, section 2c. H heads of F columns; head k owns
// columns [k*F, (k+1)*F) of a row of h. s_src / s_dst are the node scores, z = s_src[col[e]] + s_dst[d], l = LeakyReLU(z).
//
// Forward:
//   gat_score_kernel: one thread per (node, head): s_src[j,k] = att[0,k,:] . h[j,k,:] for j < n_src, s_dst[d,k] with att[1]
//     for d < n_dst, each a left-to-right sum over f.
//   gat_fwd_kernel (its body, gat_fwd_body, is in gat_common.cuh: gat_edge.hip compiles it with the edge term): one group
//     of LANES lanes per target d (LANES = 16 / 32 / 64 from the row's pieces, as agg_forward_kernel). A lane owns
//     VEC columns of one head hk and runs the softmax of that head itself: a pass over s_src for the max, one
//     for den = sum of expf(l - max) (left to right), then the pass over the neighbour rows, a batch of kAggBatch rows (and
//     their s_src) loaded back to back, alpha = expf(l - max) / den recomputed per edge with the same operations (so every
//     lane of head hk, and the alpha written out, hold the same bits). The lane at the head's first column writes alpha.
//     All three passes are walks of agg_common.cuh (for_target_pieces around three for_edge_batches).
//     With concat the group writes out; otherwise it writes the per-head rows to the workspace and gat_head_mean_kernel
//     forms ((o_0 + o_1) + ...) * fl(1/H).
//
// Backward (no atomics; one fixed order of every sum):
//   1 gat_bwd_edge_kernel (gat_bwd_dz_body in gat_common.cuh), one thread per (target, head): da = G_k . h[col[e], k, :]
//     per edge (kept in dz[]), c = sum of alpha * da, then dz = LeakyReLU'(z) * alpha * (da - c) per edge and ds_dst = sum of dz.
//   2 the library's id sort of col_ind (host), gat_bwd_prep_kernel: the target of each sorted position, run_of (as agg).
//   3 gat_bwd_chunk_kernel / gat_bwd_fold_kernel: per source j, P(j) = sum of alpha * G_k[dst] and ds_src(j) = sum of dz
//     over its edges in sorted order, cut into chunks of kAggChunkEdges exactly as the agg backward (the walk is
//     agg_common.cuh's; a chunk's ds_src rides behind the columns of its partial row); the fold then writes
//     grad_h[j] = (P + ds_src * att[0]) + ds_dst * att[1] (the last term for j < n_dst) and ds_src[j].
//   4 gat_att_chunk_kernel / gat_att_fold_kernel: grad_att[0] = sum over j of ds_src[j] * h[j] and grad_att[1] over
//     j < n_dst with ds_dst, in node chunks of kGatNodeChunk: each chunk left to right, the chunk sums in chunk order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../backend.hpp"
#include "gat_common.cuh"

namespace wm {
namespace {

// -0.0 is the identity of IEEE addition: acc = -0.0 followed by acc + t_0 + t_1 + ... is the left-to-right sum that starts
// from the first term (also when that term is -0.0)

template <int VEC>
__global__ __launch_bounds__(kAggBlock) void gat_score_kernel(wm_gat_args p)
{
  const int64_t H = p.heads, F = p.dim, n = (p.n_src + p.n_dst) * H;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t j = i / H, k = i - j * H;
    const bool dst  = j >= p.n_src;
    const float* x  = p.h + (dst ? j - p.n_src : j) * p.h_stride + k * F;
    const float* a  = p.att + (dst ? H * F : 0) + k * F;
    float acc       = -0.0f;
#pragma unroll 4
    for (int64_t f = 0; f < F; f += VEC) {
      const fvec<VEC> xv = ldv<VEC>(x + f), av = ldv<VEC>(a + f);
#pragma unroll
      for (int q = 0; q < VEC; ++q) acc = acc + av.v[q] * xv.v[q];
    }
    p.scores[i] = acc;
  }
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void gat_fwd_kernel(wm_gat_args p, float* o, int64_t o_stride)
{
  gat_fwd_body<VEC, LANES, false>(p, nullptr, o, o_stride);
}

// out[d, f] = ((o[d, 0, f] + o[d, 1, f]) + ...) * fl(1 / H)
__global__ __launch_bounds__(kAggBlock) void gat_head_mean_kernel(wm_gat_args p, const float* o, int64_t o_stride)
{
  const int64_t H = p.heads, F = p.dim, n = p.n_dst * F;
  const float r   = 1.0f / static_cast<float>(H);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t d = i / F, f = i - d * F;
    const float* row = o + d * o_stride + f;
    float acc        = row[0];
    for (int64_t k = 1; k < H; ++k) acc = acc + row[k * F];
    p.out[d * p.out_stride + f] = acc * r;
  }
}

template <int VEC>
__global__ __launch_bounds__(kAggBlock) void gat_bwd_edge_kernel(wm_gat_args p, wm_gat_bwd_state b)
{
  gat_bwd_dz_body<VEC, false>(p, nullptr, b);
}

__global__ __launch_bounds__(kAggBlock) void gat_bwd_prep_kernel(wm_gat_args p, wm_gat_bwd_state b)
{
  const int64_t nu = *b.ix.n_unique;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < p.n_edges;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    bwd_prep_at(i, p.row_ptr, p.n_dst, b.ix.order, b.ix.unique_ids, nu, b.ix.sorted_dst, b.ix.run_of);
}

// acc += alpha[e, hk] * G_k[dst(e)] and ds += dz[e, hk] for the edges at sorted positions [eb0, ee), in that order
template <int VEC, int LANES>
__device__ __forceinline__ void fold_gat_edges(fvec<VEC>& acc, float& ds, const wm_gat_args& p, const wm_gat_bwd_state& b,
                                               int64_t eb0, int64_t ee, int64_t gcol, int64_t hk, int gl)
{
  const int64_t H = p.heads;
  const float r   = 1.0f / static_cast<float>(H);
  int my_e = 0, my_d = 0;
  fvec<VEC> v[kAggBatch];
  float a[kAggBatch], z[kAggBatch];
  for_edge_batches<LANES>(
      eb0, ee, gl,
      [&](int64_t i, bool in) {
        my_e = 0, my_d = 0;
        if (in) my_e = b.ix.order[i], my_d = b.ix.sorted_dst[i];
      },
      [&](int k, int from, int64_t) {
        const int64_t e = __shfl(my_e, from, LANES);
        const int dst   = __shfl(my_d, from, LANES);
        v[k]            = ldv<VEC>(p.grad + static_cast<int64_t>(dst) * p.grad_stride + gcol);
        a[k]            = p.alpha[e * H + hk];
        z[k]            = b.dz[e * H + hk];
      },
      [&](int k, int64_t) {
        add_to(acc, scaled(p.concat ? v[k] : scaled(v[k], r), a[k]));
        ds = ds + z[k];
      });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void gat_bwd_chunk_kernel(wm_gat_args p, wm_gat_bwd_state b)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t F = p.dim;
  for_chunk_pieces<VEC, LANES>(b.ix, p.heads * F, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    const int64_t hk = cl / F;
    fvec<VEC> acc    = splat<VEC>(-0.0f);
    float ds         = -0.0f;
    fold_gat_edges<VEC, LANES>(acc, ds, p, b, cs, ce, p.concat ? cl : cl - hk * F, hk, gl);
    float* prow = b.ix.partial + t * b.ix.partial_stride;
    if (act) stv(prow + c, acc);
    if (act && c == hk * F) prow[b.ds_off + hk] = ds;
  });
}

// the ds_src of a chunk, kept behind the columns of its partial row: loaded and added with them (add_partials)
struct partial_ds {
  float& ds;
  int64_t col;   // ds_off + hk
  float pd[kAggBatch];
  __device__ __forceinline__ void load(const float* prow, int k) { pd[k] = prow[col]; }
  __device__ __forceinline__ void add(int k) { ds = ds + pd[k]; }
};

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void gat_bwd_fold_kernel(wm_gat_args p, wm_gat_bwd_state b)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t H = p.heads, F = p.dim, HF = H * F;
  const int64_t nu = *b.ix.n_unique;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; s < p.n_src;
       s += static_cast<int64_t>(gridDim.x) * kGroups) {
    const src_run r = run_of_source(b.ix, nu, s);
    for (int64_t cb = 0; cb < HF; cb += LANES * VEC) {
      const int64_t c  = cb + gl * VEC;
      const bool act   = c < HF;
      const int64_t cl = act ? c : 0;
      const int64_t hk = cl / F;
      fvec<VEC> acc    = splat<VEC>(-0.0f);
      float ds         = -0.0f;
      fold_gat_edges<VEC, LANES>(acc, ds, p, b, r.s0, r.c0e, p.concat ? cl : cl - hk * F, hk, gl);
      add_partials(acc, b.ix, r, cl, partial_ds{ds, b.ds_off + hk});
      if (!r.has) acc = splat<VEC>(0.0f), ds = 0.0f;
      fvec<VEC> res = acc;
      add_to(res, scaled(ldv<VEC>(p.att + cl), ds));
      if (s < p.n_dst) add_to(res, scaled(ldv<VEC>(p.att + HF + cl), b.ds_dst[s * H + hk]));
      if (act) stv(p.grad_h + s * p.grad_h_stride + c, res);
      if (act && c == hk * F) b.ds_src[s * H + hk] = ds;
    }
  }
}

// one thread per (node chunk q, column c of [0, 2 * H * F)): the chunk's sum of ds[j, k] * h[j, c'], left to right
__global__ __launch_bounds__(kAggBlock) void gat_att_chunk_kernel(wm_gat_args p, wm_gat_bwd_state b)
{
  const int64_t H = p.heads, F = p.dim, HF = H * F, W = 2 * HF, n = b.n_node_chunks * W;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t q = i / W, c = i - q * W;
    const bool half = c >= HF;
    const int64_t cc = half ? c - HF : c, k = cc / F;
    const int64_t rows = half ? p.n_dst : p.n_src;
    const float* ds    = half ? b.ds_dst : b.ds_src;
    const int64_t j0 = q * kGatNodeChunk, j1 = j0 + kGatNodeChunk < rows ? j0 + kGatNodeChunk : rows;
    float acc = -0.0f;
#pragma unroll 8
    for (int64_t j = j0; j < j1; ++j) acc = acc + ds[j * H + k] * p.h[j * p.h_stride + cc];
    b.att_partial[i] = acc;
  }
}

// grad_att[c]: the chunk sums in chunk order; +0.0 when the half has no rows
__global__ __launch_bounds__(kAggBlock) void gat_att_fold_kernel(wm_gat_args p, wm_gat_bwd_state b)
{
  const int64_t HF = p.heads * p.dim, W = 2 * HF;
  for (int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; c < W;
       c += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t rows = c >= HF ? p.n_dst : p.n_src;
    const int64_t nq   = (rows + kGatNodeChunk - 1) / kGatNodeChunk;
    float acc          = -0.0f;
#pragma unroll 8
    for (int64_t q = 0; q < nq; ++q) acc = acc + b.att_partial[q * W + c];
    p.grad_att[c] = nq > 0 ? acc : 0.0f;
  }
}

}  // namespace

size_t hip_gat_forward_workspace_bytes(const wm_gat_args* a)
{
  const int64_t sizes[1] = {a->n_dst * a->heads * a->dim * 4};   // the per-head rows before the mean over heads
  return a->concat ? 0 : ws_plan(sizes).bytes;
}

int gat_scores(const wm_gat_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const int64_t H = a->heads, F = a->dim, HF = H * F;
  const int64_t ns = (a->n_src + a->n_dst) * H;
  if (ns == 0) return 0;
  const bool v4 = F % 4 == 0 && aligned16(a->att) && use_vec4(HF, a->h, a->h_stride, a->h, a->h_stride);
  if (v4) hipLaunchKernelGGL(gat_score_kernel<4>, dim3(blocks_for(ns, kAggBlock)), dim3(kAggBlock), 0, stream, *a);
  else hipLaunchKernelGGL(gat_score_kernel<1>, dim3(blocks_for(ns, kAggBlock)), dim3(kAggBlock), 0, stream, *a);
  return rc_last();
}

int gat_head_mean(const wm_gat_args* a, const float* o, int64_t o_stride, void* stream_v)
{
  hipLaunchKernelGGL(gat_head_mean_kernel, dim3(blocks_for(a->n_dst * a->dim, kAggBlock)), dim3(kAggBlock), 0,
                     static_cast<hipStream_t>(stream_v), *a, o, o_stride);
  return rc_last();
}

int hip_gat_forward(const wm_gat_args* a, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const int64_t H = a->heads, F = a->dim, HF = H * F;
  const bool f4   = F % 4 == 0 && aligned16(a->att);
  if (gat_scores(a, stream_v) != 0) return -2;
  if (a->n_dst == 0) return 0;
  float* o         = a->concat ? a->out : ws_at<float>(workspace, 0);   // (the workspace's one region)
  const int64_t os = a->concat ? a->out_stride : HF;
  const bool v4    = f4 && use_vec4(HF, a->h, a->h_stride, o, os);
#define WM_GAT_FWD(V, L)                                                                                                   \
  hipLaunchKernelGGL((gat_fwd_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, *a, \
                     o, os)
  WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_GAT_FWD);
#undef WM_GAT_FWD
  if (rc_last() != 0) return -2;
  if (!a->concat && gat_head_mean(a, o, os, stream_v) != 0) return -2;
  return 0;
}

namespace {
struct gat_bwd_layout {
  int64_t n_tiles, partial_stride, ds_off, n_node_chunks;
  ws_layout<8> ws;   // sorted_dst, run_of, dz, ds_dst, ds_src, partial, att_partial, the caller's extra region
};

gat_bwd_layout bwd_layout(const wm_gat_args* a, int64_t extra_bytes)
{
  gat_bwd_layout l;
  const int64_t H = a->heads, HF = H * a->dim, E = a->n_edges;
  l.n_tiles        = (E + kAggChunkEdges - 1) / kAggChunkEdges;
  l.ds_off         = up4(HF);
  l.partial_stride = l.ds_off + up4(H);
  l.n_node_chunks  = (a->n_src + kGatNodeChunk - 1) / kGatNodeChunk;
  const int64_t sizes[8] = {E * 4, a->n_src * 4, E * H * 4, a->n_dst * H * 4, a->n_src * H * 4,
                            l.n_tiles * l.partial_stride * 4, l.n_node_chunks * 2 * HF * 4, extra_bytes};
  l.ws = ws_plan(sizes);
  return l;
}
}  // namespace

size_t gat_bwd_workspace_bytes(const wm_gat_args* a, int64_t extra_bytes) { return bwd_layout(a, extra_bytes).ws.bytes; }
size_t hip_gat_backward_workspace_bytes(const wm_gat_args* a) { return gat_bwd_workspace_bytes(a, 0); }

void* gat_bwd_carve(const wm_gat_args* a, const wm_edge_index& ix, void* workspace, int64_t extra_bytes,
                    wm_gat_bwd_state* b)
{
  const gat_bwd_layout l = bwd_layout(a, extra_bytes);
  set_sorted(b->ix, ix);
  b->ix.sorted_dst     = ws_at<int32_t>(workspace, l.ws.off[0]);
  b->ix.run_of         = ws_at<int32_t>(workspace, l.ws.off[1]);
  b->dz                = ws_at<float>(workspace, l.ws.off[2]);
  b->ds_dst            = ws_at<float>(workspace, l.ws.off[3]);
  b->ds_src            = ws_at<float>(workspace, l.ws.off[4]);
  b->ix.partial        = ws_at<float>(workspace, l.ws.off[5]);
  b->att_partial       = ws_at<float>(workspace, l.ws.off[6]);
  b->ix.n_tiles        = l.n_tiles;
  b->ix.partial_stride = l.partial_stride;
  b->ds_off            = l.ds_off;
  b->n_node_chunks     = l.n_node_chunks;
  return ws_at<void>(workspace, l.ws.off[7]);
}

int gat_bwd_after_dz(const wm_gat_args* a, const wm_gat_bwd_state* bp, void* stream_v)
{
  hipStream_t stream        = static_cast<hipStream_t>(stream_v);
  const wm_gat_bwd_state& b = *bp;
  const int64_t HF          = a->heads * a->dim;
  if (a->n_src > 0) {
    if (a->n_edges > 0) {
      const int blocks = blocks_for(a->n_edges, kAggBlock);
      hipLaunchKernelGGL(gat_bwd_prep_kernel, dim3(blocks < 8192 ? blocks : 8192), dim3(kAggBlock), 0, stream, *a, b);
      if (rc_last() != 0) return -2;
    }
    const bool v4 = gat_bwd_vec4(a) && use_vec4(HF, a->grad_h, a->grad_h_stride, a->grad_h, a->grad_h_stride);
    if (b.ix.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_GAT_CHUNK(V, L)                                                                                                   \
  hipLaunchKernelGGL((gat_bwd_chunk_kernel<V, L>), dim3(blocks_for(b.ix.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
      WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_GAT_CHUNK);
#undef WM_GAT_CHUNK
      if (rc_last() != 0) return -2;
    }
#define WM_GAT_FOLD(V, L)                                                                                                   \
  hipLaunchKernelGGL((gat_bwd_fold_kernel<V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
    WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_GAT_FOLD);
#undef WM_GAT_FOLD
    if (rc_last() != 0) return -2;
    hipLaunchKernelGGL(gat_att_chunk_kernel, dim3(blocks_for(b.n_node_chunks * 2 * HF, kAggBlock)), dim3(kAggBlock), 0,
                       stream, *a, b);
    if (rc_last() != 0) return -2;
  }
  hipLaunchKernelGGL(gat_att_fold_kernel, dim3(blocks_for(2 * HF, kAggBlock)), dim3(kAggBlock), 0, stream, *a, b);
  return rc_last();
}

int hip_gat_backward(const wm_gat_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  wm_gat_bwd_state b;
  gat_bwd_carve(a, ix, workspace, 0, &b);
  if (a->n_dst > 0) {
    const int blocks = blocks_for(a->n_dst * a->heads, kAggBlock);
    if (gat_bwd_vec4(a)) hipLaunchKernelGGL(gat_bwd_edge_kernel<4>, dim3(blocks), dim3(kAggBlock), 0, stream, *a, b);
    else hipLaunchKernelGGL(gat_bwd_edge_kernel<1>, dim3(blocks), dim3(kAggBlock), 0, stream, *a, b);
    if (rc_last() != 0) return -2;
  }
  return gat_bwd_after_dz(a, &b, stream_v);
}

}  // namespace wm
