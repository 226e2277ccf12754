// wholegraph_amd — multi-head graph attention over a sampled CSC block with an edge term in the logit (the GAT
// `mha_gat_n2n(..., edge_feat=...)` op) on gfx950. The semantics and the one order of every fp32 sum: wholegraph_amd_ext.h,
// section 2f. It is section 2c with z = (s_src[col[e]] + s_dst[d]) + s_edge[e], s_edge[e,k] = att[2,k,:] . edge_feat[e,k,:].
// The stages that do not see the logit are gat.hip's own kernels (gat_common.cuh); what is new here:
//
// Forward:
//   gat_edge_score_kernel: s_edge. edge_feat is the op's largest stream (E rows of H * F floats), so it is not read the way
//     gat_score_kernel reads h (one thread walking F floats, F floats between neighbouring threads). A block takes 256
//     consecutive (edge, head) segments. For each slab of up to 32 columns its threads copy the segments' floats to LDS in
//     memory order — neighbouring lanes read neighbouring addresses, 16-byte pieces when the rows allow — then each thread
//     walks its own segment in LDS, left to right, adding att[2,k,f] * edge_feat[e,k,f]. A segment's LDS pitch is odd, so
//     the 32 lanes of a ds_read_b32 group hit 32 banks.
//   gat_edge_fwd_kernel: gat_fwd_kernel with edge_scores[e, hk] loaded next to s_src in every batch: the same body
//     (gat_fwd_body in gat_common.cuh) compiled with the edge term.
// Backward:
//   gat_edge_bwd_dz_kernel: gat_bwd_edge_kernel with the edge term in the recomputed z (gat_bwd_dz_body, likewise); then
//     gat.hip's steps 2 - 4.
//   gat_edge_grad_chunk_kernel: one thread per (edge chunk q, piece of columns): grad_edge_feat[e] = dz[e,k] * att[2] for
//     the chunk's edges and, from the same dz, the chunk's sum of dz[e,k] * edge_feat[e], left to right; chunks of
//     kGatNodeChunk edges. gat_edge_att_fold_kernel adds the chunk sums in chunk order into grad_att[2].
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../backend.hpp"
#include "gat_common.cuh"

namespace wm {
namespace {

constexpr int kEdgeSlab = 32;   // columns of a segment staged per pass: 128 bytes, a cache line

template <int VEC>
__global__ __launch_bounds__(kAggBlock) void gat_edge_score_kernel(wm_gat_edge_args p)
{
  __shared__ float tile[kAggBlock * (kEdgeSlab + 1)];
  const int64_t H = p.g.heads, F = p.g.dim, nseg = p.g.n_edges * H;
  const float* a2 = p.g.att + 2 * H * F;
  const uint32_t h32 = static_cast<uint32_t>(H);
  for (int64_t t0 = static_cast<int64_t>(blockIdx.x) * kAggBlock; t0 < nseg;   // (block-uniform: the barriers stay in step)
       t0 += static_cast<int64_t>(gridDim.x) * kAggBlock) {
    const int ns      = static_cast<int>(nseg - t0 < kAggBlock ? nseg - t0 : kAggBlock);
    const int64_t e0  = t0 / H;
    const uint32_t k0 = static_cast<uint32_t>(t0 - e0 * H);   // segment t0 + s is (e0 + (k0 + s) / H, (k0 + s) % H)
    const bool act    = static_cast<int>(threadIdx.x) < ns;
    const uint32_t k  = act ? (k0 + threadIdx.x) % h32 : 0;
    const float* a    = a2 + static_cast<int64_t>(k) * F;
    float acc         = -0.0f;
    for (int64_t f0 = 0; f0 < F; f0 += kEdgeSlab) {
      const int fw    = static_cast<int>(F - f0 < kEdgeSlab ? F - f0 : kEdgeSlab);
      const int pitch = fw | 1;
      const int ppr   = fw / VEC;   // pieces of a segment in this slab
      const int np    = ns * ppr;
#pragma unroll 4
      for (int q = threadIdx.x; q < np; q += kAggBlock) {
        const int s       = q / ppr, c = (q - s * ppr) * VEC;
        const uint32_t t  = k0 + static_cast<uint32_t>(s), de = t / h32, kk = t - de * h32;
        const fvec<VEC> v = ldv<VEC>(p.edge_feat + (e0 + de) * p.ef_stride + static_cast<int64_t>(kk) * F + f0 + c);
#pragma unroll
        for (int i = 0; i < VEC; ++i) tile[s * pitch + c + i] = v.v[i];
      }
      __syncthreads();
      if (act) {
        const float* row = tile + threadIdx.x * pitch;
#pragma unroll 8
        for (int f = 0; f < fw; ++f) acc = acc + a[f0 + f] * row[f];
      }
      __syncthreads();
    }
    if (act) p.edge_scores[t0 + threadIdx.x] = acc;
  }
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void gat_edge_fwd_kernel(wm_gat_edge_args pe, float* o, int64_t o_stride)
{
  gat_fwd_body<VEC, LANES, true>(pe.g, pe.edge_scores, o, o_stride);
}

template <int VEC>
__global__ __launch_bounds__(kAggBlock) void gat_edge_bwd_dz_kernel(wm_gat_edge_args pe, wm_gat_bwd_state b)
{
  gat_bwd_dz_body<VEC, true>(pe.g, pe.edge_scores, b);
}

// one thread per (edge chunk q, piece of VEC columns at c): grad_edge_feat[e, c..] = dz[e, k] * att[2, c..] for the edges
// of the chunk, and partial[q, c..] = their sum of dz[e, k] * edge_feat[e, c..], left to right; a batch of rows in flight
template <int VEC>
__global__ __launch_bounds__(kAggBlock) void gat_edge_grad_chunk_kernel(wm_gat_edge_args pe, const float* dz, float* partial,
                                                                        int64_t n_chunks)
{
  const wm_gat_args& p = pe.g;
  const int64_t H = p.heads, F = p.dim, HF = H * F, W = HF / VEC, n = n_chunks * W;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t q = i / W, c = (i - q * W) * VEC, k = c / F;
    const fvec<VEC> av = ldv<VEC>(p.att + 2 * HF + c);
    const int64_t e0 = q * kGatNodeChunk, e1 = e0 + kGatNodeChunk < p.n_edges ? e0 + kGatNodeChunk : p.n_edges;
    fvec<VEC> acc = splat<VEC>(-0.0f);
    for (int64_t eb = e0; eb < e1; eb += kAggBatch) {
      fvec<VEC> x[kAggBatch];
      float z[kAggBatch];
#pragma unroll
      for (int j = 0; j < kAggBatch; ++j) {
        const int64_t e = eb + j < e1 ? eb + j : e1 - 1;
        x[j]            = ldv<VEC>(pe.edge_feat + e * pe.ef_stride + c);
        z[j]            = dz[e * H + k];
      }
#pragma unroll
      for (int j = 0; j < kAggBatch; ++j) {
        if (eb + j < e1) {
          stv(pe.grad_edge_feat + (eb + j) * pe.grad_ef_stride + c, scaled(av, z[j]));
          add_to(acc, scaled(x[j], z[j]));
        }
      }
    }
    stv(partial + q * HF + c, acc);
  }
}

// grad_att[2, c]: the chunk sums in chunk order; +0.0 when there is no edge
__global__ __launch_bounds__(kAggBlock) void gat_edge_att_fold_kernel(wm_gat_edge_args pe, const float* partial,
                                                                      int64_t n_chunks)
{
  const int64_t HF = pe.g.heads * pe.g.dim;
  for (int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; c < HF;
       c += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float acc = -0.0f;
#pragma unroll 8
    for (int64_t q = 0; q < n_chunks; ++q) acc = acc + partial[q * HF + c];
    pe.g.grad_att[2 * HF + c] = n_chunks > 0 ? acc : 0.0f;
  }
}

int64_t edge_chunks(const wm_gat_args* a) { return (a->n_edges + kGatNodeChunk - 1) / kGatNodeChunk; }

}  // namespace

int hip_gat_edge_forward(const wm_gat_edge_args* ea, void* workspace, void* stream_v)
{
  hipStream_t stream   = static_cast<hipStream_t>(stream_v);
  const wm_gat_args* a = &ea->g;
  const int64_t H = a->heads, F = a->dim, HF = H * F;
  const bool f4   = F % 4 == 0 && aligned16(a->att);
  if (gat_scores(a, stream_v) != 0) return -2;
  if (a->n_dst == 0) return 0;
  if (a->n_edges > 0) {
    const int blocks = blocks_for(a->n_edges * H, kAggBlock);
    if (f4 && use_vec4(HF, ea->edge_feat, ea->ef_stride, ea->edge_feat, ea->ef_stride))
      hipLaunchKernelGGL(gat_edge_score_kernel<4>, dim3(blocks), dim3(kAggBlock), 0, stream, *ea);
    else hipLaunchKernelGGL(gat_edge_score_kernel<1>, dim3(blocks), dim3(kAggBlock), 0, stream, *ea);
    if (rc_last() != 0) return -2;
  }
  float* o         = a->concat ? a->out : ws_at<float>(workspace, 0);   // (the workspace's one region)
  const int64_t os = a->concat ? a->out_stride : HF;
  const bool v4    = f4 && use_vec4(HF, a->h, a->h_stride, o, os);
#define WM_GAT_EDGE_FWD(V, L)                                                                                         \
  hipLaunchKernelGGL((gat_edge_fwd_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *ea, o, os)
  WM_AGG_DISPATCH(v4, v4 ? HF / 4 : HF, WM_GAT_EDGE_FWD);
#undef WM_GAT_EDGE_FWD
  if (rc_last() != 0) return -2;
  if (!a->concat && gat_head_mean(a, o, os, stream_v) != 0) return -2;
  return 0;
}

size_t hip_gat_edge_backward_workspace_bytes(const wm_gat_edge_args* ea)
{
  const wm_gat_args* a = &ea->g;
  return gat_bwd_workspace_bytes(a, edge_chunks(a) * a->heads * a->dim * 4);
}

int hip_gat_edge_backward(const wm_gat_edge_args* ea, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream   = static_cast<hipStream_t>(stream_v);
  const wm_gat_args* a = &ea->g;
  const int64_t HF     = a->heads * a->dim;
  wm_gat_bwd_state b;
  float* epart  = static_cast<float*>(gat_bwd_carve(a, ix, workspace, edge_chunks(a) * HF * 4, &b));   // [chunks, HF]
  const bool f4 = gat_bwd_vec4(a);
  if (a->n_dst > 0) {
    const int blocks = blocks_for(a->n_dst * a->heads, kAggBlock);
    if (f4) hipLaunchKernelGGL(gat_edge_bwd_dz_kernel<4>, dim3(blocks), dim3(kAggBlock), 0, stream, *ea, b);
    else hipLaunchKernelGGL(gat_edge_bwd_dz_kernel<1>, dim3(blocks), dim3(kAggBlock), 0, stream, *ea, b);
    if (rc_last() != 0) return -2;
  }
  if (gat_bwd_after_dz(a, &b, stream_v) != 0) return -2;
  const int64_t nq = edge_chunks(a);
  if (nq > 0) {
    const bool v4 = a->dim % 4 == 0 && aligned16(a->att) &&
                    use_vec4(HF, ea->edge_feat, ea->ef_stride, ea->grad_edge_feat, ea->grad_ef_stride);
    const float* dz = b.dz;
    if (v4)
      hipLaunchKernelGGL(gat_edge_grad_chunk_kernel<4>, dim3(blocks_for(nq * (HF / 4), kAggBlock)), dim3(kAggBlock), 0,
                         stream, *ea, dz, epart, nq);
    else
      hipLaunchKernelGGL(gat_edge_grad_chunk_kernel<1>, dim3(blocks_for(nq * HF, kAggBlock)), dim3(kAggBlock), 0, stream,
                         *ea, dz, epart, nq);
    if (rc_last() != 0) return -2;
  }
  hipLaunchKernelGGL(gat_edge_att_fold_kernel, dim3(blocks_for(HF, kAggBlock)), dim3(kAggBlock), 0, stream, *ea,
                     static_cast<const float*>(epart), nq);
  return rc_last();
}

}  // namespace wm
