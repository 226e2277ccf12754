// wholegraph_amd — what the attention ops of a sampled CSC block share. Two of them (kernels/gat.hip, the GAT `mha_gat_n2n`
// op, and kernels/gat_edge.hip, the same op with an edge term in the logit): the scratch of the backward; the stages of gat.hip
// that do not see the logit — the node scores and the mean over heads of the forward, and everything of the backward
// behind dz (wholegraph_amd_ext.h, section 2c), whose kernels live in gat.hip alone; and the bodies of the two stages that
// do see it (gat_fwd_body, gat_bwd_dz_body), with the edge term of section 2f compiled in or out. And what the two ops with
// a dot product per edge and head share (kernels/gatv2.hip, kernels/tconv.hip): the balanced tree of adjacent pairs.
#pragma once
#include <math.h>

#include "agg_common.cuh"

namespace wm {

// backward scratch: the index of the per-source walk and the op's own regions of the workspace (gat_bwd_carve)
struct wm_gat_bwd_state {
  csc_bwd_index ix;            // partial: P of a chunk (ds_off columns), then its ds_src (heads)
  float* dz;                   // [n_edges, heads]: da, then dz
  float* ds_dst;               // [n_dst, heads]
  float* ds_src;               // [n_src, heads]
  float* att_partial;          // [n_node_chunks, 2 * heads * dim]
  int64_t ds_off, n_node_chunks;
};

// forward: s_src / s_dst into a->scores
int gat_scores(const wm_gat_args* a, void* stream);
// forward, concat == 0: a->out from the per-head rows o [n_dst, o_stride]
int gat_head_mean(const wm_gat_args* a, const float* o, int64_t o_stride, void* stream);
// the backward's workspace with a last region of `extra_bytes` for the caller (gat_edge.hip's chunk sums; 0: none)
size_t gat_bwd_workspace_bytes(const wm_gat_args* a, int64_t extra_bytes);
// backward: fills `b` from the edge index and `workspace` (gat_bwd_workspace_bytes with the same extra_bytes); returns the
// caller's region
void* gat_bwd_carve(const wm_gat_args* a, const wm_edge_index& ix, void* workspace, int64_t extra_bytes,
                    wm_gat_bwd_state* b);
// backward behind b->dz and b->ds_dst (steps 2 - 4 of gat.hip): grad_h, ds_src and halves 0 and 1 of grad_att
int gat_bwd_after_dz(const wm_gat_args* a, const wm_gat_bwd_state* b, void* stream);

namespace {

__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.0f ? z : slope * z; }

// the softmax and the weighted sum of a target's neighbour rows (gat.hip, forward): three walks over the target's edges
// (for_edge_batches), the max, den and the rows. EDGE: the logit is (s_src[col[e]] + s_dst[d]) + edge_scores[e, hk],
// edge_scores loaded next to s_src in every batch
template <int VEC, int LANES, bool EDGE>
__device__ __forceinline__ void gat_fwd_body(const wm_gat_args& p, const float* edge_scores, float* o, int64_t o_stride)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t H = p.heads, F = p.dim, HF = H * F;
  const float* s_src = p.scores;
  for_target_pieces<VEC, LANES>(p, HF, [&](int64_t d, int64_t e0, int64_t e1, int64_t c, int64_t cl, bool act) {
    const int64_t hk  = cl / F;   // (a piece never straddles two heads: VEC = 4 only when F % 4 == 0)
    const bool writer = act && c == hk * F;
    const float sd    = s_src[(p.n_src + d) * H + hk];
    float m = -INFINITY, den = -0.0f;
    int my = 0;
    fvec<VEC> v[kAggBatch];
    float s[kAggBatch], se[kAggBatch];
    const auto fetch = [&](int64_t e, bool in) { my = in ? p.col_ind[e] : 0; };
    const auto z_of  = [&](int k) {
      float z = s[k] + sd;
      if constexpr (EDGE) z = z + se[k];
      return z;
    };
    for (int pass = 0; pass < 2; ++pass) {   // 0: the max of l, 1: den = sum of expf(l - max), left to right
      for_edge_batches<LANES>(
          e0, e1, gl, fetch,
          [&](int k, int from, int64_t e) {
            const int src = __shfl(my, from, LANES);
            s[k]          = s_src[static_cast<int64_t>(src) * H + hk];
            if constexpr (EDGE) se[k] = edge_scores[e * H + hk];
          },
          [&](int k, int64_t) {
            const float l = leaky(z_of(k), p.slope);
            if (pass == 0) m = fmaxf(m, l);
            else den = den + expf(l - m);
          });
    }
    fvec<VEC> acc = splat<VEC>(-0.0f);
    for_edge_batches<LANES>(
        e0, e1, gl, fetch,
        [&](int k, int from, int64_t e) {
          const int src = __shfl(my, from, LANES);
          v[k]          = ldv<VEC>(p.h + static_cast<int64_t>(src) * p.h_stride + cl);
          s[k]          = s_src[static_cast<int64_t>(src) * H + hk];
          if constexpr (EDGE) se[k] = edge_scores[e * H + hk];
        },
        [&](int k, int64_t e) {
          const float a = expf(leaky(z_of(k), p.slope) - m) / den;
          add_to(acc, scaled(v[k], a));
          if (writer) p.alpha[e * H + hk] = a;
        });
    if (act) stv(o + d * o_stride + c, e1 > e0 ? acc : splat<VEC>(0.0f));
  });
}

// one thread per (target d, head k): da[e] = G_k[d] . h[col[e], k] (into dz), c = sum of alpha * da, then dz and ds_dst;
// EDGE: the recomputed z has the edge term of gat_fwd_body
template <int VEC, bool EDGE>
__device__ __forceinline__ void gat_bwd_dz_body(const wm_gat_args& p, const float* edge_scores, const wm_gat_bwd_state& b)
{
  const int64_t H = p.heads, F = p.dim, n = p.n_dst * H;
  const float r   = 1.0f / static_cast<float>(H);
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t d = i / H, k = i - d * H;
    int64_t e0, e1;
    edge_range(p.row_ptr, d, p.n_edges, e0, e1);
    const float* g = p.grad + d * p.grad_stride + (p.concat ? k * F : 0);
    float c        = -0.0f;
    for (int64_t e = e0; e < e1; ++e) {
      const float* x = p.h + static_cast<int64_t>(p.col_ind[e]) * p.h_stride + k * F;
      float da       = -0.0f;
#pragma unroll 4
      for (int64_t f = 0; f < F; f += VEC) {
        const fvec<VEC> gv = ldv<VEC>(g + f), xv = ldv<VEC>(x + f);
#pragma unroll
        for (int q = 0; q < VEC; ++q) da = da + (p.concat ? gv.v[q] : gv.v[q] * r) * xv.v[q];
      }
      b.dz[e * H + k] = da;
      c               = c + p.alpha[e * H + k] * da;
    }
    const float sd = p.scores[(p.n_src + d) * H + k];
    float dd       = -0.0f;
    for (int64_t e = e0; e < e1; ++e) {
      float z = p.scores[static_cast<int64_t>(p.col_ind[e]) * H + k] + sd;
      if constexpr (EDGE) z = z + edge_scores[e * H + k];
      const float dl = p.alpha[e * H + k] * (b.dz[e * H + k] - c);
      const float dz = z > 0.0f ? dl : dl * p.slope;
      b.dz[e * H + k] = dz;
      dd              = dd + dz;
    }
    b.ds_dst[i] = e1 > e0 ? dd : 0.0f;
  }
}

// ---- the per-edge, per-head dot product of kernels/gatv2.hip and kernels/tconv.hip: the "tree sum over f" of
// wholegraph_amd_ext.h, sections 2g and 2k, in its two implementations that give the same bits ----

// the balanced tree of adjacent pairs over a stream of terms: push() them in order, 2^levels of them in all
struct pair_tree {
  static constexpr int kLevels = 31;
  float st[kLevels];
  float top;
  __device__ __forceinline__ void push(float q, uint32_t f)
  {
    bool carry = true;
#pragma unroll
    for (int lvl = 0; lvl < kLevels; ++lvl) {
      if (carry) {
        if ((f >> lvl) & 1u) {
          q = st[lvl] + q;
        } else {
          st[lvl] = q;
          carry   = false;
        }
      }
    }
    top = q;   // (after the last term of 2^levels: the root)
  }
};

__device__ __forceinline__ uint32_t pow2_at_least(int64_t f)
{
  uint32_t p = 1;
  while (p < f) p <<= 1;
  return p;
}

// the tree over the F = 4 * lh columns of a head from the 4 products of each of its lh lanes
template <int LANES>
__device__ __forceinline__ float head_tree(const fvec<4>& q, int lh)
{
  float s = (q.v[0] + q.v[1]) + (q.v[2] + q.v[3]);
  for (int w = 1; w < lh; w <<= 1) s = s + __shfl_xor(s, w, LANES);
  return s;
}

bool aligned16(const void* ptr) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0; }
bool row16(const void* ptr, int64_t stride) { return aligned16(ptr) && stride % 4 == 0; }
// 16-byte pieces in the backward: whole heads of F % 4 == 0 columns, every row start and att 16-byte aligned
bool gat_bwd_vec4(const wm_gat_args* a)
{
  return a->dim % 4 == 0 && aligned16(a->att) &&
         use_vec4(a->concat ? a->heads * a->dim : a->dim, a->grad, a->grad_stride, a->h, a->h_stride);
}

}  // namespace
}  // namespace wm
