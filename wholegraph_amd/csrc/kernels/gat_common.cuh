// wholegraph_amd — what the two attention ops of a sampled CSC block share (kernels/gat.hip, the GAT `mha_gat_n2n` op, and
// kernels/gat_edge.hip, the same op with an edge term in the logit): the scratch of the backward and the stages of gat.hip
// that do not see the logit — the node scores and the mean over heads of the forward, and everything of the backward
// behind dz (wholegraph_amd_ext.h, section 2c). The kernels of those stages live in gat.hip alone.
#pragma once
#include "agg_common.cuh"

namespace wm {

// backward scratch: the id sort's outputs and the op's workspace (gat_bwd_carve)
struct wm_gat_bwd_state {
  const int32_t* order;        // [n_edges] edge positions, sorted by source (stable)
  const int32_t* run_starts;   // [n_unique + 1]
  const int32_t* unique_ids;   // [n_unique] sources with edges, ascending
  const int64_t* n_unique;     // device scalar written by the sort
  int32_t* sorted_dst;         // [n_edges]
  int32_t* run_of;             // [n_src]
  float* dz;                   // [n_edges, heads]: da, then dz
  float* ds_dst;               // [n_dst, heads]
  float* ds_src;               // [n_src, heads]
  float* partial;              // [n_tiles, partial_stride]: P of a chunk (ds_off columns), then its ds_src (heads)
  float* att_partial;          // [n_node_chunks, 2 * heads * dim]
  int64_t n_tiles, partial_stride, ds_off, n_node_chunks;
};

// forward: s_src / s_dst into a->scores
int gat_scores(const wm_gat_args* a, void* stream);
// forward, concat == 0: a->out from the per-head rows o [n_dst, o_stride]
int gat_head_mean(const wm_gat_args* a, const float* o, int64_t o_stride, void* stream);
size_t hip_gat_backward_workspace_bytes(const wm_gat_args* a);
// backward: fills `b` from the id sort's outputs and `workspace` (hip_gat_backward_workspace_bytes); returns the bytes of
// the 256-byte aligned workspace it took (what follows them is the caller's)
size_t gat_bwd_carve(const wm_gat_args* a, const int32_t* order, const int32_t* run_starts, const int32_t* unique_ids,
                     const int64_t* n_unique_dev, void* workspace, wm_gat_bwd_state* b);
// backward behind b->dz and b->ds_dst (steps 2 - 4 of gat.hip): grad_h, ds_src and halves 0 and 1 of grad_att
int gat_bwd_after_dz(const wm_gat_args* a, const wm_gat_bwd_state* b, void* stream);

namespace {

__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.0f ? z : slope * z; }

uintptr_t up256(uintptr_t v) { return (v + 255) & ~static_cast<uintptr_t>(255); }
bool aligned16(const void* ptr) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0; }
// 16-byte pieces in the backward: whole heads of F % 4 == 0 columns, every row start and att 16-byte aligned
bool gat_bwd_vec4(const wm_gat_args* a)
{
  return a->dim % 4 == 0 && aligned16(a->att) &&
         use_vec4(a->concat ? a->heads * a->dim : a->dim, a->grad, a->grad_stride, a->h, a->h_stride);
}

}  // namespace
}  // namespace wm
