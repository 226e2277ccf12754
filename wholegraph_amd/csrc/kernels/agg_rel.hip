// wholegraph_amd — relation-typed neighbour aggregation of a sampled CSC block (`agg_concat_rel`, the aggregation behind
// the RGCN layer) on gfx950: the op of kernels/agg.hip with one int32 type per edge position and one output slot of `dim`
// columns per relation, then the self slot. Semantics and the one order of every sum: wholegraph_amd_ext.h, section (2h).
// Every product is rounded on its own before the add that follows it (-ffp-contract=off: no fused multiply-add). A type
// outside [0, R) contributes nothing anywhere and is never used to form an address.
//
// Forward (relagg_fwd_kernel): a group of LANES lanes per target row, as agg_forward_kernel. Per target the group runs
//   `rounds` of (count, reciprocal, walk):
//   * at most LANES edges (what a sampled block holds): ONE round. Lane i holds edge i; key = its type, or R for a type out
//     of range. Every lane ranks its edge by (key, position) against the others with LANES shuffles, counting the edges of
//     its own key on the way (|E_r(d)|, so fl(1 / |E_r(d)|) is one division per lane and is also edge_scale[e]); the edges
//     are pushed to the lane of their rank (ds_permute). The group then walks the ranks below the number of valid edges in
//     batches of kAggBatch row loads issued back to back — a batch runs across type boundaries, so it is full even when
//     every relation has one edge — and stores the accumulator into its slot whenever the type changes. Slots of relations
//     without an edge are filled with +0.0 afterwards (one ballot per relation).
//   * more than LANES edges: R rounds, one per relation r: the edges of type r are counted over the batches of LANES edge
//     positions (ballot + popcount), then each batch's matching lanes are walked in position order, kAggBatch row loads
//     back to back, and the slot is stored once. Both loops go by ballots, not by consecutive positions, and are written
//     out here (agg_common.cuh's header names them, and fold_edges_rel of the backward).
// Backward (relagg_chunk_bwd_kernel / relagg_fold_bwd_kernel): the per-source sums of kernels/agg_weighted.hip over the same
//   id sort, prep kernel and chunk tiles (agg_bwd_prepare) and with the walk of agg_common.cuh, with w := edge_scale (mean)
//   and the grad_out column offset type * dim per edge (fold_edges_rel); an edge with a type out of range keeps its sorted
//   position and adds nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "agg_common.cuh"

namespace wm {
namespace {

// `pred` over the lanes of this group, bit i = lane i of the group (the groups of a wave may sit in different branches:
// a ballot sees the active lanes only, and the lanes of one group are always active together)
template <int LANES>
__device__ __forceinline__ unsigned long long group_ballot(bool pred, int gl)
{
  const unsigned long long b = __ballot(pred);
  if constexpr (LANES == 64) {
    return b;
  } else {
    return (b >> ((threadIdx.x & 63) - gl)) & ((1ull << LANES) - 1);
  }
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void relagg_fwd_kernel(wm_relagg_args p)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int wbase       = (threadIdx.x & 63) - gl;   // this group's first lane in its wave
  const int64_t F       = p.dim;
  const int R           = static_cast<int>(p.num_relations);
  for (int64_t d = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; d < p.n_dst;
       d += static_cast<int64_t>(gridDim.x) * kGroups) {
    int64_t e0, e1;
    edge_range(p.row_ptr, d, p.n_edges, e0, e1);
    const int64_t deg = e1 - e0;
    const float* self = p.in + d * p.in_stride;
    float* orow       = p.out + d * p.out_stride;
    const bool small  = deg <= LANES;
    const int nb0     = small ? static_cast<int>(deg) : 0;
    // at most LANES edges: lane i holds edge i and ranks it by (key, position); lane k then gets the edge of rank k
    int key = R, s_col = 0, s_key = R, nv = 0, cnt_small = 0, to = 0;
    if (small) {
      int my = 0;
      if (gl < nb0) {
        my          = p.col_ind[e0 + gl];
        const int t = p.edge_type[e0 + gl];
        key         = (t >= 0 && t < R) ? t : R;
      }
      int rank = 0;
      for (int j = 0; j < nb0; ++j) {
        const int kj = __shfl(key, j, LANES);
        rank += (kj < key || (kj == key && j < gl)) ? 1 : 0;
        cnt_small += kj == key ? 1 : 0;
        nv += kj < R ? 1 : 0;
      }
      if (gl >= nb0) rank = gl;   // (lanes without an edge stay where they are: the ranks are a permutation of the group)
      to    = (wbase + rank) * 4;
      s_col = __builtin_amdgcn_ds_permute(to, my);
      s_key = __builtin_amdgcn_ds_permute(to, key);
    }
    const int rounds = small ? 1 : R;
    for (int r = 0; r < rounds; ++r) {
      int cnt_me = cnt_small;   // edges of this lane's relation (small) / of relation r (otherwise)
      if (!small) {
        cnt_me = 0;
        for (int64_t eb = e0; eb < e1; eb += LANES) {
          const bool match = eb + gl < e1 && p.edge_type[eb + gl] == r;
          cnt_me += __popcll(group_ballot<LANES>(match, gl));
        }
      }
      const float sc_me = cnt_me > 0 ? 1.0f / static_cast<float>(cnt_me) : 0.0f;
      if (small) {
        if (p.edge_scale != nullptr && gl < nb0) p.edge_scale[e0 + gl] = key < R ? sc_me : 0.0f;
        const float s_sc = __int_as_float(__builtin_amdgcn_ds_permute(to, __float_as_int(sc_me)));
        for (int64_t cb = 0; cb < F; cb += LANES * VEC) {   // (group-uniform trip count: the shuffles below stay in step)
          const int64_t c  = cb + gl * VEC;
          const bool act   = c < F;
          const int64_t cl = act ? c : 0;
          fvec<VEC> acc    = splat<VEC>(-0.0f);
          int cur          = -1;   // the relation whose sum `acc` holds
          float cur_sc     = 0.0f;
          for (int j = 0; j < nv; j += kAggBatch) {
            fvec<VEC> v[kAggBatch];
            int ty[kAggBatch];
            float scs[kAggBatch];
#pragma unroll
            for (int k = 0; k < kAggBatch; ++k) {
              const int from = j + k < nv ? j + k : nv - 1;
              const int src  = __shfl(s_col, from, LANES);
              ty[k]          = __shfl(s_key, from, LANES);
              scs[k]         = __shfl(s_sc, from, LANES);
              v[k]           = ldv<VEC>(p.in + static_cast<int64_t>(src) * p.in_stride + cl);
            }
#pragma unroll
            for (int k = 0; k < kAggBatch; ++k) {
              if (j + k < nv) {
                if (ty[k] != cur) {   // (ranks below nv hold valid types only: cur is in [0, R))
                  if (cur >= 0 && act) stv(orow + cur * F + c, p.mean ? scaled(acc, cur_sc) : acc);
                  cur    = ty[k];
                  cur_sc = scs[k];
                  acc    = splat<VEC>(-0.0f);
                }
                add_to(acc, v[k]);
              }
            }
          }
          if (cur >= 0 && act) stv(orow + cur * F + c, p.mean ? scaled(acc, cur_sc) : acc);
        }
      } else {
        for (int64_t cb = 0; cb < F; cb += LANES * VEC) {
          const int64_t c  = cb + gl * VEC;
          const bool act   = c < F;
          const int64_t cl = act ? c : 0;
          fvec<VEC> acc    = splat<VEC>(-0.0f);
          for (int64_t eb = e0; eb < e1; eb += LANES) {
            const bool in    = eb + gl < e1;
            const int my     = in ? p.col_ind[eb + gl] : 0;
            const int t      = in ? p.edge_type[eb + gl] : -1;
            const bool match = in && t == r;
            if (cb == 0 && p.edge_scale != nullptr && in) {
              if (match) p.edge_scale[eb + gl] = sc_me;
              else if (r == 0 && !(t >= 0 && t < R)) p.edge_scale[eb + gl] = 0.0f;
            }
            unsigned long long m = group_ballot<LANES>(match, gl);
            int from             = 0;
            while (m != 0) {   // the matching lanes in position order, a batch of their rows in flight
              fvec<VEC> v[kAggBatch];
              int n = 0;
#pragma unroll
              for (int k = 0; k < kAggBatch; ++k) {
                if (m != 0) {
                  from = __ffsll(m) - 1;
                  m &= m - 1;
                  ++n;
                }
                const int src = __shfl(my, from, LANES);
                v[k]          = ldv<VEC>(p.in + static_cast<int64_t>(src) * p.in_stride + cl);
              }
#pragma unroll
              for (int k = 0; k < kAggBatch; ++k)
                if (k < n) add_to(acc, v[k]);
            }
          }
          if (act) stv(orow + r * F + c, cnt_me > 0 ? (p.mean ? scaled(acc, sc_me) : acc) : splat<VEC>(0.0f));
        }
      }
    }
    if (small) {   // +0.0 into the slots of the relations this target has no edge of
      for (int r = 0; r < R; ++r) {
        if (group_ballot<LANES>(key == r, gl) != 0) continue;
        for (int64_t c = gl * VEC; c < F; c += LANES * VEC) stv(orow + r * F + c, splat<VEC>(0.0f));
      }
    }
    for (int64_t c = gl * VEC; c < F; c += LANES * VEC) stv(orow + R * F + c, ldv<VEC>(self + c));
  }
}

// acc += u(order[j]) for the sorted positions j in [eb0, ee), in that order (this lane's columns at cl):
// u(e) = g[dst(e), type(e) * dim + c], times edge_scale[e] first for mean; nothing for a type outside [0, R). Returns whether
// any edge added a term (the same answer in every lane of the group).
template <int VEC, int LANES>
__device__ __forceinline__ bool fold_edges_rel(fvec<VEC>& acc, const wm_relagg_args& p, const wm_agg_bwd_state& b, int64_t eb0,
                                               int64_t ee, int64_t cl, int gl)
{
  const int R = static_cast<int>(p.num_relations);
  bool any    = false;
  for (int64_t eb = eb0; eb < ee; eb += LANES) {   // (written out: on for_edge_batches the fold kernel measured slower)
    const int nb = static_cast<int>(ee - eb < LANES ? ee - eb : LANES);
    int my_d     = 0;
    int my_t     = -1;   // the type, or -1 for one out of range
    float my_w   = 0.0f;
    if (gl < nb) {
      const int64_t e = b.order[eb + gl];
      const int t     = p.edge_type[e];
      my_d            = b.sorted_dst[eb + gl];
      if (t >= 0 && t < R) {
        my_t = t;
        if (p.mean) my_w = p.edge_scale[e];
      }
    }
    for (int j = 0; j < nb; j += kAggBatch) {
      fvec<VEC> v[kAggBatch];
      float ws[kAggBatch];
      bool ok[kAggBatch];
#pragma unroll
      for (int k = 0; k < kAggBatch; ++k) {
        const int from = j + k < nb ? j + k : nb - 1;
        const int d    = __shfl(my_d, from, LANES);
        const int t    = __shfl(my_t, from, LANES);
        ws[k]          = __shfl(my_w, from, LANES);
        ok[k]          = j + k < nb && t >= 0;
        v[k]           = ldv<VEC>(p.grad + static_cast<int64_t>(d) * p.grad_stride + (t >= 0 ? t : 0) * p.dim + cl);
      }
#pragma unroll
      for (int k = 0; k < kAggBatch; ++k)
        if (ok[k]) {
          add_to(acc, p.mean ? scaled(v[k], ws[k]) : v[k]);
          any = true;
        }
    }
  }
  return any;
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void relagg_chunk_bwd_kernel(wm_relagg_args p, wm_agg_bwd_state b)
{
  const int gl = threadIdx.x % LANES;
  for_chunk_pieces<VEC, LANES>(b, p.dim, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    fvec<VEC> acc = splat<VEC>(-0.0f);
    fold_edges_rel<VEC, LANES>(acc, p, b, cs, ce, cl, gl);
    if (act) stv(b.partial + t * b.partial_stride + c, acc);
  });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void relagg_fold_bwd_kernel(wm_relagg_args p, wm_agg_bwd_state b)
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
      bool any         = fold_edges_rel<VEC, LANES>(acc, p, b, r.s0, r.c0e, cl, gl);
      // (a run longer than one chunk whose first chunk added nothing: does any later edge have a type in range?)
      for (int64_t pos = r.c0e; !any && pos < r.s1; pos += LANES) {
        const int t = pos + gl < r.s1 ? p.edge_type[b.order[pos + gl]] : -1;
        any         = group_ballot<LANES>(t >= 0 && t < p.num_relations, gl) != 0;
      }
      add_partials(acc, b, r, cl);
      // (no edge, or none with a type in range: no term at all)
      const fvec<VEC> res = with_self_term(acc, any, self, p.grad, s * p.grad_stride + p.num_relations * F + cl);
      if (act) stv(p.out + s * p.out_stride + c, res);
    }
  }
}

}  // namespace

int hip_relagg_forward(const wm_relagg_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_dst == 0 || a->dim == 0) return 0;
  const bool v4 = use_vec4(a->dim, a->in, a->in_stride, a->out, a->out_stride);
#define WM_RELAGG_FWD(V, L)                                                                                             \
  hipLaunchKernelGGL((relagg_fwd_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a)
  WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_RELAGG_FWD);
#undef WM_RELAGG_FWD
  return rc_last();
}

int hip_relagg_backward(const wm_relagg_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_src == 0 || a->dim == 0) return 0;
  wm_agg_bwd_state b;
  if (agg_bwd_prepare(*a, a->dim, ix, workspace, &b, stream_v) != 0) return -2;
  const bool v4 = use_vec4(a->dim, a->grad, a->grad_stride, a->out, a->out_stride);
  if (b.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_RELAGG_CHUNK(V, L)                                                                                            \
  hipLaunchKernelGGL((relagg_chunk_bwd_kernel<V, L>), dim3(blocks_for(b.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
    WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_RELAGG_CHUNK);
#undef WM_RELAGG_CHUNK
    if (rc_last() != 0) return -2;
  }
#define WM_RELAGG_FOLD(V, L)                                                                                          \
  hipLaunchKernelGGL((relagg_fold_bwd_kernel<V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
  WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_RELAGG_FOLD);
#undef WM_RELAGG_FOLD
  return rc_last();
}

}  // namespace wm
