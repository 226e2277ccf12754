// wholegraph_amd — the multi-aggregator neighbour aggregation of a sampled CSC block (the `agg_concat_pna` op behind the
// PNAConv layer, wholegraph_amd_ext.h section 2l) on gfx950: sum, mean, min, max and std of each target's neighbour rows out
// of one read of those rows.
//
// Forward (kernels/agg.hip's shape: one group of LANES lanes per target row d, LANES = 16 / 32 / 64 from the row width; the
// column ids of up to LANES edges come with one coalesced load and are handed out with shuffles; the neighbour rows of a
// batch of kAggBatch edges are loaded back to back; for_target_pieces and for_edge_batches of agg_common.cuh): per lane the
// running sum S, the running sum of squares Q, the running minimum and maximum and the edge positions that hold them. Which
// of them are kept is the 5-bit mask of the call: the branches on it are the same for every lane of the grid (one
// instantiation serves every subset). The slots of the selected aggregators follow each other in the order sum, mean, min,
// max, std; the target's own row comes last.
//
// Backward (grad_x[s] for every source row s; no atomics): the walk of kernels/agg.hip (agg_bwd_prepare, then a chunk
// kernel over the tiles of the sorted positions and a fold kernel per source row, both through agg_common.cuh) with this
// op's own per-edge term, pna_fold_edges: up to nine rows of the target per edge (four gradient slots, the two arg rows, the
// std gradient, its mean and its coefficient), kPnaBwdBatch edges in flight. Its loop over the sorted positions is written
// out (one loop over the batch per aggregator part; agg_common.cuh's header has the reason). x[s] is constant over a
// source's run and is loaded once per source (fold) or chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "agg_common.cuh"

namespace wm {
namespace {

constexpr int kPnaBwdBatch = 4;   // edges in flight per lane in the backward (each brings up to nine rows)

// the slot of every aggregator in a row of out / grad_out (in units of dim columns) and the slot of the target's own row
struct pna_slots {
  int sum, mean, min, max, std, self;
};

__host__ __device__ __forceinline__ pna_slots slots_of(int mask)
{
  pna_slots s;
  int n  = 0;
  s.sum  = n, n += (mask & WM_PNA_SUM) ? 1 : 0;
  s.mean = n, n += (mask & WM_PNA_MEAN) ? 1 : 0;
  s.min  = n, n += (mask & WM_PNA_MIN) ? 1 : 0;
  s.max  = n, n += (mask & WM_PNA_MAX) ? 1 : 0;
  s.std  = n, n += (mask & WM_PNA_STD) ? 1 : 0;
  s.self = n;
  return s;
}

template <int VEC>
struct ivec {
  int v[VEC];
};

template <int VEC>
__device__ __forceinline__ ivec<VEC> ldi(const int32_t* p)
{
  ivec<VEC> r;
  if constexpr (VEC == 4) {
    const int4 t = *reinterpret_cast<const int4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = p[i];
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ void sti(int32_t* p, const ivec<VEC>& a)
{
  if constexpr (VEC == 4) {
    *reinterpret_cast<int4*>(p) = make_int4(a.v[0], a.v[1], a.v[2], a.v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = a.v[i];
  }
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void pna_fwd_kernel(wm_pna_args p)
{
  const int gl        = threadIdx.x % LANES;
  const int64_t F     = p.dim;
  const pna_slots sl  = slots_of(p.mask);
  const bool want_std = p.mask & WM_PNA_STD;
  const bool want_s   = p.mask & (WM_PNA_SUM | WM_PNA_MEAN | WM_PNA_STD);
  const bool want_min = p.mask & WM_PNA_MIN;
  const bool want_max = p.mask & WM_PNA_MAX;
  for_target_pieces<VEC, LANES>(p, F, [&](int64_t d, int64_t e0, int64_t e1, int64_t c, int64_t cl, bool act) {
    const int64_t deg = e1 - e0;
    const float r     = deg > 0 ? 1.0f / static_cast<float>(deg) : 0.0f;
    const float* self = p.in + d * p.in_stride;
    float* orow       = p.out + d * p.out_stride;
    fvec<VEC> S = splat<VEC>(-0.0f), Q = splat<VEC>(-0.0f), mn = splat<VEC>(0.0f), mx = splat<VEC>(0.0f);
    ivec<VEC> amin, amax;
#pragma unroll
    for (int i = 0; i < VEC; ++i) amin.v[i] = -1, amax.v[i] = -1;
    int my = 0;
    fvec<VEC> v[kAggBatch];
    for_edge_batches<LANES>(
        e0, e1, gl, [&](int64_t pos, bool in) { my = in ? p.col_ind[pos] : 0; },
        [&](int k, int from, int64_t) {
          const int src = __shfl(my, from, LANES);
          v[k]          = ldv<VEC>(p.in + static_cast<int64_t>(src) * p.in_stride + cl);
        },
        [&](int k, int64_t pos) {
          const int e      = static_cast<int>(pos);
          const bool first = pos == e0;   // the first term is taken as it is (a NaN too)
          if (want_s) add_to(S, v[k]);
          if (want_std) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) Q.v[i] = Q.v[i] + v[k].v[i] * v[k].v[i];
          }
          if (want_min) {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
              if (first || v[k].v[i] < mn.v[i]) mn.v[i] = v[k].v[i], amin.v[i] = e;
          }
          if (want_max) {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
              if (first || v[k].v[i] > mx.v[i]) mx.v[i] = v[k].v[i], amax.v[i] = e;
          }
        });
    if (!act) return;
    const bool any = deg > 0;
    if (p.mask & WM_PNA_SUM) stv(orow + sl.sum * F + c, any ? S : splat<VEC>(0.0f));
    if (p.mask & WM_PNA_MEAN) stv(orow + sl.mean * F + c, any ? scaled(S, r) : splat<VEC>(0.0f));
    if (want_min) {
      stv(orow + sl.min * F + c, mn);
      if (p.arg_min != nullptr) sti(p.arg_min + d * F + c, amin);
    }
    if (want_max) {
      stv(orow + sl.max * F + c, mx);
      if (p.arg_max != nullptr) sti(p.arg_max + d * F + c, amax);
    }
    if (want_std) {
      fvec<VEC> sd = splat<VEC>(0.0f), m = splat<VEC>(0.0f), co = splat<VEC>(0.0f);
      if (any) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          m.v[i]         = S.v[i] * r;
          const float q  = Q.v[i] * r;
          const float va = q - m.v[i] * m.v[i];
          sd.v[i]        = sqrtf((va > 0.0f ? va : 0.0f) + p.eps);
          co.v[i]        = va > 0.0f ? r / sd.v[i] : 0.0f;
        }
      }
      stv(orow + sl.std * F + c, sd);
      if (p.std_mean != nullptr) stv(p.std_mean + d * F + c, m);
      if (p.std_coef != nullptr) stv(p.std_coef + d * F + c, co);
    }
    stv(orow + sl.self * F + c, ldv<VEC>(self + c));
  });
}

// acc += t(e) for the edges at sorted positions [eb0, ee), in that order (LANES lanes, this lane's columns at cl); xs: this
// lane's columns of the source row the positions belong to (read for std only). The parts of t(e) are added in the order
// sum, mean, min, max, std, from the first selected one; a part that is not selected, or whose arg is another edge, is not
// added at all.
template <int VEC, int LANES>
__device__ __forceinline__ void pna_fold_edges(fvec<VEC>& acc, const wm_pna_args& p, const pna_slots& sl,
                                               const csc_bwd_index& b, const fvec<VEC>& xs, int64_t eb0, int64_t ee,
                                               int64_t cl, int gl)
{
  const int64_t F     = p.dim;
  const bool want_sum = p.mask & WM_PNA_SUM, want_mean = p.mask & WM_PNA_MEAN, want_min = p.mask & WM_PNA_MIN;
  const bool want_max = p.mask & WM_PNA_MAX, want_std = p.mask & WM_PNA_STD;
  for (int64_t eb = eb0; eb < ee; eb += LANES) {
    const int nb = static_cast<int>(ee - eb < LANES ? ee - eb : LANES);
    int my_d = 0, my_e = 0;
    float my_r = 1.0f;
    if (gl < nb) {
      my_d = b.sorted_dst[eb + gl];
      my_e = b.order[eb + gl];
      if (want_mean) my_r = 1.0f / static_cast<float>(p.row_ptr[my_d + 1] - p.row_ptr[my_d]);
    }
    for (int j = 0; j < nb; j += kPnaBwdBatch) {
      fvec<VEC> gs[kPnaBwdBatch], gm[kPnaBwdBatch], gn[kPnaBwdBatch], gx[kPnaBwdBatch], gd[kPnaBwdBatch];
      fvec<VEC> sm[kPnaBwdBatch], sc[kPnaBwdBatch];
      ivec<VEC> an[kPnaBwdBatch], ax[kPnaBwdBatch];
      float rs[kPnaBwdBatch];
      int es[kPnaBwdBatch];
      const float* g[kPnaBwdBatch];
      int64_t sv[kPnaBwdBatch];
#pragma unroll
      for (int k = 0; k < kPnaBwdBatch; ++k) {
        const int from  = j + k < nb ? j + k : nb - 1;
        const int64_t d = __shfl(my_d, from, LANES);
        es[k]           = __shfl(my_e, from, LANES);
        rs[k]           = __shfl(my_r, from, LANES);
        g[k]            = p.grad + d * p.grad_stride + cl;
        sv[k]           = d * F + cl;
      }
      // (one loop over the batch per part: the branch on the mask stays outside the row loads of a batch, which then issue
      // back to back)
#define WM_PNA_BATCH(STMT)                    \
  _Pragma("unroll") for (int k = 0; k < kPnaBwdBatch; ++k) { STMT; }
      if (want_sum) WM_PNA_BATCH(gs[k] = ldv<VEC>(g[k] + sl.sum * F))
      if (want_mean) WM_PNA_BATCH(gm[k] = ldv<VEC>(g[k] + sl.mean * F))
      if (want_min) WM_PNA_BATCH(gn[k] = ldv<VEC>(g[k] + sl.min * F); an[k] = ldi<VEC>(p.arg_min + sv[k]))
      if (want_max) WM_PNA_BATCH(gx[k] = ldv<VEC>(g[k] + sl.max * F); ax[k] = ldi<VEC>(p.arg_max + sv[k]))
      if (want_std)
        WM_PNA_BATCH(gd[k] = ldv<VEC>(g[k] + sl.std * F); sm[k] = ldv<VEC>(p.std_mean + sv[k]);
                     sc[k] = ldv<VEC>(p.std_coef + sv[k]))
#undef WM_PNA_BATCH
#pragma unroll
      for (int k = 0; k < kPnaBwdBatch; ++k) {
        if (j + k < nb) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            float t = -0.0f;   // (the identity of the addition: the first part that is added is taken as it is, and
                               // acc + t is acc when no part is)
            if (want_sum) t = t + gs[k].v[i];
            if (want_mean) t = t + gm[k].v[i] * rs[k];
            if (want_min && an[k].v[i] == es[k]) t = t + gn[k].v[i];
            if (want_max && ax[k].v[i] == es[k]) t = t + gx[k].v[i];
            if (want_std) t = t + (gd[k].v[i] * sc[k].v[i]) * (xs.v[i] - sm[k].v[i]);
            acc.v[i] = acc.v[i] + t;
          }
        }
      }
    }
  }
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void pna_bwd_chunk_kernel(wm_pna_args p, wm_agg_bwd_state b)
{
  const int gl       = threadIdx.x % LANES;
  const pna_slots sl = slots_of(p.mask);
  for_chunk_pieces<VEC, LANES>(b, p.dim, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    fvec<VEC> xs = splat<VEC>(0.0f);
    if (p.mask & WM_PNA_STD) {   // (the source of the chunk: the id of any of its edges)
      const int64_t s = p.col_ind[b.order[cs]];
      xs              = ldv<VEC>(p.in + s * p.in_stride + cl);
    }
    fvec<VEC> acc = splat<VEC>(0.0f);   // (every sum of terms starts from +0.0: an edge may add nothing)
    pna_fold_edges<VEC, LANES>(acc, p, sl, b, xs, cs, ce, cl, gl);
    if (act) stv(b.partial + t * b.partial_stride + c, acc);
  });
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void pna_bwd_fold_kernel(wm_pna_args p, wm_agg_bwd_state b)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t F       = p.dim;
  const int64_t nu      = *b.n_unique;
  const pna_slots sl    = slots_of(p.mask);
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; s < p.n_src;
       s += static_cast<int64_t>(gridDim.x) * kGroups) {
    const src_run r = run_of_source(b, nu, s);
    const bool self = s < p.n_dst;
    for (int64_t cb = 0; cb < F; cb += LANES * VEC) {
      const int64_t c  = cb + gl * VEC;
      const bool act   = c < F;
      const int64_t cl = act ? c : 0;
      fvec<VEC> xs     = splat<VEC>(0.0f);
      if ((p.mask & WM_PNA_STD) && r.has) xs = ldv<VEC>(p.in + s * p.in_stride + cl);
      fvec<VEC> acc = splat<VEC>(0.0f);
      pna_fold_edges<VEC, LANES>(acc, p, sl, b, xs, r.s0, r.c0e, cl, gl);
      add_partials(acc, b, r, cl);
      const fvec<VEC> res = with_self_term(acc, r.has, self, p.grad, s * p.grad_stride + sl.self * F + cl);
      if (act) stv(p.out + s * p.out_stride + c, res);
    }
  }
}

bool aligned16(const void* q) { return reinterpret_cast<uintptr_t>(q) % 16 == 0; }   // (a null pointer counts as aligned)

// 16-byte pieces only when the saved rows ([n_dst, dim], dense) allow them as well
bool saved_vec4(const wm_pna_args* a)
{
  return aligned16(a->arg_min) && aligned16(a->arg_max) && aligned16(a->std_mean) && aligned16(a->std_coef);
}

}  // namespace

int hip_pna_forward(const wm_pna_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_dst == 0 || a->dim == 0) return 0;
  const bool v4 = use_vec4(a->dim, a->in, a->in_stride, a->out, a->out_stride) && saved_vec4(a);
#define WM_PNA_FWD(V, L)                                                                                              \
  hipLaunchKernelGGL((pna_fwd_kernel<V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a)
  WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_PNA_FWD);
#undef WM_PNA_FWD
  return rc_last();
}

size_t hip_pna_backward_workspace_bytes(int64_t n_edges, int64_t n_src, int64_t dim)
{
  return agg_bwd_plan(n_edges, n_src, dim, kAggChunkEdges).ws.bytes;
}

int hip_pna_backward(const wm_pna_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_src == 0 || a->dim == 0) return 0;
  wm_agg_bwd_state b;
  if (agg_bwd_prepare(*a, a->dim, ix, workspace, &b, stream_v) != 0) return -2;
  const bool std_rows = (a->mask & WM_PNA_STD) != 0;   // (x is read for std only)
  const bool v4       = use_vec4(a->dim, a->grad, a->grad_stride, a->out, a->out_stride) && saved_vec4(a) &&
                  (!std_rows || (a->in_stride % 4 == 0 && aligned16(a->in)));
  if (b.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_PNA_CHUNK(V, L)                                                                                                   \
  hipLaunchKernelGGL((pna_bwd_chunk_kernel<V, L>), dim3(blocks_for(b.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
    WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_PNA_CHUNK);
#undef WM_PNA_CHUNK
    if (rc_last() != 0) return -2;
  }
#define WM_PNA_FOLD(V, L)                                                                                                   \
  hipLaunchKernelGGL((pna_bwd_fold_kernel<V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, stream, \
                     *a, b)
  WM_AGG_DISPATCH(v4, v4 ? a->dim / 4 : a->dim, WM_PNA_FOLD);
#undef WM_PNA_FOLD
  return rc_last();
}

}  // namespace wm
