// wholegraph_amd — the relation-typed score of every edge of a sampled CSC block (the `kge_score_n2n` op: the decoder of the
// knowledge-graph embedding models TransE, DistMult, ComplEx and RotatE) on gfx950. The semantics and the one order of every
// fp32 sum: wholegraph_amd_ext.h, section 2u. An edge has a head row h, a tail row t (the target's row of x_dst and the
// source's row of x_src, or the other way round with head_src) and the row r of its relation. Every model is a compose step
// u = h (*, +, complex *) r and a measure step against t (dot, l1, l2) whose terms, one per column — per complex column for
// the models that read a row as [re | im] — go through the balanced tree of adjacent pairs of gat_common.cuh. One body per
// kernel, templated on (compose, measure, VEC, LANES); the five models are five (compose, measure) pairs.
//
// A lane's piece of a row (krow): VEC adjacent columns, and for the complex models the VEC columns of the imaginary half that
// belong to the same complex columns (a second load, D = dim / 2 floats further), so that the complex product needs no lane
// exchange.
//
// Forward, kge_fwd_kernel: one group of LANES lanes per target d; the tree has the two implementations of edot.hip:
//   * VEC = 4 (the number of terms a power of two in [4, 256], every row 16-byte aligned): the target's piece stays in
//     registers over the edge loop; col_ind and edge_type of up to LANES edges are fetched by one lane each and shuffled round;
//     the far rows of a batch of kAggBatch edges are loaded back to back, the relation rows behind them; the lanes of the row
//     combine with xor exchanges (head_tree); lane 0 applies `-` / sqrt and stores score[e];
//   * VEC = 1, everything else: a lane takes every LANES-th edge of the target and pushes the terms through pair_tree.
//
// Backward (no atomics; one fixed order of every sum). u is recomputed, the l2 models read n = -score[e] once per edge. One
// walk, fold_kge_edges, serves the three sums; what differs is whose row stays in registers (SIDE) and which of dh, dt, dr is
// added:
//   1 kge_bwd_dst_kernel, a lane group per target: the per-target rows, left to right in edge order.
//   2 the library's id sort of col_ind (host), agg_bwd_prepare, then kge_bwd_chunk_kernel / kge_bwd_fold_kernel<.., kSideSrc>:
//     the per-source rows out of the walk of agg_common.cuh. The source's own row stays in registers over a chunk.
//   3 the same two kernels with kSideRel over a second index, the id sort of edge_type with key bound num_relations (a type
//     outside the range is in no run): grad_rel. The relation's row stays in registers; a relation's run is typically many
//     chunks long, the chunk tiles run side by side and the fold adds their partial rows in chunk order.
//   16-byte pieces whenever the piece width (dim, or dim / 2 complex columns) is a multiple of 4 and the rows are aligned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../backend.hpp"
#include "gat_common.cuh"

namespace wm {
namespace {

enum { kMul = 0, kAdd = 1, kCmul = 2 };               // compose
enum { kDot = 0, kL1 = 1, kL2 = 2 };                  // measure
enum { kSideSrc = 0, kSideRel = 1, kSideDst = 2 };    // whose row a backward walk keeps in registers

// a lane's piece of a row: columns [c, c + VEC), and with kCmul the imaginary columns [D + c, D + c + VEC) in b
template <int VEC>
struct krow {
  fvec<VEC> a, b;
};

template <int CMP, int VEC>
__device__ __forceinline__ krow<VEC> ld_row(const float* row, int64_t c, int64_t D)
{
  krow<VEC> r;
  r.a = ldv<VEC>(row + c);
  r.b = r.a;
  if constexpr (CMP == kCmul) r.b = ldv<VEC>(row + D + c);
  return r;
}

template <int CMP, int VEC>
__device__ __forceinline__ void st_row(float* row, int64_t c, int64_t D, const krow<VEC>& r)
{
  stv(row + c, r.a);
  if constexpr (CMP == kCmul) stv(row + D + c, r.b);
}

template <int VEC>
__device__ __forceinline__ krow<VEC> pick(bool first, const krow<VEC>& x, const krow<VEC>& y)
{
  krow<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.a.v[i] = first ? x.a.v[i] : y.a.v[i], r.b.v[i] = first ? x.b.v[i] : y.b.v[i];
  return r;
}

template <int CMP, int VEC>
__device__ __forceinline__ krow<VEC> compose(const krow<VEC>& h, const krow<VEC>& r)
{
  krow<VEC> u;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if constexpr (CMP == kMul) u.a.v[i] = h.a.v[i] * r.a.v[i];
    if constexpr (CMP == kAdd) u.a.v[i] = h.a.v[i] + r.a.v[i];
    u.b.v[i] = u.a.v[i];
    if constexpr (CMP == kCmul) {
      u.a.v[i] = h.a.v[i] * r.a.v[i] - h.b.v[i] * r.b.v[i];
      u.b.v[i] = h.a.v[i] * r.b.v[i] + h.b.v[i] * r.a.v[i];
    }
  }
  return u;
}

// the terms of the measure step, one per (complex) column of the piece
template <int CMP, int MEA, int VEC>
__device__ __forceinline__ fvec<VEC> edge_terms(const krow<VEC>& h, const krow<VEC>& r, const krow<VEC>& t)
{
  const krow<VEC> u = compose<CMP>(h, r);
  fvec<VEC> q;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if constexpr (MEA == kDot) {
      q.v[i] = u.a.v[i] * t.a.v[i];
      if constexpr (CMP == kCmul) q.v[i] = q.v[i] + u.b.v[i] * t.b.v[i];
    } else {
      const float da = u.a.v[i] - t.a.v[i], db = u.b.v[i] - t.b.v[i];
      q.v[i] = MEA == kL1 ? fabsf(da) : da * da;
      if constexpr (CMP == kCmul) q.v[i] = q.v[i] + (MEA == kL1 ? fabsf(db) : db * db);
    }
  }
  return q;
}

// the score from the root of the tree
template <int MEA>
__device__ __forceinline__ float finish(float s)
{
  if constexpr (MEA == kDot) return s;
  if constexpr (MEA == kL1) return -s;
  return -sqrtf(s);
}

// (du, dt) of one component from the upstream g, u, t and, for l2, n
template <int MEA>
__device__ __forceinline__ void measure_grad(float g, float n, float u, float t, float& du, float& dt)
{
  if constexpr (MEA == kDot) {
    du = g * t, dt = g * u;
  } else {
    const float d = u - t;
    float q;
    if constexpr (MEA == kL1) q = g * (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
    else q = n == 0.0f ? 0.0f : g * (d / n);
    du = -q, dt = q;
  }
}

// the gradients of one edge's score with respect to this lane's pieces of h, t and r
template <int CMP, int MEA, int VEC>
__device__ __forceinline__ void edge_grads(const krow<VEC>& h, const krow<VEC>& r, const krow<VEC>& t, float g, float n,
                                           krow<VEC>& dh, krow<VEC>& dt, krow<VEC>& dr)
{
  const krow<VEC> u = compose<CMP>(h, r);
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    float dua, dub = 0.0f;
    measure_grad<MEA>(g, n, u.a.v[i], t.a.v[i], dua, dt.a.v[i]);
    dt.b.v[i] = dt.a.v[i];
    if constexpr (CMP == kCmul) measure_grad<MEA>(g, n, u.b.v[i], t.b.v[i], dub, dt.b.v[i]);
    if constexpr (CMP == kMul) dh.a.v[i] = dua * r.a.v[i], dr.a.v[i] = dua * h.a.v[i];
    if constexpr (CMP == kAdd) dh.a.v[i] = dua, dr.a.v[i] = dua;
    dh.b.v[i] = dh.a.v[i], dr.b.v[i] = dr.a.v[i];
    if constexpr (CMP == kCmul) {
      dh.a.v[i] = dua * r.a.v[i] + dub * r.b.v[i];
      dh.b.v[i] = dub * r.a.v[i] - dua * r.b.v[i];
      dr.a.v[i] = dua * h.a.v[i] + dub * h.b.v[i];
      dr.b.v[i] = dub * h.a.v[i] - dua * h.b.v[i];
    }
  }
}

__device__ __forceinline__ int type_or_minus_one(const wm_kge_args& p, int64_t e)
{
  const int ty = p.edge_type[e];
  return ty >= 0 && ty < p.num_relations ? ty : -1;
}

template <int CMP, int MEA, int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void kge_fwd_kernel(wm_kge_args p)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t D       = p.dim / 2;
  const int64_t T       = CMP == kCmul ? D : p.dim;   // terms of the tree
  const bool hs         = p.head_src != 0;
  for (int64_t d = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; d < p.n_dst;
       d += static_cast<int64_t>(gridDim.x) * kGroups) {
    int64_t e0, e1;
    edge_range(p.row_ptr, d, p.n_edges, e0, e1);
    if constexpr (VEC == 4) {   // the row lies within the group: T / 4 <= LANES
      const int lh        = static_cast<int>(T / 4);
      const int64_t cl    = gl < lh ? gl * 4 : 0;
      const krow<4> xd    = ld_row<CMP, 4>(p.x_dst + d * p.x_dst_stride, cl, D);
      int my = 0, my_t = 0;
      krow<4> v[kAggBatch], r[kAggBatch];
      bool ok[kAggBatch];
      for_edge_batches<LANES>(
          e0, e1, gl,
          [&](int64_t e, bool in) {
            my = 0, my_t = 0;
            if (in) my = p.col_ind[e], my_t = type_or_minus_one(p, e);
          },
          [&](int k, int from, int64_t) {
            const int src = __shfl(my, from, LANES), ty = __shfl(my_t, from, LANES);
            ok[k]         = ty >= 0;
            v[k]          = ld_row<CMP, 4>(p.x_src + static_cast<int64_t>(src) * p.x_src_stride, cl, D);
            r[k]          = ld_row<CMP, 4>(p.rel + static_cast<int64_t>(ok[k] ? ty : 0) * p.rel_stride, cl, D);
          },
          [&](int k, int64_t e) {
            const fvec<4> q = edge_terms<CMP, MEA>(pick(hs, v[k], xd), r[k], pick(hs, xd, v[k]));
            const float s   = head_tree<LANES>(q, lh);
            if (gl == 0) p.score[e] = ok[k] ? finish<MEA>(s) : 0.0f;
          });
    } else {
      const uint32_t Tp = pow2_at_least(T);
      const float* y    = p.x_dst + d * p.x_dst_stride;
      for (int64_t e = e0 + gl; e < e1; e += LANES) {
        const float* x = p.x_src + static_cast<int64_t>(p.col_ind[e]) * p.x_src_stride;
        const int ty   = type_or_minus_one(p, e);
        const float* w = p.rel + static_cast<int64_t>(ty >= 0 ? ty : 0) * p.rel_stride;
        pair_tree t;
        t.top = 0.0f;
        for (uint32_t f = 0; f < Tp; ++f) {
          float q = 0.0f;
          if (f < T) {
            const krow<1> xs = ld_row<CMP, 1>(x, f, D), xt = ld_row<CMP, 1>(y, f, D);
            q                = edge_terms<CMP, MEA>(pick(hs, xs, xt), ld_row<CMP, 1>(w, f, D), pick(hs, xt, xs)).v[0];
          }
          t.push(q, f);
        }
        p.score[e] = ty >= 0 ? finish<MEA>(t.top) : 0.0f;
      }
    }
  }
}

// acc += this side's gradient term of the positions [i0, i1), in that order (this lane's piece at cl). `own` is the row the
// walk keeps in registers: SIDE kSideDst, the target's row, the positions are edge positions; kSideSrc, the source's row, and
// kSideRel, the relation's row, the positions are sorted positions of `b`. The term of an edge whose type is out of range is
// +0.0.
template <int CMP, int MEA, int VEC, int LANES, int SIDE>
__device__ __forceinline__ void fold_kge_edges(krow<VEC>& acc, const wm_kge_args& p, const csc_bwd_index& b,
                                               const krow<VEC>& own, int64_t i0, int64_t i1, int64_t cl, int gl)
{
  const int64_t D = p.dim / 2;
  const bool hs   = p.head_src != 0;
  int my_a = 0, my_b = 0;   // the rows of the two far sides: (target, type), (target, source) or (source, type)
  float my_g = 0.0f, my_n = 0.0f;
  krow<VEC> va[kAggBatch], vb[kAggBatch];
  float g[kAggBatch], n[kAggBatch];
  bool ok[kAggBatch];
  for_edge_batches<LANES>(
      i0, i1, gl,
      [&](int64_t i, bool in) {
        my_a = 0, my_b = 0, my_g = 0.0f, my_n = 0.0f;
        if (in) {
          int64_t e = i;
          if constexpr (SIDE == kSideDst) my_a = p.col_ind[e];
          else e = b.order[i], my_a = b.sorted_dst[i];
          if constexpr (SIDE == kSideRel) my_b = p.col_ind[e];
          else my_b = type_or_minus_one(p, e);
          my_g = p.grad[e];
          if constexpr (MEA == kL2) my_n = -p.score[e];
        }
      },
      [&](int k, int from, int64_t) {
        const int ia = __shfl(my_a, from, LANES), ib = __shfl(my_b, from, LANES);
        g[k]         = __shfl(my_g, from, LANES);
        n[k]         = 0.0f;
        if constexpr (MEA == kL2) n[k] = __shfl(my_n, from, LANES);
        ok[k]            = ib >= 0;
        const int64_t ja = ia, jb = ok[k] ? ib : 0;
        const float* ra  = SIDE == kSideDst ? p.x_src + ja * p.x_src_stride : p.x_dst + ja * p.x_dst_stride;
        const float* rb  = SIDE == kSideRel ? p.x_src + jb * p.x_src_stride : p.rel + jb * p.rel_stride;
        va[k]            = ld_row<CMP, VEC>(ra, cl, D);
        vb[k]            = ld_row<CMP, VEC>(rb, cl, D);
      },
      [&](int k, int64_t) {
        const krow<VEC>& xd = SIDE == kSideDst ? own : va[k];
        const krow<VEC>& xs = SIDE == kSideDst ? va[k] : (SIDE == kSideSrc ? own : vb[k]);
        const krow<VEC>& r  = SIDE == kSideRel ? own : vb[k];
        krow<VEC> dh, dt, dr;
        edge_grads<CMP, MEA>(pick(hs, xs, xd), r, pick(hs, xd, xs), g[k], n[k], dh, dt, dr);
        const krow<VEC> mine = SIDE == kSideRel ? dr : pick(hs == (SIDE == kSideSrc), dh, dt);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          acc.a.v[i] = acc.a.v[i] + (ok[k] ? mine.a.v[i] : 0.0f);
          if constexpr (CMP == kCmul) acc.b.v[i] = acc.b.v[i] + (ok[k] ? mine.b.v[i] : 0.0f);
        }
      });
}

template <int VEC>
__device__ __forceinline__ krow<VEC> krow_of(float s)
{
  krow<VEC> r;
  r.a = splat<VEC>(s), r.b = splat<VEC>(s);
  return r;
}

template <int CMP, int MEA, int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void kge_bwd_dst_kernel(wm_kge_args p)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t D = p.dim / 2;
  for_target_pieces<VEC, LANES>(p, CMP == kCmul ? D : p.dim,
                                [&](int64_t d, int64_t e0, int64_t e1, int64_t c, int64_t cl, bool act) {
    const krow<VEC> own = ld_row<CMP, VEC>(p.x_dst + d * p.x_dst_stride, cl, D);
    krow<VEC> acc       = krow_of<VEC>(-0.0f);
    fold_kge_edges<CMP, MEA, VEC, LANES, kSideDst>(acc, p, csc_bwd_index{}, own, e0, e1, cl, gl);
    if (act) st_row<CMP>(p.grad_dst + d * p.grad_dst_stride, c, D, e1 > e0 ? acc : krow_of<VEC>(0.0f));
  });
}

// the rows a per-key walk reads its own row from and writes its sum to
template <int SIDE>
__device__ __forceinline__ const float* key_row(const wm_kge_args& p, int64_t key)
{
  return SIDE == kSideRel ? p.rel + key * p.rel_stride : p.x_src + key * p.x_src_stride;
}

template <int CMP, int MEA, int VEC, int LANES, int SIDE>
__global__ __launch_bounds__(kAggBlock) void kge_bwd_chunk_kernel(wm_kge_args p, csc_bwd_index b)
{
  const int gl    = threadIdx.x % LANES;
  const int64_t D = p.dim / 2;
  for_chunk_pieces<VEC, LANES>(b, CMP == kCmul ? D : p.dim,
                               [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    const int64_t e     = b.order[cs];   // (in a run: its key is in range)
    const int64_t key   = SIDE == kSideRel ? p.edge_type[e] : p.col_ind[e];
    const krow<VEC> own = ld_row<CMP, VEC>(key_row<SIDE>(p, key), cl, D);
    krow<VEC> acc       = krow_of<VEC>(-0.0f);
    fold_kge_edges<CMP, MEA, VEC, LANES, SIDE>(acc, p, b, own, cs, ce, cl, gl);
    if (act) st_row<CMP>(b.partial + t * b.partial_stride, c, D, acc);
  });
}

template <int CMP, int MEA, int VEC, int LANES, int SIDE>
__global__ __launch_bounds__(kAggBlock) void kge_bwd_fold_kernel(wm_kge_args p, csc_bwd_index b)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t D       = p.dim / 2;
  const int64_t W       = CMP == kCmul ? D : p.dim;
  const int64_t n_keys  = SIDE == kSideRel ? p.num_relations : p.n_src;
  float* out            = SIDE == kSideRel ? p.grad_rel : p.grad_src;
  const int64_t stride  = SIDE == kSideRel ? p.grad_rel_stride : p.grad_src_stride;
  const int64_t nu      = *b.n_unique;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; s < n_keys;
       s += static_cast<int64_t>(gridDim.x) * kGroups) {
    const src_run r = run_of_source(b, nu, s);
    for (int64_t cb = 0; cb < W; cb += LANES * VEC) {
      const int64_t c     = cb + gl * VEC;
      const bool act      = c < W;
      const int64_t cl    = act ? c : 0;
      const krow<VEC> own = ld_row<CMP, VEC>(key_row<SIDE>(p, s), cl, D);
      krow<VEC> acc       = krow_of<VEC>(-0.0f);
      fold_kge_edges<CMP, MEA, VEC, LANES, SIDE>(acc, p, b, own, r.s0, r.c0e, cl, gl);
      add_partials(acc.a, b, r, cl);
      if constexpr (CMP == kCmul) add_partials(acc.b, b, r, D + cl);
      if (act) st_row<CMP>(out + s * stride, c, D, r.has ? acc : krow_of<VEC>(0.0f));
    }
  }
}

template <int C, int M>
struct kge_model {
  static constexpr int cmp = C, mea = M;
};

// f(kge_model<compose, measure>) of the model
template <class F>
int by_model(int model, F f)
{
  switch (model) {
    case WM_KGE_DISTMULT: return f(kge_model<kMul, kDot>());
    case WM_KGE_TRANSE_L1: return f(kge_model<kAdd, kL1>());
    case WM_KGE_TRANSE_L2: return f(kge_model<kAdd, kL2>());
    case WM_KGE_COMPLEX: return f(kge_model<kCmul, kDot>());
    case WM_KGE_ROTATE: return f(kge_model<kCmul, kL2>());
    default: return -1;
  }
}

bool is_complex(const wm_kge_args* a) { return a->model == WM_KGE_COMPLEX || a->model == WM_KGE_ROTATE; }
// the width a lane group splits: columns, or complex columns
int64_t piece_width(const wm_kge_args* a) { return is_complex(a) ? a->dim / 2 : a->dim; }
bool inputs16(const wm_kge_args* a)
{
  return row16(a->x_src, a->x_src_stride) && row16(a->x_dst, a->x_dst_stride) && row16(a->rel, a->rel_stride);
}
// the lane-split tree: the terms a power of two in [4, 256] (for the complex models the imaginary half then starts on a
// 16-byte boundary too)
bool fwd_vec4(const wm_kge_args* a)
{
  const int64_t T = piece_width(a);
  return T >= 4 && T <= 256 && (T & (T - 1)) == 0 && inputs16(a);
}
bool bwd_vec4(const wm_kge_args* a, const float* out, int64_t out_stride)
{
  return piece_width(a) % 4 == 0 && inputs16(a) && row16(out, out_stride);
}

template <class M>
int launch_fwd(const wm_kge_args* a, hipStream_t stream)
{
  const bool v4 = fwd_vec4(a);
#define WM_KGE_FWD(V, L)                                                                                                   \
  hipLaunchKernelGGL((kge_fwd_kernel<M::cmp, M::mea, V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a)
  WM_AGG_DISPATCH(v4, v4 ? piece_width(a) / 4 : piece_width(a), WM_KGE_FWD);
#undef WM_KGE_FWD
  return rc_last();
}

template <class M>
int launch_bwd_dst(const wm_kge_args* a, hipStream_t stream)
{
  const bool v4 = bwd_vec4(a, a->grad_dst, a->grad_dst_stride);
#define WM_KGE_DST(V, L)                                                                                                  \
  hipLaunchKernelGGL((kge_bwd_dst_kernel<M::cmp, M::mea, V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), \
                     0, stream, *a)
  WM_AGG_DISPATCH(v4, v4 ? piece_width(a) / 4 : piece_width(a), WM_KGE_DST);
#undef WM_KGE_DST
  return rc_last();
}

// the chunk and fold kernels of one keyed sum over its index `b`
template <class M, int SIDE>
int launch_bwd_keyed(const wm_kge_args* a, const csc_bwd_index& b, hipStream_t stream)
{
  const bool rel       = SIDE == kSideRel;
  const bool v4        = bwd_vec4(a, rel ? a->grad_rel : a->grad_src, rel ? a->grad_rel_stride : a->grad_src_stride);
  const int64_t pieces = v4 ? piece_width(a) / 4 : piece_width(a);
  if (b.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_KGE_CHUNK(V, L)                                                                                             \
  hipLaunchKernelGGL((kge_bwd_chunk_kernel<M::cmp, M::mea, V, L, SIDE>), dim3(blocks_for(b.n_tiles, kAggBlock / (L))), \
                     dim3(kAggBlock), 0, stream, *a, b)
    WM_AGG_DISPATCH(v4, pieces, WM_KGE_CHUNK);
#undef WM_KGE_CHUNK
    if (rc_last() != 0) return -2;
  }
  const int64_t n_keys = rel ? a->num_relations : a->n_src;
#define WM_KGE_FOLD(V, L)                                                                                          \
  hipLaunchKernelGGL((kge_bwd_fold_kernel<M::cmp, M::mea, V, L, SIDE>), dim3(blocks_for(n_keys, kAggBlock / (L))), \
                     dim3(kAggBlock), 0, stream, *a, b)
  WM_AGG_DISPATCH(v4, pieces, WM_KGE_FOLD);
#undef WM_KGE_FOLD
  return rc_last();
}

bool wants_src(const wm_kge_args* a) { return a->grad_src != nullptr && a->n_src > 0; }
bool wants_rel(const wm_kge_args* a) { return a->grad_rel != nullptr && a->num_relations > 0; }
// the workspace of one keyed walk: sorted_dst, run_of and the partial rows (ws_plan lays them out); regions of no size when
// the sum is not asked for
agg_bwd_layout keyed_plan(const wm_kge_args* a, bool wanted, int64_t n_keys)
{
  return agg_bwd_plan(wanted ? a->n_edges : 0, wanted ? n_keys : 0, a->dim, kAggChunkEdges);
}

}  // namespace

int hip_kge_forward(const wm_kge_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->n_dst == 0 || a->n_edges == 0) return 0;
  return by_model(a->model, [&](auto m) { return launch_fwd<decltype(m)>(a, stream); });
}

// the per-source walk's workspace, then the per-relation walk's behind it
size_t hip_kge_backward_workspace_bytes(const wm_kge_args* a)
{
  return keyed_plan(a, wants_src(a), a->n_src).ws.bytes + keyed_plan(a, wants_rel(a), a->num_relations).ws.bytes;
}

int hip_kge_backward(const wm_kge_args* a, const wm_edge_index& ix, const wm_edge_index& rel_ix, void* workspace,
                     void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->grad_dst != nullptr && a->n_dst > 0) {
    if (by_model(a->model, [&](auto m) { return launch_bwd_dst<decltype(m)>(a, stream); }) != 0) return -2;
  }
  if (wants_src(a)) {
    csc_bwd_index b;
    if (agg_bwd_prepare(*a, a->dim, ix, workspace, &b, stream_v) != 0) return -2;
    if (by_model(a->model, [&](auto m) { return launch_bwd_keyed<decltype(m), kSideSrc>(a, b, stream); }) != 0) return -2;
  }
  if (wants_rel(a)) {
    wm_csc_block keyed = *a;   // the walk's "sources" are the relations
    keyed.n_src        = a->num_relations;
    char* ws_rel       = ws_at<char>(workspace, keyed_plan(a, wants_src(a), a->n_src).ws.bytes - 256);
    csc_bwd_index b;
    if (agg_bwd_prepare(keyed, a->dim, rel_ix, ws_rel, &b, stream_v) != 0) return -2;
    if (by_model(a->model, [&](auto m) { return launch_bwd_keyed<decltype(m), kSideRel>(a, b, stream); }) != 0) return -2;
  }
  return 0;
}

}  // namespace wm
