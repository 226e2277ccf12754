// wholegraph_amd — the GraphSAGE `agg_concat` op (kernels/agg.hip) on rows of 16-bit floats, fp16 or bf16, on gfx950.
//
// x, out, grad_out and grad_x all hold T. Every sum is the fp32 sum of kernels/agg.hip, term by term in the same order
// (widening T -> fp32 is exact), and each output element is rounded to T once, to nearest even, at the store: the running
// sum never lives in T. So op_T(x) == round_T(op_fp32(fp32(x))) bit for bit, forward and backward. Rows that are only
// copied (the target's own row of the forward, a self term without edges in the backward) keep their bits.
//
// Same structure as the fp32 kernels: one group of 16 / 32 / 64 lanes per row, sized from the row's 16-byte pieces (a
// piece is 8 elements here: F = 128 is 16 pieces) or, on the element-wise path, from its elements; column ids loaded
// coalesced and handed out with shuffles; the rows of a batch of kAggBatch edges issued back to back as raw pieces and
// widened when they are added (the walk of agg_common.cuh: for_target_pieces, for_edge_batches). The edge index,
// agg_bwd_prep_kernel and the fp32 partial rows of chunks are those of kernels/agg.hip (agg_bwd_prepare); the walk over
// them is agg_common.cuh's. The self term stays here: the result is narrowed once, and a self term without edges keeps its
// bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "agg_common.cuh"

namespace wm {
// the two row types (tags: a row is handled as raw 16-bit words)
struct f16_rows {};
struct bf16_rows {};

namespace {

// ---- conversions: T -> fp32 exact; fp32 -> T round to nearest even, once
template <class T>
__device__ __forceinline__ float widen(uint32_t h);   // h: the 16 bits of one element, in the low half
template <>
__device__ __forceinline__ float widen<bf16_rows>(uint32_t h)
{
  return __uint_as_float(h << 16);
}
template <>
__device__ __forceinline__ float widen<f16_rows>(uint32_t h)
{
  const uint16_t s = static_cast<uint16_t>(h);
  _Float16 v;
  __builtin_memcpy(&v, &s, 2);
  return static_cast<float>(v);   // (subnormals included: fp16 denormals are not flushed in this mode)
}

template <class T>
__device__ __forceinline__ uint32_t narrow(float f);   // the 16 bits of round_T(f), in the low half
template <>
__device__ __forceinline__ uint32_t narrow<bf16_rows>(float f)
{
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;   // NaN stays NaN (made quiet)
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;                     // ties to even; past the largest finite: inf
}
template <>
__device__ __forceinline__ uint32_t narrow<f16_rows>(float f)
{
  const _Float16 v = static_cast<_Float16>(f);   // IEEE: ties to even, overflow to inf, subnormal results kept
  uint16_t s;
  __builtin_memcpy(&s, &v, 2);
  return s;
}

// ---- a lane's raw piece of a row: VEC == 8: 16 bytes (element 2i in the low half of word i); VEC == 1: one element
template <int VEC>
struct hraw {
  uint32_t w[VEC == 8 ? 4 : 1];
};

template <int VEC>
__device__ __forceinline__ hraw<VEC> ldh(const uint16_t* p)
{
  hraw<VEC> r;
  if constexpr (VEC == 8) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    r.w[0] = t.x, r.w[1] = t.y, r.w[2] = t.z, r.w[3] = t.w;
  } else {
    r.w[0] = *p;
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ void sth(uint16_t* p, const hraw<VEC>& a)
{
  if constexpr (VEC == 8) *reinterpret_cast<uint4*>(p) = make_uint4(a.w[0], a.w[1], a.w[2], a.w[3]);
  else *p = static_cast<uint16_t>(a.w[0]);
}

template <class T, int VEC>
__device__ __forceinline__ fvec<VEC> widened(const hraw<VEC>& a)
{
  fvec<VEC> r;
  if constexpr (VEC == 8) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[2 * i] = widen<T>(a.w[i] & 0xffffu), r.v[2 * i + 1] = widen<T>(a.w[i] >> 16);
  } else {
    r.v[0] = widen<T>(a.w[0]);
  }
  return r;
}

template <class T, int VEC>
__device__ __forceinline__ hraw<VEC> narrowed(const fvec<VEC>& a)
{
  hraw<VEC> r;
  if constexpr (VEC == 8) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = narrow<T>(a.v[2 * i]) | (narrow<T>(a.v[2 * i + 1]) << 16);
  } else {
    r.w[0] = narrow<T>(a.v[0]);
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ hraw<VEC> zero_raw()
{
  hraw<VEC> r;
#pragma unroll
  for (int i = 0; i < (VEC == 8 ? 4 : 1); ++i) r.w[i] = 0u;
  return r;
}

// fp32 pieces of a partial row (the workspace), stored as ldp (agg_common.cuh) loads them
template <int VEC>
__device__ __forceinline__ void stp(float* p, const fvec<VEC>& a)
{
  if constexpr (VEC == 8) {
    fvec<4> lo, hi;
#pragma unroll
    for (int i = 0; i < 4; ++i) lo.v[i] = a.v[i], hi.v[i] = a.v[4 + i];
    stv(p, lo);
    stv(p + 4, hi);
  } else {
    stv(p, a);
  }
}

template <class T, int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void agg16_forward_kernel(wm_agg16_args p)
{
  const int gl       = threadIdx.x % LANES;
  const int64_t F    = p.dim;
  const uint16_t* in = static_cast<const uint16_t*>(p.in);
  uint16_t* out      = static_cast<uint16_t*>(p.out);
  for_target_pieces<VEC, LANES>(p, F, [&](int64_t d, int64_t e0, int64_t e1, int64_t c, int64_t cl, bool act) {
    const int64_t deg    = e1 - e0;
    const float r        = deg > 0 ? 1.0f / static_cast<float>(deg) : 0.0f;
    const uint16_t* self = in + d * p.in_stride;
    uint16_t* orow       = out + d * p.out_stride;
    fvec<VEC> acc        = splat<VEC>(-0.0f);
    int my               = 0;
    hraw<VEC> v[kAggBatch];
    for_edge_batches<LANES>(
        e0, e1, gl, [&](int64_t e, bool in_range) { my = in_range ? p.col_ind[e] : 0; },
        [&](int k, int from, int64_t) {
          const int src = __shfl(my, from, LANES);
          v[k]          = ldh<VEC>(in + static_cast<int64_t>(src) * p.in_stride + cl);
        },
        [&](int k, int64_t) { add_to(acc, widened<T, VEC>(v[k])); });
    if (act) {
      sth(orow + c, deg == 0 ? zero_raw<VEC>() : narrowed<T, VEC>(p.mean ? scaled(acc, r) : acc));
      sth(orow + F + c, ldh<VEC>(self + c));
    }
  });
}

// acc += t(e) for the edges at sorted positions [eb0, ee), in that order (LANES lanes, this lane's columns at cl)
template <class T, int VEC, int LANES>
__device__ __forceinline__ void fold_edges16(fvec<VEC>& acc, const wm_agg16_args& p, const int32_t* sorted_dst, int64_t eb0,
                                             int64_t ee, int64_t cl, int gl)
{
  const uint16_t* grad = static_cast<const uint16_t*>(p.grad);
  int my_d   = 0;
  float my_r = 1.0f;
  hraw<VEC> v[kAggBatch];
  float rs[kAggBatch];
  for_edge_batches<LANES>(
      eb0, ee, gl,
      [&](int64_t i, bool in) {
        my_d = 0, my_r = 1.0f;
        if (in) {
          my_d = sorted_dst[i];
          if (p.mean) my_r = 1.0f / static_cast<float>(p.row_ptr[my_d + 1] - p.row_ptr[my_d]);
        }
      },
      [&](int k, int from, int64_t) {
        const int d = __shfl(my_d, from, LANES);
        rs[k]       = __shfl(my_r, from, LANES);
        v[k]        = ldh<VEC>(grad + static_cast<int64_t>(d) * p.grad_stride + cl);
      },
      [&](int k, int64_t) { add_to(acc, p.mean ? scaled(widened<T, VEC>(v[k]), rs[k]) : widened<T, VEC>(v[k])); });
}

template <class T, int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void agg16_bwd_chunk_kernel(wm_agg16_args p, wm_agg_bwd_state b)
{
  const int gl = threadIdx.x % LANES;
  for_chunk_pieces<VEC, LANES>(b, p.dim, [&](int64_t t, int64_t cs, int64_t ce, int64_t c, int64_t cl, bool act) {
    fvec<VEC> acc = splat<VEC>(-0.0f);
    fold_edges16<T, VEC, LANES>(acc, p, b.sorted_dst, cs, ce, cl, gl);
    if (act) stp(b.partial + t * b.partial_stride + c, acc);   // (the partial row stays fp32)
  });
}

template <class T, int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void agg16_bwd_fold_kernel(wm_agg16_args p, wm_agg_bwd_state b)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t F       = p.dim;
  const int64_t nu      = *b.n_unique;
  const uint16_t* grad  = static_cast<const uint16_t*>(p.grad);
  uint16_t* out         = static_cast<uint16_t*>(p.out);
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; s < p.n_src;
       s += static_cast<int64_t>(gridDim.x) * kGroups) {
    const src_run r = run_of_source(b, nu, s);
    const bool has  = r.has;
    const bool self = s < p.n_dst;
    for (int64_t cb = 0; cb < F; cb += LANES * VEC) {
      const int64_t c  = cb + gl * VEC;
      const bool act   = c < F;
      const int64_t cl = act ? c : 0;
      fvec<VEC> acc    = splat<VEC>(-0.0f);
      fold_edges16<T, VEC, LANES>(acc, p, b.sorted_dst, r.s0, r.c0e, cl, gl);
      add_partials(acc, b, r, cl);
      hraw<VEC> res = zero_raw<VEC>();
      if (self) {
        res = ldh<VEC>(grad + s * p.grad_stride + F + cl);   // only the self term: its bits
        if (has) {
          add_to(acc, widened<T, VEC>(res));
          res = narrowed<T, VEC>(acc);
        }
      } else if (has) {
        res = narrowed<T, VEC>(acc);
      }
      if (act) sth(out + s * p.out_stride + c, res);
    }
  }
}

// 16-byte pieces when every row start is 16-byte aligned (8 elements a piece)
bool use_vec8(int64_t dim, const void* a, int64_t a_stride, const void* b, int64_t b_stride)
{
  return dim % 8 == 0 && a_stride % 8 == 0 && b_stride % 8 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(b) % 16 == 0;
}

#define WM_AGG16_LANES(T_, V_, PIECES_, LAUNCH_)  \
  do {                                            \
    const int lanes__ = lanes_for(PIECES_);       \
    if (lanes__ == 16) LAUNCH_(T_, V_, 16);       \
    else if (lanes__ == 32) LAUNCH_(T_, V_, 32);  \
    else LAUNCH_(T_, V_, 64);                     \
  } while (0)

#define WM_AGG16_DISPATCH(BF16_, VEC_, DIM_, LAUNCH_)                  \
  do {                                                                 \
    if (BF16_) {                                                       \
      if (VEC_) WM_AGG16_LANES(bf16_rows, 8, (DIM_) / 8, LAUNCH_);     \
      else WM_AGG16_LANES(bf16_rows, 1, DIM_, LAUNCH_);                \
    } else {                                                           \
      if (VEC_) WM_AGG16_LANES(f16_rows, 8, (DIM_) / 8, LAUNCH_);      \
      else WM_AGG16_LANES(f16_rows, 1, DIM_, LAUNCH_);                 \
    }                                                                  \
  } while (0)

}  // namespace

int hip_agg16_forward(const wm_agg16_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->dtype != WHOLEMEMORY_DT_HALF && a->dtype != WHOLEMEMORY_DT_BF16) return -1;
  if (a->n_dst == 0 || a->dim == 0) return 0;
  const bool bf = a->dtype == WHOLEMEMORY_DT_BF16;
  const bool v8 = use_vec8(a->dim, a->in, a->in_stride, a->out, a->out_stride);
#define WM_AGG16_FWD(T, V, L)                                                                                         \
  hipLaunchKernelGGL((agg16_forward_kernel<T, V, L>), dim3(blocks_for(a->n_dst, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a)
  WM_AGG16_DISPATCH(bf, v8, a->dim, WM_AGG16_FWD);
#undef WM_AGG16_FWD
  return rc_last();
}

int hip_agg16_backward(const wm_agg16_args* a, const wm_edge_index& ix, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->dtype != WHOLEMEMORY_DT_HALF && a->dtype != WHOLEMEMORY_DT_BF16) return -1;
  if (a->n_src == 0 || a->dim == 0) return 0;
  wm_agg_bwd_state b;
  if (agg_bwd_prepare(*a, a->dim, ix, workspace, &b, stream_v) != 0) return -2;
  const bool bf = a->dtype == WHOLEMEMORY_DT_BF16;
  const bool v8 = use_vec8(a->dim, a->grad, a->grad_stride, a->out, a->out_stride);
  if (b.n_tiles > 1) {   // (one tile holds no chunk k >= 1)
#define WM_AGG16_CHUNK(T, V, L)                                                                                          \
  hipLaunchKernelGGL((agg16_bwd_chunk_kernel<T, V, L>), dim3(blocks_for(b.n_tiles, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
    WM_AGG16_DISPATCH(bf, v8, a->dim, WM_AGG16_CHUNK);
#undef WM_AGG16_CHUNK
    if (rc_last() != 0) return -2;
  }
#define WM_AGG16_FOLD(T, V, L)                                                                                         \
  hipLaunchKernelGGL((agg16_bwd_fold_kernel<T, V, L>), dim3(blocks_for(a->n_src, kAggBlock / (L))), dim3(kAggBlock), 0, \
                     stream, *a, b)
  WM_AGG16_DISPATCH(bf, v8, a->dim, WM_AGG16_FOLD);
#undef WM_AGG16_FOLD
  return rc_last();
}

}  // namespace wm
