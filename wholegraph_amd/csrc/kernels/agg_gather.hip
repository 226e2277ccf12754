// wholegraph_amd — the GraphSAGE `agg_concat` op (kernels/agg.hip) whose rows come straight from a WholeMemory table by
// global id (`gather_agg_concat`, wholegraph_amd_ext.h section 2e) on gfx950: layer 0 of a GNN without the gathered
// [n_src, F] intermediate that a gather writes and the aggregation reads back once per edge.
//
// x[i] = fp32(T[node_ids[i]]) is virtual. out [n_dst, 2F] fp32 holds, per target d, the sum or mean of x[col_ind[e]] over
// its edges — the fp32 sum of kernels/agg.hip, term by term in the same order (widening a 16-bit row is exact) — and x[d].
// So the result equals agg_concat over the gathered rows bit for bit.
//
// Same structure as agg_forward_kernel / agg16_forward_kernel: one group of 16 / 32 / 64 lanes per target, sized from the
// row's 16-byte pieces (or, on the element-wise path, its elements); the column ids of up to LANES edges loaded with one
// coalesced load; the rows of a batch of kAggBatch edges issued back to back as raw pieces and widened when they are added,
// in edge order, into fp32 accumulators that are stored once (for_edge_batches of agg_common.cuh; the frame around it stays
// here, because the target's own row is resolved once per target). What is new is the address chain in front of the row loads,
// taken from kernels/rows.hip, where each lane resolves its own row: lane k loads node_ids[col_ind[eb + k]] and resolves
// that row's address in the table (continuous base; chunked: owner by multiply-high when every rank holds the same amount,
// else the search over the rank offsets), and the group then fetches each 64-bit address with two shuffles. The id lookup
// is one more dependent load per LANES edges, not per edge. The target's own row goes through the same resolve.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "agg_common.cuh"
#include "device_common.cuh"

namespace wm {
// rows of 16-bit floats are handled as raw 16-bit words (the tags of kernels/agg_half.hip)
struct f16_rows {};
struct bf16_rows {};

namespace {

// the table as the kernel sees it (the gref, the view's offset and row stride in bytes) and the block
struct aggg_params {
  const char* base;                // continuous: flat base
  const char* const* rank_ptrs;    // chunked: per-rank bases (device array)
  const size_t* rank_offsets;      // chunked, !same_chunk: byte offsets [world + 1] (device array)
  size_t chunk_stride;             // 0 = continuous; else bytes per rank
  uint64_t chunk_magic;            // same_chunk: rank = off / chunk_stride as umulhi(off, magic) >> shift; 0: stride 1
  int chunk_shift;
  int world_size;
  int same_chunk;
  int ids64;                       // node_ids are int64 (else int32)
  int64_t table_stride_bytes;
  int64_t table_offset_bytes;
  int64_t table_rows;              // rows of the view
  const void* node_ids;            // [n_src]
  const int32_t* row_ptr;          // [n_dst + 1]
  const int32_t* col_ind;          // [n_edges]
  int64_t n_edges, n_dst, n_src, dim;
  int mean;
  float* out;                      // [n_dst, out_stride], 2 * dim columns
  int64_t out_stride;
};

template <class T>
struct elt_bytes {
  static constexpr int value = 2;
};
template <>
struct elt_bytes<float> {
  static constexpr int value = 4;
};

// ---- T -> fp32, exact
template <class T>
__device__ __forceinline__ float widen16(uint32_t h);   // h: the 16 bits of one element, in the low half
template <>
__device__ __forceinline__ float widen16<bf16_rows>(uint32_t h)
{
  return __uint_as_float(h << 16);
}
template <>
__device__ __forceinline__ float widen16<f16_rows>(uint32_t h)
{
  const uint16_t s = static_cast<uint16_t>(h);
  _Float16 v;
  __builtin_memcpy(&v, &s, 2);
  return static_cast<float>(v);   // (subnormals included)
}

// ---- a lane's raw piece of a table row: VEC > 1: 16 bytes (4 floats, or 8 16-bit elements); VEC == 1: one element
template <int VEC>
struct graw {
  uint32_t w[VEC > 1 ? 4 : 1];
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // (a native vector: loadable through an address-space pointer)

// rows are global memory (device, pinned host or a peer's mapping); an address that came out of a shuffle is an integer,
// and without the address space hipcc would emit flat loads, whose waits also drain the shuffles' counter
template <class T, int VEC>
__device__ __forceinline__ graw<VEC> ldrow(uint64_t addr)
{
  graw<VEC> r;
  const void* p = reinterpret_cast<const void*>(addr);
  if constexpr (VEC > 1) {
    const u32x4 t = ld_global<u32x4>(p);
    r.w[0] = t[0], r.w[1] = t[1], r.w[2] = t[2], r.w[3] = t[3];
  } else if constexpr (elt_bytes<T>::value == 4) {
    r.w[0] = ld_global<uint32_t>(p);
  } else {
    r.w[0] = ld_global<uint16_t>(p);
  }
  return r;
}

template <class T, int VEC>
__device__ __forceinline__ fvec<VEC> widened_row(const graw<VEC>& a)
{
  fvec<VEC> r;
  if constexpr (elt_bytes<T>::value == 4) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = __uint_as_float(a.w[i]);
  } else if constexpr (VEC == 8) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[2 * i] = widen16<T>(a.w[i] & 0xffffu), r.v[2 * i + 1] = widen16<T>(a.w[i] >> 16);
  } else {
    r.v[0] = widen16<T>(a.w[0]);
  }
  return r;
}

// VEC fp32 values of an output row (16-byte accesses when VEC > 1)
template <int VEC>
__device__ __forceinline__ void stout(float* p, const fvec<VEC>& a)
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

// byte address of the first element of the table row of virtual row i: T[node_ids[i]]. Ids outside the view are the
// caller's contract (the result is unspecified); they are folded into it so that no load leaves the table.
__device__ __forceinline__ uint64_t row_address(const aggg_params& p, int64_t i)
{
  int64_t id = p.ids64 ? static_cast<const int64_t*>(p.node_ids)[i] : static_cast<int64_t>(static_cast<const int32_t*>(p.node_ids)[i]);
  id         = id < 0 ? 0 : (id >= p.table_rows ? p.table_rows - 1 : id);
  const size_t off = static_cast<size_t>(p.table_offset_bytes) + static_cast<size_t>(id) * static_cast<size_t>(p.table_stride_bytes);
  if (p.chunk_stride == 0) return reinterpret_cast<uint64_t>(p.base) + off;
  int rank;
  size_t rank_start;
  if (p.same_chunk) {
    rank       = static_cast<int>(p.chunk_magic == 0 ? off : (__umul64hi(off, p.chunk_magic) >> p.chunk_shift));
    rank       = rank < p.world_size ? rank : p.world_size - 1;
    rank_start = static_cast<size_t>(rank) * p.chunk_stride;
  } else {
    rank = 0;
    for (int r = 1; r < p.world_size; r++)
      if (off >= p.rank_offsets[r]) rank = r;
    rank_start = p.rank_offsets[rank];
  }
  return reinterpret_cast<uint64_t>(p.rank_ptrs[rank]) + (off - rank_start);
}

template <int LANES>
__device__ __forceinline__ uint64_t shfl_address(uint64_t a, int from)
{
  const uint32_t lo = __shfl(static_cast<uint32_t>(a), from, LANES);
  const uint32_t hi = __shfl(static_cast<uint32_t>(a >> 32), from, LANES);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

template <class T, int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void aggg_forward_kernel(aggg_params p)
{
  constexpr int kGroups = kAggBlock / LANES;
  constexpr int kElt    = elt_bytes<T>::value;
  const int gl          = threadIdx.x % LANES;
  const int64_t F       = p.dim;
  const int64_t last    = p.n_src - 1;
  // (its own frame, not for_target_pieces: the resolve of the target's own row is a chain of loads, done once per target)
  for (int64_t d = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; d < p.n_dst;
       d += static_cast<int64_t>(gridDim.x) * kGroups) {
    int64_t e0, e1;
    edge_range(p.row_ptr, d, p.n_edges, e0, e1);
    const int64_t deg   = e1 - e0;
    const float r       = deg > 0 ? 1.0f / static_cast<float>(deg) : 0.0f;
    const uint64_t self = row_address(p, d);   // (group-uniform)
    float* orow         = p.out + d * p.out_stride;
    for (int64_t cb = 0; cb < F; cb += LANES * VEC) {   // (group-uniform trip count: the shuffles below stay in step)
      const int64_t c   = cb + gl * VEC;
      const bool act    = c < F;
      const uint64_t cl = static_cast<uint64_t>(act ? c : 0) * kElt;
      fvec<VEC> acc     = splat<VEC>(-0.0f);
      uint64_t my       = 0;
      graw<VEC> v[kAggBatch];
      for_edge_batches<LANES>(
          e0, e1, gl,
          [&](int64_t e, bool in) {
            my = 0;
            if (in) {
              int64_t src = p.col_ind[e];
              src         = src < 0 ? 0 : (src > last ? last : src);   // (as the ids: no load outside node_ids)
              my          = row_address(p, src);
            }
          },
          [&](int k, int from, int64_t) { v[k] = ldrow<T, VEC>(shfl_address<LANES>(my, from) + cl); },
          [&](int k, int64_t) { add_to(acc, widened_row<T, VEC>(v[k])); });
      if (act) {
        const fvec<VEC> a = deg == 0 ? splat<VEC>(0.0f) : (p.mean ? scaled(acc, r) : acc);
        stout(orow + c, a);
        stout(orow + F + c, widened_row<T, VEC>(ldrow<T, VEC>(self + cl)));
      }
    }
  }
}

// rank = off / chunk_stride as multiply-high + shift (kernels/rows.hip: magic_for): with l = ceil(log2 d) and
// m = ceil(2^(63 + l) / d), floor(n / d) = umulhi64(n, m) >> (l - 1) for every n < 2^63
void magic_for(uint64_t d, uint64_t* m, int* shift)
{
  if (d <= 1) {
    *m = 0, *shift = 0;
    return;
  }
  int l = 0;
  while (l < 63 && (uint64_t(1) << l) < d) l++;
  const unsigned __int128 num = static_cast<unsigned __int128>(1) << (63 + l);
  *m     = static_cast<uint64_t>((num + d - 1) / d);
  *shift = l - 1;
}

// every row start of the table 16-byte aligned?
bool rows_aligned16(const wm_gather_agg_args* a, int64_t stride_bytes, int64_t offset_bytes)
{
  if (stride_bytes % 16 != 0 || offset_bytes % 16 != 0) return false;
  const wholememory_gref_t& g = a->gref;
  if (g.stride == 0) return reinterpret_cast<uintptr_t>(g.pointer) % 16 == 0;
  // chunked: the per-rank bases are allocations (aligned far beyond 16 bytes); a row sits at base + (off - rank start)
  if (g.same_chunk) return g.stride % 16 == 0;
  gref_host_tables t;   // rank starts are a device array: judged from the handle's host copies, when it registered them
  if (!lookup_gref_tables(g.pointer, &t) || t.world_size != g.world_size) return false;
  for (int r = 0; r < t.world_size; r++)
    if (t.rank_offsets[r] % 16 != 0 || reinterpret_cast<uintptr_t>(t.rank_ptrs[r]) % 16 != 0) return false;
  return true;
}

#define WM_AGGG_LANES(T_, V_, PIECES_)                                                                                 \
  do {                                                                                                                 \
    const int lanes__ = lanes_for(PIECES_);                                                                            \
    if (lanes__ == 16) WM_AGGG_LAUNCH(T_, V_, 16);                                                                     \
    else if (lanes__ == 32) WM_AGGG_LAUNCH(T_, V_, 32);                                                                \
    else WM_AGGG_LAUNCH(T_, V_, 64);                                                                                   \
  } while (0)
#define WM_AGGG_LAUNCH(T_, V_, L_)                                                                                     \
  hipLaunchKernelGGL((aggg_forward_kernel<T_, V_, L_>), dim3(blocks_for(p.n_dst, kAggBlock / (L_))), dim3(kAggBlock), 0, \
                     stream, p)

}  // namespace

int hip_gather_agg_forward(const wm_gather_agg_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const auto dt      = a->table_dtype;
  if (dt != WHOLEMEMORY_DT_FLOAT && dt != WHOLEMEMORY_DT_HALF && dt != WHOLEMEMORY_DT_BF16) return -1;
  if (a->node_id_dtype != WHOLEMEMORY_DT_INT && a->node_id_dtype != WHOLEMEMORY_DT_INT64) return -1;
  if (a->n_dst == 0 || a->dim == 0) return 0;
  if (a->table_rows < 1) return -1;
  const int64_t es = dt == WHOLEMEMORY_DT_FLOAT ? 4 : 2;
  aggg_params p{};
  p.chunk_stride = a->gref.stride;
  p.world_size   = a->gref.world_size;
  p.same_chunk   = a->gref.same_chunk ? 1 : 0;
  if (a->gref.stride == 0) {
    p.base = static_cast<const char*>(a->gref.pointer);
  } else {
    p.rank_ptrs    = static_cast<const char* const*>(a->gref.pointer);
    p.rank_offsets = a->gref.rank_memory_offsets;
    magic_for(p.chunk_stride, &p.chunk_magic, &p.chunk_shift);
  }
  p.ids64              = a->node_id_dtype == WHOLEMEMORY_DT_INT64 ? 1 : 0;
  p.table_stride_bytes = a->table_stride * es;
  p.table_offset_bytes = a->table_storage_offset * es;
  p.table_rows         = a->table_rows;
  p.node_ids           = a->node_ids;
  p.row_ptr            = a->row_ptr;
  p.col_ind            = a->col_ind;
  p.n_edges            = a->n_edges;
  p.n_dst              = a->n_dst;
  p.n_src              = a->n_src;
  p.dim                = a->dim;
  p.mean               = a->mean;
  p.out                = a->out;
  p.out_stride         = a->out_stride;
  const int64_t piece  = 16 / es;   // elements of a 16-byte piece
  const bool vec       = a->dim % piece == 0 && rows_aligned16(a, p.table_stride_bytes, p.table_offset_bytes) &&
                   a->out_stride % 4 == 0 && reinterpret_cast<uintptr_t>(a->out) % 16 == 0;
  if (dt == WHOLEMEMORY_DT_FLOAT) {
    if (vec) WM_AGGG_LANES(float, 4, a->dim / 4);
    else WM_AGGG_LANES(float, 1, a->dim);
  } else if (dt == WHOLEMEMORY_DT_BF16) {
    if (vec) WM_AGGG_LANES(bf16_rows, 8, a->dim / 8);
    else WM_AGGG_LANES(bf16_rows, 1, a->dim);
  } else {
    if (vec) WM_AGGG_LANES(f16_rows, 8, a->dim / 8);
    else WM_AGGG_LANES(f16_rows, 1, a->dim);
  }
  return rc_last();
}

}  // namespace wm
