// wholegraph_amd — the GraphSAGE `agg_concat` op (kernels/agg.hip) whose rows come straight from an 8-bit row-quantized
// WholeMemory table by global id (wholegraph_amd_ext.h section 2j) on gfx950: kernels/agg_gather.hip with rows in the format
// of kernels/qrows.hip. Layer 0 of a GNN over a quantized feature table without the dequantized [n_src, F] intermediate that
// the quantized gather writes at full width and the aggregation reads back once per edge.
//
// A table row is Q = round_up(dim, 4) code bytes (the bytes past dim are zero), then fp32 scale and fp32 bias. The virtual row
// is x[i][j] = float(code[j]) * scale + bias of table row node_ids[i] — dequant<float> of kernels/qrows.hip: one multiply and
// one add, rounded separately (the file is built with -ffp-contract=off). out [n_dst, 2F] fp32 holds, per target d, the sum
// or mean of x[col_ind[e]] over its edges — the fp32 sum of kernels/agg.hip, from -0.0f, term by term in edge order, the mean
// as acc * (1.0f / float(deg)), +0.0 without edges — and x[d]. So the result equals agg_concat over the rows the quantized
// gather writes as fp32, bit for bit.
//
// The structure is the one of aggg_forward_kernel: one group of 16 / 32 / 64 lanes per target, sized from the row's dwords
// of codes; one lane owns one dword = 4 codes, 4 fp32 accumulators and (VEC == 4) one 16-byte store, so a 128-wide row is
// 32 lanes and a wave serves two targets; rows of more than 64 dwords are walked in column blocks with a group-uniform trip
// count; the column ids of up to LANES edges come from one coalesced load, lane k resolves the table address of edge eb + k
// (continuous base; chunked: owner by multiply-high when every rank holds the same amount, else the search over the rank
// offsets; ids and column indices folded into range so that no load leaves the table) and the group fetches each 64-bit
// address with two shuffles. The loads of a batch of kAggBatch edges — the lane's code dword, and scale and bias at the
// group-uniform address row + Q, as kernels/qrows.hip loads them (DESIGN.md section 3.14 has the choice) — are issued back to
// back as global loads; a batch shorter than kAggBatch repeats its last edge's loads and skips the add (for_edge_batches of
// agg_common.cuh).
//
// Table rows are only 4-byte aligned by format (a 136-byte stride): dword loads are always legal, so there is no aligned /
// unaligned split on the table side. VEC == 1, the element-wise instantiation (dim % 4 != 0, or an out whose rows are not
// aligned to a lane's 4 floats), takes the same loads and stores single floats under the column bound: the zero bytes behind
// column dim never reach out, and the trailer's dword is never read as codes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "agg_common.cuh"
#include "device_common.cuh"

namespace wm {
namespace {

// the table as the kernel sees it (the gref, the view's offset and row stride in bytes) and the block
struct aggq_params {
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
  int64_t words;                   // dwords of codes per row: Q / 4
  int mean;
  float* out;                      // [n_dst, out_stride], 2 * dim columns
  int64_t out_stride;
};

// a lane's loads of one table row: its dword of codes, and the row's trailer
struct qraw {
  uint32_t w, scale, bias;
};

// rows are global memory (device, pinned host or a peer's mapping); an address that came out of a shuffle is an integer,
// and without the address space hipcc would emit flat loads, whose waits also drain the shuffles' counter
__device__ __forceinline__ qraw ldrow(uint64_t row, uint64_t code_off, uint64_t q_bytes)
{
  qraw r;
  const char* p = reinterpret_cast<const char*>(row);
  r.w           = ld_global<uint32_t>(p + code_off);
  r.scale       = ld_global<uint32_t>(p + q_bytes);
  r.bias        = ld_global<uint32_t>(p + q_bytes + 4);
  return r;
}

// the 4 values of a dword of codes (kernels/qrows.hip: dequant<float>)
__device__ __forceinline__ fvec<4> dequantized(const qraw& a)
{
  const float scale = __uint_as_float(a.scale), bias = __uint_as_float(a.bias);
  fvec<4> r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float c = static_cast<float>((a.w >> (8 * k)) & 0xffu);
    r.v[k]        = c * scale + bias;
  }
  return r;
}

// a lane's 4 values of an output row: one 16-byte store, or (VEC == 1) single floats under the column bound
template <int VEC>
__device__ __forceinline__ void stout(float* p, const fvec<4>& a, int64_t left)
{
  if constexpr (VEC == 4) {
    stv(p, a);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < left) p[k] = a.v[k];
  }
}

// byte address of the table row of virtual row i: T[node_ids[i]] (kernels/agg_gather.hip: row_address). Ids outside the
// view are the caller's contract (the result is unspecified); they are folded into it so that no load leaves the table.
__device__ __forceinline__ uint64_t row_address(const aggq_params& p, int64_t i)
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

template <int VEC, int LANES>
__global__ __launch_bounds__(kAggBlock) void aggq_forward_kernel(aggq_params p)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t F       = p.dim;
  const int64_t W       = p.words;
  const uint64_t q      = static_cast<uint64_t>(W) * 4;
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
    for (int64_t cb = 0; cb < W; cb += LANES) {   // (group-uniform trip count: the shuffles below stay in step)
      const int64_t c   = cb + gl;
      const bool act    = c < W;
      const uint64_t cl = static_cast<uint64_t>(act ? c : 0) * 4;   // (a lane past the row's codes repeats dword 0)
      fvec<4> acc       = splat<4>(-0.0f);
      uint64_t my       = 0;
      qraw v[kAggBatch];
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
          [&](int k, int from, int64_t) { v[k] = ldrow(shfl_address<LANES>(my, from), cl, q); },
          [&](int k, int64_t) { add_to(acc, dequantized(v[k])); });
      if (act) {
        const fvec<4> a    = deg == 0 ? splat<4>(0.0f) : (p.mean ? scaled(acc, r) : acc);
        const int64_t left = F - c * 4;   // columns of the row from this lane's first on (>= 1)
        stout<VEC>(orow + c * 4, a, left);
        stout<VEC>(orow + F + c * 4, dequantized(ldrow(self, cl, q)), left);
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

#define WM_AGGQ_LANES(V_, WORDS_)                                                                                      \
  do {                                                                                                                 \
    const int lanes__ = lanes_for(WORDS_);                                                                             \
    if (lanes__ == 16) WM_AGGQ_LAUNCH(V_, 16);                                                                         \
    else if (lanes__ == 32) WM_AGGQ_LAUNCH(V_, 32);                                                                    \
    else WM_AGGQ_LAUNCH(V_, 64);                                                                                       \
  } while (0)
#define WM_AGGQ_LAUNCH(V_, L_)                                                                                         \
  hipLaunchKernelGGL((aggq_forward_kernel<V_, L_>), dim3(blocks_for(p.n_dst, kAggBlock / (L_))), dim3(kAggBlock), 0,   \
                     stream, p)

}  // namespace

int hip_qagg_forward(const wm_qagg_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->node_id_dtype != WHOLEMEMORY_DT_INT && a->node_id_dtype != WHOLEMEMORY_DT_INT64) return -1;
  if (a->dim < 1 || a->table_stride % 4 != 0 || a->table_storage_offset % 4 != 0) return -1;
  const int64_t words = (a->dim + 3) / 4;
  if (words * 4 + 8 > a->table_stride) return -1;
  if (a->n_dst == 0) return 0;
  if (a->table_rows < 1) return -1;
  aggq_params p{};
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
  p.table_stride_bytes = a->table_stride;
  p.table_offset_bytes = a->table_storage_offset;
  p.table_rows         = a->table_rows;
  p.node_ids           = a->node_ids;
  p.row_ptr            = a->row_ptr;
  p.col_ind            = a->col_ind;
  p.n_edges            = a->n_edges;
  p.n_dst              = a->n_dst;
  p.n_src              = a->n_src;
  p.dim                = a->dim;
  p.words              = words;
  p.mean               = a->mean;
  p.out                = a->out;
  p.out_stride         = a->out_stride;
  // a lane's 4 values as one store: whole dwords of codes only, and every row of out aligned to those 4 floats
  const bool wide = a->dim % 4 == 0 && a->out_stride % 4 == 0 && reinterpret_cast<uintptr_t>(a->out) % 16 == 0;
  if (wide) WM_AGGQ_LANES(4, words);
  else WM_AGGQ_LANES(1, words);
  return rc_last();
}

}  // namespace wm
