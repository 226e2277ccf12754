// wholegraph_amd — `rank_rows` (wholegraph_amd_ext.h section 2w) on gfx950: per query, how many rows of a WholeMemory table
// score above, and exactly, the score of the query's target row. The evaluation of every embedding model of the library
// (filtered MRR / Hits@k of KGEModel), without the [B, N] score matrix.
//
// The contract fixes the arithmetic: one fp32 accumulator per (query, row), the columns in ascending order, every operation
// rounded on its own. rank_step is that step; the three passes call it, so a row scores the same bits wherever it is scored.
// MFMA cannot keep that order, so the sweep is a register-tiled VALU kernel.
//
//   threshold  one lane per query: thr[b] = score(b, target[b]), NaN for a target outside the table; greater / equal start at
//              0 (-1 for such a target). No memset: the outputs are cleared here.
//   sweep      a workgroup of 256 lanes owns kRankEntityTile = 256 rows x kRankQueryTile = 64 queries and walks the columns
//              in slices of kRankSlice = 32. Per slice it stages both tiles in LDS, row-major with a row pitch of 36 floats:
//              a lane's 16-byte store and its 16-byte read of 4 columns of one row start at bank 4 * row mod 32 (36 r mod 64
//              with 64 banks: 16 consecutive rows cover them once), so neither conflicts. Table rows are loaded 16 bytes a
//              lane, 8 lanes a row slice (one 128-byte line); their addresses are resolved once per row and tile through the
//              chunked view and kept in LDS. Lane (tx, ty), tx = lane % 32, ty = lane / 32, holds the 8 x 8 accumulators of
//              rows tx + 32 i and queries ty + 8 j: a wave reads two query rows (a broadcast each) and 32 consecutive table
//              rows per 16-byte read, 16 reads per 4 columns and 64 pairs. After the last slice a lane compares its pairs
//              with thr, leaves out the target and the rows past the range, the 32 lanes of a query add their counts with
//              shuffles, and one lane adds them to greater / equal with an integer atomic (the order of integer adds does not
//              matter; a partials buffer would be tiles x B x 16 bytes). Columns past F are staged as +0.0 in both tiles:
//              they add +0.0 in every measure, so any F >= 1 is served. The grid walks (row tile, query tile) pairs, query
//              tiles fastest, so that the workgroups resident together read the same table rows; it is sized by blocks_for
//              and strides.
//   filter     one lane per entry of the filter block: the query it belongs to (a search of filter_row_ptr), the score of
//              its row, and one taken from greater or equal where the sweep counted that row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../rank.hpp"
#include "agg_common.cuh"
#include "device_common.cuh"
#include "gref_view.cuh"

namespace wm {
namespace {

constexpr int kRkBlock = 256;
constexpr int kRkTx    = 32;                        // lanes along the table rows
constexpr int kRkTy    = kRkBlock / kRkTx;          // lanes along the queries
constexpr int kRkRe    = kRankEntityTile / kRkTx;   // table rows of a lane
constexpr int kRkRq    = kRankQueryTile / kRkTy;    // queries of a lane
constexpr int kRkPitch = kRankSlice + 4;            // floats between two rows of a staged tile
constexpr int kRkQuads = kRankSlice / 4;            // 16-byte pieces of a row slice
static_assert(kRkRe == 8 && kRkRq == 8, "a lane holds 8 x 8 accumulators");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct rank_params {
  gref_view table;
  int64_t table_rows, stride, offset;   // elements
  int64_t F;
  const float* query;
  int64_t query_stride, B;
  const void* target;
  int ids64;
  int64_t begin, end;
  const void* filter_row_ptr;
  int row_ptr64;
  const void* filter_ids;
  int64_t M;
  float* thr;
  int64_t* greater;
  int64_t* equal;
};

// the per-column step of section 2w and the score of a finished accumulator
template <int MEASURE>
__device__ __forceinline__ float rank_step(float acc, float u, float t)
{
  if constexpr (MEASURE == 0) {
    return acc + u * t;
  } else if constexpr (MEASURE == 1) {
    return acc + fabsf(u - t);
  } else {
    const float d = u - t;
    return acc + d * d;
  }
}
template <int MEASURE>
__device__ __forceinline__ float rank_score(float acc)
{
  return MEASURE == 0 ? acc : -acc;
}

__device__ __forceinline__ int64_t id_at(const void* ids, int is64, int64_t i)
{
  return is64 ? static_cast<const int64_t*>(ids)[i] : static_cast<int64_t>(static_cast<const int32_t*>(ids)[i]);
}

__device__ __forceinline__ const float* table_row(const rank_params& p, int64_t e)
{
  return gref_address<float>(p.table, p.offset + e * p.stride);
}

// s(b, e) by one lane; e in [0, table_rows)
template <int MEASURE>
__device__ float score_row(const rank_params& p, int64_t b, int64_t e)
{
  const float* u = p.query + b * p.query_stride;
  const float* t = table_row(p, e);
  float acc      = 0.0f;
  for (int64_t c = 0; c < p.F; ++c) acc = rank_step<MEASURE>(acc, u[c], t[c]);
  return rank_score<MEASURE>(acc);
}

template <int MEASURE>
__global__ __launch_bounds__(kRkBlock) void rank_threshold_kernel(rank_params p)
{
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kRkBlock + threadIdx.x; b < p.B; b += static_cast<int64_t>(gridDim.x) * kRkBlock) {
    const int64_t t = id_at(p.target, p.ids64, b);
    const bool in   = t >= 0 && t < p.table_rows;
    p.thr[b]        = in ? score_row<MEASURE>(p, b, t) : __builtin_nanf("");
    p.greater[b]    = in ? 0 : -1;
    p.equal[b]      = in ? 0 : -1;
  }
}

// columns c .. c + 3 of a row, +0.0 past F and for a row that is not there. VEC == 4: every row start is 16-byte aligned
// and F a multiple of 4
template <int VEC>
__device__ __forceinline__ f32x4 load_quad(const float* row, int64_t c, int64_t F)
{
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (row == nullptr || c >= F) return v;
  if constexpr (VEC == 4) {
    v = ld_global<f32x4>(row + c);
  } else {
    v[0] = row[c];
    if (c + 1 < F) v[1] = row[c + 1];
    if (c + 2 < F) v[2] = row[c + 2];
    if (c + 3 < F) v[3] = row[c + 3];
  }
  return v;
}

template <int MEASURE, int VEC>
__global__ __launch_bounds__(kRkBlock) void rank_sweep_kernel(rank_params p, int64_t n_qtiles, int64_t n_tiles)
{
  __shared__ __attribute__((aligned(16))) float es[kRankEntityTile * kRkPitch];
  __shared__ __attribute__((aligned(16))) float qs[kRankQueryTile * kRkPitch];
  __shared__ const float* erow[kRankEntityTile];
  const int tid = threadIdx.x;
  const int tx = tid % kRkTx, ty = tid / kRkTx;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t e0 = p.begin + (tile / n_qtiles) * kRankEntityTile;
    const int64_t b0 = (tile % n_qtiles) * kRankQueryTile;
    {
      const int64_t e = e0 + tid;   // (kRankEntityTile == kRkBlock: a row per lane)
      erow[tid]       = e < p.end ? table_row(p, e) : nullptr;
    }
    float acc[kRkRq][kRkRe];
#pragma unroll
    for (int j = 0; j < kRkRq; ++j)
#pragma unroll
      for (int i = 0; i < kRkRe; ++i) acc[j][i] = 0.0f;
    __syncthreads();
    for (int64_t k0 = 0; k0 < p.F; k0 += kRankSlice) {
#pragma unroll
      for (int n = 0; n < kRankEntityTile * kRkQuads / kRkBlock; ++n) {
        const int l = tid + n * kRkBlock;
        const int r = l / kRkQuads, c = (l % kRkQuads) * 4;
        *reinterpret_cast<f32x4*>(&es[r * kRkPitch + c]) = load_quad<VEC>(erow[r], k0 + c, p.F);
      }
#pragma unroll
      for (int n = 0; n < kRankQueryTile * kRkQuads / kRkBlock; ++n) {
        const int l = tid + n * kRkBlock;
        const int r = l / kRkQuads, c = (l % kRkQuads) * 4;
        const int64_t b = b0 + r;
        *reinterpret_cast<f32x4*>(&qs[r * kRkPitch + c]) =
          load_quad<VEC>(b < p.B ? p.query + b * p.query_stride : nullptr, k0 + c, p.F);
      }
      __syncthreads();
      const int64_t left = p.F - k0;
      const int kend     = left < kRankSlice ? static_cast<int>((left + 3) & ~int64_t(3)) : kRankSlice;
      for (int kk = 0; kk < kend; kk += 4) {
        f32x4 ev[kRkRe], qv[kRkRq];
#pragma unroll
        for (int i = 0; i < kRkRe; ++i) ev[i] = *reinterpret_cast<const f32x4*>(&es[(tx + kRkTx * i) * kRkPitch + kk]);
#pragma unroll
        for (int j = 0; j < kRkRq; ++j) qv[j] = *reinterpret_cast<const f32x4*>(&qs[(ty + kRkTy * j) * kRkPitch + kk]);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < kRkRq; ++j)
#pragma unroll
            for (int i = 0; i < kRkRe; ++i) acc[j][i] = rank_step<MEASURE>(acc[j][i], qv[j][c], ev[i][c]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < kRkRq; ++j) {
      const int64_t b = b0 + ty + kRkTy * j;
      int counts      = 0;   // greater in the low half, equal in the high half: at most 256 each per query and tile
      if (b < p.B) {
        const float thr   = p.thr[b];
        const int64_t tgt = id_at(p.target, p.ids64, b);
#pragma unroll
        for (int i = 0; i < kRkRe; ++i) {
          const int64_t e = e0 + tx + kRkTx * i;
          const float s   = rank_score<MEASURE>(acc[j][i]);
          if (e < p.end && e != tgt) counts += (s > thr ? 1 : 0) + (s == thr ? 1 << 16 : 0);
        }
      }
#pragma unroll
      for (int o = kRkTx / 2; o > 0; o >>= 1) counts += __shfl_xor(counts, o, kRkTx);
      if (tx == 0 && counts != 0) {
        const unsigned long long g = counts & 0xffff, q = static_cast<unsigned>(counts) >> 16;
        if (g != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.greater + b), g);
        if (q != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.equal + b), q);
      }
    }
  }
}

template <int MEASURE>
__global__ __launch_bounds__(kRkBlock) void rank_filter_kernel(rank_params p)
{
  for (int64_t m = static_cast<int64_t>(blockIdx.x) * kRkBlock + threadIdx.x; m < p.M; m += static_cast<int64_t>(gridDim.x) * kRkBlock) {
    // the last query whose row starts at or before m; the entry is its own when it also ends after m
    int64_t lo = 0, hi = p.B;
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (id_at(p.filter_row_ptr, p.row_ptr64, mid) <= m) lo = mid;
      else hi = mid;
    }
    const int64_t b = lo;
    if (id_at(p.filter_row_ptr, p.row_ptr64, b) > m || m >= id_at(p.filter_row_ptr, p.row_ptr64, b + 1)) continue;
    const int64_t tgt = id_at(p.target, p.ids64, b);
    const int64_t e   = id_at(p.filter_ids, p.ids64, m);
    if (tgt < 0 || tgt >= p.table_rows || e < p.begin || e >= p.end || e == tgt) continue;
    const float s = score_row<MEASURE>(p, b, e), thr = p.thr[b];
    if (s > thr) atomicAdd(reinterpret_cast<unsigned long long*>(p.greater + b), ~0ull);
    else if (s == thr) atomicAdd(reinterpret_cast<unsigned long long*>(p.equal + b), ~0ull);
  }
}

rank_params make_params(const wm_rank_args* a)
{
  rank_params p{};
  p.table          = make_view(a->gref);
  p.table_rows     = a->table_rows;
  p.stride         = a->table_stride;
  p.offset         = a->table_storage_offset;
  p.F              = a->dim;
  p.query          = a->query;
  p.query_stride   = a->query_stride;
  p.B              = a->n_queries;
  p.target         = a->target;
  p.ids64          = a->id_dtype == WHOLEMEMORY_DT_INT64 ? 1 : 0;
  p.begin          = a->entity_begin;
  p.end            = a->entity_end;
  p.filter_row_ptr = a->filter_row_ptr;
  p.row_ptr64      = a->filter_row_ptr_dtype == WHOLEMEMORY_DT_INT64 ? 1 : 0;
  p.filter_ids     = a->filter_ids;
  p.M              = a->n_filter;
  p.thr            = a->thr;
  p.greater        = a->greater;
  p.equal          = a->equal;
  return p;
}

bool args_ok(const wm_rank_args* a)
{
  return a->measure >= 0 && a->measure < kRankMeasures && rank_sizes_ok(a->n_queries, a->dim) && a->entity_begin >= 0 &&
         a->entity_begin <= a->entity_end && a->entity_end <= a->table_rows && a->query_stride >= a->dim &&
         (a->id_dtype == WHOLEMEMORY_DT_INT || a->id_dtype == WHOLEMEMORY_DT_INT64);
}

// every row start of the table and of the queries 16-byte aligned, and a row a whole number of 16-byte pieces?
bool quads_ok(const wm_rank_args* a)
{
  if (a->dim % 4 != 0 || a->table_stride % 4 != 0 || a->table_storage_offset % 4 != 0 || a->query_stride % 4 != 0 ||
      reinterpret_cast<uintptr_t>(a->query) % 16 != 0)
    return false;
  const wholememory_gref_t& g = a->gref;
  if (g.stride == 0) return reinterpret_cast<uintptr_t>(g.pointer) % 16 == 0;
  if (g.same_chunk) return g.stride % 16 == 0;   // (the per-rank bases are allocations)
  gref_host_tables t;
  if (!lookup_gref_tables(g.pointer, &t) || t.world_size != g.world_size) return false;
  for (int r = 0; r < t.world_size; r++)
    if (t.rank_offsets[r] % 16 != 0 || reinterpret_cast<uintptr_t>(t.rank_ptrs[r]) % 16 != 0) return false;
  return true;
}

#define WM_RANK_BY_MEASURE(LAUNCH_)   \
  do {                                \
    if (a->measure == 0) LAUNCH_(0);  \
    else if (a->measure == 1) LAUNCH_(1); \
    else LAUNCH_(2);                  \
  } while (0)

}  // namespace

int hip_rank_threshold(const wm_rank_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!args_ok(a)) return -1;
  if (a->n_queries == 0) return 0;
  const rank_params p = make_params(a);
#define WM_RANK_THR(M_) \
  hipLaunchKernelGGL((rank_threshold_kernel<M_>), dim3(blocks_for(p.B, kRkBlock)), dim3(kRkBlock), 0, stream, p)
  WM_RANK_BY_MEASURE(WM_RANK_THR);
#undef WM_RANK_THR
  return rc_last();
}

int hip_rank_sweep(const wm_rank_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!args_ok(a)) return -1;
  if (a->n_queries == 0 || a->entity_begin == a->entity_end) return 0;
  const rank_params p    = make_params(a);
  const int64_t n_etiles = (p.end - p.begin + kRankEntityTile - 1) / kRankEntityTile;
  const int64_t n_qtiles = (p.B + kRankQueryTile - 1) / kRankQueryTile;
  const int64_t n_tiles  = n_etiles * n_qtiles;
  const bool quads       = quads_ok(a);
#define WM_RANK_SWEEP(M_)                                                                                              \
  do {                                                                                                                 \
    if (quads)                                                                                                         \
      hipLaunchKernelGGL((rank_sweep_kernel<M_, 4>), dim3(blocks_for(n_tiles, 1)), dim3(kRkBlock), 0, stream, p, n_qtiles, \
                         n_tiles);                                                                                     \
    else                                                                                                               \
      hipLaunchKernelGGL((rank_sweep_kernel<M_, 1>), dim3(blocks_for(n_tiles, 1)), dim3(kRkBlock), 0, stream, p, n_qtiles, \
                         n_tiles);                                                                                     \
  } while (0)
  WM_RANK_BY_MEASURE(WM_RANK_SWEEP);
#undef WM_RANK_SWEEP
  return rc_last();
}

int hip_rank_filter(const wm_rank_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!args_ok(a)) return -1;
  if (a->filter_row_ptr == nullptr || a->n_filter == 0 || a->n_queries == 0 || a->entity_begin == a->entity_end) return 0;
  if (a->filter_ids == nullptr || a->n_filter < 0) return -1;
  const rank_params p = make_params(a);
#define WM_RANK_FILTER(M_) \
  hipLaunchKernelGGL((rank_filter_kernel<M_>), dim3(blocks_for(p.M, kRkBlock)), dim3(kRkBlock), 0, stream, p)
  WM_RANK_BY_MEASURE(WM_RANK_FILTER);
#undef WM_RANK_FILTER
  return rc_last();
}

}  // namespace wm
