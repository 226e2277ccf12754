// wholegraph_amd — `rank_rows` (wholegraph_amd_ext.h section 2w) on gfx950: per query, how many rows of a WholeMemory table
// score above, and exactly, the score of the query's target row. The evaluation of every embedding model of the library
// (filtered MRR / Hits@k of KGEModel), without the [B, N] score matrix.
//
// The contract fixes the arithmetic: one fp32 accumulator per (query, row), the columns in ascending order, every operation
// rounded on its own. rank_step (rank_tile.cuh) is that step; the three passes call it, so a row scores the same bits wherever it is scored.
// MFMA cannot keep that order, so the sweep is a register-tiled VALU kernel.
//
//   threshold  one lane per query: thr[b] = score(b, target[b]), NaN for a target outside the table; greater / equal start at
//              0 (-1 for such a target). No memset: the outputs are cleared here.
//   sweep      a workgroup of 256 lanes owns kRankEntityTile = 256 rows x kRankQueryTile = 64 queries and scores them with
//              the staged tile walk of rank_tile.cuh (shared with kernels/topk.hip: LDS staging at a pitch of 36 floats,
//              8 x 8 accumulators a lane). After the last slice a lane compares its pairs with thr, leaves out the target
//              and the rows past the range, the 32 lanes of a query add their counts with shuffles, and one lane adds them
//              to greater / equal with an integer atomic (the order of integer adds does not matter; a partials buffer
//              would be tiles x B x 16 bytes). The grid walks (row tile, query tile) pairs, query tiles fastest, so that
//              the workgroups resident together read the same table rows; it is sized by blocks_for and strides.
//   filter     one lane per entry of the filter block: the query it belongs to (a search of filter_row_ptr), the score of
//              its row, and one taken from greater or equal where the sweep counted that row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../rank.hpp"
#include "agg_common.cuh"
#include "device_common.cuh"
#include "gref_view.cuh"
#include "rank_tile.cuh"

namespace wm {
namespace {

struct rank_params : rank_operands {
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

template <int MEASURE, int VEC>
__global__ __launch_bounds__(kRkBlock) void rank_sweep_kernel(rank_params p, int64_t n_qtiles, int64_t n_tiles)
{
  __shared__ rank_tile_lds lds;
  const int tid = threadIdx.x;
  const int tx = tid % kRkTx, ty = tid / kRkTx;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t e0 = p.begin + (tile / n_qtiles) * kRankEntityTile;
    const int64_t b0 = (tile % n_qtiles) * kRankQueryTile;
    float acc[kRkRq][kRkRe];
    rank_tile_walk<MEASURE, VEC>(p, e0, p.end, b0, lds, acc);
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
  const bool quads       = rank_quads_ok(a->gref, a->dim, a->table_stride, a->table_storage_offset, a->query, a->query_stride);
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
