// wholegraph_amd — `topk_rows` (wholegraph_amd_ext.h section 2x) on gfx950: per query, the k best rows of a WholeMemory table
// under the score of section 2w, higher first and the lower id first among equal scores, a filter block left out. What an
// embedding model is served with ("which k entities complete (h, r, ?)"), without the [B, N] score matrix.
//
// The score is rank_rows': rank_tile.cuh's step function and staged tile walk, so a row gets the same bits in both ops. The
// contract fixes an unfused column-ascending order of one fp32 accumulator, which MFMA cannot keep: no matrix instructions.
//
// A candidate is one 64-bit key: the high word an order-preserving map of the bits of s + 0.0f (which folds -0.0 into +0.0),
// the low word ~(e - entity_begin). A larger key is a better row and, on equal score, a lower id; keys of distinct rows are
// distinct, and 0 is no row's key (the map of -inf is 0x007fffff): the empty key. The answer is the set of the largest keys,
// so it depends on no order in which candidates meet.
//
//   sweep  a workgroup of 256 lanes owns one query tile (64 queries) and one of S row splits and walks the split's row tiles
//          (256 rows each) one after another. The running top of each query, its best kTopkMax = 64 keys so far in descending
//          order, lives in LDS (64 x 64 x 8 B = 32 KB); the key of a query's current 64th is the last of them. After a tile's
//          walk a lane holds 64 scores. In rounds: a lane compares each pending score's key with its query's 64th; a survivor
//          (not NaN, inside the range) takes a slot of the query's candidate buffer through an LDS counter and writes its
//          key there. A survivor without a slot stays pending. Behind a barrier each wave takes 16 of the queries: for a
//          query with candidates it loads the batch, one per lane, looks each up in the query's filter row (a binary search
//          per lane: the row is ascending; once per candidate, in one place of the code) and empties the filtered ones,
//          merges the batch into the running top with top_merge<64> (top_merge.cuh) and clears the counter. Rounds repeat until no lane has a pending survivor: four on
//          the first tile of a split (every row survives an empty top), one later, where survivors are rare (about
//          64 ln(rows / 64) per query over a whole split). The candidate buffer (32 KB) lies over the table tile's staging
//          array, which is free between two walks. After the walk a lane turns its accumulators, in place, into the high
//          words of its keys (0: not or no longer a candidate), which is all the state the rounds keep; every loop over them
//          is unrolled, so they are never indexed by a register. After its last tile the workgroup writes its 64 keys per query
//          to the workspace [S, B, 64]. No global atomics.
//   merge  one wave per query: the S partial tops, each descending, merged with the same top_merge<64>; the first k keys are
//          decoded into ids (entity_begin added back) and scores, an empty key into -1 / NaN.
//
// S: the host wants two workgroups per CU (what the LDS allows) and has ceil(B / 64) query tiles, so S = ceil(2 CUs / query
// tiles), at most the number of row tiles. The grid is blocks_for((query tile, split) pairs) and strides over them, query
// tiles fastest, so that the workgroups resident together read the same table rows. S does not depend on the grid's cap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../rank.hpp"
#include "agg_common.cuh"
#include "device_common.cuh"
#include "gref_view.cuh"
#include "rank_tile.cuh"
#include "top_merge.cuh"

namespace wm {
namespace {

constexpr int kTkWaves        = kRkBlock / 64;
constexpr int kTkQueriesAWave = kRankQueryTile / kTkWaves;
static_assert(kTopkMax == 64, "a query's running top is one key per lane of a wave");
static_assert(kRankQueryTile * kTopkMax * sizeof(uint64_t) <= sizeof(rank_tile_lds::es), "the candidates lie over the table tile");

struct topk_params : rank_operands {
  int64_t begin, end;
  const void* filter_row_ptr;
  int row_ptr64;
  const void* filter_ids;
  int ids64;
  int64_t M;
  uint64_t* part;   // [S, B, kTopkMax]
};

struct topk_lds {
  rank_tile_lds tile;
  uint64_t top[kRankQueryTile * kTopkMax];   // the running top of query q: top[q * 64 ..], descending
  int cnt[kRankQueryTile];                   // candidates of query q this round (may pass 64: the rest stay pending)
};

// larger word <=> larger score (any two non-NaN floats), and back
__device__ __forceinline__ uint32_t score_word(float s)
{
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float word_score(uint32_t h)
{
  return __uint_as_float((h & 0x80000000u) ? (h ^ 0x80000000u) : ~h);
}

// is row e in query b's filter row? The row is ascending; its bounds are held to [0, M]
__device__ bool in_filter_row(const topk_params& p, int64_t b, int64_t e)
{
  if (p.filter_row_ptr == nullptr) return false;
  int64_t lo       = id_at(p.filter_row_ptr, p.row_ptr64, b);
  int64_t hi       = id_at(p.filter_row_ptr, p.row_ptr64, b + 1);
  lo               = lo < 0 ? 0 : lo;
  hi               = hi > p.M ? p.M : hi;
  const int64_t up = hi;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (id_at(p.filter_ids, p.ids64, mid) < e) lo = mid + 1;
    else hi = mid;
  }
  return lo < up && id_at(p.filter_ids, p.ids64, lo) == e;
}

template <int MEASURE, int VEC>
__global__ __launch_bounds__(kRkBlock) void topk_sweep_kernel(topk_params p, int64_t n_qtiles, int64_t n_etiles, int64_t n_splits)
{
  __shared__ topk_lds lds;
  uint64_t* cand = reinterpret_cast<uint64_t*>(lds.tile.es);   // [64 queries][64 slots], between two walks
  const int tid  = threadIdx.x;
  const int tx = tid % kRkTx, ty = tid / kRkTx;
  const int lane = tid % 64, wave = tid / 64;
  for (int64_t pair = blockIdx.x; pair < n_qtiles * n_splits; pair += gridDim.x) {
    const int64_t split  = pair / n_qtiles;
    const int64_t b0     = (pair % n_qtiles) * kRankQueryTile;
    const int64_t t_end  = (split + 1) * n_etiles / n_splits;
    for (int n = tid; n < kRankQueryTile * kTopkMax; n += kRkBlock) lds.top[n] = 0;
    if (tid < kRankQueryTile) lds.cnt[tid] = 0;
    __syncthreads();
    for (int64_t t = split * n_etiles / n_splits; t < t_end; ++t) {
      const int64_t e0 = p.begin + t * kRankEntityTile;
      float acc[kRkRq][kRkRe];
      rank_tile_walk<MEASURE, VEC>(p, e0, p.end, b0, lds.tile, acc);
      // the accumulators become the high words of the pairs' keys, 0 for a pair that is not a candidate (a NaN score, a row
      // past the range) or no longer one: the rounds below keep no other state per pair. A query past B is staged as zeros
      // and selects like any other; its top is never looked up in the filter and never written
      const uint32_t r0    = static_cast<uint32_t>(e0 - p.begin) + tx;   // row tx of the tile, counted from entity_begin
      const int rows_there = static_cast<int>(p.end - e0 < kRankEntityTile ? p.end - e0 : kRankEntityTile);
      uint32_t word[kRkRq][kRkRe];
#pragma unroll
      for (int i = 0; i < kRkRe; ++i) {
        const uint32_t there = tx + kRkTx * i < rows_there ? ~0u : 0u;
#pragma unroll
        for (int j = 0; j < kRkRq; ++j) {
          const float s = rank_score<MEASURE>(acc[j][i]) + 0.0f;
          word[j][i]    = (s == s ? score_word(s) : 0u) & there;
        }
      }
      bool more = true;
      while (__syncthreads_or(more)) {
        more = false;
#pragma unroll
        for (int j = 0; j < kRkRq; ++j) {
          const int q        = ty + kRkTy * j;
          const uint64_t kth = lds.top[q * kTopkMax + kTopkMax - 1];
#pragma unroll
          for (int i = 0; i < kRkRe; ++i) {
            const uint64_t key = (static_cast<uint64_t>(word[j][i]) << 32) | static_cast<uint32_t>(~(r0 + kRkTx * i));
            bool waits         = false;
            if (word[j][i] != 0 && key > kth) {
              const int slot = atomicAdd(&lds.cnt[q], 1);
              if (slot < kTopkMax) cand[q * kTopkMax + slot] = key;
              else waits = true;
            }
            if (!waits) word[j][i] = 0;
            more |= waits;
          }
        }
        __syncthreads();
        for (int qq = 0; qq < kTkQueriesAWave; ++qq) {
          const int q = wave * kTkQueriesAWave + qq;
          const int n = __builtin_amdgcn_readfirstlane(lds.cnt[q]);
          if (n == 0) continue;
          uint64_t batch = lane < n ? cand[q * kTopkMax + lane] : 0;
          if (batch != 0 && b0 + q < p.B && in_filter_row(p, b0 + q, p.begin + static_cast<uint32_t>(~static_cast<uint32_t>(batch)))) batch = 0;
          int gl = lane;   // opaque here: the 27 lane masks of the merge network are made where they are used, not kept in
          asm volatile("" : "+v"(gl));   // scalar registers across the tile walk (the resource report showed them spilled)
          lds.top[q * kTopkMax + lane] = top_merge<kTopkMax>(lds.top[q * kTopkMax + lane], batch, gl);
          if (lane == 0) lds.cnt[q] = 0;
        }
      }
    }
    for (int n = tid; n < kRankQueryTile * kTopkMax; n += kRkBlock) {
      const int64_t b = b0 + n / kTopkMax;
      if (b < p.B) p.part[(split * p.B + b) * kTopkMax + n % kTopkMax] = lds.top[n];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kRkBlock) void topk_merge_kernel(const uint64_t* part, int64_t n_splits, int64_t B, int k, int64_t begin,
                                                              int64_t* ids, int64_t ids_stride, float* scores, int64_t scores_stride)
{
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * kTkWaves + wave; b < B; b += static_cast<int64_t>(gridDim.x) * kTkWaves) {
    uint64_t top = part[b * kTopkMax + lane];
    for (int64_t s = 1; s < n_splits; ++s) top = top_merge<kTopkMax>(top, part[(s * B + b) * kTopkMax + lane], lane);
    if (lane < k) {
      const bool none              = top == 0;
      ids[b * ids_stride + lane]   = none ? -1 : begin + static_cast<int64_t>(~static_cast<uint32_t>(top));
      scores[b * scores_stride + lane] = none ? __builtin_nanf("") : word_score(static_cast<uint32_t>(top >> 32));
    }
  }
}

bool args_ok(const wm_topk_args* a)
{
  return a->measure >= 0 && a->measure < kRankMeasures && rank_sizes_ok(a->n_queries, a->dim) && a->entity_begin >= 0 &&
         a->entity_begin <= a->entity_end && a->entity_end <= a->table_rows && a->entity_end - a->entity_begin <= kTopkMaxRange &&
         a->query_stride >= a->dim && a->k >= 1 && a->k <= kTopkMax && a->ids_stride >= a->k && a->scores_stride >= a->k &&
         (a->filter_row_ptr == nullptr || (a->n_filter >= 0 && (a->n_filter == 0 || a->filter_ids != nullptr)));
}

int64_t tiles_of(int64_t n, int64_t tile) { return (n + tile - 1) / tile; }

// two workgroups per CU of the current device over the query tiles, at most one split per row tile, at least one
int64_t splits_of(const wm_topk_args* a)
{
  static int cus_of[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cus_of[dev] == 0) {
    hipDeviceProp_t prop;
    cus_of[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  (void)hipGetLastError();
  const int64_t n_qtiles = tiles_of(a->n_queries, kRankQueryTile), n_etiles = tiles_of(a->entity_end - a->entity_begin, kRankEntityTile);
  const int64_t want     = n_qtiles > 0 ? tiles_of(2 * cus_of[dev], n_qtiles) : 1;
  const int64_t s        = want < n_etiles ? want : n_etiles;
  return s < 1 ? 1 : s;
}

}  // namespace

size_t hip_topk_workspace_bytes(const wm_topk_args* a)
{
  if (!args_ok(a)) return 0;
  return static_cast<size_t>(splits_of(a)) * static_cast<size_t>(a->n_queries) * kTopkMax * sizeof(uint64_t);
}

int hip_topk_sweep(const wm_topk_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!args_ok(a)) return -1;
  if (a->n_queries == 0) return 0;
  if (a->workspace == nullptr) return -1;
  topk_params p{};
  p.table          = make_view(a->gref);
  p.table_rows     = a->table_rows;
  p.stride         = a->table_stride;
  p.offset         = a->table_storage_offset;
  p.F              = a->dim;
  p.query          = a->query;
  p.query_stride   = a->query_stride;
  p.B              = a->n_queries;
  p.begin          = a->entity_begin;
  p.end            = a->entity_end;
  p.filter_row_ptr = a->n_filter > 0 ? a->filter_row_ptr : nullptr;
  p.row_ptr64      = a->filter_row_ptr_dtype == WHOLEMEMORY_DT_INT64 ? 1 : 0;
  p.filter_ids     = a->filter_ids;
  p.ids64          = a->filter_ids_dtype == WHOLEMEMORY_DT_INT64 ? 1 : 0;
  p.M              = a->n_filter;
  p.part           = static_cast<uint64_t*>(a->workspace);
  const int64_t n_qtiles = tiles_of(p.B, kRankQueryTile), n_etiles = tiles_of(p.end - p.begin, kRankEntityTile);
  const int64_t n_splits = splits_of(a);
  const dim3 grid(blocks_for(n_qtiles * n_splits, 1));
  const bool quads = rank_quads_ok(a->gref, a->dim, a->table_stride, a->table_storage_offset, a->query, a->query_stride);
#define WM_TOPK_SWEEP(M_)                                                                                                      \
  do {                                                                                                                         \
    if (quads) hipLaunchKernelGGL((topk_sweep_kernel<M_, 4>), grid, dim3(kRkBlock), 0, stream, p, n_qtiles, n_etiles, n_splits); \
    else hipLaunchKernelGGL((topk_sweep_kernel<M_, 1>), grid, dim3(kRkBlock), 0, stream, p, n_qtiles, n_etiles, n_splits);       \
  } while (0)
  if (a->measure == 0) WM_TOPK_SWEEP(0);
  else if (a->measure == 1) WM_TOPK_SWEEP(1);
  else WM_TOPK_SWEEP(2);
#undef WM_TOPK_SWEEP
  return rc_last();
}

int hip_topk_merge(const wm_topk_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!args_ok(a)) return -1;
  if (a->n_queries == 0) return 0;
  if (a->workspace == nullptr || a->ids == nullptr || a->scores == nullptr) return -1;
  hipLaunchKernelGGL(topk_merge_kernel, dim3(blocks_for(a->n_queries, kTkWaves)), dim3(kRkBlock), 0, stream,
                     static_cast<const uint64_t*>(a->workspace), splits_of(a), a->n_queries, a->k, a->entity_begin, a->ids,
                     a->ids_stride, a->scores, a->scores_stride);
  return rc_last();
}

}  // namespace wm
