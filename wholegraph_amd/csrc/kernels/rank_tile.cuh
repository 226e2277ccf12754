// wholegraph_amd — the score of wholegraph_amd_ext.h sections 2w and 2x and the staged tile walk that computes it, shared by
// kernels/rank.hip (`rank_rows`) and kernels/topk.hip (`topk_rows`): both ops score a (query, row) pair with the same step
// function in the same column order, so a row gets the same bits in both.
//
// The contract fixes the arithmetic: one fp32 accumulator per (query, row), the columns in ascending order, every operation
// rounded on its own. rank_step is that step. MFMA cannot keep that order, so the walk is a register-tiled VALU loop.
//
// rank_tile_walk: a workgroup of 256 lanes scores kRankEntityTile = 256 rows against kRankQueryTile = 64 queries and walks the
// columns in slices of kRankSlice = 32. Per slice it stages both tiles in LDS, row-major with a row pitch of 36 floats: a
// lane's 16-byte store and its 16-byte read of 4 columns of one row start at bank 4 * row mod 32 (36 r mod 64 with 64 banks:
// 16 consecutive rows cover them once), so neither conflicts. Table rows are loaded 16 bytes a lane, 8 lanes a row slice (one
// 128-byte line); their addresses are resolved once per row and tile through the chunked view and kept in LDS. Lane (tx, ty),
// tx = lane % 32, ty = lane / 32, holds the 8 x 8 accumulators of rows tx + 32 i and queries ty + 8 j: a wave reads two query
// rows (a broadcast each) and 32 consecutive table rows per 16-byte read, 16 reads per 4 columns and 64 pairs. Columns past F
// are staged as +0.0 in both tiles: they add +0.0 in every measure, so any F >= 1 is served. The walk ends behind a barrier:
// the staging arrays are free when it returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../rank.hpp"
#include "device_common.cuh"
#include "gref_view.cuh"

namespace wm {

constexpr int kRkBlock = 256;
constexpr int kRkTx    = 32;                        // lanes along the table rows
constexpr int kRkTy    = kRkBlock / kRkTx;          // lanes along the queries
constexpr int kRkRe    = kRankEntityTile / kRkTx;   // table rows of a lane
constexpr int kRkRq    = kRankQueryTile / kRkTy;    // queries of a lane
constexpr int kRkPitch = kRankSlice + 4;            // floats between two rows of a staged tile
constexpr int kRkQuads = kRankSlice / 4;            // 16-byte pieces of a row slice
static_assert(kRkRe == 8 && kRkRq == 8, "a lane holds 8 x 8 accumulators");
static_assert(kRankEntityTile == kRkBlock, "a lane resolves the address of one table row per tile");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the table and the queries of both ops: the first fields of their kernel parameters
struct rank_operands {
  gref_view table;
  int64_t table_rows, stride, offset;   // elements
  int64_t F;
  const float* query;
  int64_t query_stride, B;
};

// the LDS of a tile walk: 36 KB + 9 KB + 2 KB
struct rank_tile_lds {
  __attribute__((aligned(16))) float es[kRankEntityTile * kRkPitch];
  __attribute__((aligned(16))) float qs[kRankQueryTile * kRkPitch];
  const float* erow[kRankEntityTile];
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

__device__ __forceinline__ const float* table_row(const rank_operands& p, int64_t e)
{
  return gref_address<float>(p.table, p.offset + e * p.stride);
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

// acc[j][i] = the finished accumulator of query b0 + ty + 8 j against row e0 + tx + 32 i (rows from `end` on and queries from
// B on are staged as +0.0: their accumulators mean nothing). All 256 lanes call this together
template <int MEASURE, int VEC>
__device__ __forceinline__ void rank_tile_walk(const rank_operands& p, int64_t e0, int64_t end, int64_t b0, rank_tile_lds& s,
                                               float (&acc)[kRkRq][kRkRe])
{
  const int tid = threadIdx.x;
  const int tx = tid % kRkTx, ty = tid / kRkTx;
  {
    const int64_t e = e0 + tid;   // (kRankEntityTile == kRkBlock: a row per lane)
    s.erow[tid]     = e < end ? table_row(p, e) : nullptr;
  }
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
      *reinterpret_cast<f32x4*>(&s.es[r * kRkPitch + c]) = load_quad<VEC>(s.erow[r], k0 + c, p.F);
    }
#pragma unroll
    for (int n = 0; n < kRankQueryTile * kRkQuads / kRkBlock; ++n) {
      const int l = tid + n * kRkBlock;
      const int r = l / kRkQuads, c = (l % kRkQuads) * 4;
      const int64_t b = b0 + r;
      *reinterpret_cast<f32x4*>(&s.qs[r * kRkPitch + c]) =
        load_quad<VEC>(b < p.B ? p.query + b * p.query_stride : nullptr, k0 + c, p.F);
    }
    __syncthreads();
    const int64_t left = p.F - k0;
    const int kend     = left < kRankSlice ? static_cast<int>((left + 3) & ~int64_t(3)) : kRankSlice;
    for (int kk = 0; kk < kend; kk += 4) {
      f32x4 ev[kRkRe], qv[kRkRq];
#pragma unroll
      for (int i = 0; i < kRkRe; ++i) ev[i] = *reinterpret_cast<const f32x4*>(&s.es[(tx + kRkTx * i) * kRkPitch + kk]);
#pragma unroll
      for (int j = 0; j < kRkRq; ++j) qv[j] = *reinterpret_cast<const f32x4*>(&s.qs[(ty + kRkTy * j) * kRkPitch + kk]);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < kRkRq; ++j)
#pragma unroll
          for (int i = 0; i < kRkRe; ++i) acc[j][i] = rank_step<MEASURE>(acc[j][i], qv[j][c], ev[i][c]);
    }
    __syncthreads();
  }
}

// every row start of the table and of the queries 16-byte aligned, and a row a whole number of 16-byte pieces? (host)
inline bool rank_quads_ok(const wholememory_gref_t& g, int64_t dim, int64_t table_stride, int64_t table_storage_offset,
                          const float* query, int64_t query_stride)
{
  if (dim % 4 != 0 || table_stride % 4 != 0 || table_storage_offset % 4 != 0 || query_stride % 4 != 0 ||
      reinterpret_cast<uintptr_t>(query) % 16 != 0)
    return false;
  if (g.stride == 0) return reinterpret_cast<uintptr_t>(g.pointer) % 16 == 0;
  if (g.same_chunk) return g.stride % 16 == 0;   // (the per-rank bases are allocations)
  gref_host_tables t;
  if (!lookup_gref_tables(g.pointer, &t) || t.world_size != g.world_size) return false;
  for (int r = 0; r < t.world_size; r++)
    if (t.rank_offsets[r] % 16 != 0 || reinterpret_cast<uintptr_t>(t.rank_ptrs[r]) % 16 != 0) return false;
  return true;
}

}  // namespace wm
