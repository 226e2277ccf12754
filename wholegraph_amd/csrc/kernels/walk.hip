// wholegraph_amd — random walks over a CSR graph held in WholeMemory (gfx950 HIP; wholegraph_amd_ext.h section 2m).
//
// A walk is a chain of dependent random reads: row_ptr[v] and row_ptr[v + 1], then one col_ind entry, which is the v of
// the next step. A step costs two memory round trips (about 900 cycles each when they miss to HBM on an idle chip, more
// under load: DESIGN.md 3.17 has the measured time per step), so what the kernels can do is keep many walks in flight and
// ask for nothing else. The output shape [n, L + 1] is known before the launch, so the whole batch is ONE launch that
// allocates nothing and reads nothing back, however long the walks are.
//   uniform:  one LANE per walk. A lane keeps its walk's generator and current node in registers (26 VGPRs: eight waves per
//             SIMD, 2048 walks resident per CU, half a million on the chip — batches up to that size are resident at once,
//             and from about 65 k walks on every SIMD has a wave to run). The two row_ptr reads of a step are issued
//             together, the col_ind read depends on both. Grid = ceil(n / block): no cap and no stride loop, a lane's walk
//             number is its global thread number, which is also the number of its random stream.
//   weighted: a GROUP of kWalkGroup lanes per walk. The lanes stride over the row; each loads a weight, forms the
//             A-Res key of that neighbour from the neighbour's own stream and keeps its best (key, j); a butterfly of
//             shuffles leaves the winner — largest key, ties to the lowest j — in every lane of the group, and only the
//             winner's col_ind entry is read. The result is a function of (seed, walk, step, neighbour) alone: neither
//             the group size nor the launch geometry enters it.
// Every loop is bounded by L or by a row's degree; no atomics, no waiting on other lanes' progress, no scratch, no LDS.
// An id read from col_ind indexes row_ptr in the next step, so it is range-checked before it becomes the current node:
// a damaged graph ends a walk (-1 from there on), it does not read out of bounds. For the same reason a row whose bounds
// do not lie in [0, n_edges] is not stepped from.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../pcg.hpp"
#include "walk_common.cuh"

namespace wm {
namespace {

constexpr int kWalkBlock = 128;   // uniform: walks per block (a 100 k-walk batch is 782 blocks: three per CU, spread over its SIMDs)
constexpr int kWalkWBlock = 256;  // weighted: lanes per block
// weighted: lanes per walk. Measured on the papers100M-shaped bench graph (degrees 0 .. 58, 100 k walks of 80 steps; DESIGN.md
// 3.17): 8 lanes 2.35 ms, 16 lanes 2.25 ms, 32 lanes 2.53 ms. The result does not depend on it.
constexpr int kWalkGroup = 16;

template <typename IdT, typename ColT>
__global__ __launch_bounds__(kWalkBlock) void rwalk_uniform_kernel(walk_params p)
{
  const int64_t w = static_cast<int64_t>(blockIdx.x) * kWalkBlock + threadIdx.x;
  if (w >= p.n) return;
  const int L   = p.walk_length;
  ColT* out     = static_cast<ColT*>(p.out_walks) + w * (L + 1);
  int64_t* eout = p.out_edge_ids != nullptr ? p.out_edge_ids + w * L : nullptr;
  int64_t v     = walk_start<IdT>(p, w);
  out[0]        = static_cast<ColT>(v);
  pcg32 rng     = walk_stream(p.seed, static_cast<uint64_t>(w), 0);
  for (int t = 0; t < L; t++) {
    const uint32_t r = rng.next_u32();   // step t takes the t-th draw whether or not the walk still runs
    int64_t next = -1, eid = -1;
    if (v >= 0) {
      int64_t s;
      int deg;
      if (walk_row(p, v, &s, &deg)) {
        const int64_t pos = s + walk_uniform_pick(r, static_cast<uint32_t>(deg));
        const int64_t c   = static_cast<int64_t>(gref_load<ColT>(p.g.col_ptr, p.g.col_off + pos));
        if (c >= 0 && c < p.g.n_nodes) next = c, eid = pos;
      }
    }
    out[t + 1] = static_cast<ColT>(next);
    if (eout != nullptr) eout[t] = eid;
    v = next;
  }
}

template <typename IdT, typename ColT, typename WT, int G>
__global__ __launch_bounds__(kWalkWBlock) void rwalk_weighted_kernel(walk_params p)
{
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kWalkWBlock + threadIdx.x;
  const int64_t w   = tid / G;
  const int gl      = static_cast<int>(threadIdx.x) & (G - 1);
  const bool live   = w < p.n;   // a group past the end sits out: the groups of a wave share the shuffles below
  const int L       = p.walk_length;
  ColT* out         = static_cast<ColT*>(p.out_walks) + (live ? w * (L + 1) : 0);
  int64_t* eout     = live && p.out_edge_ids != nullptr ? p.out_edge_ids + w * L : nullptr;
  int64_t v         = live ? walk_start<IdT>(p, w) : -1;
  if (live && gl == 0) out[0] = static_cast<ColT>(v);
  for (int t = 0; t < L; t++) {
    int64_t s = 0;
    int deg   = 0;
    if (v >= 0) (void)walk_row(p, v, &s, &deg);
    float best_key = 0.f;
    int best_j     = -1;
    for (int j = gl; j < deg; j += G) {   // j ascending in a lane: the comparison alone keeps the lowest j of equal keys
      const float wt = static_cast<float>(gref_load<WT>(p.wt.weight_ptr, p.wt.weight_off + s + j));
      if (walk_weight_eligible(wt)) {
        const float key = walk_weighted_key(p.seed, static_cast<uint64_t>(w), static_cast<uint64_t>(L), static_cast<uint64_t>(t),
                                            static_cast<uint64_t>(j), wt);
        if (walk_key_replaces(key, j, best_key, best_j)) best_key = key, best_j = j;
      }
    }
#pragma unroll
    for (int d = G >> 1; d > 0; d >>= 1) {
      const float ok = __shfl_xor(best_key, d, 64);
      const int oj   = __shfl_xor(best_j, d, 64);
      if (oj >= 0 && walk_key_replaces(ok, oj, best_key, best_j)) best_key = ok, best_j = oj;
    }
    int64_t next = -1, eid = -1;
    if (best_j >= 0) {   // (every lane of the group reads the one address)
      const int64_t pos = s + best_j;
      const int64_t c   = static_cast<int64_t>(gref_load<ColT>(p.g.col_ptr, p.g.col_off + pos));
      if (c >= 0 && c < p.g.n_nodes) next = c, eid = pos;
    }
    if (live && gl == 0) {
      out[t + 1] = static_cast<ColT>(next);
      if (eout != nullptr) eout[t] = eid;
    }
    v = next;
  }
}

template <typename IdT, typename ColT>
int launch_uniform(const walk_params& p, hipStream_t stream)
{
  if (p.n == 0) return 0;
  const unsigned blocks = static_cast<unsigned>((p.n + kWalkBlock - 1) / kWalkBlock);
  hipLaunchKernelGGL((rwalk_uniform_kernel<IdT, ColT>), dim3(blocks), dim3(kWalkBlock), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename IdT, typename ColT, typename WT>
int launch_weighted(const walk_params& p, hipStream_t stream)
{
  if (p.n == 0) return 0;
  constexpr int per_block = kWalkWBlock / kWalkGroup;
  const unsigned blocks   = static_cast<unsigned>((p.n + per_block - 1) / per_block);   // n < 2^30: below 2^26 blocks
  hipLaunchKernelGGL((rwalk_weighted_kernel<IdT, ColT, WT, kWalkGroup>), dim3(blocks), dim3(kWalkWBlock), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int hip_walk_uniform(const wm_walk_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!walk_args_ok(a)) return -1;
  const walk_params p = walk_params_of(a);
  return dispatch_id_col(a->start_dtype, a->col_dtype,
                         [&](auto id, auto col) { return launch_uniform<decltype(id), decltype(col)>(p, stream); });
}

int hip_walk_weighted(const wm_walk_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!walk_args_ok(a)) return -1;
  const walk_params p = walk_params_of(a);
  return dispatch_id_col_weight(a->start_dtype, a->col_dtype, a->weight_dtype, [&](auto id, auto col, auto wt) {
    return launch_weighted<decltype(id), decltype(col), decltype(wt)>(p, stream);
  });
}

}  // namespace wm
