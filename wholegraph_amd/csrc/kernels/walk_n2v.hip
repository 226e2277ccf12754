// wholegraph_amd — node2vec (p, q) second-order walks over a CSR graph held in WholeMemory (gfx950 HIP; wholegraph_amd_ext.h
// section 2n). The walk of walk.hip's weighted kernel — a GROUP of kN2vGroup lanes per walk, the lanes stride over the row of
// the current node v, every neighbour j gets the A-Res key of its own stream, a butterfly leaves the winner in every lane —
// with one thing added: at a step t >= 1 the weight of neighbour x = col_ind[row_ptr[v] + j] is multiplied by a bias that
// depends on where x stands to the previous node u (x == u: 1 / p; x in u's row: 1; else 1 / q; ../walk_n2v.hpp).
//   - The walk keeps u and the bounds of u's row in registers: they were read one step earlier, when u was v.
//   - A lane loads the col_ind entries (and weights) of its next kN2vBatch neighbours back to back, then classifies them.
//   - "x in u's row" is answered on one of two routes, chosen by a kernel argument (wave-uniform): a private binary search per
//     lane when the caller promises ascending rows (at most 32 dependent reads), else a scan of u's row that the group does
//     TOGETHER — each round a lane loads one of the next kN2vGroup entries and the group passes them round by shuffles,
//     every lane comparing against its own x — so the row is read once per group, not once per lane.
//   - Nothing second-order runs at t = 0, and no search runs when 1 / q == 1.0f (the answer would not change the bias).
//   - The winning lane holds the winner's x, which rides through the butterfly: col_ind is not read again.
// The shuffles sit in loops whose trip counts (deg(v), deg(u)) are the same in all lanes of a group; the groups of a wave only
// read their own lanes. No atomics, no LDS, no scratch; every loop is bounded by L, deg(v) or deg(u). x is compared, never
// used as an index before it is chosen and range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../backend.hpp"
#include "../pcg.hpp"
#include "../walk_n2v.hpp"
#include "walk_common.cuh"

namespace wm {
namespace {

constexpr int kN2vBlock = 256;  // lanes per block
// lanes per walk. Measured on the papers100M-shaped bench graph with sorted rows (100 k walks of 80 steps, (p, q) = (0.25, 4), with
// weights): search route 8 lanes 5.10 ms, 16 lanes 5.03 ms, 32 lanes 6.24 ms; scan route 6.34, 4.95, 5.66 ms.
// The result does not depend on it.
constexpr int kN2vGroup = 16;
constexpr int kN2vBatch = 2;    // neighbours a lane loads before it classifies them

struct n2v_params {
  walk_params walk;
  float inv_p, inv_q;
  int col_sorted;
};

// WT = void: no weight tensor, every edge has weight 1.0f
template <typename IdT, typename ColT, typename WT, int G>
__global__ __launch_bounds__(kN2vBlock) void n2v_walk_kernel(n2v_params q)
{
  const walk_params& p = q.walk;
  const int64_t tid    = static_cast<int64_t>(blockIdx.x) * kN2vBlock + threadIdx.x;
  const int64_t w      = tid / G;
  const int gl         = static_cast<int>(threadIdx.x) & (G - 1);
  const bool live      = w < p.n;   // a group past the end sits out: the groups of a wave share the shuffles below
  const int L          = p.walk_length;
  ColT* out            = static_cast<ColT*>(p.out_walks) + (live ? w * (L + 1) : 0);
  int64_t* eout        = live && p.out_edge_ids != nullptr ? p.out_edge_ids + w * L : nullptr;
  const bool search    = q.inv_q != 1.0f;   // the same in every lane of the launch
  const bool sorted    = q.col_sorted != 0;
  int64_t v            = live ? walk_start<IdT>(p, w) : -1;
  int64_t u = -1, us = 0, ue = 0;   // the previous node and its row
  if (live && gl == 0) out[0] = static_cast<ColT>(v);
  for (int t = 0; t < L; t++) {
    int64_t s = 0;
    int deg   = 0;
    if (v >= 0) (void)walk_row(p, v, &s, &deg);
    const bool second = t > 0;   // (deg > 0 at t > 0 means the last step was taken: u is a node)
    float best_key    = 0.f;
    int best_j        = -1;
    ColT best_x       = ColT(-1);
    for (int j0 = 0; j0 < deg; j0 += G * kN2vBatch) {   // j ascending in a lane
      ColT x[kN2vBatch];
      float wt[kN2vBatch];
#pragma unroll
      for (int b = 0; b < kN2vBatch; b++) {
        const int j = j0 + b * G + gl;
        x[b]        = ColT(-1);
        wt[b]       = 0.f;
        if (j < deg) {
          x[b] = gref_load<ColT>(p.g.col_ptr, p.g.col_off + s + j);
          if constexpr (std::is_void<WT>::value) {
            wt[b] = 1.0f;
          } else {
            wt[b] = static_cast<float>(gref_load<WT>(p.wt.weight_ptr, p.wt.weight_off + s + j));
          }
        }
      }
#pragma unroll
      for (int b = 0; b < kN2vBatch; b++) {
        const int j = j0 + b * G + gl;
        bool in_row = false;
        if (second && search && j0 + b * G < deg) {   // the same in every lane of the group
          if (sorted) {
            if (j < deg && static_cast<int64_t>(x[b]) != u)
              in_row = n2v_row_has_sorted(
                [&](int64_t pos) { return static_cast<int64_t>(gref_load<ColT>(p.g.col_ptr, p.g.col_off + pos)); }, us, ue,
                static_cast<int64_t>(x[b]));
          } else {
            in_row = csr_group_scan<ColT, G>(p.g, us, ue, x[b], gl);
          }
        }
        if (j < deg) {
          const float bias = second ? n2v_bias(static_cast<int64_t>(x[b]), u, in_row, q.inv_p, q.inv_q) : 1.0f;
          const float ew   = n2v_effective_weight(wt[b], bias);
          if (walk_weight_eligible(ew)) {
            const float key = walk_weighted_key(p.seed, static_cast<uint64_t>(w), static_cast<uint64_t>(L),
                                                static_cast<uint64_t>(t), static_cast<uint64_t>(j), ew);
            if (walk_key_replaces(key, j, best_key, best_j)) best_key = key, best_j = j, best_x = x[b];
          }
        }
      }
    }
#pragma unroll
    for (int d = G >> 1; d > 0; d >>= 1) {
      const float ok = __shfl_xor(best_key, d, 64);
      const int oj   = __shfl_xor(best_j, d, 64);
      const ColT ox  = __shfl_xor(best_x, d, 64);
      if (oj >= 0 && walk_key_replaces(ok, oj, best_key, best_j)) best_key = ok, best_j = oj, best_x = ox;
    }
    int64_t next = -1, eid = -1;
    if (best_j >= 0) {
      const int64_t c = static_cast<int64_t>(best_x);
      if (c >= 0 && c < p.g.n_nodes) next = c, eid = s + best_j;
    }
    if (live && gl == 0) {
      out[t + 1] = static_cast<ColT>(next);
      if (eout != nullptr) eout[t] = eid;
    }
    u = v, us = s, ue = s + deg;
    v = next;
  }
}

template <typename IdT, typename ColT, typename WT>
int launch_n2v(const n2v_params& q, hipStream_t stream)
{
  if (q.walk.n == 0) return 0;
  constexpr int per_block = kN2vBlock / kN2vGroup;
  const unsigned blocks   = static_cast<unsigned>((q.walk.n + per_block - 1) / per_block);   // n < 2^30: below 2^26 blocks
  hipLaunchKernelGGL((n2v_walk_kernel<IdT, ColT, WT, kN2vGroup>), dim3(blocks), dim3(kN2vBlock), 0, stream, q);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int hip_walk_node2vec(const wm_n2v_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a == nullptr || !walk_args_ok(&a->walk)) return -1;
  const float big = 3.402823466e+38f;
  if (!(a->inv_p > 0.0f && a->inv_p <= big && a->inv_q > 0.0f && a->inv_q <= big)) return -1;
  n2v_params q{};
  q.walk  = walk_params_of(&a->walk);
  q.inv_p = a->inv_p, q.inv_q = a->inv_q, q.col_sorted = a->col_sorted;
  const wm_walk_args& w = a->walk;
  if (w.weight_dtype == WHOLEMEMORY_DT_UNKNOWN)
    return dispatch_id_col(w.start_dtype, w.col_dtype,
                           [&](auto id, auto col) { return launch_n2v<decltype(id), decltype(col), void>(q, stream); });
  return dispatch_id_col_weight(w.start_dtype, w.col_dtype, w.weight_dtype, [&](auto id, auto col, auto wt) {
    return launch_n2v<decltype(id), decltype(col), decltype(wt)>(q, stream);
  });
}

}  // namespace wm
