// wholegraph_amd — negative sampling over a CSR graph held in WholeMemory (gfx950 HIP; wholegraph_amd_ext.h section 2o): for
// every source node u, K nodes drawn uniformly or by degree that are not u and not in u's row, as ONE launch.
//   - A GROUP of kNegGroup lanes per source; lane gl owns the samples k = gl, gl + G, ... and takes them one pass after the
//     other. Sample (i, k) has its own stream, stream(seed, i * K + k, 0); attempt a takes its a-th 64-bit draw.
//   - A pass works in rounds: in round a every lane whose sample is still open forms its a-th candidate (../neg_sample.hpp),
//     range-checks it and compares it with u. A candidate that survives is looked up in u's row on one of two routes, chosen
//     by a kernel argument (wave-uniform): a private binary search per lane when the caller promises ascending rows, else a
//     scan of u's row that the group does TOGETHER — each trip a lane loads one of the next kNegGroup entries and the group
//     passes them round by shuffles, every lane comparing against its own candidate — so the row is read once per group and
//     round, not once per lane. A group none of whose lanes has a surviving candidate skips the scan.
//   - The rounds of a pass end when a wave-wide vote finds no open sample. Without exclude & 1 no row is read at all.
// The shuffles sit in a loop whose trip count (deg(u)) is the same in all lanes of a group, entered by all of them or none;
// the groups of a wave only read their own lanes, and a group past the end sits out but takes part. No atomics, no LDS, no
// scratch; every loop is bounded by T, K or deg(u). A candidate is compared, never used as an index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../neg_sample.hpp"
#include "../pcg.hpp"
#include "csr_view.cuh"

namespace wm {
namespace {

constexpr int kNegBlock = 256;  // lanes per block
// lanes per source. Measured on the papers100M-shaped bench graph with sorted rows (100 k sources, exclude = 3, 8 tries;
// DESIGN.md 3.19): uniform, K = 5, scan route 8 lanes 0.028 ms, 16 lanes 0.047 ms, 32 lanes 0.091 ms; by degree, K = 20, search
// route 0.085, 0.116, 0.159 ms; 8 is ahead in all eight forms. The result does not depend on it.
constexpr int kNegGroup = 8;

struct neg_params {
  csr_view g;
  const void* src;
  int64_t n;
  int num_negatives, mode, exclude, max_tries, col_sorted;
  uint64_t seed;
  void* out;  // ColT [n, K]
};

template <typename IdT, typename ColT, int G>
__global__ __launch_bounds__(kNegBlock) void neg_sample_kernel(neg_params p)
{
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kNegBlock + threadIdx.x;
  const int64_t i   = tid / G;
  const int gl      = static_cast<int>(threadIdx.x) & (G - 1);
  const int first   = static_cast<int>(threadIdx.x) & 63 & ~(G - 1);   // the group's first lane in its wave
  const bool live   = i < p.n;   // a group past the end sits out: the groups of a wave share the vote and the shuffles below
  const int K = p.num_negatives, T = p.max_tries;
  const bool edges  = (p.exclude & 1) != 0;   // the same in every lane of the launch, as is sorted
  const bool sorted = p.col_sorted != 0;
  int64_t u         = live ? static_cast<int64_t>(static_cast<const IdT*>(p.src)[i]) : -1;
  if (u < 0 || u >= p.g.n_nodes) u = -1;
  int64_t s = 0, e = 0;   // the row that excludes its entries; empty where the bounds are not a row
  if (edges && u >= 0) {
    s = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + u);
    e = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + u + 1);
    if (!neg_row_valid(s, e, p.g.n_edges)) s = e = 0;
  }
  ColT* out       = static_cast<ColT*>(p.out) + (live ? i * K : 0);
  const auto load = [&](int64_t pos) { return static_cast<int64_t>(gref_load<ColT>(p.g.col_ptr, p.g.col_off + pos)); };
  for (int k0 = 0; k0 < K; k0 += G) {
    const int k     = k0 + gl;
    const bool mine = live && k < K;
    bool open       = mine && u >= 0;
    int64_t result  = -1;
    pcg32 g;
    if (open) g = walk_stream(p.seed, static_cast<uint64_t>(i) * static_cast<uint64_t>(K) + static_cast<uint64_t>(k), 0);
    for (int a = 0; a < T; a++) {
      if (!__any(open)) break;
      int64_t c = -1;
      bool kept = false;   // the candidate is in range and is not an excluded source
      if (open) {
        c    = neg_candidate(load, g.next_u64(), p.mode, p.g.n_nodes, p.g.n_edges);
        kept = !neg_rejected_early(c, u, p.g.n_nodes, p.exclude);
      }
      bool in_row = false;
      if (edges) {
        const bool look = kept && e > s;
        if (sorted) {
          if (look) in_row = n2v_row_has_sorted(load, s, e, c);
        } else {
          const unsigned long long vote = __ballot(look);
          if (((vote >> first) & ((1ull << G) - 1ull)) != 0) in_row = csr_group_scan<ColT, G>(p.g, s, e, c, gl);
        }
      }
      if (kept && !in_row) result = c, open = false;
    }
    if (mine) out[k] = static_cast<ColT>(result);
  }
}

template <typename IdT, typename ColT>
int launch_neg(const neg_params& p, hipStream_t stream)
{
  if (p.n == 0) return 0;
  constexpr int per_block = kNegBlock / kNegGroup;
  const unsigned blocks   = static_cast<unsigned>((p.n + per_block - 1) / per_block);   // n < 2^31: below 2^28 blocks
  hipLaunchKernelGGL((neg_sample_kernel<IdT, ColT, kNegGroup>), dim3(blocks), dim3(kNegBlock), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int hip_negative_sample(const wm_neg_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  // what the launcher refuses (-1, nothing queued): the host side has answered all of it before it gets here
  if (a == nullptr || a->n < 0 || a->n_nodes < 0 || a->n_edges < 0) return -1;
  if (!neg_scalars_ok(a->num_negatives, a->mode, a->exclude, a->max_tries)) return -1;
  if (a->n * static_cast<int64_t>(a->num_negatives) >= (INT64_C(1) << 31)) return -1;
  if (a->n > 0 && (a->src == nullptr || a->out == nullptr)) return -1;
  neg_params p{};
  p.g   = csr_view_of(*a);
  p.src = a->src, p.n = a->n;
  p.num_negatives = a->num_negatives, p.mode = a->mode, p.exclude = a->exclude, p.max_tries = a->max_tries;
  p.col_sorted = a->col_sorted, p.seed = a->random_seed, p.out = a->out;
  return dispatch_id_col(a->src_dtype, a->col_dtype,
                         [&](auto id, auto col) { return launch_neg<decltype(id), decltype(col)>(p, stream); });
}

}  // namespace wm
