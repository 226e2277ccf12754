// wholegraph_amd — what the random-walk units share (walk.hip: first-order walks, section 2m; walk_n2v.hip: node2vec walks,
// section 2n): the kernel argument block, the row of a node, the start of a walk, and the launchers' argument checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "csr_view.cuh"

namespace wm {

struct walk_params {
  csr_view g;
  csr_weights wt;
  const void* starts;
  int64_t n;
  int walk_length;
  uint64_t seed;
  void* out_walks;        // ColT [n, L + 1]
  int64_t* out_edge_ids;  // [n, L] or nullptr
};

// the row of v: true when a step can be taken from it (1 .. 2^31 - 1 neighbours, bounds inside the edge arrays). Both
// reads are issued before either is used.
__device__ __forceinline__ bool walk_row(const walk_params& p, int64_t v, int64_t* s_out, int* deg_out)
{
  const int64_t s = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + v);
  const int64_t e = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + v + 1);
  const bool ok   = s >= 0 && e > s && e <= p.g.n_edges && e - s < (INT64_C(1) << 31);
  *s_out          = s;
  *deg_out        = ok ? static_cast<int>(e - s) : 0;
  return ok;
}

template <typename IdT>
__device__ __forceinline__ int64_t walk_start(const walk_params& p, int64_t w)
{
  const int64_t v = static_cast<int64_t>(static_cast<const IdT*>(p.starts)[w]);
  return v >= 0 && v < p.g.n_nodes ? v : -1;
}

inline walk_params walk_params_of(const wm_walk_args* a)
{
  walk_params p{};
  p.g = csr_view_of(*a), p.wt = csr_weights_of(*a);
  p.starts = a->starts, p.n = a->n, p.walk_length = a->walk_length, p.seed = a->random_seed;
  p.out_walks = a->out_walks, p.out_edge_ids = a->out_edge_ids;
  return p;
}

// what both launchers refuse (-1, nothing queued): the host side has answered all of it before it gets here
inline bool walk_args_ok(const wm_walk_args* a)
{
  if (a == nullptr || a->n < 0 || a->walk_length < 1 || a->n * (static_cast<int64_t>(a->walk_length) + 1) >= (INT64_C(1) << 31)) return false;
  if (a->n_nodes < 0 || a->n_edges < 0) return false;
  return a->n == 0 || (a->starts != nullptr && a->out_walks != nullptr);
}

}  // namespace wm
