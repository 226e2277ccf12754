// wholegraph_amd — the step rule of a node2vec (p, q) second-order walk (wholegraph_amd_ext.h section 2n), usable from host and
// device code: the bias of a neighbour, its effective weight, and the two answers to "does x occur in the row of the previous
// node". kernels/walk_n2v.hip calls these with readers of a WholeMemory tensor, tests/cpp/n2v_walk_test.cpp with plain arrays.
//
// The searches are written over a loader: load(pos) returns col_ind[pos] widened to int64. Only ids are compared; x is never
// an index. Every pos a search forms lies in [s, e), whatever the array holds, so a row that is not ascending (a broken
// col_sorted promise, a damaged graph) gives some answer and reads nothing outside the row.
#pragma once
#include <cstdint>

#include "pcg.hpp"

namespace wm {

// membership by scanning the row [s, e): right on every graph, e - s compares
template <typename Load>
WM_HD bool n2v_row_has_scan(Load load, int64_t s, int64_t e, int64_t x)
{
  bool found = false;
  for (int64_t pos = s; pos < e; pos++) found |= load(pos) == x;
  return found;
}

// membership in an ASCENDING row [s, e), e - s < 2^31: lower_bound by halving, selects instead of branches, then one compare.
// The range at least halves per iteration, so 31 iterations empty it; mid lies in [lo, lo + n), which stays inside [s, e).
template <typename Load>
WM_HD bool n2v_row_has_sorted(Load load, int64_t s, int64_t e, int64_t x)
{
  int64_t lo = s, n = e - s;
  for (int it = 0; it < 31 && n > 0; it++) {
    const int64_t half = n >> 1, mid = lo + half;
    const bool less    = load(mid) < x;
    lo                 = less ? mid + 1 : lo;
    n                  = less ? n - half - 1 : half;
  }
  return lo < e && load(lo) == x;
}

// bias of neighbour x of the current node at a step t >= 1 (at t = 0 there is no previous node and the bias is 1.0f):
// 1 / p back to the previous node u, 1 for a neighbour of u, 1 / q for anything else. in_u_row is looked at only when x != u.
WM_HD float n2v_bias(int64_t x, int64_t u, bool in_u_row, float inv_p, float inv_q)
{
  return x == u ? inv_p : (in_u_row ? 1.0f : inv_q);
}

// effective weight: ONE fp32 multiply (the units that include this are built with -ffp-contract=off), so that a bias of 1.0f
// returns w32 bit for bit and p = q = 1 reduces to the weighted walk of section 2m
WM_HD float n2v_effective_weight(float w32, float bias) { return w32 * bias; }

// what the entry point requires of p and q: both, and both fp32 reciprocals, finite and > 0 (refuses 0, negatives, NaN, inf
// and a subnormal whose reciprocal overflows)
WM_HD bool n2v_pq_ok(float p, float q)
{
  const float big = 3.402823466e+38f;
  const float ip = 1.0f / p, iq = 1.0f / q;
  return p > 0.0f && p <= big && q > 0.0f && q <= big && ip > 0.0f && ip <= big && iq > 0.0f && iq <= big;
}

}  // namespace wm
