// wholegraph_amd — the rule of one negative sample over a CSR graph (wholegraph_amd_ext.h section 2o), usable from host and
// device code: the candidate that a 64-bit draw names, in both modes, and when an attempt is rejected. kernels/neg_sample.hip
// calls these with readers of a WholeMemory tensor, tests/cpp/neg_sample_test.cpp with plain arrays.
//
// The rejection rule is written over a loader: load(pos) returns col_ind[pos] widened to int64. Only ids are compared; a
// candidate is never an index before it is range-checked. "c occurs in the row of u" is answered by the searches of
// walk_n2v.hpp, so every pos that is read lies inside the row, whatever the array holds.
#pragma once
#include <cstdint>

#include "pcg.hpp"
#include "walk_n2v.hpp"

namespace wm {

// the high 64 bits of the 128-bit product a * b: the same bits from unsigned __int128 (host) and __umul64hi (device; a unit
// that has included the HIP runtime header, as every kernel unit has — the host units built as HIP never run this on a device)
WM_HD uint64_t neg_mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__) && defined(HIP_INCLUDE_HIP_HIP_RUNTIME_H)
  return __umul64hi(a, b);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * static_cast<unsigned __int128>(b)) >> 64);
#endif
}

// the candidate of the 64-bit draw r. mode 0 (uniform): (r * n_nodes) >> 64. mode 1 (by degree): col_ind[(r * n_edges) >> 64],
// a node drawn as often as it occurs in col_ind. -1 (which every attempt rejects) when mode 1 has no edge to draw from.
// n_nodes >= 0 and n_edges >= 0, so both products stay below the multiplier: the position read lies in [0, n_edges).
template <typename Load>
WM_HD int64_t neg_candidate(Load load, uint64_t r, int mode, int64_t n_nodes, int64_t n_edges)
{
  if (mode == 0) return static_cast<int64_t>(neg_mulhi64(r, static_cast<uint64_t>(n_nodes)));
  if (n_edges <= 0) return -1;
  return load(static_cast<int64_t>(neg_mulhi64(r, static_cast<uint64_t>(n_edges))));
}

// is [s, e) a row that excludes its edges: 0 <= s <= e <= n_edges and fewer than 2^31 entries. A source whose bounds are
// not such a row excludes no edge.
WM_HD bool neg_row_valid(int64_t s, int64_t e, int64_t n_edges)
{
  return s >= 0 && s <= e && e <= n_edges && e - s < (INT64_C(1) << 31);
}

// rejected without looking at the row: c outside [0, n_nodes) (a damaged col_ind entry), or c == u with exclude & 2
WM_HD bool neg_rejected_early(int64_t c, int64_t u, int64_t n_nodes, int exclude)
{
  return c < 0 || c >= n_nodes || ((exclude & 2) != 0 && c == u);
}

// the whole rule for source u with the VALID row [s, e) (s == e where the bounds were not a row): sorted != 0 is the
// caller's promise of ascending rows
template <typename Load>
WM_HD bool neg_rejected(Load load, int64_t c, int64_t u, int64_t n_nodes, int exclude, int64_t s, int64_t e, int sorted)
{
  if (neg_rejected_early(c, u, n_nodes, exclude)) return true;
  if ((exclude & 1) == 0 || e <= s) return false;
  return sorted != 0 ? n2v_row_has_sorted(load, s, e, c) : n2v_row_has_scan(load, s, e, c);
}

// what the entry point requires of the scalar arguments
WM_HD bool neg_scalars_ok(int num_negatives, int mode, int exclude, int max_tries)
{
  return num_negatives >= 1 && (mode == 0 || mode == 1) && exclude >= 0 && exclude <= 3 && max_tries >= 1 && max_tries <= 64;
}

}  // namespace wm
