// wholegraph_amd — the rules of one LABOR layer-neighbour sample over a CSR graph (wholegraph_amd_ext.h section 2v), usable from
// host and device code: the variate of a neighbour NODE, when the Poisson mode takes a neighbour, the key a neighbour competes
// with under the fixed-count mode, c_i, and what the entry point requires of the scalars. kernels/labor.hip and graph_ops.cpp
// call these; tests/_labor_ref.py restates them.
//
// The variate belongs to the node, not to the (centre, position) pair: every centre of a hop ranks a node by the same number,
// so the samples of centres that share neighbours overlap as much as uniform samples can (Balin and Catalyurek, "Layer-Neighbor
// Sampling", NeurIPS 2023). The fixed-count key is the two-word ts_key of tsample.hpp, {0xFFFFFFFF - v, 0xFFFFFFFF - j}: the
// LARGEST key wins there, so the smallest variate does here, ties to the lowest j, and kernels/top_merge.cuh serves unchanged.
#pragma once
#include <cstdint>

#include "pcg.hpp"
#include "tsample.hpp"

namespace wm {

constexpr int kLaborMaxFanout = kTsampleMaxFanout;   // fixed-count mode: the running top M sits in the registers of one group

// v(c): the first 32-bit output of stream(seed, (uint64)c, 0) of section 2m, c a col_ind entry sign-extended to 64 bits
WM_HD uint32_t labor_variate(uint64_t seed, int64_t c)
{
  pcg32 g = walk_stream(seed, static_cast<uint64_t>(c), 0);
  return g.next_u32();
}

// mode 1: a neighbour with variate v of a row of N entries (N < 2^31) is taken when v / 2^32 < M / N, in integers: both sides
// are below 2^63. With N <= M every v passes: such a row is taken whole
WM_HD bool labor_takes(uint32_t v, int N, int M)
{
  return static_cast<uint64_t>(v) * static_cast<uint64_t>(N) < (static_cast<uint64_t>(M) << 32);
}

// mode 0: the key of the neighbour at position j whose node has variate v
WM_HD ts_key labor_key(uint32_t v, uint32_t j) { return {static_cast<uint64_t>(0xFFFFFFFFu - v), 0xFFFFFFFFu - j}; }

// what the entry point requires of the scalar arguments
WM_HD bool labor_scalars_ok(int max_sample_count, int mode)
{
  return mode == 0 ? max_sample_count <= kLaborMaxFanout : mode == 1 && max_sample_count >= 1;
}

// mode 0: c_i of a row of N entries
WM_HD int labor_fixed_count(int N, int max_sample_count) { return max_sample_count <= 0 || N < max_sample_count ? N : max_sample_count; }

}  // namespace wm
