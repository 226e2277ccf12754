// wholegraph_amd — the rules of PinSAGE importance neighbourhoods (wholegraph_amd_ext.h section 2s) that the host and the
// kernel share: the limits of the scalar arguments, the restart threshold, the size of a seed's visit table, and the 64-bit
// key under which a visited node is ranked. graph_ops.cpp checks with these, kernels/rwr.hip walks and selects with them.
#pragma once
#include <cstdint>

#include "pcg.hpp"

namespace wm {

constexpr int kRwrMaxVisits  = 2048;   // V = num_walks * walk_length: the steps of one seed, all counted in one LDS table
constexpr int kRwrMaxTop     = 64;     // T: the running top is one key per lane of a wave
constexpr int kRwrMinSlots   = 128;
constexpr int kRwrMaxSlots   = 2 * kRwrMaxVisits;
constexpr int kRwrNodeBits   = 52;     // a node id below 2^52 and a count below 2^12 share one 64-bit key
constexpr uint64_t kRwrNodeMask = (UINT64_C(1) << kRwrNodeBits) - 1;

// restart_prob in [0, 1) (NaN fails both comparisons)
WM_HD bool rwr_restart_prob_ok(double restart_prob) { return restart_prob >= 0.0 && restart_prob < 1.0; }

// a step restarts when its first 32-bit draw, widened, is below this: one exact double multiplication (a power of two),
// truncated. restart_prob < 1 keeps it below 2^32; 0 never restarts
WM_HD uint64_t rwr_threshold(double restart_prob) { return static_cast<uint64_t>(restart_prob * 4294967296.0); }

WM_HD bool rwr_scalars_ok(int num_walks, int walk_length, double restart_prob, int num_neighbors)
{
  return num_walks >= 1 && walk_length >= 1 && static_cast<int64_t>(num_walks) * walk_length <= kRwrMaxVisits &&
         num_neighbors >= 1 && num_neighbors <= kRwrMaxTop && rwr_restart_prob_ok(restart_prob);
}

// slots of the visit table of a seed with V steps: 2 * V rounded up to a power of two, at least 128 — at most half full,
// whatever the walks do
WM_HD int rwr_table_slots(int visits)
{
  int slots = kRwrMinSlots;
  while (slots < 2 * visits) slots <<= 1;
  return slots;
}

// the rank of a visited node: more visits first, then the lower id. count in 1 .. 4095, node in [0, 2^52); an occupied slot
// never packs to 0, which is the key of "nothing"
WM_HD uint64_t rwr_pack(uint32_t count, uint64_t node)
{
  return (static_cast<uint64_t>(count) << kRwrNodeBits) | (kRwrNodeMask - node);
}
WM_HD int64_t rwr_key_node(uint64_t key) { return static_cast<int64_t>(kRwrNodeMask - (key & kRwrNodeMask)); }
WM_HD int32_t rwr_key_count(uint64_t key) { return static_cast<int32_t>(key >> kRwrNodeBits); }

}  // namespace wm
