// wholegraph_amd — the rules of one per-relation fan-out neighbour sample over a CSR graph (wholegraph_amd_ext.h section 2t),
// usable from host and device code: the fan-outs as the kernels carry them, when a neighbour is live, the key it competes
// with, c_i, and which lane of the selecting group holds which slot. kernels/tysample.hip calls these with readers of a
// WholeMemory tensor, tests/cpp/tysample_test.cpp with plain arrays.
//
// The lane layout. With base_r the exclusive prefix of the fan-outs and F their sum, lanes [base_r, base_r + f_r) of a group
// hold the running top f_r keys of relation r in descending order, lanes >= F nothing. A slot is a ts_key (tsample.hpp) whose
// hi word carries the relation above the draw: {(64 - r) << 32 | draw, 0xFFFFFFFF - j}. Under ts_key_less the whole register
// file of the group is therefore always in DESCENDING order — relation ascending, key descending within it —, and one sorting
// network on that one key keeps all relations apart. Inside a relation the order of two keys is the composite
// (uint64(draw) << 32) | (0xFFFFFFFF - j) of section 2t, which is the strategy-0 key of section 2r word for word. j < 2^31,
// so lo of a neighbour's key is never 0: {(64 - r) << 32, 0} is below every key of relation r and above every key of the
// relations behind it — an empty slot of r —, and {0, 0} is below everything: no slot.
#pragma once
#include <cstdint>

#include "pcg.hpp"
#include "tsample.hpp"

namespace wm {

constexpr int kTysampleMaxRelations = 64;
constexpr int kTysampleMaxFanout    = 64;   // of the sum: a group of lanes holds every relation's candidates

// the fan-outs as a kernel takes them by value: fanout[r] and base[r] = fanout[0] + ... + fanout[r - 1], 0 behind num_relations
struct ty_fanouts {
  uint8_t fanout[kTysampleMaxRelations];
  uint8_t base[kTysampleMaxRelations];
  int num_relations;
  int total;   // F
};

// what the entry point requires of R, the f_r and F; *out (optional) is filled when they pass
WM_HD bool ty_fanouts_ok(int num_relations, const int* fanouts, ty_fanouts* out)
{
  if (num_relations < 1 || num_relations > kTysampleMaxRelations || fanouts == nullptr) return false;
  ty_fanouts f{};
  int sum = 0;
  for (int r = 0; r < num_relations; r++) {
    if (fanouts[r] < 0 || fanouts[r] > kTysampleMaxFanout) return false;
    f.fanout[r] = static_cast<uint8_t>(fanouts[r]);
    f.base[r]   = static_cast<uint8_t>(sum);
    sum += fanouts[r];
    if (sum > kTysampleMaxFanout) return false;
  }
  if (sum < 1) return false;
  f.num_relations = num_relations, f.total = sum;
  if (out != nullptr) *out = f;
  return true;
}

// is a neighbour of type ty sampled at all: a relation of the call with a fan-out. A type outside [0, R) contributes nothing
WM_HD bool ty_live(int32_t ty, const ty_fanouts& f) { return ty >= 0 && ty < f.num_relations && f.fanout[ty] > 0; }

// the relation of lane `slot` of the layout, -1 for a lane >= F (host side and tests: a kernel lane finds it once, by a walk)
WM_HD int ty_slot_relation(int slot, const ty_fanouts& f)
{
  for (int r = 0; r < f.num_relations; r++)
    if (slot >= f.base[r] && slot < f.base[r] + f.fanout[r]) return r;
  return -1;
}

// c_i from the live neighbours per relation
WM_HD int ty_count(const int* per_relation, const ty_fanouts& f, bool* any_over)
{
  int c     = 0;
  bool over = false;
  for (int r = 0; r < f.num_relations; r++) {
    const int e = per_relation[r], m = f.fanout[r];
    c += e < m ? e : m;
    over |= e > m;
  }
  if (any_over != nullptr) *any_over = over;
  return c;
}

WM_HD uint64_t ty_relation_word(int r) { return static_cast<uint64_t>(kTysampleMaxRelations - r) << 32; }
// the key of live neighbour j of centre i, of relation r: the draw of tsample.hpp's strategy 0 under the relation
WM_HD ts_key ty_key(uint64_t seed, uint64_t i, uint32_t j, int r)
{
  const ts_key k = ts_uniform_key(seed, i, j);
  return {ty_relation_word(r) | k.hi, k.lo};
}
WM_HD ts_key ty_empty_slot(int r) { return r < 0 ? ts_key{0, 0} : ts_key{ty_relation_word(r), 0}; }
// the relation a slot or key belongs to (-1: no slot), and whether it holds a neighbour
WM_HD int ty_key_relation(ts_key k) { return (k.hi >> 32) == 0 ? -1 : kTysampleMaxRelations - static_cast<int>(k.hi >> 32); }
WM_HD bool ty_key_occupied(ts_key k) { return k.lo != 0; }

}  // namespace wm
