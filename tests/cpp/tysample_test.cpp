// The rules of a per-relation fan-out sample (wholegraph_amd_ext.h section 2t) on the HOST against hand-written cases: includes
// csrc/tysample.hpp (with csrc/tsample.hpp and csrc/pcg.hpp) alone, is built with the host compiler's address and
// undefined-behaviour sanitizers by tests/test_tysample_surface.py, prints the line of a case that fails and exits 0 when none does.
#include <cstdio>

#include "tysample.hpp"

static int failures = 0;
#define CHECK(cond) \
  if (!(cond)) failures++, std::printf("line %d: %s\n", __LINE__, #cond)

int main()
{
  using namespace wm;
  const int ok[3] = {3, 0, 5}, neg[2] = {1, -1}, wide[2] = {64, 1}, zero[2] = {0, 0}, one65[1] = {65};
  int ones[65];
  for (int& v : ones) v = 1;
  ty_fanouts f{};
  CHECK(ty_fanouts_ok(3, ok, &f) && f.num_relations == 3 && f.total == 8);
  CHECK(!ty_fanouts_ok(0, ok, nullptr) && !ty_fanouts_ok(65, ones, nullptr) && !ty_fanouts_ok(3, nullptr, nullptr));
  CHECK(!ty_fanouts_ok(2, neg, nullptr) && !ty_fanouts_ok(2, wide, nullptr) && !ty_fanouts_ok(2, zero, nullptr));
  CHECK(!ty_fanouts_ok(1, one65, nullptr) && ty_fanouts_ok(1, wide, nullptr) && ty_fanouts_ok(64, ones, nullptr));
  // base_r and the lane layout of {3, 0, 5}: lanes 0 .. 2 relation 0, lanes 3 .. 7 relation 2, nothing behind
  CHECK(f.base[0] == 0 && f.base[1] == 3 && f.base[2] == 3 && f.fanout[1] == 0 && f.fanout[3] == 0);
  const int want_slot[10] = {0, 0, 0, 2, 2, 2, 2, 2, -1, -1};
  for (int s = 0; s < 10; s++) CHECK(ty_slot_relation(s, f) == want_slot[s]);
  CHECK(ty_live(0, f) && !ty_live(1, f) && ty_live(2, f) && !ty_live(3, f) && !ty_live(-1, f) && !ty_live(64, f));
  bool over      = true;   // c_i = sum min(E_ir, f_r), and whether any relation is over
  const int a[3] = {3, 0, 5}, b[3] = {4, 0, 2}, c[3] = {0, 0, 0};
  CHECK(ty_count(a, f, &over) == 8 && !over);   // exactly f_r of both: nothing to select
  CHECK(ty_count(b, f, &over) == 5 && over);
  CHECK(ty_count(c, f, &over) == 0 && !over);
  // the key: section 2r's strategy-0 key under the relation; relation ascending, then draw descending, then j ascending
  const ts_key t = ts_uniform_key(7, 3, 11), k0 = ty_key(7, 3, 11, 0), k2 = ty_key(7, 3, 11, 2);
  CHECK(k0.lo == t.lo && (k0.hi & 0xFFFFFFFFu) == t.hi && ts_key_position(k0) == 11);
  CHECK(ty_key_relation(k0) == 0 && ty_key_relation(k2) == 2 && ty_key_relation(ts_key{0, 0}) == -1);
  CHECK(ts_key_less(k2, k0) && ts_key_less(ty_empty_slot(0), k0) && ts_key_less(k2, ty_empty_slot(0)));   // the empty slot between
  CHECK(ts_key_less(ty_empty_slot(2), k2) && ts_key_less(ts_key{0, 0}, ty_empty_slot(63)));
  CHECK(!ty_key_occupied(ty_empty_slot(5)) && ty_key_occupied(k2) && ty_key_relation(ty_empty_slot(5)) == 5);
  CHECK(ts_key_less(ts_key{k0.hi, k0.lo - 1}, k0));   // the same draw at position 12: the tie goes to the lowest j
  return failures == 0 ? 0 : 1;
}
