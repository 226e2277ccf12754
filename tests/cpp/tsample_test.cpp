// Temporal neighbour samples (wholegraph_amd_ext.h section 2r) computed on the HOST, one centre after the other, with the
// functions the kernel uses: this program includes csrc/pcg.hpp and csrc/tsample.hpp alone, is built with the host compiler's
// address and undefined-behaviour sanitizers and -ffp-contract=off, and prints what tests/test_tsample_streams.py compares with
// the Python restatement of the definition (tests/_tsample_ref.py).
//
// argv[1]: a text file of integers — n_nodes n_edges n_centres M strategy inclusive time_window seed, then row_ptr
// [n_nodes + 1], edge_time [n_edges], the centre nodes [n_centres], the centre times [n_centres].
// Output: one line per centre, `T i E : positions`, E the number of eligible neighbours, the positions (in the row) of the
// samples in ascending order.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "pcg.hpp"
#include "tsample.hpp"

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (f == nullptr) return 2;
  int64_t n_nodes, n_edges, window;
  long long n_centres, M, strategy, inclusive;
  unsigned long long seed;
  if (std::fscanf(f, "%" SCNd64 " %" SCNd64 " %lld %lld %lld %lld %" SCNd64 " %llu", &n_nodes, &n_edges, &n_centres, &M, &strategy,
                  &inclusive, &window, &seed) != 8)
    return 3;
  std::vector<int64_t> row_ptr(n_nodes + 1), etime(n_edges), centres(n_centres), ctimes(n_centres);
  for (auto* v : {&row_ptr, &etime, &centres, &ctimes})
    for (auto& x : *v)
      if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  std::fclose(f);
  if (!wm::ts_scalars_ok(static_cast<int>(M), static_cast<int>(strategy))) return 4;

  for (int64_t i = 0; i < n_centres; i++) {
    const int64_t u = centres[i], t = ctimes[i];
    int64_t s = 0, e = 0;
    if (u >= 0 && u < n_nodes) {
      s = row_ptr[u], e = row_ptr[u + 1];
      if (!(s >= 0 && s <= e && e <= n_edges && e - s < (INT64_C(1) << 31))) s = e = 0;
    }
    std::vector<wm::ts_key> keys;   // of the eligible neighbours, in row order
    std::vector<uint32_t> picked;
    for (int64_t j = 0; j < e - s; j++) {
      const int64_t ts = etime.at(static_cast<size_t>(s + j));   // (a checked read: nothing may leave the array)
      if (!wm::ts_eligible(ts, t, static_cast<int>(inclusive), window)) continue;
      picked.push_back(static_cast<uint32_t>(j));
      keys.push_back(wm::ts_key_of(static_cast<int>(strategy), seed, static_cast<uint64_t>(i), static_cast<uint32_t>(j), ts));
    }
    const int64_t eligible = static_cast<int64_t>(picked.size());
    const int64_t count    = wm::ts_count(eligible, static_cast<int>(M));
    if (count < eligible) {   // the `count` largest keys, then back into row order
      std::sort(keys.begin(), keys.end(), [](wm::ts_key a, wm::ts_key b) { return wm::ts_key_less(b, a); });
      picked.clear();
      for (int64_t k = 0; k < count; k++) picked.push_back(wm::ts_key_position(keys[static_cast<size_t>(k)]));
      std::sort(picked.begin(), picked.end());
    }
    std::printf("T %" PRId64 " %" PRId64 " :", i, eligible);
    for (uint32_t j : picked) std::printf(" %u", j);
    std::printf("\n");
  }
  return 0;
}
