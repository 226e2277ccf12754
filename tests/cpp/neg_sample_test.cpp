// Negative samples (wholegraph_amd_ext.h section 2o) computed on the HOST, one sample after the other, with the functions the
// kernel uses: this program includes csrc/pcg.hpp, csrc/walk_n2v.hpp and csrc/neg_sample.hpp alone, is built with the host
// compiler's address and undefined-behaviour sanitizers and -ffp-contract=off, and prints what tests/test_neg_streams.py
// compares with the Python restatement of the definition (tests/_neg_ref.py).
//
// argv[1]: a text file of integers — n_nodes n_edges n_sources K mode exclude max_tries route seed, then row_ptr [n_nodes + 1],
// col [n_edges], the source nodes [n_sources]. route is 0 (membership by scanning the source's row) or 1 (by binary search:
// the rows must be ascending for the answer to be specified).
// Output: one line per source, `N i : negatives`.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "neg_sample.hpp"
#include "pcg.hpp"
#include "walk_n2v.hpp"

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (f == nullptr) return 2;
  int64_t n_nodes, n_edges;
  long long n_sources, K, mode, exclude, tries, route;
  unsigned long long seed;
  if (std::fscanf(f, "%" SCNd64 " %" SCNd64 " %lld %lld %lld %lld %lld %lld %llu", &n_nodes, &n_edges, &n_sources, &K, &mode,
                  &exclude, &tries, &route, &seed) != 9)
    return 3;
  std::vector<int64_t> row_ptr(n_nodes + 1), col(n_edges), src(n_sources);
  for (auto& x : row_ptr)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  for (auto& x : col)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  for (auto& x : src)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  std::fclose(f);
  if (!wm::neg_scalars_ok(static_cast<int>(K), static_cast<int>(mode), static_cast<int>(exclude), static_cast<int>(tries))) return 4;
  const auto load = [&](int64_t pos) { return col.at(static_cast<size_t>(pos)); };   // (a checked read: nothing may leave the array)

  for (int64_t i = 0; i < n_sources; i++) {
    const int64_t u = src[i] >= 0 && src[i] < n_nodes ? src[i] : -1;
    int64_t s = 0, e = 0;
    if (u >= 0 && (exclude & 1) != 0) {
      s = row_ptr[u], e = row_ptr[u + 1];
      if (!wm::neg_row_valid(s, e, n_edges)) s = e = 0;
    }
    std::printf("N %" PRId64 " :", i);
    for (int64_t k = 0; k < K; k++) {
      int64_t result = -1;
      if (u >= 0) {
        wm::pcg32 g = wm::walk_stream(seed, static_cast<uint64_t>(i) * static_cast<uint64_t>(K) + static_cast<uint64_t>(k), 0);
        for (int a = 0; a < tries; a++) {
          const int64_t c = wm::neg_candidate(load, g.next_u64(), static_cast<int>(mode), n_nodes, n_edges);
          if (wm::neg_rejected(load, c, u, n_nodes, static_cast<int>(exclude), s, e, static_cast<int>(route))) continue;
          result = c;
          break;
        }
      }
      std::printf(" %" PRId64, result);
    }
    std::printf("\n");
  }
  return 0;
}
