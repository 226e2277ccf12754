// node2vec (p, q) walks (wholegraph_amd_ext.h section 2n) computed on the HOST, one walk after the other, with the functions
// the kernel uses: this program includes csrc/pcg.hpp and csrc/walk_n2v.hpp alone, is built with the host compiler's address
// and undefined-behaviour sanitizers and -ffp-contract=off, and prints what tests/test_n2v_streams.py compares with the
// Python restatement of the definition (tests/_n2v_ref.py).
//
// argv[1]: a text file of integers — n_nodes n_edges n_starts length seed p q weights route, then row_ptr [n_nodes + 1], col
// [n_edges], the weights as bit patterns [n_edges] (absent when weights = 0), the start nodes [n_starts]. p and q are fp32 bit
// patterns; weights is 0 (none: every edge 1.0f), 1 (fp32 bit patterns) or 2 (fp64 bit patterns); route is 0 (membership by
// scanning the previous node's row) or 1 (by binary search: the rows must be ascending).
// Output: one line per walk, `N w : nodes | edge ids`.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcg.hpp"
#include "walk_n2v.hpp"

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (f == nullptr) return 2;
  int64_t n_nodes, n_edges;
  long long n_starts, length, p_bits, q_bits, weights, route;
  unsigned long long seed, v;
  if (std::fscanf(f, "%" SCNd64 " %" SCNd64 " %lld %lld %llu %lld %lld %lld %lld", &n_nodes, &n_edges, &n_starts, &length, &seed,
                  &p_bits, &q_bits, &weights, &route) != 9)
    return 3;
  std::vector<int64_t> row_ptr(n_nodes + 1), col(n_edges), starts(n_starts);
  std::vector<float> w32(n_edges, 1.0f);
  for (auto& x : row_ptr)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  for (auto& x : col)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  if (weights != 0) {
    for (auto& x : w32) {
      if (std::fscanf(f, "%llu", &v) != 1) return 3;
      if (weights == 1) {
        const uint32_t bits = static_cast<uint32_t>(v);
        std::memcpy(&x, &bits, 4);
      } else {
        double d;
        std::memcpy(&d, &v, 8);
        x = static_cast<float>(d);   // the weight converted to fp32, as the kernel does
      }
    }
  }
  for (auto& x : starts)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  std::fclose(f);
  float p, q;
  const uint32_t pb = static_cast<uint32_t>(p_bits), qb = static_cast<uint32_t>(q_bits);
  std::memcpy(&p, &pb, 4), std::memcpy(&q, &qb, 4);
  if (!wm::n2v_pq_ok(p, q)) return 4;
  const float inv_p = 1.0f / p, inv_q = 1.0f / q;
  const int L       = static_cast<int>(length);
  const auto load   = [&](int64_t pos) { return col.at(static_cast<size_t>(pos)); };   // (a checked read: a search may not leave the row)

  for (int64_t w = 0; w < n_starts; w++) {
    std::vector<int64_t> nodes(L + 1, -1), edges(L, -1);
    int64_t cur = starts[w] >= 0 && starts[w] < n_nodes ? starts[w] : -1;
    int64_t u = -1, us = 0, ue = 0;
    nodes[0] = cur;
    for (int t = 0; t < L && cur >= 0; t++) {
      const int64_t s = row_ptr[cur], e = row_ptr[cur + 1], deg = e - s;
      if (deg <= 0 || deg >= (INT64_C(1) << 31)) break;
      float best_key = 0.f;
      int best_j     = -1;
      for (int j = static_cast<int>(deg) - 1; j >= 0; j--) {   // descending on purpose: the order of the visits must not matter
        const int64_t x = col[s + j];
        float bias      = 1.0f;
        if (t > 0) {
          bool in_row = false;
          if (x != u) in_row = route != 0 ? wm::n2v_row_has_sorted(load, us, ue, x) : wm::n2v_row_has_scan(load, us, ue, x);
          bias = wm::n2v_bias(x, u, in_row, inv_p, inv_q);
        }
        const float ew = wm::n2v_effective_weight(w32[s + j], bias);
        if (!wm::walk_weight_eligible(ew)) continue;
        const float key = wm::walk_weighted_key(seed, static_cast<uint64_t>(w), static_cast<uint64_t>(L), static_cast<uint64_t>(t),
                                                static_cast<uint64_t>(j), ew);
        if (wm::walk_key_replaces(key, j, best_key, best_j)) best_key = key, best_j = j;
      }
      if (best_j < 0) break;
      const int64_t c = col[s + best_j];
      if (c < 0 || c >= n_nodes) break;
      nodes[t + 1] = c, edges[t] = s + best_j;
      u = cur, us = s, ue = e;
      cur = c;
    }
    std::printf("N %" PRId64 " :", w);
    for (int64_t x : nodes) std::printf(" %" PRId64, x);
    std::printf(" |");
    for (int64_t x : edges) std::printf(" %" PRId64, x);
    std::printf("\n");
  }
  return 0;
}
