// The random streams and steps of a random walk (wholegraph_amd_ext.h section 2m) computed on the HOST with the functions
// the kernels use: this program includes csrc/pcg.hpp alone, is built with the host compiler's address and
// undefined-behaviour sanitizers and -ffp-contract=off, and prints what tests/test_walk_streams.py compares with the Python
// restatement of the definition (tests/_walk_ref.py) and with the known answers of the header.
//
// argv[1]: a text file of integers — n_nodes n_edges n_starts length seed, then row_ptr [n_nodes + 1], col [n_edges], the
// weights as fp32 bit patterns [n_edges], the start nodes [n_starts].
// Output: `mix0 <hex>`, `stream0 ...` (4 draws of stream(42, 3, 0)), `stream5 ...` (3 draws of stream(42, 3, 5)), then one
// line per walk, `U w : nodes | edge ids` for the uniform form and `W w : ...` for the weighted one.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcg.hpp"

namespace {

struct graph {
  int64_t n_nodes, n_edges;
  std::vector<int64_t> row_ptr, col;
  std::vector<float> weight;
};

// one step from v: the edge taken or -1 (then the walk ends)
template <typename Pick>
int64_t step(const graph& g, int64_t v, Pick pick, int64_t* next)
{
  const int64_t s = g.row_ptr[v], e = g.row_ptr[v + 1], deg = e - s;
  if (deg <= 0 || deg >= (INT64_C(1) << 31)) return -1;
  const int k = pick(s, static_cast<int>(deg));
  if (k < 0) return -1;
  const int64_t c = g.col[s + k];
  if (c < 0 || c >= g.n_nodes) return -1;
  *next = c;
  return s + k;
}

template <typename Pick>
void walk(const graph& g, char tag, int64_t w, int64_t start, int length, Pick pick)
{
  std::vector<int64_t> nodes(length + 1, -1), edges(length, -1);
  int64_t v = start >= 0 && start < g.n_nodes ? start : -1;
  nodes[0]  = v;
  for (int t = 0; t < length && v >= 0; t++) {
    int64_t next    = -1;
    const int64_t e = step(g, v, [&](int64_t s, int deg) { return pick(t, s, deg); }, &next);
    if (e < 0) break;
    nodes[t + 1] = next, edges[t] = e;
    v = next;
  }
  std::printf("%c %" PRId64 " :", tag, w);
  for (int64_t x : nodes) std::printf(" %" PRId64, x);
  std::printf(" |");
  for (int64_t x : edges) std::printf(" %" PRId64, x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv)
{
  std::printf("mix0 %016" PRIx64 "\n", wm::walk_mix(0));
  wm::pcg32 a = wm::walk_stream(42, 3, 0), b = wm::walk_stream(42, 3, 5);
  std::printf("stream0");
  for (int i = 0; i < 4; i++) std::printf(" %u", a.next_u32());
  std::printf("\nstream5");
  for (int i = 0; i < 3; i++) std::printf(" %u", b.next_u32());
  std::printf("\n");
  if (argc < 2) return 0;
  FILE* f = std::fopen(argv[1], "r");
  if (f == nullptr) return 2;
  graph g;
  long long n_starts, length, v;
  unsigned long long seed;
  if (std::fscanf(f, "%" SCNd64 " %" SCNd64 " %lld %lld %llu", &g.n_nodes, &g.n_edges, &n_starts, &length, &seed) != 5) return 3;
  g.row_ptr.resize(g.n_nodes + 1), g.col.resize(g.n_edges), g.weight.resize(g.n_edges);
  for (auto& x : g.row_ptr)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  for (auto& x : g.col)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  for (auto& x : g.weight) {
    if (std::fscanf(f, "%lld", &v) != 1) return 3;
    const uint32_t bits = static_cast<uint32_t>(v);
    std::memcpy(&x, &bits, 4);
  }
  std::vector<int64_t> starts(n_starts);
  for (auto& x : starts)
    if (std::fscanf(f, "%" SCNd64, &x) != 1) return 3;
  std::fclose(f);
  const int L = static_cast<int>(length);
  for (int64_t w = 0; w < n_starts; w++) {
    wm::pcg32 rng = wm::walk_stream(seed, static_cast<uint64_t>(w), 0);
    std::vector<uint32_t> draws(L);
    for (auto& d : draws) d = rng.next_u32();   // step t takes the t-th draw
    walk(g, 'U', w, starts[w], L,
         [&](int t, int64_t, int deg) { return static_cast<int>(wm::walk_uniform_pick(draws[t], static_cast<uint32_t>(deg))); });
  }
  for (int64_t w = 0; w < n_starts; w++) {
    walk(g, 'W', w, starts[w], L, [&](int t, int64_t s, int deg) {
      float best_key = 0.f;
      int best_j     = -1;
      for (int j = deg - 1; j >= 0; j--) {   // descending on purpose: the order of the visits must not matter
        const float wt = g.weight[s + j];
        if (!wm::walk_weight_eligible(wt)) continue;
        const float key = wm::walk_weighted_key(seed, static_cast<uint64_t>(w), static_cast<uint64_t>(L), static_cast<uint64_t>(t),
                                                static_cast<uint64_t>(j), wt);
        if (wm::walk_key_replaces(key, j, best_key, best_j)) best_key = key, best_j = j;
      }
      return best_j;
    });
  }
  return 0;
}
