// Brute-force check of wholegraph_amd/csrc/csc_workspace.hpp (tests/test_csc_workspace.py builds and runs it): for every
// combination of three region sizes from a ladder around the 256-byte granule and every misalignment of the workspace's
// start, every region starts on a 256-byte boundary, no two regions overlap and every region ends inside the bytes the
// layout asks for. Each layout is also carved out of a heap block of exactly that many bytes and every region written, so
// the address sanitizer sees the same bound. Exits 1 at the first violation and prints its tuple.
#include "csc_workspace.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace {

int64_t g_cases = 0;

template <size_t N>
void check(const wm::ws_layout<N>& l, const int64_t (&sizes)[N], uintptr_t start, const char* what)
{
  uintptr_t at[N];
  for (size_t i = 0; i < N; ++i) at[i] = reinterpret_cast<uintptr_t>(wm::ws_at<char>(reinterpret_cast<void*>(start), l.off[i]));
  for (size_t i = 0; i < N; ++i) {
    const uintptr_t end = at[i] + static_cast<uintptr_t>(sizes[i]);
    bool ok             = at[i] % 256 == 0 && at[i] >= start && end <= start + l.bytes;
    for (size_t j = 0; j < N && ok; ++j)   // disjoint: one of the two ends where the other starts, or before
      if (j != i) ok = end <= at[j] || at[j] + static_cast<uintptr_t>(sizes[j]) <= at[i];
    if (!ok) {
      std::printf("FAILED: %s region %zu of %zu [start %% 256 = %d, size %lld, offset %zu, bytes %zu]\n", what, i, N,
                  static_cast<int>(start % 256), static_cast<long long>(sizes[i]), l.off[i], l.bytes);
      std::exit(1);
    }
  }
  ++g_cases;
}

}  // namespace

int main()
{
  const int64_t ladder[] = {0, 1, 4, 252, 256, 260, 4096 + 4};
  for (int64_t a : ladder)
    for (int64_t b : ladder)
      for (int64_t c : ladder) {
        const int64_t sizes[3]   = {a, b, c};
        const wm::ws_layout<3> l = wm::ws_plan(sizes);
        for (int m = 0; m < 256; ++m) check(l, sizes, 0x100000u + static_cast<uintptr_t>(m), "ladder");
        // the same layout in a block of exactly l.bytes, at whatever alignment the heap gives and one byte further on
        for (int m = 0; m < 2; ++m) {
          char* block = static_cast<char*>(std::malloc(l.bytes + m));
          check(l, sizes, reinterpret_cast<uintptr_t>(block + m), "heap");
          for (int i = 0; i < 3; ++i) std::memset(wm::ws_at<char>(block + m, l.off[i]), 0x5a, static_cast<size_t>(sizes[i]));
          std::free(block);
        }
      }
  // the agg_concat backward at its smallest: one edge, one source, one column (partial rows of 4 floats, one tile)
  const wm::agg_bwd_layout g = wm::agg_bwd_plan(1, 1, 1, 512);
  if (g.n_tiles != 1 || g.partial_stride != 4) {
    std::printf("FAILED: agg_bwd_plan(1, 1, 1, 512) gives %lld tiles of %lld floats\n", static_cast<long long>(g.n_tiles),
                static_cast<long long>(g.partial_stride));
    return 1;
  }
  const int64_t agg_sizes[3] = {4, 4, 16};
  for (int m : {0, 8, 9, 255}) check(g.ws, agg_sizes, 0x100000u + static_cast<uintptr_t>(m), "agg (1, 1, 1)");
  std::printf("%lld cases hold\n", static_cast<long long>(g_cases));
  return 0;
}
