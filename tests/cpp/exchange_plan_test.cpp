// Brute-force check of wholegraph_amd/csrc/exchange_plan.hpp (tests/test_exchange_plan.py builds and runs it): for every
// world size, chunk count, mode and count matrix of the grid, every rank's plan is compared with what the scheme is defined
// to be — the cuts [n*c/C, n*(c+1)/C), the peer-major arrays and the chunk-major order of permute_chunks, each written out
// here as a literal loop. Exits 1 at the first violation and prints its tuple.
#include "exchange_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>

namespace {

using wm::exchange_plan;
using wm::exchange_side;
using vec    = std::vector<int64_t>;
using matrix = std::vector<vec>;   // m[a][b]: rows rank a asks of (or sends to) owner b

std::string g_case;

[[noreturn]] void fail(const char* what, int rank, int c, int p)
{
  std::printf("FAILED: %s  [%s rank=%d chunk=%d peer=%d]\n", what, g_case.c_str(), rank, c, p);
  std::exit(1);
}

// what one rank holds after the ids exchange (ops.cpp: bucket_and_exchange_ids)
struct rank_state {
  vec send_counts, recv_counts, bucket_offsets, recv_offsets;
  int64_t self_offset, self_count, total_valid, total_recv;
};

rank_state state_of(const matrix& m, int W, int r, bool self_local)
{
  rank_state s;
  s.send_counts = m[r];
  s.recv_counts.resize(W);
  for (int p = 0; p < W; p++) s.recv_counts[p] = m[p][r];
  s.bucket_offsets.assign(W + 1, 0);
  for (int p = 0; p < W; p++) s.bucket_offsets[p + 1] = s.bucket_offsets[p] + m[r][p];
  s.self_count  = m[r][r];
  s.self_offset = s.bucket_offsets[r];
  s.total_valid = s.bucket_offsets[W];
  if (self_local) s.send_counts[r] = s.recv_counts[r] = 0;
  s.recv_offsets.assign(W + 1, 0);
  for (int p = 0; p < W; p++) s.recv_offsets[p + 1] = s.recv_offsets[p] + s.recv_counts[p];
  s.total_recv = s.recv_offsets[W];
  return s;
}

// element (peer, index inside the peer's segment) at every position of a side's array; {-1, -1}: nothing that travels
// (one buffer for all cases: the sanitizer's allocator makes a fresh half-megabyte vector per rank and side the slowest step)
using element = std::pair<int, int>;
const std::vector<element>& elements_of(const vec& counts, const vec& offsets, int64_t size, int C, bool chunk_major)
{
  const int W = static_cast<int>(counts.size());
  static std::vector<element> at;
  at.clear();
  if (chunk_major) {   // the order permute_chunks defines (backend.hpp)
    for (int c = 0; c < C; c++)
      for (int p = 0; p < W; p++)
        for (int64_t i = counts[p] * c / C; i < counts[p] * (c + 1) / C; i++) at.emplace_back(p, static_cast<int>(i));
    return at;
  }
  at.assign(size, element(-1, -1));
  for (int p = 0; p < W; p++)
    for (int64_t i = 0; i < counts[p]; i++) at[offsets[p] + i] = element(p, static_cast<int>(i));
  return at;
}

// ranges of all chunks: disjoint, inside the array, and covering exactly the positions whose rows travel
void check_side(const exchange_side& side, const vec& counts, const std::vector<element>& at, int W, int C, int r, size_t max_ranges)
{
  static std::vector<int> hits;
  hits.assign(at.size(), 0);
  for (int c = 0; c < C; c++) {
    const auto ranges = side.ranges(c);
    if (side.chunk_major() ? ranges.size() != 1 : ranges.size() > max_ranges) fail("number of ranges", r, c, -1);
    for (const auto& g : ranges) {
      if (g.first < 0 || g.second < 0 || g.first + g.second > static_cast<int64_t>(at.size())) fail("range outside the array", r, c, -1);
      for (int64_t i = g.first; i < g.first + g.second; i++) hits[i]++;
    }
    for (int p = 0; p < W; p++) {   // the chunk's segment of peer p: the cut, its place, and a range that launches over it
      const int64_t n = side.count(c, p), first = side.first(c, p), off = side.offset(c, p);
      if (first != counts[p] * c / C || first + n != counts[p] * (c + 1) / C) fail("chunk cut", r, c, p);
      for (int64_t i = 0; i < n; i++)
        if (off + i >= static_cast<int64_t>(at.size()) || at[off + i] != element(p, static_cast<int>(first + i))) fail("segment position", r, c, p);
      bool inside = n == 0;
      for (const auto& g : ranges) inside = inside || (off >= g.first && off + n <= g.first + g.second);
      if (!inside) fail("segment outside the chunk's ranges", r, c, p);
    }
  }
  for (size_t i = 0; i < at.size(); i++)
    if (hits[i] != (at[i].first >= 0 ? 1 : 0)) fail(hits[i] > 1 ? "position covered twice" : "coverage", r, -1, static_cast<int>(i));
}

void check_matrix(const matrix& m, int W, int C, bool per_peer, bool self_local, bool in_place)
{
  std::vector<rank_state> st;
  std::vector<std::unique_ptr<exchange_plan>> plans;
  for (int r = 0; r < W; r++) st.push_back(state_of(m, W, r, self_local));
  for (int r = 0; r < W; r++) {
    const rank_state& s = st[r];
    plans.emplace_back(new exchange_plan(s, r, C, self_local, per_peer || in_place, per_peer));
    const exchange_plan& plan = *plans.back();
    if (plan.want.chunk_major() != (!per_peer && !in_place && C > 1) || plan.serve.chunk_major() != (!per_peer && C > 1))
      fail("which side is chunk-major", r, -1, -1);
    // want side: bucketed order (self segment in place, travelling only in loopback) or its chunk-major copy
    check_side(plan.want, s.send_counts, elements_of(s.send_counts, s.bucket_offsets, s.total_valid, C, plan.want.chunk_major()), W, C, r,
               per_peer || in_place ? W : 2);
    if (!in_place)   // (in place only the want side differs: the serve side was checked a case earlier)
      check_side(plan.serve, s.recv_counts, elements_of(s.recv_counts, s.recv_offsets, s.total_recv, C, plan.serve.chunk_major()), W, C, r,
               per_peer ? W : 1);
    // the all-to-all-v vectors are the sides' segments, in either direction (the gather sends what it serves); a caller's
    // receive bases — rank-major with the self slot, as the gradient routes receive — replace the receive side's order only
    vec base(W + 1, 0);
    for (int p = 0; p < W; p++) base[p + 1] = base[p] + (p == r ? s.self_count : s.recv_counts[p]);
    for (int c = 0; c < C; c++) {
      const auto back = wm::segments_of(plan.serve, plan.want, c);
      for (int p = 0; p < W; p++)
        if (back.sc[p] != plan.serve.count(c, p) || back.so[p] != plan.serve.offset(c, p) || back.rc[p] != plan.want.count(c, p) ||
            back.ro[p] != plan.want.offset(c, p))
          fail("segments serve -> want", r, c, p);
      if (in_place) continue;   // only the gather receives in place
      const auto grad = wm::segments_of(plan.want, plan.serve, c, &base);
      for (int p = 0; p < W; p++)
        if (grad.sc[p] != plan.want.count(c, p) || grad.so[p] != plan.want.offset(c, p) || grad.rc[p] != plan.serve.count(c, p) ||
            grad.ro[p] != base[p] + s.recv_counts[p] * c / C)
          fail("segments want -> serve with receive bases", r, c, p);
    }
  }
  for (int a = 0; a < W; a++)   // what a sends to b is what b receives from a
    for (int b = 0; b < W; b++)
      for (int c = 0; c < C; c++)
        if (plans[a]->want.count(c, b) != plans[b]->serve.count(c, a)) fail("pair sizes", a, c, b);
}

}  // namespace

int main()
{
  long cases = 0;
  for (int W : {1, 2, 3, 5, 8, 16, 17})
    for (int C : {1, 2, 3, 4, 16}) {
      std::vector<std::pair<std::string, matrix>> ms;
      ms.emplace_back("zero", matrix(W, vec(W, 0)));
      ms.emplace_back("one", matrix(W, vec(W, 1)));
      const int64_t around[4] = {C - 1, C, C + 1, 97};   // counts around the number of chunks, where a cut can come out empty
      matrix mixed(W, vec(W, 0));
      for (int a = 0; a < W; a++)
        for (int b = 0; b < W; b++) mixed[a][b] = around[(3 * a + b) % 4];
      ms.emplace_back("C-1, C, C+1, 97", mixed);
      matrix silent(W, vec(W, 5));   // one rank asks nothing (it still serves)
      silent[W / 2].assign(W, 0);
      ms.emplace_back("rank asking nothing", silent);
      std::mt19937_64 rng(1000 * W + C);
      matrix rnd(W, vec(W, 0));
      for (auto& row : rnd)
        for (auto& v : row) v = rng() % 4 == 0 ? 0 : static_cast<int64_t>(rng() % 120);
      ms.emplace_back("random", rnd);
      for (const auto& m : ms)
        for (int per_peer = 0; per_peer < 2; per_peer++)
          for (int self_local = 0; self_local < 2; self_local++)
            for (int in_place = 0; in_place < 2 - per_peer; in_place++) {   // (per peer, the in-place gather has the same plan)
              g_case = "W=" + std::to_string(W) + " C=" + std::to_string(C) + " counts=" + m.first + " per_peer=" +
                       std::to_string(per_peer) + " self_local=" + std::to_string(self_local) + " in_place=" + std::to_string(in_place);
              check_matrix(m.second, W, C, per_peer != 0, self_local != 0, in_place != 0);
              cases++;
            }
    }
  std::printf("exchange_plan: %ld cases hold\n", cases);
  return 0;
}
