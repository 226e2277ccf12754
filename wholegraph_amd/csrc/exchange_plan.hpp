// wholegraph_amd — index arithmetic of the chunked row exchange that the distributed gather, the distributed scatter and the
// sparse gradient apply share: which positions a chunk covers on either side and where its all-to-all-v segments lie.
// Standard library only (no backend, no communicator, no device header): tests/cpp/exchange_plan_test.cpp checks it alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace wm {

// Chunk-major order of per-peer segments (backend.hpp: permute_chunks): chunk c of a segment of n rows is rows
// [n*c/C, n*(c+1)/C) of it — the same cut on both ends of a pair, so the sizes of an exchanged chunk always match — and the
// chunk-major order lists chunk 0 of every segment (in peer order), then chunk 1 of every segment, ... A chunk of the
// pipelined exchange is then ONE contiguous range of ids, positions and row buffer: one row kernel per chunk and side
// whatever the number of ranks (distributed gather since round 5; distributed scatter and gradient apply since round 6).
struct chunk_layout {
  chunk_layout(const std::vector<int64_t>& counts, int n_chunks) : counts_(counts), C_(n_chunks), start_(n_chunks + 1, 0)
  {
    for (int c = 0; c < C_; c++) {
      int64_t s = 0;
      for (size_t p = 0; p < counts_.size(); p++) s += count(c, static_cast<int>(p));
      start_[c + 1] = start_[c] + s;
    }
  }
  int64_t first(int c, int p) const { return counts_[p] * c / C_; }                 // first row of chunk c inside segment p
  int64_t count(int c, int p) const { return counts_[p] * (c + 1) / C_ - counts_[p] * c / C_; }
  int64_t start(int c) const { return start_[c]; }                                   // where chunk c begins, chunk-major
  int64_t size(int c) const { return start_[c + 1] - start_[c]; }
  int64_t pos(int c, int p) const                                                    // where chunk c of segment p begins
  {
    int64_t at = start_[c];
    for (int q = 0; q < p; q++) at += count(c, q);
    return at;
  }
  int64_t total() const { return start_[C_]; }

 private:
  std::vector<int64_t> counts_;
  int C_;
  std::vector<int64_t> start_;
};

// One side of the exchange: the row ranges chunk c launches over — (first, count) pairs, empty ones included, the launchers
// skip them — and where its per-peer segments lie. Positions are those of the side's peer-major array (bucketed order, or
// recv_ids) or, when chunk_major(), of the chunk-major copy of it.
class exchange_side {
 public:
  using range = std::pair<int64_t, int64_t>;
  // per_peer: one range per peer (`skip` left out); else with one chunk the peer-major array is contiguous as it is — the
  // whole of [0, total) but for the hole [hole_b, hole_e) — and with several chunks the order is chunk-major
  exchange_side(const std::vector<int64_t>& counts, const std::vector<int64_t>& offsets, int C, bool per_peer, int skip,
                int64_t hole_b, int64_t hole_e, int64_t total)
    : cuts_(counts, C), counts_(counts), offsets_(offsets), W_(static_cast<int>(counts.size())), C_(C), per_peer_(per_peer), chunk_major_(!per_peer && C > 1),
      skip_(skip), hole_b_(hole_b), hole_e_(hole_e), total_(total)
  {
  }
  bool chunk_major() const { return chunk_major_; }
  int peers() const { return W_; }
  int chunks() const { return C_; }
  int64_t rows() const { return cuts_.total(); }                     // all segments together
  const int64_t* seg_counts() const { return counts_.data(); }       // the peer-major segments, as permute_chunks takes them
  const int64_t* seg_offsets() const { return offsets_.data(); }
  int64_t first(int c, int p) const { return cuts_.first(c, p); }   // inside peer p's segment
  int64_t count(int c, int p) const { return cuts_.count(c, p); }
  int64_t offset(int c, int p) const { return chunk_major_ ? cuts_.pos(c, p) : offsets_[p] + cuts_.first(c, p); }
  std::vector<range> ranges(int c) const
  {
    if (chunk_major_) return {{cuts_.start(c), cuts_.size(c)}};
    if (!per_peer_) {
      if (hole_b_ >= total_) return {{0, total_}};           // no hole (the self segment travels, or nothing follows it)
      return {{0, hole_b_}, {hole_e_, total_ - hole_e_}};   // the rows before the self segment and the ones after it
    }
    std::vector<range> r;
    r.reserve(W_);
    for (int p = 0; p < W_; p++)
      if (p != skip_) r.emplace_back(offset(c, p), count(c, p));
    return r;
  }

 private:
  chunk_layout cuts_;
  std::vector<int64_t> counts_, offsets_;
  int W_, C_;
  bool per_peer_, chunk_major_;
  int skip_;
  int64_t hole_b_, hole_e_, total_;
};

// Both sides of one rank's exchange. `want`: the rows of this rank's own batch, in bucketed order — sent by the scatter and
// the gradient apply, received by the gather. `serve`: the rows of recv_ids, which this rank owns. The sides take the
// per-peer decision separately because a gather into presorted ids receives straight into its dense output: its want side
// stays peer-major (and launches nothing) while its serve side may be chunk-major.
struct exchange_plan {
  // x: what the ids exchange left (ops_internal.hpp: id_exchange, or anything with its counts, offsets, self_* and total_*);
  // self_local: the self segment does not travel (no loopback)
  template <class id_exchange_t>
  exchange_plan(const id_exchange_t& x, int rank, int C, bool self_local, bool want_per_peer, bool serve_per_peer)
    : want(x.send_counts, x.bucket_offsets, C, want_per_peer, self_local ? rank : -1, self_local ? x.self_offset : x.total_valid,
           self_local ? x.self_offset + x.self_count : x.total_valid, x.total_valid),
      serve(x.recv_counts, x.recv_offsets, C, serve_per_peer, -1, x.total_recv, x.total_recv, x.total_recv)
  {
  }
  exchange_side want, serve;
};

// The four per-peer vectors (in rows) of chunk c's all-to-all-v from `send` to `recv`. recv_base: the caller's own peer-major
// receive layout — segment p then lands at recv_base[p] + recv.first(c, p) whatever order `recv` has (the gradient apply
// receives rank-major, the order of its fp32 sums).
struct chunk_segments { std::vector<int64_t> sc, so, rc, ro; };
inline chunk_segments segments_of(const exchange_side& send, const exchange_side& recv, int c,
                                  const std::vector<int64_t>* recv_base = nullptr)
{
  const int W = send.peers();
  chunk_segments s{std::vector<int64_t>(W), std::vector<int64_t>(W), std::vector<int64_t>(W), std::vector<int64_t>(W)};
  for (int p = 0; p < W; p++) {
    s.sc[p] = send.count(c, p), s.so[p] = send.offset(c, p);
    s.rc[p] = recv.count(c, p), s.ro[p] = recv_base != nullptr ? (*recv_base)[p] + recv.first(c, p) : recv.offset(c, p);
  }
  return s;
}

}  // namespace wm
