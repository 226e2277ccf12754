// wholegraph_amd — device and launch helpers shared by the ops of a sampled CSC block (kernels/agg.hip, agg_half.hip,
// agg_weighted.hip, agg_rel.hip, agg_gather.hip, agg_quant.hip and pna.hip, the `agg_concat` family; kernels/gat.hip,
// gat_edge.hip, gatv2.hip and tconv.hip, the attention ops; kernels/edot.hip), whose args all begin with the wm_csc_block of
// backend.hpp:
// fp32 pieces of a row, the clamped edge range of a target, the launch shape, and the two walks every op is built from.
//   * The per-target walk of every forward and every per-target backward: a lane group per target and its column pieces
//     (for_target_pieces), and within it the walk over a range of positions, LANES at a time, the rows of kAggBatch of them
//     loaded back to back (for_edge_batches). for_edge_batches alone decides which positions a lane may fetch, which lane a
//     slot reads from and which slots are used; the fold_*_edges of the per-source walk run on it too (all but three, below).
//   * The walk of the deterministic per-source backward over the host's wm_edge_index: its index (csc_bwd_index), the run of
//     a source (run_of_source), the partial rows of a run's later chunks (add_partials), the tile loop of a chunk kernel
//     (for_chunk_pieces) and the self term of the agg_concat ops (with_self_term).
// What stays in the op's own file: what a lane fetches for its position, the loads of a slot and what a slot adds (the three
// callables of for_edge_batches, in the kernels and in fold_edges*), and everything per target around them.
// Loops over LANES positions that are written out where they stand, and why:
//   * pna.hip, pna_fold_edges: a batch loads up to nine rows per edge, one loop over the batch per aggregator part, so that
//     the branch on the mask stays outside the row loads; with the loads of a slot in one callable the chunk kernel kept 3
//     row loads in flight instead of 12. Its batch is kPnaBwdBatch.
//   * agg.hip, fold_edges, and agg_rel.hip, fold_edges_rel: the same loads and arithmetic, but hipcc schedules and allocates
//     the fold kernels differently on the helper (relagg_fold_bwd_kernel<4, *> 91 -> 97 VGPRs), and they measured slower in
//     every run against the parent: agg_bwd_fold_kernel by 2 to 7 %, the agg_concat_rel backward by 7 to 9 %
//     (profiles/target_walk_refactor_bench.json). Written out, both kernels are the parent's instruction for instruction.
//   * agg_rel.hip, relagg_fwd_kernel with more than LANES edges, two loops: the count of a relation's edges (one ballot per
//     LANES positions, no row loads) and the walk of a batch's matching lanes, whose slots are filled in ballot order, not
//     from consecutive positions.
// (aggw_bwd_weight_kernel of agg_weighted.hip is no such walk: a group takes kAggBatch edges, shuffles once and then walks
// column blocks.) Frames that stay with their kernel: aggg_forward_kernel and aggq_forward_kernel resolve the target's own
// table row once per target, ahead of the column loop; edot_fwd_kernel has no column loop; relagg_fwd_kernel runs rounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cstdlib>

#include "../backend.hpp"
#include "../csc_workspace.hpp"
#include "../knobs.hpp"

namespace wm {

extern std::atomic<int64_t> g_agg_grid_launches, g_agg_grid_truncated;   // wm_common.cpp: bumped by blocks_for()

// index of the per-source backward: the id sort's outputs and what the prep kernel derives from them (in the op's workspace)
struct csc_bwd_index {
  const int32_t* order;        // [n_edges] edge positions, sorted by source (stable)
  const int32_t* run_starts;   // [n_unique + 1]
  const int32_t* unique_ids;   // [n_unique] sources with edges, ascending
  const int64_t* n_unique;     // device scalar written by the sort
  int32_t* sorted_dst;         // [n_edges]
  int32_t* run_of;             // [n_src]
  float* partial;              // [n_tiles, partial_stride] fp32, whatever the type of the rows
  int64_t n_tiles, partial_stride;
};
using wm_agg_bwd_state = csc_bwd_index;   // the agg_concat ops need nothing more

// the id sort's outputs, as the host hands them over, into the index
inline void set_sorted(csc_bwd_index& b, const wm_edge_index& ix)
{
  b.order      = ix.order;
  b.run_starts = ix.run_starts;
  b.unique_ids = ix.unique_ids;
  b.n_unique   = ix.n_unique_dev;
}

// fills `b` from the edge index and `workspace` (hip_agg_backward_workspace_bytes: agg_bwd_plan lays out both) for partial
// rows of `dim` columns and queues agg_bwd_prep_kernel (kernels/agg.hip). 0 or -2.
int agg_bwd_prepare(const wm_csc_block& blk, int64_t dim, const wm_edge_index& ix, void* workspace, csc_bwd_index* b,
                    void* stream);

namespace {

constexpr int kAggBlock = 256;
constexpr int kAggBatch = 8;   // neighbour rows in flight per lane
constexpr int64_t kAggMaxBlocks = 1 << 20;

template <int VEC>
struct fvec {
  float v[VEC];
};

template <int VEC>
__device__ __forceinline__ fvec<VEC> ldv(const float* p)
{
  fvec<VEC> r;
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) r.v[i] = p[i];
  }
  return r;
}

template <int VEC>
__device__ __forceinline__ void stv(float* p, const fvec<VEC>& a)
{
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = a.v[i];
  }
}

template <int VEC>
__device__ __forceinline__ fvec<VEC> splat(float s)
{
  fvec<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = s;
  return r;
}

template <int VEC>
__device__ __forceinline__ void add_to(fvec<VEC>& acc, const fvec<VEC>& b)
{
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc.v[i] = acc.v[i] + b.v[i];
}

template <int VEC>
__device__ __forceinline__ fvec<VEC> scaled(const fvec<VEC>& a, float s)
{
  fvec<VEC> r;
#pragma unroll
  for (int i = 0; i < VEC; ++i) r.v[i] = a.v[i] * s;
  return r;
}

// edges of target d, clamped to [0, n_edges) so that an inconsistent row_ptr cannot send a load out of col_ind
__device__ __forceinline__ void edge_range(const int32_t* row_ptr, int64_t d, int64_t n_edges, int64_t& e0, int64_t& e1)
{
  int64_t a = row_ptr[d], b = row_ptr[d + 1];
  a  = a < 0 ? 0 : (a > n_edges ? n_edges : a);
  b  = b < a ? a : (b > n_edges ? n_edges : b);
  e0 = a, e1 = b;
}

// the lookups of the per-source backward (the id sort of col_ind: order, run_starts, unique_ids, n_unique):
// sorted_dst[i] = the target whose edge range holds position order[i]; run_of[unique[i]] = i
__device__ __forceinline__ void bwd_prep_at(int64_t i, const int32_t* row_ptr, int64_t n_dst, const int32_t* order,
                                            const int32_t* unique_ids, int64_t nu, int32_t* sorted_dst, int32_t* run_of)
{
  const int64_t pos = order[i];
  int64_t lo = 0, hi = n_dst;   // the last d in [0, n_dst) with row_ptr[d] <= pos
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (row_ptr[mid] <= pos) lo = mid;
    else hi = mid;
  }
  sorted_dst[i] = static_cast<int32_t>(lo);
  if (i < nu) run_of[unique_ids[i]] = static_cast<int32_t>(i);
}

// the chunk k >= 1 of a run that starts in tile t = [t*C, (t+1)*C) of the sorted positions, if any: [cs, ce)
__device__ __forceinline__ bool chunk_in_tile(int64_t t, const int32_t* run_starts, int64_t nu, int64_t& cs, int64_t& ce)
{
  constexpr int64_t C   = kAggChunkEdges;
  const int64_t covered = run_starts[nu];   // sorted positions that belong to runs (ids out of range sort behind them)
  const int64_t pos0    = t * C;
  if (pos0 >= covered) return false;
  int64_t lo = 0, hi = nu;   // the run that covers pos0: last u with run_starts[u] <= pos0
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (run_starts[mid] <= pos0) lo = mid;
    else hi = mid;
  }
  const int64_t s0 = run_starts[lo], s1 = run_starts[lo + 1];
  const int64_t k  = (pos0 - s0 + C - 1) / C;
  cs               = s0 + k * C;
  if (k < 1 || cs >= s1 || cs >= pos0 + C) return false;   // no chunk k >= 1 starts in this tile
  ce = cs + C < s1 ? cs + C : s1;
  return true;
}

// fp32 pieces of a partial row: VEC floats, as 16-byte accesses when VEC is 4 or 8 (8: a piece of 16-bit rows)
template <int VEC>
__device__ __forceinline__ fvec<VEC> ldp(const float* p)
{
  if constexpr (VEC == 8) {
    const fvec<4> lo = ldv<4>(p), hi = ldv<4>(p + 4);
    fvec<8> r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = lo.v[i], r.v[4 + i] = hi.v[i];
    return r;
  } else {
    return ldv<VEC>(p);
  }
}

// the run of source s in the sorted positions: [s0, s1), chunk 0 = [s0, c0e), nchunks chunks in all; all 0 without edges
struct src_run {
  bool has;
  int64_t s0, s1, c0e, nchunks;
};

__device__ __forceinline__ src_run run_of_source(const csc_bwd_index& b, int64_t nu, int64_t s)
{
  constexpr int64_t C = kAggChunkEdges;
  src_run r;
  const int64_t u = b.run_of[s];   // (uninitialised unless s has edges: checked against unique_ids)
  r.has           = u >= 0 && u < nu && b.unique_ids[u] == s;
  r.s0 = 0, r.s1 = 0;
  if (r.has) r.s0 = b.run_starts[u], r.s1 = b.run_starts[u + 1];
  r.c0e     = r.s1 - r.s0 > C ? r.s0 + C : r.s1;
  r.nchunks = (r.s1 - r.s0 + C - 1) / C;
  return r;
}

// what an op keeps next to the columns of a partial row: load(prow, k) runs with the load of batch slot k, add(k) with its
// add. The attention op of kernels/gat.hip carries a scalar per head there; the others nothing.
struct no_partial_extra {
  __device__ __forceinline__ void load(const float*, int) {}
  __device__ __forceinline__ void add(int) {}
};

// acc += the partial rows of chunks 1 .. nchunks-1 of run r, in chunk order, a batch of them in flight (this lane's columns
// at cl)
template <int VEC, class Extra = no_partial_extra>
__device__ __forceinline__ void add_partials(fvec<VEC>& acc, const csc_bwd_index& b, const src_run& r, int64_t cl,
                                             Extra extra = Extra())
{
  constexpr int64_t C   = kAggChunkEdges;
  const int64_t nchunks = r.nchunks;
  for (int64_t k0 = 1; k0 < nchunks; k0 += kAggBatch) {
    fvec<VEC> v[kAggBatch];
#pragma unroll
    for (int k = 0; k < kAggBatch; ++k) {
      const int64_t kk = k0 + k < nchunks ? k0 + k : nchunks - 1;   // (a ragged last batch loads its last row again)
      const float* prow = b.partial + ((r.s0 + kk * C) / C) * b.partial_stride;
      v[k]              = ldp<VEC>(prow + cl);
      extra.load(prow, k);
    }
#pragma unroll
    for (int k = 0; k < kAggBatch; ++k) {
      if (k0 + k < nchunks) {
        add_to(acc, v[k]);
        extra.add(k);
      }
    }
  }
}

// the walk of a chunk kernel: a group of LANES lanes per tile t of the sorted positions; for the chunk [cs, ce) that starts
// in it, if any, body(t, cs, ce, c, cl, act) once per piece of `width` columns of this lane (c: its first column, act: c is
// inside the row, cl: c, or 0 for a lane outside it)
template <int VEC, int LANES, class Body>
__device__ __forceinline__ void for_chunk_pieces(const csc_bwd_index& b, int64_t width, Body body)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  const int64_t nu      = *b.n_unique;
  if (nu == 0) return;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; t < b.n_tiles;
       t += static_cast<int64_t>(gridDim.x) * kGroups) {
    int64_t cs, ce;
    if (!chunk_in_tile(t, b.run_starts, nu, cs, ce)) continue;
    for (int64_t cb = 0; cb < width; cb += LANES * VEC) {
      const int64_t c  = cb + gl * VEC;
      const bool act   = c < width;
      const int64_t cl = act ? c : 0;
      body(t, cs, ce, c, cl, act);
    }
  }
}

// the walk of a per-target kernel, the twin of for_chunk_pieces: a group of LANES lanes per target d of the block (anything
// with row_ptr, n_dst and n_edges); with its clamped edge range [e0, e1), body(d, e0, e1, c, cl, act) once per piece of
// `width` columns of this lane. The trip count of the column loop is the same in every lane of the group, so the shuffles of
// an edge walk inside the body stay in step.
template <int VEC, int LANES, class Block, class Body>
__device__ __forceinline__ void for_target_pieces(const Block& blk, int64_t width, Body body)
{
  constexpr int kGroups = kAggBlock / LANES;
  const int gl          = threadIdx.x % LANES;
  for (int64_t d = static_cast<int64_t>(blockIdx.x) * kGroups + threadIdx.x / LANES; d < blk.n_dst;
       d += static_cast<int64_t>(gridDim.x) * kGroups) {
    int64_t e0, e1;
    edge_range(blk.row_ptr, d, blk.n_edges, e0, e1);
    for (int64_t cb = 0; cb < width; cb += LANES * VEC) {
      const int64_t c  = cb + gl * VEC;
      const bool act   = c < width;
      const int64_t cl = act ? c : 0;
      body(d, e0, e1, c, cl, act);
    }
  }
}

// the walk of a group of LANES lanes (this one is lane gl) over the positions [begin, end): a target's edges, or sorted
// positions of the per-source backward. LANES positions at a time:
//   lane_fetch(pos, in_range)  once per lane: what this lane holds of its own position pos = eb + gl for the others to
//                              fetch with __shfl(..., from, LANES). Only with in_range is pos inside [begin, end): without
//                              it the op loads nothing and keeps a harmless default.
//   load_slot(k, from, pos)    for the slots k = 0 .. kAggBatch-1 back to back: the loads of position pos, which lane
//                              `from` holds. A ragged last batch names its last position again, never one past it.
//   use_slot(k, pos)           for the slots that hold a position of their own, in position order.
// No bound of an array enters anywhere else: an op's loads are inside its arrays when lane_fetch honours in_range and
// load_slot forms its addresses from `pos` and from what it shuffles.
template <int LANES, class Fetch, class Load, class Use>
__device__ __forceinline__ void for_edge_batches(int64_t begin, int64_t end, int gl, Fetch lane_fetch, Load load_slot,
                                                 Use use_slot)
{
  for (int64_t eb = begin; eb < end; eb += LANES) {
    const int nb = static_cast<int>(end - eb < LANES ? end - eb : LANES);
    lane_fetch(eb + gl, gl < nb);
    for (int j = 0; j < nb; j += kAggBatch) {
#pragma unroll
      for (int k = 0; k < kAggBatch; ++k) {
        const int from = j + k < nb ? j + k : nb - 1;
        load_slot(k, from, eb + from);
      }
#pragma unroll
      for (int k = 0; k < kAggBatch; ++k)
        if (j + k < nb) use_slot(k, eb + j + k);
    }
  }
}

// grad_x of the agg_concat ops from the sum over the edges: + the self term grad[self_off ...] when `self` (s < n_dst);
// a row without a term from any edge gets the self term alone, or +0.0
template <int VEC>
__device__ __forceinline__ fvec<VEC> with_self_term(const fvec<VEC>& acc, bool has, bool self, const float* grad,
                                                    int64_t self_off)
{
  fvec<VEC> res;
  if (self) {
    const fvec<VEC> g = ldv<VEC>(grad + self_off);
    res               = g;
    if (has) {
      res = acc;
      add_to(res, g);
    }
  } else {
    res = has ? acc : splat<VEC>(0.0f);
  }
  return res;
}

int rc_last() { return hipGetLastError() == hipSuccess ? 0 : -2; }

// the most workgroups of a launch: kAggMaxBlocks, or min(WM_AGG_MAX_BLOCKS, kAggMaxBlocks) when that knob is a positive
// integer. The knob exists for tests: with a cap of a few blocks a small CSC block runs the later trips of every grid-stride
// loop. Unset (every launch of a normal process) this is one pointer test.
int64_t agg_max_blocks()
{
  const char* s = WM_KNOB("WM_AGG_MAX_BLOCKS");
  if (s == nullptr) return kAggMaxBlocks;
  char* end         = nullptr;
  const long long v = strtoll(s, &end, 10);
  if (end == s || *end != '\0' || v < 1) return kAggMaxBlocks;
  return v < kAggMaxBlocks ? static_cast<int64_t>(v) : kAggMaxBlocks;
}

// workgroups for `groups` units of work at `groups_per_block` a block, at most agg_max_blocks(): every kernel launched with
// this grid strides over its work by the grid. Counted for wholememory_ext_agg_grid_stats.
int blocks_for(int64_t groups, int groups_per_block)
{
  int64_t n = (groups + groups_per_block - 1) / groups_per_block;
  if (n < 1) n = 1;
  const int64_t cap = agg_max_blocks();
  g_agg_grid_launches.fetch_add(1, std::memory_order_relaxed);
  if (n > cap) g_agg_grid_truncated.fetch_add(1, std::memory_order_relaxed);
  return static_cast<int>(n < cap ? n : cap);
}

// 16-byte pieces when every row start is 16-byte aligned; group width from the number of pieces (or floats) of a row
bool use_vec4(int64_t dim, const void* a, int64_t a_stride, const void* b, int64_t b_stride)
{
  return dim % 4 == 0 && a_stride % 4 == 0 && b_stride % 4 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 &&
         reinterpret_cast<uintptr_t>(b) % 16 == 0;
}
int lanes_for(int64_t pieces) { return pieces <= 16 ? 16 : (pieces <= 32 ? 32 : 64); }

#define WM_AGG_DISPATCH(VEC_, PIECES_, LAUNCH_)                          \
  do {                                                                   \
    const int lanes__ = lanes_for(PIECES_);                              \
    if (VEC_) {                                                          \
      if (lanes__ == 16) LAUNCH_(4, 16);                                 \
      else if (lanes__ == 32) LAUNCH_(4, 32);                            \
      else LAUNCH_(4, 64);                                               \
    } else {                                                             \
      if (lanes__ == 16) LAUNCH_(1, 16);                                 \
      else if (lanes__ == 32) LAUNCH_(1, 32);                            \
      else LAUNCH_(1, 64);                                               \
    }                                                                    \
  } while (0)

}  // namespace
}  // namespace wm
