// wholegraph_amd — per-relation fan-out neighbour sampling over a CSR graph held in WholeMemory (gfx950 HIP; wholegraph_amd_ext.h
// section 2t): per centre i and relation r, the live neighbours of centers[i] with edge_type == r, at most f_r of them,
// uniformly without replacement, all relations together in row order. Count, scan, one host round trip, select: the shape
// of tsample.hip.
//   - Count: a group of kTyCountGroup lanes per centre walks the row's types, kTyCountBatch loads per lane in flight, and adds
//     each live one to its relation's counter, one of 64 words per group in LDS (LDS atomic add). c_i = sum min(cnt_r, f_r),
//     and one byte per centre says whether any relation has more than its fan-out: only then is anything drawn.
//   - Select: a group of G = 32 or 64 lanes per centre (F <= 32: two centres per wave), no LDS, no barrier. A centre whose
//     byte is clear emits every live neighbour, placed by ballot and popcount. Otherwise ALL relations are selected in one
//     walk: the lanes of the group are partitioned by relation (tysample.hpp), lanes [base_r, base_r + f_r) holding relation
//     r's running top f_r keys, so that the group's registers are one descending sequence of (relation, key). A batch of G
//     neighbours in which some key beats its own relation's f_r-th is sorted and merged with them (top_merge_both) into the
//     order of all 2G; an element's rank inside its relation is its distance to the last segment head at or below it (heads:
//     the relation differs from the neighbour's; ballot; count leading zeros), and the elements of rank < f_r, in order, are
//     exactly the new contents of lanes 0 .. F - 1: lane d fetches the d-th of them with one lane permute per word.
//     The winners' positions are then sorted ascending across the lanes, which is the output order.
// The fan-outs travel by value; lane r of a wave keeps (f_r, base_r) in a register and the select's lookup by type is a lane
// permute (the count's, whose walk is not wave-uniform, a read of an LDS copy). A col_ind value is copied, never used as an
// index; a position leaves a key only if it entered one, and is checked against the row again before it is used. Groups past
// the end sit out (an empty row) but take part in the votes and shuffles; the select's trips are the same for all lanes of a
// wave. No global atomics, no scratch beyond the n flag bytes; every loop is bounded by the row or by the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../neg_sample.hpp"
#include "../tysample.hpp"
#include "csr_view.cuh"
#include "top_merge.cuh"

namespace wm {
namespace {

constexpr int kTyBlock      = 256;    // lanes per block
constexpr int kTyMaxBlocks  = 2048;   // the cap of both grids: 8 blocks per CU
constexpr int kTyCountBatch = 4;      // types a lane of the count has in flight
constexpr int kTySelBatch   = 2;      // ... and a lane of the select
// lanes per centre in the count (the width of tsample.hip's count); the select's group is 32 for F <= 32 and
// 64 above (hip_tysample_select)
constexpr int kTyCountGroup = 16;
static_assert(kTysampleMaxRelations == 64, "lane r of a wave holds relation r's fan-out; a group of the count has 64 counters");

constexpr size_t ty_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

int ty_blocks(int64_t n, int group)
{
  const int64_t per_block = kTyBlock / group;
  const int64_t b         = (n + per_block - 1) / per_block;
  return static_cast<int>(b < 1 ? 1 : (b < kTyMaxBlocks ? b : kTyMaxBlocks));
}

struct ty_params {
  csr_view g;
  csr_types ty;
  const void* centers;
  int64_t n;
  ty_fanouts f;
  uint64_t seed;
  int* counts;
  uint8_t* over;   // [n]: does any relation of the centre have more live neighbours than its fan-out
  const int* offsets;
  void* out_ids;
  int* out_lid;
  int64_t* out_egid;
  int* out_type;
};

// (f_r | base_r << 8) of relation r = the lane's number in its wave: a select per relation over the by-value argument, no
// indexed read of it
__device__ __forceinline__ uint32_t ty_lane_info(const ty_fanouts& f, int lane)
{
  uint32_t v = 0;
#pragma unroll
  for (int r = 0; r < kTysampleMaxRelations; r++)
    if (lane == r) v = static_cast<uint32_t>(f.fanout[r]) | static_cast<uint32_t>(f.base[r]) << 8;
  return v;
}

// the row [s, s + N) of centre i. A group past the end, a centre that is no node and bounds that are no row: N = 0
template <typename IdT>
__device__ __forceinline__ int ty_row(const ty_params& p, int64_t i, int64_t* s)
{
  *s = 0;
  if (i >= p.n) return 0;
  const int64_t u = static_cast<int64_t>(static_cast<const IdT*>(p.centers)[i]);
  if (u < 0 || u >= p.g.n_nodes) return 0;
  const int64_t b = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + u);
  const int64_t e = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + u + 1);
  if (!neg_row_valid(b, e, p.g.n_edges)) return 0;
  *s = b;
  return static_cast<int>(e - b);   // below 2^31
}

template <int G>
__device__ __forceinline__ unsigned long long ty_slice(unsigned long long ballot, int first)
{
  constexpr unsigned long long kSlice = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
  return (ballot >> first) & kSlice;
}

template <typename IdT, int G>
__global__ __launch_bounds__(kTyBlock) void tysample_count_kernel(ty_params p)
{
  constexpr int kPerBlock = kTyBlock / G;
  constexpr int kPerLane  = kTysampleMaxRelations / G;   // counters a lane clears and reads back
  __shared__ unsigned int cnt[kPerBlock][kTysampleMaxRelations];
  __shared__ unsigned int fan[kTysampleMaxRelations];    // f_r, 0 behind R
  const int gl         = static_cast<int>(threadIdx.x) & (G - 1);
  const int grp        = static_cast<int>(threadIdx.x) / G;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kPerBlock;
  if (threadIdx.x < kTysampleMaxRelations) fan[threadIdx.x] = ty_lane_info(p.f, static_cast<int>(threadIdx.x)) & 0xFFu;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kPerBlock; base < p.n; base += stride) {   // block-uniform trips
    const int64_t i = base + grp;
    int64_t s;
    const int N = ty_row<IdT>(p, i, &s);
#pragma unroll
    for (int k = 0; k < kPerLane; k++) cnt[grp][gl + k * G] = 0;   // the words this same lane reads back below
    __syncthreads();
    for (int64_t r = 0; r < N; r += G * kTyCountBatch) {   // (64-bit: N may be 2^31 - 1, r + k * G + gl passes it)
      int32_t ty[kTyCountBatch];
#pragma unroll
      for (int k = 0; k < kTyCountBatch; k++)   // index clamped: the loads of a trip go out together, unguarded
        ty[k] = gref_load<int32_t>(p.ty.type_ptr, p.ty.type_off + s + min(r + k * G + gl, static_cast<int64_t>(N) - 1));
#pragma unroll
      for (int k = 0; k < kTyCountBatch; k++) {
        const bool known = r + k * G + gl < N && ty[k] >= 0 && ty[k] < p.f.num_relations;
        if (known && fan[ty[k] & 63] > 0) atomicAdd(&cnt[grp][ty[k] & 63], 1u);
      }
    }
    __syncthreads();
    int c = 0, over = 0;
#pragma unroll
    for (int k = 0; k < kPerLane; k++) {
      const unsigned int e = cnt[grp][gl + k * G], f = fan[gl + k * G];
      c += static_cast<int>(min(e, f));
      over |= e > f ? 1 : 0;
    }
#pragma unroll
    for (int d = G >> 1; d >= 1; d >>= 1) {
      c += __shfl_xor(c, d, 64);
      over |= __shfl_xor(over, d, 64);
    }
    if (gl == 0 && i < p.n) {
      p.counts[i] = c;
      p.over[i]   = static_cast<uint8_t>(over);
      if (i == p.n - 1) p.counts[p.n] = 0;   // the scan runs over n + 1 entries
    }
  }
}

__device__ __forceinline__ ts_key ty_key_from(ts_key a, int lane)
{
  return {__shfl(static_cast<unsigned long long>(a.hi), lane, 64), __shfl(a.lo, lane, 64)};
}

// the position of the n-th (0-based) set bit of w by halving: at most 63, whatever n
__device__ __forceinline__ int ty_nth_bit(unsigned long long w, int n)
{
  int pos = 0;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int c = __popcll((w >> pos) & ((1ull << s) - 1ull));
    if (n >= c) n -= c, pos += s;
  }
  return pos;
}

// the highest set bit of w at or below bit gl, w != 0 there
__device__ __forceinline__ int ty_last_head(unsigned long long w) { return 63 - __clzll(static_cast<long long>(w)); }

// The running slots of a group (`top`, the layout of tysample.hpp) and a batch of G keys, {0, 0} where a lane has no
// candidate, merged: the new slots. All lanes of the wave call this together; info is ty_lane_info.
template <int G>
__device__ __forceinline__ ts_key ty_merge(ts_key top, ts_key batch, uint32_t info, int gl, int gbase)
{
  top_merge_both<G>(top, batch, gl);   // top ++ batch: relation ascending, key descending, "no slot" last
  // heads of the relation segments of the 2G elements
  const uint32_t rel_t = static_cast<uint32_t>(top.hi >> 32), rel_b = static_cast<uint32_t>(batch.hi >> 32);
  const uint32_t up_t  = __shfl(rel_t, gbase + ((gl + G - 1) & (G - 1)), 64);   // of the element before; lane 0: top's last
  const uint32_t up_b  = __shfl(rel_b, gbase + ((gl + G - 1) & (G - 1)), 64);
  const unsigned long long head_t = ty_slice<G>(__ballot(gl == 0 || rel_t != up_t), gbase);
  const unsigned long long head_b = ty_slice<G>(__ballot(rel_b != (gl == 0 ? up_t : up_b)), gbase);
  const unsigned long long at_or_below = gl == 63 ? ~0ull : (2ull << gl) - 1ull;
  const int rank_t = gl - ty_last_head(head_t & at_or_below);   // (bit 0 of head_t is set)
  const unsigned long long hb = head_b & at_or_below;
  const int rank_b = hb != 0 ? gl - ty_last_head(hb) : gl + G - ty_last_head(head_t);
  // an element stays when it has a relation and is among its first f_r. Every relation with a fan-out has its f_r slots in
  // `top`, so exactly F elements stay, and in order they are the slots of lanes 0 .. F - 1
  const int f_t = static_cast<int>(__shfl(info, (kTysampleMaxRelations - rel_t) & 63, 64) & 0xFFu);
  const int f_b = static_cast<int>(__shfl(info, (kTysampleMaxRelations - rel_b) & 63, 64) & 0xFFu);
  const unsigned long long stay_t = ty_slice<G>(__ballot(rel_t != 0 && rank_t < f_t), gbase);
  const unsigned long long stay_b = ty_slice<G>(__ballot(rel_b != 0 && rank_b < f_b), gbase);
  const int n_t       = __popcll(stay_t);
  const bool from_top = gl < n_t;
  const bool any      = gl < n_t + __popcll(stay_b);
  const int src       = gbase + (ty_nth_bit(from_top ? stay_t : stay_b, from_top ? gl : gl - n_t) & (G - 1));
  const ts_key a = ty_key_from(top, src), b = ty_key_from(batch, src);
  return any ? (from_top ? a : b) : ts_key{0, 0};
}

template <typename IdT, typename ColT, int G>
__global__ __launch_bounds__(kTyBlock) void tysample_select_kernel(ty_params p)
{
  constexpr int kPerBlock   = kTyBlock / G;
  constexpr uint32_t kNoPos = 0xFFFFFFFFu;   // no position: behind every position in the sort, refused by the row check
  const int lane            = static_cast<int>(threadIdx.x) & 63;
  const int gl              = lane & (G - 1);
  const int gbase           = lane & ~(G - 1);
  const int64_t stride      = static_cast<int64_t>(gridDim.x) * kPerBlock;
  const uint32_t info       = ty_lane_info(p.f, lane);
  const int R = p.f.num_relations, F = p.f.total;
  ColT* out = static_cast<ColT*>(p.out_ids);
  // the relation whose slot this lane is: the one with base_r <= gl < base_r + f_r, none for gl >= F
  ts_key empty{0, 0};
  for (int r = 0; r < R; r++) {
    const uint32_t fr = __shfl(info, r, 64);
    const int b       = static_cast<int>(fr >> 8);
    if (gl >= b && gl < b + static_cast<int>(fr & 0xFFu)) empty = ty_empty_slot(r);
  }
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kPerBlock; base < p.n; base += stride) {   // block-uniform trips
    const int64_t i = base + threadIdx.x / G;
    int64_t s;
    int N   = ty_row<IdT>(p, i, &s);
    int off = 0, c = 0;
    bool pick = false;
    if (i < p.n) off = p.offsets[i], c = p.offsets[i + 1] - off, pick = p.over[i] != 0;
    if (c <= 0) N = 0, pick = false;   // nothing to emit: the row is not read again
    const int n_wave = G == 64 ? __builtin_amdgcn_readlane(N, 0) : max(__builtin_amdgcn_readlane(N, 0), __builtin_amdgcn_readlane(N, 32));
    auto emit = [&](int k, uint32_t j, int32_t ty) {
      const int64_t pos = s + j;
      if (out != nullptr) out[off + k] = gref_load<ColT>(p.g.col_ptr, p.g.col_off + pos);
      if (p.out_lid != nullptr) p.out_lid[off + k] = static_cast<int>(i);
      if (p.out_egid != nullptr) p.out_egid[off + k] = pos;
      if (p.out_type != nullptr) p.out_type[off + k] = ty;
    };
    ts_key top  = empty;
    int emitted = 0;
    for (int64_t r = 0; r < n_wave; r += G * kTySelBatch) {   // wave-uniform trips: the groups of a wave share votes and shuffles
      int32_t ty[kTySelBatch];
#pragma unroll
      for (int k = 0; k < kTySelBatch; k++) ty[k] = -1;
      if (N > 0) {
#pragma unroll
        for (int k = 0; k < kTySelBatch; k++)   // ONE guard, index clamped
          ty[k] = gref_load<int32_t>(p.ty.type_ptr, p.ty.type_off + s + min(r + k * G + gl, static_cast<int64_t>(N) - 1));
      }
#pragma unroll
      for (int k = 0; k < kTySelBatch; k++) {
        if (r + k * G >= n_wave) break;
        const int64_t j      = r + k * G + gl;
        const uint32_t fr    = __shfl(info, ty[k] & 63, 64);   // of the neighbour's relation, if it has one
        const int f_r        = static_cast<int>(fr & 0xFFu), last = static_cast<int>(fr >> 8) + f_r - 1;
        const bool live      = j < N && ty[k] >= 0 && ty[k] < R && f_r > 0;
        const unsigned long long mine = ty_slice<G>(__ballot(live), gbase);
        if (!pick) {
          const int rank = emitted + __popcll(mine & ((1ull << gl) - 1ull));
          if (live && rank < c) emit(rank, static_cast<uint32_t>(j), ty[k]);
          emitted += __popcll(mine);
        }
        ts_key key{0, 0};
        if (pick && live) key = ty_key(p.seed, static_cast<uint64_t>(i), static_cast<uint32_t>(j), ty[k]);
        const ts_key thr = ty_key_from(top, gbase + (live ? last : 0));   // the running f_r-th largest of the relation
        if (!ts_key_less(thr, key) || !(pick && live)) key = ts_key{0, 0};
        if (__any(key.lo != 0)) top = ty_merge<G>(top, key, info, gl, gbase);
      }
    }
    if (__any(pick)) {
      // the winners in ascending position; with fewer than c of them (the graph changed under the call) the rest are kNoPos
      const uint32_t j = top_sort_ascending<G>(pick && gl < F && ty_key_occupied(top) ? ts_key_position(top) : kNoPos, gl);
      if (pick && gl < c && j < static_cast<uint32_t>(N)) {
        const int32_t ty = p.out_type != nullptr ? gref_load<int32_t>(p.ty.type_ptr, p.ty.type_off + s + j) : 0;
        emit(gl, j, ty);
      }
    }
  }
}

bool ty_args_ok(const wm_tysample_args* a)
{
  return a != nullptr && a->n > 0 && a->n < (INT64_C(1) << 31) - 1 && a->n_nodes >= 0 && a->n_edges >= 0 && a->centers != nullptr &&
         a->workspace != nullptr && ty_fanouts_ok(a->num_relations, a->fanouts, nullptr);
}

ty_params ty_params_of(const wm_tysample_args* a)
{
  ty_params p{};
  p.g  = csr_view_of(*a);
  p.ty = csr_types_of(*a);
  p.centers = a->centers, p.n = a->n, p.seed = a->random_seed;
  (void)ty_fanouts_ok(a->num_relations, a->fanouts, &p.f);
  p.counts = a->counts, p.over = static_cast<uint8_t*>(a->workspace), p.offsets = a->offsets;
  p.out_ids = a->out_ids, p.out_lid = a->out_center_lid, p.out_egid = a->out_edge_gid, p.out_type = a->out_edge_type;
  return p;
}

template <typename IdT, typename ColT, int G>
int launch_select(const ty_params& p, hipStream_t stream)
{
  hipLaunchKernelGGL((tysample_select_kernel<IdT, ColT, G>), dim3(ty_blocks(p.n, G)), dim3(kTyBlock), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

// the flag byte per centre
size_t hip_tysample_workspace_bytes(int64_t n) { return ty_align(static_cast<size_t>(n < 1 ? 1 : n)); }

// what the launchers refuse (-1, nothing queued): the host side has answered all of it before it gets here
int hip_tysample_count(const wm_tysample_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!ty_args_ok(a) || a->counts == nullptr) return -1;
  const ty_params p = ty_params_of(a);
  const int blocks  = ty_blocks(a->n, kTyCountGroup);
  if (a->center_dtype == WHOLEMEMORY_DT_INT)
    hipLaunchKernelGGL((tysample_count_kernel<int32_t, kTyCountGroup>), dim3(blocks), dim3(kTyBlock), 0, stream, p);
  else if (a->center_dtype == WHOLEMEMORY_DT_INT64)
    hipLaunchKernelGGL((tysample_count_kernel<int64_t, kTyCountGroup>), dim3(blocks), dim3(kTyBlock), 0, stream, p);
  else
    return -1;
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int hip_tysample_select(const wm_tysample_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!ty_args_ok(a) || a->offsets == nullptr || a->out_ids == nullptr) return -1;
  const ty_params p = ty_params_of(a);
  return dispatch_id_col(a->center_dtype, a->col_dtype, [&](auto id, auto col) {
    using IdT  = decltype(id);
    using ColT = decltype(col);
    return p.f.total <= 32 ? launch_select<IdT, ColT, 32>(p, stream) : launch_select<IdT, ColT, 64>(p, stream);
  });
}

}  // namespace wm
