// wholegraph_amd — temporal neighbour sampling over a CSR graph held in WholeMemory (gfx950 HIP; wholegraph_amd_ext.h section
// 2r): per centre i, the neighbours of centers[i] whose int64 timestamp passes the rule of tsample.hpp against center_times[i],
// at most M of them — uniformly without replacement or the latest — in row order. Count, scan, one host round trip, select:
// the shape of the sampler (graph.hip) and of isub.hip.
//   - Count: a GROUP of kTsCountGroup lanes per centre walks the row's timestamps, kTsCountBatch loads per lane in flight, and
//     counts the eligible ones by ballot and popcount. The grid is capped and strides over the centres; a wave keeps a 64-bit
//     sum of what it counted and one wave adds those up (the int32 scan of the counts cannot see a total of 2^31 or more).
//   - Select: a group of G = 32 or 64 lanes per centre (M <= 32: two centres per wave), no LDS, no barrier. A centre that
//     emits fewer than M entries (or with M <= 0) emits every eligible neighbour, placed by ballot and popcount, no key drawn.
//     Otherwise lane k of the group holds the k-th largest key seen so far ({0, 0} = none yet); a batch of G neighbours with a
//     key above the running M-th largest is merged by the shuffle network of top_merge.cuh. The M winners' positions are then
//     sorted ascending across the lanes (a bitonic network again), which is the output order.
// The key is the two-word key of tsample.hpp under both strategies: the order (ts, -j) of strategy 1 does not fit 64 bits, and
// one network serves both. A col_ind value is copied, never used as an index; a position leaves a key only if it entered
// one, and is checked against the row again before it is used. Groups past the end sit out (an empty row) but take part in
// the votes and shuffles; the trips of a wave are the same for all its lanes. No atomics, no LDS, no scratch; every loop is
// bounded by the row or by the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../neg_sample.hpp"
#include "../tsample.hpp"
#include "csr_view.cuh"
#include "top_merge.cuh"

namespace wm {
namespace {

constexpr int kTsBlock      = 256;    // lanes per block
constexpr int kTsMaxBlocks  = 2048;   // the cap of both grids: 8 blocks per CU
constexpr int kTsCountBatch = 4;      // timestamps a lane of the count has in flight
constexpr int kTsSelBatch   = 2;      // ... and a lane of the select
// lanes per centre in the count (the width of isub.hip's walk); the select's group is 32 for M <= 32 and 64
// above (hip_tsample_select)
constexpr int kTsCountGroup = 16;
static_assert(kTsCountGroup >= 2 && kTsCountGroup <= 64 && (kTsCountGroup & (kTsCountGroup - 1)) == 0, "a power of two within a wave");

}  // namespace

// the two-word key of tsample.hpp as top_merge.cuh's key type
__device__ __forceinline__ ts_key top_key_max(ts_key a, ts_key b) { return ts_key_max(a, b); }
__device__ __forceinline__ ts_key top_key_min(ts_key a, ts_key b) { return ts_key_min(a, b); }
__device__ __forceinline__ ts_key top_key_xor(ts_key a, int j)
{
  return {__shfl_xor(static_cast<unsigned long long>(a.hi), j, 64), __shfl_xor(a.lo, j, 64)};
}

namespace {

constexpr size_t ts_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

int ts_blocks(int64_t n, int group)
{
  const int64_t per_block = kTsBlock / group;
  const int64_t b         = (n + per_block - 1) / per_block;
  return static_cast<int>(b < 1 ? 1 : (b < kTsMaxBlocks ? b : kTsMaxBlocks));
}
int64_t ts_count_waves(int64_t n) { return static_cast<int64_t>(ts_blocks(n, kTsCountGroup)) * (kTsBlock / 64); }

struct ts_params {
  csr_view g;
  csr_times tm;
  const void* centers;
  const int64_t* center_times;
  int64_t n;
  int M, strategy, inclusive;
  int64_t window;
  uint64_t seed;
  int* counts;
  int64_t* wave_sums;
  const int* offsets;
  void* out_ids;
  int* out_lid;
  int64_t* out_egid;
};

// the row [s, s + N) and the time of centre i. A group past the end, a centre that is no node and bounds that are no row: N = 0
template <typename IdT>
__device__ __forceinline__ int ts_row(const ts_params& p, int64_t i, int64_t* s, int64_t* t)
{
  *s = 0, *t = 0;
  if (i >= p.n) return 0;
  *t              = p.center_times[i];
  const int64_t u = static_cast<int64_t>(static_cast<const IdT*>(p.centers)[i]);
  if (u < 0 || u >= p.g.n_nodes) return 0;
  const int64_t b = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + u);
  const int64_t e = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + u + 1);
  if (!neg_row_valid(b, e, p.g.n_edges)) return 0;
  *s = b;
  return static_cast<int>(e - b);   // below 2^31
}

template <int G>
__device__ __forceinline__ unsigned long long ts_slice(unsigned long long ballot, int first)
{
  constexpr unsigned long long kSlice = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
  return (ballot >> first) & kSlice;
}

template <typename IdT, int G>
__global__ __launch_bounds__(kTsBlock) void tsample_count_kernel(ts_params p)
{
  constexpr int kPerBlock = kTsBlock / G;
  const int gl            = static_cast<int>(threadIdx.x) & (G - 1);
  const int first         = static_cast<int>(threadIdx.x) & 63 & ~(G - 1);   // the group's first lane in its wave
  const int64_t stride    = static_cast<int64_t>(gridDim.x) * kPerBlock;
  long long wave_sum      = 0;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kPerBlock; base < p.n; base += stride) {   // block-uniform trips
    const int64_t i = base + threadIdx.x / G;
    int64_t s, t;
    const int N  = ts_row<IdT>(p, i, &s, &t);
    int eligible = 0;
    for (int64_t r = 0; r < N; r += G * kTsCountBatch) {   // (64-bit: N may be 2^31 - 1, r + k * G + gl passes it)
      int64_t ts[kTsCountBatch];
#pragma unroll
      for (int k = 0; k < kTsCountBatch; k++)   // index clamped: the loads of a trip go out together, unguarded
        ts[k] = gref_load<int64_t>(p.tm.time_ptr, p.tm.time_off + s + min(r + k * G + gl, static_cast<int64_t>(N) - 1));
#pragma unroll
      for (int k = 0; k < kTsCountBatch; k++) {
        const bool ok = r + k * G + gl < N && ts_eligible(ts[k], t, p.inclusive, p.window);
        eligible += __popcll(ts_slice<G>(__ballot(ok), first));
      }
    }
    const int cnt = static_cast<int>(ts_count(eligible, p.M));
    if (gl == 0 && i < p.n) {
      p.counts[i] = cnt;
      if (i == p.n - 1) p.counts[p.n] = 0;   // the scan runs over n + 1 entries
      wave_sum += cnt;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wave_sum += __shfl_xor(wave_sum, d, 64);
  if ((threadIdx.x & 63) == 0) p.wave_sums[static_cast<int64_t>(blockIdx.x) * (kTsBlock / 64) + (threadIdx.x >> 6)] = wave_sum;
}

// one wave adds the per-wave sums up: a fixed order, and a word the host may be reading from pinned memory
__global__ __launch_bounds__(64) void tsample_total_kernel(const int64_t* wave_sums, int64_t n_waves, int64_t* total)
{
  long long sum = 0;
  for (int64_t b = 0; b < n_waves; b += 64 * 8) {
    long long v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int64_t j = b + k * 64 + threadIdx.x;
      v[k]            = j < n_waves ? wave_sums[j] : 0;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) sum += v[k];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if (threadIdx.x == 0) *total = sum;
}

// v of the G lanes of a group in ascending order, lane 0 the smallest
template <int G>
__device__ __forceinline__ uint32_t ts_sort_ascending(uint32_t v, int gl)
{
#pragma unroll
  for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint32_t o    = __shfl_xor(v, j, 64);
      const bool keep_min = ((gl & k) == 0) == ((gl & j) == 0);   // ascending where (gl & k) == 0; k == G: everywhere
      v                   = keep_min ? min(v, o) : max(v, o);
    }
  }
  return v;
}

template <typename IdT, typename ColT, int G>
__global__ __launch_bounds__(kTsBlock) void tsample_select_kernel(ts_params p)
{
  constexpr int kPerBlock   = kTsBlock / G;
  constexpr uint32_t kNoPos = 0xFFFFFFFFu;   // no position: behind every position in the sort, refused by the row check
  const int lane            = static_cast<int>(threadIdx.x) & 63;
  const int gl              = lane & (G - 1);
  const int gbase           = lane & ~(G - 1);
  const int64_t stride      = static_cast<int64_t>(gridDim.x) * kPerBlock;
  ColT* out                 = static_cast<ColT*>(p.out_ids);
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kPerBlock; base < p.n; base += stride) {   // block-uniform trips
    const int64_t i = base + threadIdx.x / G;
    int64_t s, t;
    int N   = ts_row<IdT>(p, i, &s, &t);
    int off = 0, c = 0;
    if (i < p.n) off = p.offsets[i], c = p.offsets[i + 1] - off;
    if (c <= 0) N = 0;   // nothing to emit: the row is not read again
    // c == M: the count found M eligible neighbours or more, the largest M keys are the answer (with exactly M, all of them);
    // c < M, or no M: every eligible neighbour, in row order
    const bool pick = p.M > 0 && c == p.M;
    const int n_wave = G == 64 ? __builtin_amdgcn_readlane(N, 0) : max(__builtin_amdgcn_readlane(N, 0), __builtin_amdgcn_readlane(N, 32));
    auto emit = [&](int k, uint32_t j) {
      const int64_t pos = s + j;
      if (out != nullptr) out[off + k] = gref_load<ColT>(p.g.col_ptr, p.g.col_off + pos);
      if (p.out_lid != nullptr) p.out_lid[off + k] = static_cast<int>(i);
      if (p.out_egid != nullptr) p.out_egid[off + k] = pos;
    };
    ts_key top{0, 0};
    int emitted = 0;
    for (int64_t r = 0; r < n_wave; r += G * kTsSelBatch) {   // wave-uniform trips: the groups of a wave share votes and shuffles (64-bit as in the count)
      int64_t ts[kTsSelBatch];
#pragma unroll
      for (int k = 0; k < kTsSelBatch; k++) ts[k] = 0;
      if (N > 0) {
#pragma unroll
        for (int k = 0; k < kTsSelBatch; k++)   // ONE guard, index clamped
          ts[k] = gref_load<int64_t>(p.tm.time_ptr, p.tm.time_off + s + min(r + k * G + gl, static_cast<int64_t>(N) - 1));
      }
#pragma unroll
      for (int k = 0; k < kTsSelBatch; k++) {
        if (r + k * G >= n_wave) break;
        const int64_t j = r + k * G + gl;
        const bool ok   = j < N && ts_eligible(ts[k], t, p.inclusive, p.window);
        const unsigned long long mine = ts_slice<G>(__ballot(ok), gbase);
        if (!pick) {
          const int rank = emitted + __popcll(mine & ((1ull << gl) - 1ull));
          if (ok && rank < c) emit(rank, static_cast<uint32_t>(j));
          emitted += __popcll(mine);
        }
        ts_key key{0, 0};
        if (pick && ok) key = ts_key_of(p.strategy, p.seed, static_cast<uint64_t>(i), static_cast<uint32_t>(j), ts[k]);
        const ts_key thr = {__shfl(static_cast<unsigned long long>(top.hi), gbase + max(p.M, 1) - 1, 64),
                            __shfl(top.lo, gbase + max(p.M, 1) - 1, 64)};   // the running M-th largest
        if (__any(ts_key_less(thr, key))) top = top_merge<G>(top, key, gl);
      }
    }
    if (__any(pick)) {
      // the winners in ascending position; with fewer than M keys (the graph changed under the call) the rest are kNoPos
      const uint32_t j = ts_sort_ascending<G>(pick && gl < p.M && top.lo != 0 ? ts_key_position(top) : kNoPos, gl);
      if (pick && gl < p.M && j < static_cast<uint32_t>(N)) emit(gl, j);
    }
  }
}

bool ts_args_ok(const wm_tsample_args* a)
{
  return a != nullptr && a->n > 0 && a->n < (INT64_C(1) << 31) - 1 && a->n_nodes >= 0 && a->n_edges >= 0 && a->centers != nullptr &&
         a->center_times != nullptr && a->workspace != nullptr && ts_scalars_ok(a->max_sample_count, a->strategy);
}

ts_params ts_params_of(const wm_tsample_args* a)
{
  ts_params p{};
  p.g  = csr_view_of(*a);
  p.tm = csr_times_of(*a);
  p.centers = a->centers, p.center_times = a->center_times, p.n = a->n;
  p.M = a->max_sample_count, p.strategy = a->strategy, p.inclusive = a->inclusive, p.window = a->time_window, p.seed = a->random_seed;
  p.counts = a->counts, p.wave_sums = static_cast<int64_t*>(a->workspace), p.offsets = a->offsets;
  p.out_ids = a->out_ids, p.out_lid = a->out_center_lid, p.out_egid = a->out_edge_gid;
  return p;
}

template <typename IdT, typename ColT, int G>
int launch_select(const ts_params& p, hipStream_t stream)
{
  hipLaunchKernelGGL((tsample_select_kernel<IdT, ColT, G>), dim3(ts_blocks(p.n, G)), dim3(kTsBlock), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

// the per-wave sums of the count
size_t hip_tsample_workspace_bytes(int64_t n) { return ts_align(sizeof(int64_t) * static_cast<size_t>(ts_count_waves(n < 0 ? 0 : n))); }

// what the launchers refuse (-1, nothing queued): the host side has answered all of it before it gets here
int hip_tsample_count(const wm_tsample_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!ts_args_ok(a) || a->counts == nullptr || a->total == nullptr) return -1;
  const ts_params p = ts_params_of(a);
  const int blocks  = ts_blocks(a->n, kTsCountGroup);
  if (a->center_dtype == WHOLEMEMORY_DT_INT)
    hipLaunchKernelGGL((tsample_count_kernel<int32_t, kTsCountGroup>), dim3(blocks), dim3(kTsBlock), 0, stream, p);
  else if (a->center_dtype == WHOLEMEMORY_DT_INT64)
    hipLaunchKernelGGL((tsample_count_kernel<int64_t, kTsCountGroup>), dim3(blocks), dim3(kTsBlock), 0, stream, p);
  else
    return -1;
  if (hipGetLastError() != hipSuccess) return -2;
  hipLaunchKernelGGL(tsample_total_kernel, dim3(1), dim3(64), 0, stream, p.wave_sums, ts_count_waves(a->n), a->total);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int hip_tsample_select(const wm_tsample_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!ts_args_ok(a) || a->offsets == nullptr || a->out_ids == nullptr) return -1;
  const ts_params p = ts_params_of(a);
  return dispatch_id_col(a->center_dtype, a->col_dtype, [&](auto id, auto col) {
    using IdT  = decltype(id);
    using ColT = decltype(col);
    return a->max_sample_count <= 32 ? launch_select<IdT, ColT, 32>(p, stream) : launch_select<IdT, ColT, 64>(p, stream);
  });
}

}  // namespace wm
