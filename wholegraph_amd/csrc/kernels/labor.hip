// wholegraph_amd — LABOR layer-neighbour sampling over a CSR graph held in WholeMemory (gfx950 HIP; wholegraph_amd_ext.h section
// 2v): per centre i, neighbours of centers[i] chosen by the variate of the neighbour NODE (labor.hpp) — the M smallest (mode 0) or
// those below M / N (mode 1, LABOR-0) — in row order. Count, scan, one host round trip, select: the shape of tsample.hip. What
// differs is where the time goes: there is no per-edge attribute, the only array walked is col_ind, and the work per entry is
// the generator's initialisation (five 64-bit multiplies), so the kernels avoid drawing wherever the rules allow it.
//   - Count, mode 0: c_i = min(N, M) needs row_ptr alone. One LANE per centre, no col_ind read, nothing drawn.
//   - Count, mode 1: a group of kLbWalkGroup lanes per centre walks the row, kLbWalkBatch col_ind loads per lane issued back to
//     back, the variate and the predicate evaluated per entry, the takers counted by ballot and popcount. A row of at most M
//     entries is taken whole by the rule, so it is counted from row_ptr and not walked.
//   - Both keep a 64-bit sum per wave, which one wave adds up in a fixed order (the int32 scan cannot see a total of 2^31).
//   - Select, mode 1: the same walk, the predicate RECOMPUTED (no bitmask travels through the workspace: a row of N entries would
//     need N bits of it, and the entries are re-read anyway, for the ids); a survivor is placed by ballot and popcount and written
//     from the register its id was loaded into. A row with c == N is copied, nothing drawn.
//   - Select, mode 0: a group of G = 32 or 64 lanes per centre (M <= 32: two centres per wave). c == N: the row is copied, no key
//     drawn. Otherwise lane k holds the k-th largest two-word key seen so far, a batch above the running M-th key is merged by
//     top_merge.cuh, the winners' positions are sorted ascending and their ids loaded again (M loads).
// A col_ind value is copied and hashed, never used as an index. Groups past the end sit out (an empty row) but take part in the
// votes and shuffles; the trips of a wave are the same for all its lanes in every kernel. No atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../labor.hpp"
#include "../neg_sample.hpp"
#include "csr_view.cuh"
#include "top_merge.cuh"

namespace wm {
namespace {

constexpr int kLbBlock     = 256;    // lanes per block
constexpr int kLbMaxBlocks = 2048;   // the cap of every grid: 8 blocks per CU
// the walk of mode 1 (count and select): lanes per centre and col_ind loads a lane has in flight. 16 is the width of
// tsample.hip's count; neither was swept
constexpr int kLbWalkGroup = 16;
constexpr int kLbWalkBatch = 4;
constexpr int kLbTopBatch  = 2;      // loads in flight per lane of the mode-0 select (its group is 32 or 64 wide)
static_assert(kLbWalkGroup >= 2 && kLbWalkGroup <= 64 && (kLbWalkGroup & (kLbWalkGroup - 1)) == 0, "a power of two within a wave");

constexpr size_t lb_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

int lb_blocks(int64_t n, int group)
{
  const int64_t per_block = kLbBlock / group;
  const int64_t b         = (n + per_block - 1) / per_block;
  return static_cast<int>(b < 1 ? 1 : (b < kLbMaxBlocks ? b : kLbMaxBlocks));
}
int64_t lb_waves(int blocks) { return static_cast<int64_t>(blocks) * (kLbBlock / 64); }

struct lb_params {
  csr_view g;
  const void* centers;
  int64_t n;
  int M;
  uint64_t seed;
  int* counts;
  int64_t* wave_sums;
  const int* offsets;
  void* out_ids;
  int* out_lid;
  int64_t* out_egid;
};

// the row [s, s + N) of centre i. A group past the end, a centre that is no node and bounds that are no row: N = 0
template <typename IdT>
__device__ __forceinline__ int lb_row(const lb_params& p, int64_t i, int64_t* s)
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

// the votes of the G lanes from `first` on
template <int G>
__device__ __forceinline__ unsigned long long lb_slice(unsigned long long ballot, int first)
{
  constexpr unsigned long long kSlice = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
  return (ballot >> first) & kSlice;
}

// the largest v of the wave's groups, v being the same in all lanes of a group: what makes a walk's trips wave-uniform
template <int G>
__device__ __forceinline__ int lb_wave_max(int v)
{
  int m = __builtin_amdgcn_readlane(v, 0);
#pragma unroll
  for (int f = G; f < 64; f += G) m = max(m, __builtin_amdgcn_readlane(v, f));
  return m;
}

// kLbWalkBatch or kLbTopBatch entries of the row per lane, the loads of a trip going out together: ONE guard (a group whose row
// is not walked loads nothing), the index clamped to the row. (64-bit: N may be 2^31 - 1, r + k * G + gl passes it)
template <typename ColT, int G, int B>
__device__ __forceinline__ void lb_load(const lb_params& p, int64_t s, int N, int64_t r, int gl, ColT (&cv)[B])
{
#pragma unroll
  for (int k = 0; k < B; k++) cv[k] = 0;
  if (N > 0) {
#pragma unroll
    for (int k = 0; k < B; k++) cv[k] = gref_load<ColT>(p.g.col_ptr, p.g.col_off + s + min(r + k * G + gl, static_cast<int64_t>(N) - 1));
  }
}

// the counts of a wave's centres summed over the wave, one word per wave
__device__ __forceinline__ void lb_store_wave_sum(const lb_params& p, long long wave_sum)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wave_sum += __shfl_xor(wave_sum, d, 64);
  if ((threadIdx.x & 63) == 0) p.wave_sums[static_cast<int64_t>(blockIdx.x) * (kLbBlock / 64) + (threadIdx.x >> 6)] = wave_sum;
}

__device__ __forceinline__ void lb_store_count(const lb_params& p, int64_t i, int cnt)
{
  p.counts[i] = cnt;
  if (i == p.n - 1) p.counts[p.n] = 0;   // the scan runs over n + 1 entries
}

// mode 0: min(N, M) per centre from row_ptr alone, a lane per centre
template <typename IdT>
__global__ __launch_bounds__(kLbBlock) void labor_count_fixed_kernel(lb_params p)
{
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kLbBlock;
  long long wave_sum   = 0;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kLbBlock; base < p.n; base += stride) {   // block-uniform trips
    const int64_t i = base + threadIdx.x;
    int64_t s;
    const int cnt = labor_fixed_count(lb_row<IdT>(p, i, &s), p.M);
    if (i < p.n) {
      lb_store_count(p, i, cnt);
      wave_sum += cnt;
    }
  }
  lb_store_wave_sum(p, wave_sum);
}

// mode 1: the takers of every row longer than M, by a walk of G lanes
template <typename IdT, typename ColT, int G>
__global__ __launch_bounds__(kLbBlock) void labor_count_poisson_kernel(lb_params p)
{
  constexpr int kPerBlock = kLbBlock / G;
  const int gl            = static_cast<int>(threadIdx.x) & (G - 1);
  const int first         = static_cast<int>(threadIdx.x) & 63 & ~(G - 1);   // the group's first lane in its wave
  const int64_t stride    = static_cast<int64_t>(gridDim.x) * kPerBlock;
  long long wave_sum      = 0;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kPerBlock; base < p.n; base += stride) {   // block-uniform trips
    const int64_t i = base + threadIdx.x / G;
    int64_t s;
    const int N      = lb_row<IdT>(p, i, &s);
    const int walk   = N > p.M ? N : 0;   // a row of at most M entries is taken whole: not read
    const int n_wave = lb_wave_max<G>(walk);
    int taken        = 0;
    for (int64_t r = 0; r < n_wave; r += G * kLbWalkBatch) {   // wave-uniform trips
      ColT cv[kLbWalkBatch];
      lb_load<ColT, G>(p, s, walk, r, gl, cv);
#pragma unroll
      for (int k = 0; k < kLbWalkBatch; k++) {
        const bool ok = r + k * G + gl < walk && labor_takes(labor_variate(p.seed, static_cast<int64_t>(cv[k])), walk, p.M);
        taken += __popcll(lb_slice<G>(__ballot(ok), first));
      }
    }
    if (gl == 0 && i < p.n) {
      const int cnt = walk > 0 ? taken : N;
      lb_store_count(p, i, cnt);
      wave_sum += cnt;
    }
  }
  lb_store_wave_sum(p, wave_sum);
}

// one wave adds the per-wave sums up: a fixed order, and a word the host may be reading from pinned memory
__global__ __launch_bounds__(64) void labor_total_kernel(const int64_t* wave_sums, int64_t n_waves, int64_t* total)
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

template <typename IdT, typename ColT, int G, bool kPoisson>
__global__ __launch_bounds__(kLbBlock) void labor_select_kernel(lb_params p)
{
  constexpr int kPerBlock   = kLbBlock / G;
  constexpr int kBatch      = kPoisson ? kLbWalkBatch : kLbTopBatch;
  const int lane            = static_cast<int>(threadIdx.x) & 63;
  const int gl              = lane & (G - 1);
  const int gbase           = lane & ~(G - 1);
  const int64_t stride      = static_cast<int64_t>(gridDim.x) * kPerBlock;
  ColT* out                 = static_cast<ColT*>(p.out_ids);
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kPerBlock; base < p.n; base += stride) {   // block-uniform trips
    const int64_t i = base + threadIdx.x / G;
    int64_t s;
    int N   = lb_row<IdT>(p, i, &s);
    int off = 0, c = 0;
    if (i < p.n) off = p.offsets[i], c = p.offsets[i + 1] - off;
    if (c <= 0) N = 0;   // nothing to emit: the row is not read again
    const bool whole = c == N;   // the count kept every entry: the row is copied, nothing is drawn
    const int n_wave = lb_wave_max<G>(N);
    auto emit = [&](int k, int64_t j, ColT id) {   // k < c at every call
      out[off + k] = id;
      if (p.out_lid != nullptr) p.out_lid[off + k] = static_cast<int>(i);
      if (p.out_egid != nullptr) p.out_egid[off + k] = s + j;
    };
    ts_key top{0, 0};
    int emitted = 0;
    for (int64_t r = 0; r < n_wave; r += G * kBatch) {   // wave-uniform trips: the groups of a wave share votes and shuffles
      ColT cv[kBatch];
      lb_load<ColT, G>(p, s, N, r, gl, cv);
#pragma unroll
      for (int k = 0; k < kBatch; k++) {
        if (r + k * G >= n_wave) break;
        const int64_t j = r + k * G + gl;
        const bool in   = j < N;
        if constexpr (kPoisson) {
          const bool take = in && (whole || labor_takes(labor_variate(p.seed, static_cast<int64_t>(cv[k])), N, p.M));
          const unsigned long long mine = lb_slice<G>(__ballot(take), gbase);
          const int rank                = emitted + __popcll(mine & ((1ull << gl) - 1ull));
          if (take && rank < c) emit(rank, j, cv[k]);
          emitted += __popcll(mine);
        } else {
          if (whole && in) emit(static_cast<int>(j), j, cv[k]);   // (j < N == c)
          ts_key key{0, 0};
          if (!whole && in) key = labor_key(labor_variate(p.seed, static_cast<int64_t>(cv[k])), static_cast<uint32_t>(j));
          const ts_key thr = {__shfl(static_cast<unsigned long long>(top.hi), gbase + max(p.M, 1) - 1, 64),
                              __shfl(top.lo, gbase + max(p.M, 1) - 1, 64)};   // the running M-th largest
          if (__any(ts_key_less(thr, key))) top = top_merge<G>(top, key, gl);
        }
      }
    }
    if constexpr (!kPoisson) {
      constexpr uint32_t kNoPos = 0xFFFFFFFFu;   // no position: behind every position in the sort, refused by the row check
      const bool pick           = !whole && N > 0;   // (then c == M: the count saw more than M entries)
      if (__any(pick)) {
        // the winners in ascending position; with fewer than M keys (the graph changed under the call) the rest are kNoPos
        const uint32_t j = top_sort_ascending<G>(pick && gl < p.M && top.lo != 0 ? ts_key_position(top) : kNoPos, gl);
        if (pick && gl < p.M && gl < c && j < static_cast<uint32_t>(N)) emit(gl, j, gref_load<ColT>(p.g.col_ptr, p.g.col_off + s + j));
      }
    }
  }
}

bool lb_args_ok(const wm_labor_args* a)
{
  return a != nullptr && a->n > 0 && a->n < (INT64_C(1) << 31) - 1 && a->n_nodes >= 0 && a->n_edges >= 0 && a->centers != nullptr &&
         a->workspace != nullptr && labor_scalars_ok(a->max_sample_count, a->mode);
}

lb_params lb_params_of(const wm_labor_args* a)
{
  lb_params p{};
  p.g       = csr_view_of(*a);
  p.centers = a->centers, p.n = a->n, p.M = a->max_sample_count, p.seed = a->random_seed;
  p.counts = a->counts, p.wave_sums = static_cast<int64_t*>(a->workspace), p.offsets = a->offsets;
  p.out_ids = a->out_ids, p.out_lid = a->out_center_lid, p.out_egid = a->out_edge_gid;
  return p;
}

template <typename IdT, typename ColT, int G, bool kPoisson>
int launch_select(const lb_params& p, hipStream_t stream)
{
  hipLaunchKernelGGL((labor_select_kernel<IdT, ColT, G, kPoisson>), dim3(lb_blocks(p.n, G)), dim3(kLbBlock), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

// the per-wave sums of the count: the walk of mode 1 has the larger grid
size_t hip_labor_workspace_bytes(int64_t n)
{
  return lb_align(sizeof(int64_t) * static_cast<size_t>(lb_waves(lb_blocks(n < 0 ? 0 : n, kLbWalkGroup))));
}

// what the launchers refuse (-1, nothing queued): the host side has answered all of it before it gets here
int hip_labor_count(const wm_labor_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!lb_args_ok(a) || a->counts == nullptr || a->total == nullptr) return -1;
  const lb_params p = lb_params_of(a);
  const int blocks  = lb_blocks(a->n, a->mode == 0 ? 1 : kLbWalkGroup);
  const int rc      = dispatch_id_col(a->center_dtype, a->col_dtype, [&](auto id, auto col) {
    using IdT  = decltype(id);
    using ColT = decltype(col);
    if (a->mode == 0)
      hipLaunchKernelGGL((labor_count_fixed_kernel<IdT>), dim3(blocks), dim3(kLbBlock), 0, stream, p);
    else
      hipLaunchKernelGGL((labor_count_poisson_kernel<IdT, ColT, kLbWalkGroup>), dim3(blocks), dim3(kLbBlock), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  });
  if (rc != 0) return rc;
  hipLaunchKernelGGL(labor_total_kernel, dim3(1), dim3(64), 0, stream, p.wave_sums, lb_waves(blocks), a->total);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int hip_labor_select(const wm_labor_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!lb_args_ok(a) || a->offsets == nullptr || a->out_ids == nullptr) return -1;
  const lb_params p = lb_params_of(a);
  return dispatch_id_col(a->center_dtype, a->col_dtype, [&](auto id, auto col) {
    using IdT  = decltype(id);
    using ColT = decltype(col);
    if (a->mode == 1) return launch_select<IdT, ColT, kLbWalkGroup, true>(p, stream);
    return a->max_sample_count <= 32 ? launch_select<IdT, ColT, 32, false>(p, stream) : launch_select<IdT, ColT, 64, false>(p, stream);
  });
}

}  // namespace wm
