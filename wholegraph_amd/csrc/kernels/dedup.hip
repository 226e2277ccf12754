// wholegraph_amd — the owner-side id sort: gradient de-duplication in front of the fused step (optim.hip), and the locality
// sort of gathered ids (gfx950 HIP). Reference behaviour (cpp/src/wholememory_ops/functions/exchange_embeddings_nccl_func.cu:
// 76-174): stable radix sort of received ids (payload = receive position) -> unique_by_key.
//
// The id sort itself is rocPRIM's radix sort restricted to the significant key bits
// (ids at the owner are non-negative and < table rows): same stable order as the reference's
// full-width signed sort, fewer passes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

// rocPRIM's radix sort copies its inputs to scratch first whenever input and output "can alias", and answers "yes" for
// every iterator that is not a plain pointer (detail/various.hpp) — 26 us per 10 M (key, position) pairs for the narrowing
// key iterator and the counting payload used below. The exact answers for those two, declared before the sort's templates
// are defined (the call there is a qualified name: only overloads visible at that point take part):
#include <iterator>
#include <rocprim/config.hpp>
#include <rocprim/detail/various.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
namespace wm {
// random-access iterator over ids[i] - base, narrowed to 32 bits (rocprim::transform_iterator keeps its pointer private).
// An id outside [base, base + span) — negative ("skip me") or past the range — reads as the key `span`: all such ids sort
// behind every real key, as ONE run that the run detection drops (see run_dedup).
template <typename InT>
struct narrow_key_iterator {
  using value_type        = uint32_t;
  using reference         = uint32_t;
  using pointer           = const uint32_t*;
  using difference_type   = std::ptrdiff_t;
  using iterator_category = std::random_access_iterator_tag;
  const InT* ptr;  // InT is the UNSIGNED index type: a negative id is a huge offset
  InT base;
  uint32_t span;
  __host__ __device__ uint32_t key(InT v) const
  {
    const InT off = v - base;
    return off < static_cast<InT>(span) ? static_cast<uint32_t>(off) : span;
  }
  __host__ __device__ uint32_t operator*() const { return key(*ptr); }
  __host__ __device__ uint32_t operator[](difference_type i) const { return key(ptr[i]); }
  __host__ __device__ narrow_key_iterator operator+(difference_type d) const { return {ptr + d, base, span}; }
  __host__ __device__ narrow_key_iterator operator-(difference_type d) const { return {ptr - d, base, span}; }
  __host__ __device__ difference_type operator-(const narrow_key_iterator& o) const { return ptr - o.ptr; }
  __host__ __device__ narrow_key_iterator& operator+=(difference_type d) { ptr += d; return *this; }
  __host__ __device__ narrow_key_iterator& operator-=(difference_type d) { ptr -= d; return *this; }
  __host__ __device__ narrow_key_iterator& operator++() { ++ptr; return *this; }
  __host__ __device__ narrow_key_iterator operator++(int) { narrow_key_iterator t = *this; ++ptr; return t; }
  __host__ __device__ narrow_key_iterator& operator--() { --ptr; return *this; }
  __host__ __device__ narrow_key_iterator operator--(int) { narrow_key_iterator t = *this; --ptr; return t; }
  __host__ __device__ bool operator==(const narrow_key_iterator& o) const { return ptr == o.ptr; }
  __host__ __device__ bool operator!=(const narrow_key_iterator& o) const { return ptr != o.ptr; }
  __host__ __device__ bool operator<(const narrow_key_iterator& o) const { return ptr < o.ptr; }
};
}  // namespace wm
BEGIN_ROCPRIM_NAMESPACE
namespace detail {
template <class InT, class Out>
inline bool can_iterators_alias(::wm::narrow_key_iterator<InT> it, Out* out, const size_t size)
{
  return can_iterators_alias(it.ptr, out, size);  // the ids array against the output array
}
template <class I, class D, class Out>
inline bool can_iterators_alias(counting_iterator<I, D>, Out*, const size_t)
{
  return false;  // generates its values, reads no memory
}
}  // namespace detail
END_ROCPRIM_NAMESPACE
#include <rocprim/rocprim.hpp>

#include "../knobs.hpp"
#include "../backend.hpp"
#include "../wm_common.hpp"
#include "device_common.cuh"
#include "onesweep.cuh"
#include "split_sort.cuh"
#include "sort_handoff.cuh"

#include <atomic>
#include <mutex>
#include <wholememory/wholegraph_amd_ext.h>

namespace wm {
namespace {

constexpr int kBlock = 256;

// Run detection over the sorted keys, three small launches instead of head-flags + a device-wide scan + compaction
// (10 M keys: 185 us -> ~65 us): a tile is kRunTile consecutive sorted keys;
//   run_count_kernel   heads per tile (a head = first key, or a key that differs from its predecessor)
//   run_scan_kernel    one workgroup: exclusive prefix of the tile counts (a few thousand numbers) + the total
//   run_compact_kernel recomputes its tile's heads, ranks them with a block scan on top of the tile's prefix and writes
//                      unique_ids[rank] (widened to the caller's index type) and run_starts[rank]; the last tile adds the
//                      closing run_starts entry and the count.
// No tile waits for another one (a chained look-back scan serialises on the prefix hand-over while thousands of tiles are
// resident), and the keys are read twice out of L2 / Infinity Cache rather than flags and ranks written and re-read.
constexpr int kRunItems = 8;
constexpr int kRunTile  = kBlock * kRunItems;  // 2048 keys

template <typename KeyT>
__device__ __forceinline__ int tile_heads(const KeyT* sorted, int64_t n, int64_t base, bool head[kRunItems], KeyT key[kRunItems])
{
  // thread t owns keys base + t * kRunItems + [0, kRunItems): contiguous, so its heads are already in rank order
  const int64_t first = base + static_cast<int64_t>(threadIdx.x) * kRunItems;
  KeyT prev           = first > 0 && first <= n ? sorted[first - 1] : KeyT(0);
  int heads           = 0;
  if (first + kRunItems <= n && (reinterpret_cast<uint64_t>(sorted) & 15) == 0) {
    // the thread's 8 keys as whole 16-byte loads (the sorted array starts on a 256-byte boundary and `first` is a multiple of
    // 8 keys): element-wise guarded loads at a 32-byte lane stride made the two run-detection kernels 23 + 33 us per 10 M keys
    typedef uint32_t raw4 __attribute__((ext_vector_type(4)));
    constexpr int kVecs = static_cast<int>(sizeof(KeyT)) * kRunItems / 16;
    raw4 raw[kVecs];
#pragma unroll
    for (int v = 0; v < kVecs; v++) raw[v] = reinterpret_cast<const raw4*>(sorted + first)[v];
    __builtin_memcpy(key, raw, sizeof(KeyT) * kRunItems);
#pragma unroll
    for (int i = 0; i < kRunItems; i++) {
      head[i] = (first + i == 0) || key[i] != prev;
      prev    = key[i];
      heads += head[i] ? 1 : 0;
    }
    return heads;
  }
#pragma unroll
  for (int i = 0; i < kRunItems; i++) {
    const int64_t g = first + i;
    key[i]          = g < n ? sorted[g] : KeyT(0);
    head[i]         = g < n && (g == 0 || key[i] != prev);
    prev            = key[i];
    heads += head[i] ? 1 : 0;
  }
  return heads;
}

__device__ __forceinline__ int block_exclusive_sum(int v, int* total)
{
  __shared__ int wave_sums[kBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_sums[wv] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; w++) {
    if (w < wv) before += wave_sums[w];
    all += wave_sums[w];
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// `gate` (all three kernels): device word, 0 = the split sort has already written the runs, return at once (nullptr: always run)
template <typename KeyT>
__global__ __launch_bounds__(kBlock) void run_count_kernel(const KeyT* sorted, int64_t n, int32_t* tile_counts, const uint32_t* gate)
{
  if (gate != nullptr && *gate == 0u) return;
  // (a bounded grid that walks the tiles: gated off, a launch of 4883 workgroups that only read the gate still takes ~7 us of
  // the machine, of 1024 about 3)
  const int n_tiles = static_cast<int>((n + kRunTile - 1) / kRunTile);
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    bool head[kRunItems];
    KeyT key[kRunItems];
    const int heads = tile_heads(sorted, n, static_cast<int64_t>(tile) * kRunTile, head, key);
    int total;
    (void)block_exclusive_sum(heads, &total);
    if (threadIdx.x == 0) tile_counts[tile] = total;
  }
}

// `last_key` / `drop_key`: when the LAST sorted key equals drop_key (the out-of-range marker of narrow_key_iterator), its run —
// the last one — does not count (last_key == nullptr: nothing is dropped)
__global__ __launch_bounds__(1024) void run_scan_kernel(int32_t* tile_counts, int n_tiles, int64_t* n_unique,
                                                        const uint32_t* last_key, uint32_t drop_key, const uint32_t* gate)
{
  if (gate != nullptr && *gate == 0u) return;
  // one workgroup walks the tile counts in chunks of 1024, carrying the running total
  __shared__ int wave_sums[16];
  __shared__ int carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int base = 0; base < n_tiles; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < n_tiles ? tile_counts[i] : 0;
    int incl    = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sums[wv] = incl;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wv; w++) before += wave_sums[w];
    if (i < n_tiles) tile_counts[i] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_unique = carry_s - (last_key != nullptr && *last_key == drop_key ? 1 : 0);
}

template <typename KeyT, typename OutT>
__global__ __launch_bounds__(kBlock) void run_compact_kernel(const KeyT* sorted, int64_t n, const int32_t* tile_prefix,
                                                             const int64_t* n_unique, OutT* unique_ids, int32_t* run_starts,
                                                             OutT key_base, bool drop_last, KeyT drop_key, const uint32_t* gate)
{
  if (gate != nullptr && *gate == 0u) return;
  // heads are ranked inside the tile, parked in LDS at their rank and written out as two coalesced streams (a thread's
  // own heads are kRunItems apart in rank order: written directly they cost a scattered store per item — 82 us vs ~35)
  __shared__ KeyT s_key[kRunTile];
  __shared__ int32_t s_pos[kRunTile];
  const int n_tiles = static_cast<int>((n + kRunTile - 1) / kRunTile);
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    bool head[kRunItems];
    KeyT key[kRunItems];
    const int64_t base = static_cast<int64_t>(tile) * kRunTile;
    const int heads    = tile_heads(sorted, n, base, head, key);
    int total;
    int rank = block_exclusive_sum(heads, &total);
#pragma unroll
    for (int i = 0; i < kRunItems; i++) {
      if (head[i]) {
        s_key[rank] = key[i];
        s_pos[rank] = static_cast<int32_t>(base + static_cast<int64_t>(threadIdx.x) * kRunItems + i);
        rank++;
      }
    }
    __syncthreads();
    const int64_t out0 = tile_prefix[tile];
    for (int i = threadIdx.x; i < total; i += kBlock) {
      // ids are stored in the caller's (signed) index type: the keys are its two's-complement bits, possibly narrowed to
      // 32 bits when the caller bounded them (then they are non-negative and the widening is exact)
      const KeyT k         = s_key[i];
      // (key_base: the keys were sorted relative to the first row of the owner's range, see run_dedup)
      unique_ids[out0 + i] = (sizeof(KeyT) == sizeof(OutT) ? static_cast<OutT>(k) : static_cast<OutT>(static_cast<uint64_t>(k))) + key_base;
      run_starts[out0 + i] = s_pos[i];
    }
    // end marker — unless the out-of-range run was dropped: then its own start (written above, at index *n_unique) ends the
    // last real run
    if (tile == n_tiles - 1 && threadIdx.x == 0 && !(drop_last && sorted[n - 1] == drop_key))
      run_starts[*n_unique] = static_cast<int32_t>(n);
    __syncthreads();   // s_key / s_pos are reused by the block's next tile
  }
}

inline unsigned significant_bits(int64_t upper_bound, unsigned full)
{
  if (upper_bound <= 0) return full;
  unsigned b = 1;
  while (b < full && (static_cast<uint64_t>(upper_bound - 1) >> b) != 0) b++;
  return b;
}

// keys narrowed on the fly: ids the caller bounded to a range of less than 2^32 rows are sorted as 32-bit keys RELATIVE to
// the start of the range (8 + 4 bytes per element and pass instead of 8 + 8, and only the bits of the range's width: a
// 125 M-row shard of a 1 B-row table sorts 27 bits in 3 passes, not 30 in 4) ... the first pass reads the ids through this
// iterator (narrow_key_iterator, top of the file), no conversion pass

// rocPRIM's onesweep with 9 radix bits per pass and 1024 x 8 keys per workgroup: ids of a 100 M-row shard (27 bits) sort
// in 3 passes instead of the tuned default's 4 x 8 bits (10 M (key, position) pairs: 398 -> 251 us;
// experiments/sort_variants.hip has the sweep). 64-bit keys keep the library default.
constexpr int64_t kSortRadixMin = 3 << 16;   // 196608 (crossover between 131072 and 262144 items: profiles/r04_small_sort.txt)
template <typename SortKeyT>
struct sort_config {
  using type = rocprim::default_config;
};
template <>
struct sort_config<uint32_t> {
  using type = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, 12>, rocprim::kernel_config<1024, 8>, 9,
                                        rocprim::block_radix_rank_algorithm::match>>;
};

// rocPRIM sorts up to 2^20 items with a MERGE sort (radix_sort_config's MergeSortLimit): block sort + 10 merge passes of two
// launches each for 1 M (key, position) pairs — 160 us where three onesweep passes over 24 bits take ~70 (the batch of a cached
// C1 gather, the gradients of a 1024-seed mini-batch: profiles/r04_small_sort.txt). The second configuration never merges;
// sort_pairs32 picks by size (WM_SORT_RADIX_MIN, items from which the radix passes are taken).
struct sort_config_radix32 {
  using type = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, 12>, rocprim::kernel_config<1024, 8>, 9,
                                        rocprim::block_radix_rank_algorithm::match>,
    0>;
};
inline int64_t sort_radix_min()
{
  const char* e = WM_KNOB("WM_SORT_RADIX_MIN");
  return e != nullptr && atoll(e) > 0 ? atoll(e) : kSortRadixMin;
}
template <typename KeysIn, typename ValsIn>
hipError_t sort_pairs32(void* temp, size_t& temp_bytes, KeysIn keys, uint32_t* keys_out, ValsIn vals, int32_t* vals_out, size_t n,
                        unsigned lo, unsigned hi, hipStream_t stream)
{
  if (temp == nullptr) {   // size query: room for either configuration
    size_t a = 0, b = 0;
    hipError_t e = rocprim::radix_sort_pairs<sort_config<uint32_t>::type>(nullptr, a, keys, keys_out, vals, vals_out, n, lo, hi, stream);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs<sort_config_radix32::type>(nullptr, b, keys, keys_out, vals, vals_out, n, lo, hi, stream);
    temp_bytes = std::max(a, b);
    return e;
  }
  if (static_cast<int64_t>(n) >= sort_radix_min())
    return rocprim::radix_sort_pairs<sort_config_radix32::type>(temp, temp_bytes, keys, keys_out, vals, vals_out, n, lo, hi, stream);
  return rocprim::radix_sort_pairs<sort_config<uint32_t>::type>(temp, temp_bytes, keys, keys_out, vals, vals_out, n, lo, hi, stream);
}

template <typename SortKeyT>
struct dedup_layout {
  SortKeyT* sorted;
  int32_t* tile_counts;
  void* temp;
  size_t temp_bytes;
  size_t total;
};

// ---- the split sort (split_sort.cuh) in front of the generic sort --------------------------------------------------------
// Batches of bounded ids (the owner's row range is known) from kSplitMin ids up take the two-stage split sort; what it cannot
// take — a bucket that does not fit LDS — it finds out on the device, so the generic path (onesweep.cuh + the run detection
// above, every kernel gated on the split sort's overflow word) is enqueued behind it either way: ~7 launches that return at
// once in the usual case. WM_DEDUP_SPLIT=0 switches the split sort off, WM_DEDUP_SPLIT_MIN moves the threshold.
constexpr int64_t kSplitMin = 1 << 16;
constexpr int kOswBlock = 512, kOswIpt = 16;   // profiles/r03_onesweep_ab.txt
inline int64_t split_min()
{
  const char* off = WM_KNOB("WM_DEDUP_SPLIT");
  if (off != nullptr && off[0] == '0') return INT64_MAX;
  const char* e = WM_KNOB("WM_DEDUP_SPLIT_MIN");
  return e != nullptr && atoll(e) > 0 ? atoll(e) : kSplitMin;
}
// The generic path's ~7 launches return at once in the usual case, but each still costs 5-8 us of the stream's time (47 us per
// call in profiles/r05_grad_timeline_serial.txt). They depend on nothing but the overflow word (known after the split sort's
// SECOND kernel), so they go to a side stream that forks there and joins after the split sort's last kernel: idle, they hide
// under its two long kernels; when the batch overflowed, those two return at once and the caller's stream waits for the side.
__global__ void waits_probe_set_kernel(uint32_t* word) { __hip_atomic_store(word, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }
struct sort_lane {
  std::mutex mu;   // one fork .. join sequence at a time: the events are shared
  // Do two kernels on two streams of this device RUN side by side? Every device-side wait of the gradient path needs that (a wave
  // polls a word another stream's kernel sets). Measured once per device, when the lane is made: a one-wave kernel waits ~10 ms
  // at most for a word that a kernel on the other stream sets. A tool that executes one kernel at a time (any tool: round 5
  // only knew rocprofv3's counter collection by its environment variables) lets the wait give up -> events only, for the
  // life of the process, one WARN line.
  bool waits_work = true;
  hipStream_t stream = nullptr, stream_high = nullptr;
  hipEvent_t forked = nullptr, joined = nullptr;
  bool ok = false;
  hipStream_t side() const
  {
    const char* pe = WM_KNOB("WM_DEDUP_LANE_PRIO");
    return pe != nullptr && pe[0] == 'h' ? stream_high : stream;
  }
  // Fork without an event on the caller's stream: the split sort's scan kernel publishes "verdict final" = the sort's sequence
  // number in one word of this ring (zero at the start, values only grow, a word comes round again after kRing sorts), and the
  // side stream's first kernel waits for it (split_wait_kernel). An event recorded between the scan and the scatter kernel
  // delayed the scatter kernel by ~7 us on every call (profiles/r05_grad_timeline_split_sort.txt: "gap 7.1").
  static constexpr uint32_t kRing = 4096;
  uint32_t* ring = nullptr;
  uint32_t seq   = 0;
  // Which sort a batch gets follows the batches before it (run_dedup: "adaptive route"). Per row range (lower, upper) of the
  // sorted ids: did the last split sort (or probe) overflow a bucket? The word is copied to pinned memory behind the kernels
  // that decide it and read by the host without synchronising, so it lags a call.
  static constexpr int kAdapt = 8, kProbeEvery = 4;
  struct adapt_entry {
    int64_t lower = -1, upper = -1;
    unsigned calls = 0;
    bool generic = false;   // the range's batches go to rocPRIM's sort (its last split sort or probe overflowed)
  };
  adapt_entry adapt[kAdapt];
  // pinned, one word per row range: the overflow word of its last split sort or probe
  volatile int32_t* adapt_flags = nullptr;
  unsigned adapt_generation     = ~0u;       // a knob reload forgets what was learnt (tests, A/B runs)
  int adapt_next                = 0;
  void* probe_ws                = nullptr;   // split::probe_workspace_bytes(), allocated at the first probe
  int adapt_slot(int64_t lower, int64_t upper)
  {
    if (adapt_flags == nullptr) {
      void* h = nullptr;
      if (hipHostMalloc(&h, kAdapt * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) return -1;
      adapt_flags = static_cast<volatile int32_t*>(h);
      for (int i = 0; i < kAdapt; i++) adapt_flags[i] = 0;
    }
    const unsigned g = g_knob_generation.load(std::memory_order_acquire);
    if (g != adapt_generation) {
      for (int i = 0; i < kAdapt; i++) adapt[i] = adapt_entry{}, adapt_flags[i] = 0;
      adapt_generation = g;
    }
    for (int i = 0; i < kAdapt; i++)
      if (adapt[i].lower == lower && adapt[i].upper == upper) return i;
    const int i = adapt_next;
    adapt_next  = (adapt_next + 1) % kAdapt;
    adapt[i]    = adapt_entry{lower, upper, 0, false};
    adapt_flags[i] = 0;
    return i;
  }
  // Device-side waits that gave up (split_sort.cuh: wait_cfg) leave their code in this word of pinned, device-mapped host
  // memory — split_join_kernel ORs it in after it has turned the failed sort into "no runs", split_wait_kernel when it stops
  // waiting. The host looks at it (take_error) whenever it enters the sort or the join and after every synchronise of the
  // gradient path (backend: device_error): a stalled wait becomes WHOLEMEMORY_CUDA_ERROR with one ERROR line, never a step
  // applied over runs that were not final.
  volatile uint32_t* host_err = nullptr;   // pinned
  uint32_t* host_err_dev      = nullptr;   // the same word as the device addresses it
  uint32_t take_error()
  {
    if (host_err == nullptr) return 0;
    const uint32_t e = *host_err;
    if (e != 0) *host_err = 0;
    return e;
  }
  sort_lane()
  {
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) == hipSuccess) {
      void* d = nullptr;
      if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
        host_err     = static_cast<volatile uint32_t*>(h);
        *host_err    = 0;
        host_err_dev = static_cast<uint32_t*>(d);
      } else {
        (void)hipHostFree(h);
      }
    }
    // two streams, plain and highest priority; WM_DEDUP_LANE_PRIO=n|h picks one per call (see side())
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    ok = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithPriority(&stream_high, hipStreamNonBlocking, greatest) == hipSuccess &&
         hipEventCreateWithFlags(&forked, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&joined, hipEventDisableTiming) == hipSuccess;
    if (ok) {
      void* r = nullptr;
      if (hipMalloc(&r, kRing * sizeof(uint32_t)) == hipSuccess) {
        if (hipMemsetAsync(r, 0, kRing * sizeof(uint32_t), stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess)
          ring = static_cast<uint32_t*>(r);
        else
          (void)hipFree(r);
      }
    }
    if (ok) {
      uint32_t* probe = nullptr;   // [0] the word waited for, [1] the waiter's error word
      if (hipMalloc(reinterpret_cast<void**>(&probe), 2 * sizeof(uint32_t)) == hipSuccess) {
        uint32_t err = 1;
        if (hipMemsetAsync(probe, 0, 2 * sizeof(uint32_t), stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess) {
          hipLaunchKernelGGL(split::split_wait_kernel, dim3(1), dim3(64), 0, stream, probe, 1u, probe + 1, 6000u, static_cast<uint32_t*>(nullptr));
          hipLaunchKernelGGL(waits_probe_set_kernel, dim3(1), dim3(1), 0, stream_high, probe);
          if (hipStreamSynchronize(stream_high) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess &&
              hipMemcpy(&err, probe + 1, sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess && err != 0) {
            waits_work = false;
            WM_WARN("kernels on two streams of this device do not run side by side (a tool that executes one kernel at a time?): "
                    "the gradient path synchronises its side streams with events only");
          }
        }
        (void)hipFree(probe);
      }
    }
  }
  // one lane per DEVICE (round 6; a process-wide one put device 0's streams, ring and events under device 1's kernels): created
  // on the device that is current at the first call that needs it there, kept for the life of the process
  static sort_lane& get() { return per_device<sort_lane>(); }
};
// Kernels that wait for a word another stream's kernel sets (split_wait_kernel, split_join_kernel) need that other kernel to be
// able to RUN beside them. A tool that lets one kernel execute at a time — rocprofv3's counter collection does, and not in
// submission order: the --pmc passes of scripts/collect_profiles.sh sat in a waiter until their timeout — turns every such
// wait into a hang. So: events only (the round's first arrangement, ~20 us slower per call) when rocprofv3 collects counters
// (it exports ROCPROF_COUNTER_COLLECTION to the profiled process) or when WM_DEVICE_WAITS=0 says so.
inline bool device_waits_allowed()
{
  const char* e = WM_KNOB("WM_DEVICE_WAITS");
  if (e != nullptr) return e[0] != '0';
  if (WM_KNOB("ROCPROF_COUNTER_COLLECTION") != nullptr || WM_KNOB("ROCPROF_COUNTERS") != nullptr) return false;
  return sort_lane::get().waits_work;   // (round 6: measured per device, whatever the tool is called)
}
// limits of the device-side waits (split_sort.cuh: wait_cfg). WM_DEBUG_SPIN_LIMIT=n shortens every one of them to n polls and
// WM_DEBUG_STALL=lookback|join keeps a gate shut (a stage-2 bucket that never publishes / a generic path that never reports
// done): tests/test_dedup_split_gpu.py forces each timeout and sees the error code and an untouched table.
inline split::wait_cfg wait_limits(const split::plan* sp = nullptr)
{
  split::wait_cfg wc;
  if (const char* e = WM_KNOB("WM_DEBUG_SPIN_LIMIT")) {
    const long long v = atoll(e);
    if (v > 0 && v < (1ll << 31)) wc.look_back_polls = wc.join_polls = wc.wait_polls = static_cast<uint32_t>(v);
  }
  const char* st = WM_KNOB("WM_DEBUG_STALL");
  if (st != nullptr && st[0] == 'l' && sp != nullptr) wc.stall_bucket = sp->buckets / 2;
  return wc;
}
inline bool stall_join() { const char* st = WM_KNOB("WM_DEBUG_STALL"); return st != nullptr && st[0] == 'j'; }
std::atomic<int64_t> g_split_sorts{0};
// The optimizer step that follows a split sort on the same thread finds the sort's control words through the run_starts array
// both were given: its long-run counters live there (zeroed by the sort's first kernel: no fill in front of the step), and
// the listing kernels return at once when the sort saw neither an overflow nor a bucket with a run of more than kMaxDup ids —
// then no run is longer than kMaxDup, far below any long-run threshold (fill 5.7 + listing 13 us per call otherwise).
// The record is cleared by EVERY id sort of the thread (whatever path it takes) and consumed by the next step, and it has to
// match the three arrays a sort hands to a step — run starts, unique ids, run count — so a step can only pick up the control
// words of the sort that produced exactly its inputs, whose workspace its caller still holds.
struct last_split_record {
  const int32_t* run_starts = nullptr;
  const void* unique_ids    = nullptr;
  const int64_t* n_unique   = nullptr;
  uint32_t* ctl             = nullptr;
};
thread_local last_split_record g_last_split;
// Deferred join (backend: dedup_defer_join / dedup_join). The generic path's launches on the side stream take ~35 us even when
// they have nothing to do, longer than the split sort of a mini-batch (profiles/r05_grad_timeline_small_batch.txt). A caller
// that goes on to the optimizer step asks for the join to be split in two: a one-wave kernel on its stream that waits ON THE
// DEVICE, and only when the batch overflowed; and the event wait, enqueued after the step (dedup_join) — by then the idle
// launches have long drained under the tile kernel. The event wait still comes before anything else the caller queues, so
// the sort's workspace is not handed back while a side-stream kernel may still look at it.
thread_local bool g_defer_join     = false;
thread_local bool g_join_pending   = false;
struct split_layout {
  void* split_ws;        // split::plan offsets apply; its first two arrays double as the generic sort's second (key, position) pair
  uint32_t* sorted;      // generic path: sorted keys
  int32_t* tile_counts;  // generic path: run detection
  uint32_t* osw_ctrl;    // generic path: control words, zeroed by split_hist_kernel
  size_t osw_ctrl_words;
  size_t total;
};
inline split_layout split_carve(void* ws, int64_t n)
{
  auto align = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  split_layout l;
  char* p  = static_cast<char*>(ws);
  size_t o = 0;
  l.split_ws       = p + o, o += align(split::workspace_bound(n));
  l.sorted         = reinterpret_cast<uint32_t*>(p + o), o += align(4 * static_cast<size_t>(n));
  l.tile_counts    = reinterpret_cast<int32_t*>(p + o), o += align(4 * static_cast<size_t>((n + kBlock * 8 - 1) / (kBlock * 8) + 1));
  l.osw_ctrl_words = osw::ctrl_words_bound<kOswBlock, kOswIpt>(n);
  l.osw_ctrl        = reinterpret_cast<uint32_t*>(p + o), o += align(4 * l.osw_ctrl_words);
  l.total           = o + 256;
  return l;
}

inline int run_tiles(int64_t n) { return static_cast<int>((n + kRunTile - 1) / kRunTile); }

template <typename SortKeyT>
dedup_layout<SortKeyT> layout(void* ws, int64_t n)
{
  auto align = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  size_t sort_bytes = 0;
  if constexpr (sizeof(SortKeyT) == 4)
    (void)sort_pairs32(nullptr, sort_bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                       rocprim::counting_iterator<int32_t>(0), static_cast<int32_t*>(nullptr), static_cast<size_t>(n), 0, 32, nullptr);
  else
    (void)rocprim::radix_sort_pairs<typename sort_config<SortKeyT>::type>(
      nullptr, sort_bytes, static_cast<const SortKeyT*>(nullptr), static_cast<SortKeyT*>(nullptr),
      rocprim::counting_iterator<int32_t>(0), static_cast<int32_t*>(nullptr), static_cast<size_t>(n), 0, 8 * sizeof(SortKeyT),
      nullptr);
  dedup_layout<SortKeyT> l;
  char* p       = static_cast<char*>(ws);
  size_t o      = 0;
  l.sorted      = reinterpret_cast<SortKeyT*>(p + o), o += align(sizeof(SortKeyT) * n);
  l.tile_counts = reinterpret_cast<int32_t*>(p + o), o += align(4 * static_cast<size_t>(run_tiles(n) + 1));
  l.temp        = p + o;
  l.temp_bytes  = sort_bytes;
  l.total       = o + align(l.temp_bytes) + 256;
  return l;
}

// closing kernel of the generic path behind a split sort: "done" for split_join_kernel — after the onesweep passes' error word
// (a look-back that gave up) has been folded into the split sort's, which is the one the join kernel reports
__global__ void set_word_kernel(uint32_t* word, uint32_t value, const uint32_t* osw_error, uint32_t* ctl_error)
{
  if (osw_error != nullptr && *osw_error != 0u) atomicOr(ctl_error, static_cast<uint32_t>(split::kErrOnesweep));
  __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename SortKeyT, typename OutT>
int detect_runs(const SortKeyT* sorted, int32_t* tile_counts, int64_t n, OutT* unique_ids, int32_t* run_starts,
                int64_t* n_unique_out, hipStream_t stream, OutT key_base = 0, bool drop_last = false, SortKeyT drop_key = 0,
                const uint32_t* gate = nullptr, uint32_t* done_word = nullptr, const uint32_t* osw_error = nullptr,
                uint32_t* ctl_error = nullptr)
{
  const int tiles = run_tiles(n);
  const uint32_t* last_key = nullptr;
  if constexpr (sizeof(SortKeyT) == 4) {
    if (drop_last) last_key = reinterpret_cast<const uint32_t*>(sorted + (n - 1));
  }
  // (one block per tile: looping 1024 blocks over the tiles made an ACTIVE run_compact_kernel 77 us instead of 18)
  const int run_grid = tiles;
  hipLaunchKernelGGL((run_count_kernel<SortKeyT>), dim3(run_grid), dim3(kBlock), 0, stream, sorted, n, tile_counts, gate);
  hipLaunchKernelGGL(run_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_counts, tiles, n_unique_out, last_key,
                     static_cast<uint32_t>(drop_key), gate);
  hipLaunchKernelGGL((run_compact_kernel<SortKeyT, OutT>), dim3(run_grid), dim3(kBlock), 0, stream, sorted, n, tile_counts,
                     n_unique_out, unique_ids, run_starts, key_base, last_key != nullptr, drop_key, gate);
  // the generic path behind a split sort, joined on the device: one more (tiny) kernel says so when everything above has
  // finished — the end of a kernel makes its writes visible; a fence + counter per block of the kernel above made that kernel
  // 302 us instead of 18
  if (done_word != nullptr)
    hipLaunchKernelGGL(set_word_kernel, dim3(1), dim3(1), 0, stream, done_word, 1u, osw_error, ctl_error);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename KeyT>
int run_dedup(const void* ids, int64_t n, int64_t key_upper_bound, int64_t key_lower_bound, void* unique_ids,
              int32_t* run_starts, int32_t* order, int64_t* n_unique_out, void* workspace, hipStream_t stream)
{
  using UKey = typename std::make_unsigned<KeyT>::type;
  if (key_upper_bound <= 0 || key_lower_bound < 0 || key_lower_bound >= key_upper_bound) key_lower_bound = 0;
  // the payload 0, 1, 2 ... is generated by the sort's first pass (counting iterator): no iota array
  rocprim::counting_iterator<int32_t> positions(0);
  const int64_t span = key_upper_bound > 0 ? key_upper_bound - key_lower_bound : 0;
  // Adaptive route. A batch that overflows a bucket of the split sort (hot ids of a skewed batch) is sorted by the gated generic
  // path instead — correct, but 0.11-0.13 ms slower per 10 M ids than rocPRIM's sort on the caller's stream would have been
  // (its passes take 61-69 us on such ids, the hand-written ones 98-121: profiles/r05_grad_timeline_zipf_*.txt), and skewed
  // batches come in series (the same power-law rows every step). So while the last split sort of this row range overflowed, the
  // batch goes straight to rocPRIM (below), and every kProbeEvery-th such call runs the split sort's first two kernels as a
  // probe in front (30 us / 4); the first batch that would not overflow switches back. A wrong guess costs time, once.
  // WM_DEDUP_ADAPT=0: always the split sort. Not while a stream is captured (a graph replays ONE route).
  bool expect_overflow = false;
  int adapt_slot       = -1;
  if (span > 0 && span < INT64_C(0xFFFFFFFF) && n >= split_min() && WM_KNOB("WM_DEDUP_SERIAL") == nullptr &&
      !(WM_KNOB("WM_DEDUP_ADAPT") != nullptr && WM_KNOB("WM_DEDUP_ADAPT")[0] == '0')) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone && sort_lane::get().ok) {
      sort_lane& lane = sort_lane::get();
      std::lock_guard<std::mutex> lk(lane.mu);
      adapt_slot = lane.adapt_slot(key_lower_bound, key_upper_bound);
      if (adapt_slot >= 0) {
        auto& e                   = lane.adapt[adapt_slot];
        volatile int32_t* verdict = lane.adapt_flags + adapt_slot;
        if (!e.generic && *verdict != 0) e.generic = true, e.calls = 0;
        if (e.generic) {
          const split::plan sp = split::make_plan(n, span);
          if (!sp.ok) {
            e.generic = false, *verdict = 0;   // (a batch the split sort would not take anyway)
          } else if (*verdict == 0) {
            e.generic = false;   // the last probe found room: back to the split sort
          } else if (++e.calls % sort_lane::kProbeEvery == 0) {
            if (lane.probe_ws == nullptr && hipMalloc(&lane.probe_ws, split::probe_workspace_bytes()) != hipSuccess) lane.probe_ws = nullptr;
            if (lane.probe_ws != nullptr) {
              if (split::launch_probe<UKey>(sp, static_cast<const UKey*>(ids), n, static_cast<UKey>(key_lower_bound),
                                            static_cast<uint32_t>(span), lane.probe_ws, stream) != 0)
                return -2;
              (void)hipMemcpyAsync(const_cast<int32_t*>(verdict), split::probe_overflow_word(sp, lane.probe_ws), sizeof(int32_t),
                                   hipMemcpyDeviceToHost, stream);
            }
          }
        }
        expect_overflow = e.generic;
      }
    }
  }
  if (!expect_overflow && span > 0 && span < INT64_C(0xFFFFFFFF) && n >= split_min()) {
    const split::plan sp = split::make_plan(n, span);
    if (sp.ok) {
      const split_layout sl = split_carve(workspace, n);
      const unsigned bits   = significant_bits(span + 1, 32);
      const size_t ctrl     = osw::ctrl_words<kOswBlock, kOswIpt>(n, bits);
      const int64_t zero_n  = static_cast<int64_t>(ctrl);
      // the generic path, gated on the overflow word, between the split sort's second and third kernel — on the side stream
      // (WM_DEDUP_SERIAL=1: on the caller's stream, for measurements)
      const uint32_t* gate = split::overflow_word(sp, sl.split_ws);
      char* sw             = static_cast<char*>(sl.split_ws);
      uint32_t* ctl        = reinterpret_cast<uint32_t*>(sw + sp.off_ctl);
      const split::wait_cfg wc = wait_limits(&sp);
      narrow_key_iterator<UKey> keys{static_cast<const UKey*>(ids), static_cast<UKey>(key_lower_bound), static_cast<uint32_t>(span)};
      const bool serial = WM_KNOB("WM_DEDUP_SERIAL") != nullptr;
      std::unique_lock<std::mutex> lane_lock;
      if (!serial) lane_lock = std::unique_lock<std::mutex>(sort_lane::get().mu);
      int generic_rc = 0;
      auto generic = [&](hipStream_t gs) {
        generic_rc = osw::sort_pairs<kOswBlock, kOswIpt>(keys, sl.sorted, reinterpret_cast<uint32_t*>(order), n, bits,
                                                         reinterpret_cast<uint32_t*>(sw + sp.off_keys),
                                                         reinterpret_cast<uint32_t*>(sw + sp.off_pos), sl.osw_ctrl, gate, gs,
                                                         WM_KNOB("WM_DEBUG_SPIN_LIMIT") != nullptr ? wc.look_back_polls : 1u << 26);
        if (generic_rc == 0)
          generic_rc = detect_runs<uint32_t, UKey>(sl.sorted, sl.tile_counts, n, static_cast<UKey*>(unique_ids), run_starts,
                                                   n_unique_out, gs, static_cast<UKey>(key_lower_bound), true,
                                                   static_cast<uint32_t>(span), gate,
                                                   stall_join() ? nullptr : ctl + split::kCtlGenericDone,
                                                   osw::error_word<kOswBlock, kOswIpt>(sl.osw_ctrl, n, bits), ctl + split::kCtlError);
      };
      bool forked = false;
      uint32_t* verdict_word = nullptr;
      uint32_t verdict_value = 0;
      // (a stream that is being captured gets events only: a wave that waits for a word needs the other side to be RUNNING,
      // and the branches of a graph may be replayed one after the other)
      hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
      const bool capturing = hipStreamIsCapturing(stream, &capture) != hipSuccess || capture != hipStreamCaptureStatusNone;
      const bool by_event = WM_KNOB("WM_DEDUP_FORK_EVENT") != nullptr && WM_KNOB("WM_DEDUP_FORK_EVENT")[0] == '1';   // (A/B switch)
      const bool waits_ok = !capturing && device_waits_allowed();
      if (!serial && waits_ok && !by_event && sort_lane::get().ok && sort_lane::get().ring != nullptr) {
        sort_lane& lane = sort_lane::get();
        verdict_value   = ++lane.seq;
        verdict_word    = lane.ring + (verdict_value % sort_lane::kRing);
      }
      auto between = [&]() {
        sort_lane& lane = sort_lane::get();
        if (verdict_word != nullptr) {
          hipLaunchKernelGGL(split::split_wait_kernel, dim3(1), dim3(64), 0, lane.side(), verdict_word, verdict_value,
                             ctl + split::kCtlError, wc.wait_polls, lane.host_err_dev);
          forked = hipGetLastError() == hipSuccess;
          if (!forked) {   // (the caller's kernels and the join kernel are queued already: nothing of the generic path behind them)
            generic_rc = -2;
            return;
          }
        } else {
          forked = !serial && lane.ok && hipEventRecord(lane.forked, stream) == hipSuccess &&
                   hipStreamWaitEvent(lane.side(), lane.forked, 0) == hipSuccess;
        }
        generic(forked ? lane.side() : stream);
        if (forked && adapt_slot >= 0)   // (what this batch did decides the route of the next: see "adaptive route")
          (void)hipMemcpyAsync(const_cast<int32_t*>(lane.adapt_flags) + adapt_slot, gate, sizeof(int32_t), hipMemcpyDeviceToHost,
                               lane.side());
        if (forked) forked = hipEventRecord(lane.joined, lane.side()) == hipSuccess;
      };
      // With the fork by a word nothing ties the side stream's launches to a place in the caller's queue: the caller's kernels
      // — the split sort's four — are enqueued FIRST (a mini-batch is bound by the host's launch rate — the nine side launches in the middle delayed the
      // scatter kernel by as many launch times), then the side stream, then the join kernel.
      // (forked by an event, the side stream is enqueued between the scan and the scatter kernel: the event has to follow the scan)
      const bool side_last = verdict_word != nullptr;
      auto nothing         = []() {};
      const int launched =
        side_last ? split::launch<UKey>(sp, static_cast<const UKey*>(ids), n, static_cast<UKey>(key_lower_bound),
                                        static_cast<uint32_t>(span), unique_ids, run_starts, order, n_unique_out, sl.split_ws,
                                        sl.osw_ctrl, zero_n, stream, nothing, verdict_word, verdict_value, wc)
                  : split::launch<UKey>(sp, static_cast<const UKey*>(ids), n, static_cast<UKey>(key_lower_bound),
                                        static_cast<uint32_t>(span), unique_ids, run_starts, order, n_unique_out, sl.split_ws,
                                        sl.osw_ctrl, zero_n, stream, between, verdict_word, verdict_value, wc);
      if (launched != 0) return -2;
      // (every wave that waits is enqueued BEHIND the kernel it waits for — the side stream's behind the split sort's kernels,
      // the join kernel behind the side stream's last — so that even one in-order hardware queue makes progress)
      if (side_last) between();
      const bool defer = g_defer_join && waits_ok && forked;
      if (!defer && forked && hipStreamWaitEvent(stream, sort_lane::get().joined, 0) != hipSuccess) return -2;
      // the sort's LAST kernel on the caller's stream, whichever way the side stream is joined: waits for the generic path when
      // the join is deferred and the batch overflowed (1 = what detect_runs' closing kernel sets), and turns any wait of this
      // sort that gave up into "no runs" + an error word the host will see (split_sort.cuh: split_join_kernel)
      hipLaunchKernelGGL(split::split_join_kernel, dim3(1), dim3(64), 0, stream, ctl, 1u, wc.join_polls, n_unique_out,
                         sort_lane::get().host_err_dev);
      if (defer) g_join_pending = true;
      g_split_sorts.fetch_add(1, std::memory_order_relaxed);
      g_last_split.run_starts = run_starts;
      g_last_split.unique_ids = unique_ids;
      g_last_split.n_unique   = n_unique_out;
      g_last_split.ctl        = ctl;
      return generic_rc;
    }
  }
  if (span > 0 && span < INT64_C(0xFFFFFFFF)) {
    // a bounded range of fewer than 2^32 - 1 rows: 32-bit keys relative to its start, the value `span` marks ids outside it
    const unsigned bits = significant_bits(span + 1, 32);
    auto l    = layout<uint32_t>(workspace, n);
    size_t tb = l.temp_bytes;
    narrow_key_iterator<UKey> keys{static_cast<const UKey*>(ids), static_cast<UKey>(key_lower_bound), static_cast<uint32_t>(span)};
    if (sort_pairs32(l.temp, tb, keys, l.sorted, positions, order, static_cast<size_t>(n), 0, bits, stream) != hipSuccess) return -2;
    return detect_runs<uint32_t, UKey>(l.sorted, l.tile_counts, n, static_cast<UKey*>(unique_ids), run_starts, n_unique_out,
                                       stream, static_cast<UKey>(key_lower_bound), true, static_cast<uint32_t>(span));
  }
  const unsigned bits = significant_bits(key_upper_bound > 0 ? key_upper_bound : 0, 8 * sizeof(KeyT));
  auto l    = layout<UKey>(workspace, n);
  size_t tb = l.temp_bytes;
  if (rocprim::radix_sort_pairs<typename sort_config<UKey>::type>(l.temp, tb, static_cast<const UKey*>(ids), l.sorted, positions,
                                                                  order, static_cast<size_t>(n), 0, bits, stream) != hipSuccess)
    return -2;
  return detect_runs<UKey, UKey>(l.sorted, l.tile_counts, n, static_cast<UKey*>(unique_ids), run_starts, n_unique_out, stream);
}

}  // namespace
}  // namespace wm
extern "C" int64_t wholememory_ext_split_sorts(void) { return wm::g_split_sorts.load(std::memory_order_relaxed); }
namespace wm {

void hip_dedup_defer_join(int on)
{
  const char* e = WM_KNOB("WM_DEDUP_DEFER_JOIN");   // =0: the side stream is joined in front of the step again (A/B switch)
  g_defer_join  = on != 0 && !(e != nullptr && e[0] == '0');
}
// A device-side wait of an earlier sort gave up (sort_lane::host_err): say so ONCE, as an error. Non-blocking — what it sees is
// what has finished; callers that synchronise (the multi-rank gradient apply, WM_DEBUG_SYNC=1) ask again afterwards.
int hip_device_error()
{
  const uint32_t e = sort_lane::get().take_error();
  if (e == 0) return 0;
  if (e & split::kErrTreeBounds)
    WM_ERROR("the tree fold of duplicate gradient rows listed more long runs or segments than its workspace was carved for (code "
             "0x%x): the long runs of that optimizer step were NOT applied. The step's count must be the batch's number of "
             "gradient rows.", e);
  if ((e & ~split::kErrTreeBounds) == 0) return static_cast<int>(e);
  WM_ERROR("a device-side wait of the gradient path's id sort timed out (code 0x%x:%s%s%s%s): the optimizer step of that call was "
           "NOT applied (its run count was zeroed on the device). A tool that runs one kernel at a time (counter collection, some "
           "debuggers) stalls these waits: set WM_DEVICE_WAITS=0 for event-only synchronisation.",
           e, (e & split::kErrLookBack) ? " bucket look-back" : "", (e & split::kErrJoin) ? " join of the generic sort" : "",
           (e & split::kErrWait) ? " side-stream wait" : "", (e & split::kErrOnesweep) ? " radix-pass look-back" : "");
  return static_cast<int>(e);
}
int hip_dedup_join(void* stream_v)
{
  if (!g_join_pending) return hip_device_error() != 0 ? -2 : 0;
  g_join_pending = false;
  if (hipStreamWaitEvent(static_cast<hipStream_t>(stream_v), sort_lane::get().joined, 0) != hipSuccess) return -2;
  return hip_device_error() != 0 ? -2 : 0;
}

size_t hip_dedup_workspace_bytes(int64_t n, wholememory_dtype_t index_dtype)
{
  if (n <= 0) return 256;
  // the bounded-key path carves the 32-bit layout whatever the index type, and the split sort its own (advisor, round 4:
  // the 64-bit layout alone can be the smaller one)
  size_t most = layout<uint32_t>(nullptr, n).total;
  if (index_dtype != WHOLEMEMORY_DT_INT) most = std::max(most, layout<uint64_t>(nullptr, n).total);
  // (only batches that can take the split sort: its layout has a fixed ~17 MB term — kMaxTiles x kMaxPitch counters — that a
  // mini-batch of a few hundred ids would otherwise ask the caller's allocator for on every call; run_dedup tests the same
  // two conditions before it carves that layout: advisor, round 5)
  if (n < (INT64_C(1) << 30) && n >= split_min()) most = std::max(most, split_carve(nullptr, n).total);
  return most;
}

int hip_dedup_ids(const void* ids, wholememory_dtype_t index_dtype, int64_t n, int64_t key_upper_bound, int64_t key_lower_bound,
                  void* unique_ids, int32_t* run_starts, int32_t* order, int64_t* n_unique_out, void* workspace,
                  void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  g_last_split = last_split_record{};   // (set again below when this sort is a split sort)
  if (hip_dedup_join(stream_v) != 0) return -2;   // (a deferred join nobody collected: before this sort touches anything)
  if (n >= (1ll << 31)) return -1;  // reference casts the receive count to int (exchange_embeddings_nccl_func.cu:118)
  if (n == 0) return hipMemsetAsync(n_unique_out, 0, sizeof(int64_t), stream) == hipSuccess ? 0 : -2;
  if (index_dtype == WHOLEMEMORY_DT_INT)
    return run_dedup<int32_t>(ids, n, key_upper_bound, key_lower_bound, unique_ids, run_starts, order, n_unique_out, workspace, stream);
  if (index_dtype == WHOLEMEMORY_DT_INT64)
    return run_dedup<int64_t>(ids, n, key_upper_bound, key_lower_bound, unique_ids, run_starts, order, n_unique_out, workspace, stream);
  return -1;
}

// ---- ids in ascending row order for locality (HOST-table gather, backend.hpp: sort_ids) ----
namespace {
template <typename KeyT>
__global__ void expand_sorted_ids_kernel(const KeyT* ids, const int32_t* order, int64_t n, KeyT* sorted_ids, int64_t* raw)
{
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t o = order[i];
  sorted_ids[i]   = ids[o];   // the id as the caller wrote it (a negative one stays negative: the gather skips it)
  raw[i]          = o;
}

struct sort_ids_layout {
  uint32_t* keys;
  int32_t* order;
  void* temp;
  size_t temp_bytes, total;
};
sort_ids_layout sort_ids_carve(void* ws, int64_t n)
{
  auto align = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  size_t sort_bytes = 0;
  (void)sort_pairs32(nullptr, sort_bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                     rocprim::counting_iterator<int32_t>(0), static_cast<int32_t*>(nullptr), static_cast<size_t>(n), 0, 32, nullptr);
  sort_ids_layout l;
  char* p  = static_cast<char*>(ws);
  size_t o = 0;
  l.keys   = reinterpret_cast<uint32_t*>(p + o), o += align(4 * static_cast<size_t>(n));
  l.order  = reinterpret_cast<int32_t*>(p + o), o += align(4 * static_cast<size_t>(n));
  l.temp   = p + o;
  l.temp_bytes = sort_bytes;
  l.total  = o + align(sort_bytes) + 256;
  return l;
}

template <typename KeyT>
int run_sort_ids(const void* ids, int64_t n, int64_t key_upper_bound, int low_bit, void* sorted_ids, int64_t* raw, void* ws,
                 hipStream_t stream)
{
  using UKey = typename std::make_unsigned<KeyT>::type;
  auto l     = sort_ids_carve(ws, n);
  size_t tb  = l.temp_bytes;
  // ids outside [0, key_upper_bound) — negative ones above all — read as the key `key_upper_bound` and land behind every row
  narrow_key_iterator<UKey> keys{static_cast<const UKey*>(ids), static_cast<UKey>(0), static_cast<uint32_t>(key_upper_bound)};
  const unsigned bits = significant_bits(key_upper_bound + 1, 32);
  const unsigned lo   = static_cast<unsigned>(std::max(0, std::min<int>(low_bit, static_cast<int>(bits) - 1)));
  if (sort_pairs32(l.temp, tb, keys, l.keys, rocprim::counting_iterator<int32_t>(0), l.order, static_cast<size_t>(n), lo, bits, stream) != hipSuccess)
    return -2;
  hipLaunchKernelGGL((expand_sorted_ids_kernel<KeyT>), dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     stream, static_cast<const KeyT*>(ids), l.order, n, static_cast<KeyT*>(sorted_ids), raw);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // namespace

size_t hip_sort_ids_workspace_bytes(int64_t n) { return n <= 0 ? 256 : sort_ids_carve(nullptr, n).total; }

int hip_sort_ids(const void* ids, wholememory_dtype_t index_dtype, int64_t n, int64_t key_upper_bound, int low_bit,
                 void* sorted_ids, int64_t* raw, void* workspace, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (n <= 0) return 0;
  if (key_upper_bound <= 0 || key_upper_bound >= INT64_C(0xFFFFFFFF) || n >= (INT64_C(1) << 31)) return -3;
  if (index_dtype == WHOLEMEMORY_DT_INT) return run_sort_ids<int32_t>(ids, n, key_upper_bound, low_bit, sorted_ids, raw, workspace, stream);
  if (index_dtype == WHOLEMEMORY_DT_INT64) return run_sort_ids<int64_t>(ids, n, key_upper_bound, low_bit, sorted_ids, raw, workspace, stream);
  return -1;
}

// ---- what the optimizer step asks of the sort (sort_handoff.cuh) ----
uint32_t* take_split_ctl(const int32_t* run_starts, const void* unique_ids, const int64_t* n_unique)
{
  const last_split_record r = g_last_split;
  g_last_split              = last_split_record{};
  return r.run_starts == run_starts && r.unique_ids == unique_ids && r.n_unique == n_unique ? r.ctl : nullptr;
}
std::unique_lock<std::mutex> lock_pending_join_side(hipStream_t* side)
{
  if (!g_join_pending || !sort_lane::get().ok) return {};
  std::unique_lock<std::mutex> lk(sort_lane::get().mu);
  *side = sort_lane::get().side();
  return lk;
}
hipError_t record_sort_joined(hipStream_t stream) { return hipEventRecord(sort_lane::get().joined, stream); }
uint32_t* device_error_word() { return sort_lane::get().host_err_dev; }
void enqueue_final_runs_wait(const uint32_t* ctl, hipStream_t stream)
{
  hipLaunchKernelGGL(split::split_wait_kernel, dim3(1), dim3(64), 0, stream, ctl + split::kCtlSortDone, 1u,
                     const_cast<uint32_t*>(ctl) + split::kCtlError, wait_limits().wait_polls, sort_lane::get().host_err_dev);
}

template <typename IdxT>
__global__ void run_inverse_kernel(const int32_t* run_starts, const int32_t* order, const IdxT* unique_ids,
                                   const int64_t* n_unique, int64_t n, int64_t id_limit, int64_t* inverse)
{
  // the run of sorted position j: last u with run_starts[u] <= j. The 256 positions of a workgroup are consecutive, so
  // their runs lie between the run of the first and the run of the last one: two full-range searches per workgroup, then
  // every thread searches a window of at most 256 runs (8 steps instead of 23 on 5 M runs: 369 -> ~120 us per 10 M ids)
  __shared__ int64_t s_lo, s_hi;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * blockDim.x;
  const int64_t j  = j0 + threadIdx.x;
  auto search      = [&](int64_t pos, int64_t lo, int64_t hi) {
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (run_starts[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
  };
  if (threadIdx.x == 0) s_lo = search(j0, 0, *n_unique - 1);
  if (threadIdx.x == 64) s_hi = search(min(j0 + static_cast<int64_t>(blockDim.x) - 1, n - 1), 0, *n_unique - 1);
  __syncthreads();
  if (j >= n) return;
  const int64_t u   = search(j, s_lo, s_hi);
  const int64_t id  = static_cast<int64_t>(unique_ids[u]);
  inverse[order[j]] = (id < 0 || (id_limit > 0 && id >= id_limit)) ? -1 : u;
}

int hip_run_inverse(const int32_t* run_starts, const int32_t* order, const void* unique_ids, wholememory_dtype_t index_dtype,
                    const int64_t* n_unique_dev, int64_t n, int64_t id_limit, int64_t* inverse, void* stream)
{
  if (n == 0) return 0;
  const int blocks = static_cast<int>((n + kBlock - 1) / kBlock);
  if (index_dtype == WHOLEMEMORY_DT_INT)
    hipLaunchKernelGGL((run_inverse_kernel<int32_t>), dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       run_starts, order, static_cast<const int32_t*>(unique_ids), n_unique_dev, n, id_limit, inverse);
  else if (index_dtype == WHOLEMEMORY_DT_INT64)
    hipLaunchKernelGGL((run_inverse_kernel<int64_t>), dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       run_starts, order, static_cast<const int64_t*>(unique_ids), n_unique_dev, n, id_limit, inverse);
  else
    return -1;
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

__global__ void remap_self_order_kernel(int32_t* order, int64_t n, int64_t self_begin, int64_t self_count,
                                        const int64_t* self_rows)
{
  int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t pos = order[i] - self_begin;
  if (pos >= 0 && pos < self_count) order[i] = static_cast<int32_t>(-(self_rows[pos] + 1));
}

int hip_remap_self_order(int32_t* order, int64_t n, int64_t self_begin, int64_t self_count, const int64_t* self_rows,
                         void* stream)
{
  if (n == 0 || self_count == 0) return 0;
  const int blocks = static_cast<int>((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(remap_self_order_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), order, n,
                     self_begin, self_count, self_rows);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // namespace wm
