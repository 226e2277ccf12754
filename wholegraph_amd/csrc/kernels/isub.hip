// wholegraph_amd — the node-induced subgraph of a CSR graph held in WholeMemory (gfx950 HIP; wholegraph_amd_ext.h section 2q):
// row i of the result holds, in the graph's order, the entries of row nodes[i] whose node occurs in `nodes`, as the lowest
// position it occurs at, with the entry's position in col_ind beside it. Count, scan, one host round trip, fill: the shape of
// the sampler (graph.hip), with a membership table in front.
//   - The table: open addressing with linear probing in the workspace, 2n slots rounded up to a power of two, a 64-bit key per
//     slot (all-ones = empty: only ids in [0, n_nodes) are inserted, so no key looks like it) and, in a second array, the lowest
//     position the key occurs at. One compare-and-swap and one atomic min per node, append_unique's scheme with its hash
//     (id_hash.cuh). Min does not depend on the order of the inserts, so neither does anything downstream.
//   - Count and fill walk the rows alike: a GROUP of kIsubGroup lanes per row, each trip a lane loads one of the next
//     kIsubGroup entries (the loads of a trip go out together) and probes the table for it. A vote tells the group how many of
//     the trip's entries survive and, in the fill, where: a survivor's place is the running base plus the survivors in the
//     lower lanes of its group's slice of the mask, which keeps the row's order. The count leaves the row's number and, per
//     wave, a 64-bit sum; one wave adds those up (the int32 scan of the row numbers cannot see a total of 2^31 or more).
// A col_ind value is range-checked and compared, never used as an index. Groups past the end sit out (an empty row) but take
// part in the votes; the trips of a row are the same for all lanes of its group. No atomics outside the insert, no LDS, no
// scratch; every probe loop is bounded by the table's capacity and every row loop by the row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../backend.hpp"
#include "../neg_sample.hpp"
#include "csr_view.cuh"
#include "id_hash.cuh"

namespace wm {
namespace {

constexpr int kIsubBlock = 256;  // lanes per block
// lanes per row. Measured on the papers100M-shaped bench graph (degrees uniform in [0, 58]) with the node sets of 3 000 x 2,
// 20 000 x 4 and 100 000 x 4 walks (8 459, 85 864 and 402 066 nodes; scripts/bench_induced_subgraph.py), the
// whole call: 8 lanes 0.082 / 0.165 / 0.574 ms, 16 lanes 0.075 / 0.164 / 0.613 ms, 32 lanes 0.073 / 0.202 / 0.742 ms, 64 lanes
// 0.075 / 0.241 / 1.004 ms. 16 is within 3 % of the best on the two smaller sets and 7 % behind 8 on the largest, where 8 is
// 9 % behind on the smallest. The result does not depend on it. Overridable for that sweep alone: a build with
// -DWM_ISUB_GROUP=8|16|32|64 is a variant, not the product.
#ifndef WM_ISUB_GROUP
#define WM_ISUB_GROUP 16
#endif
constexpr int kIsubGroup = WM_ISUB_GROUP;
static_assert(kIsubGroup >= 2 && kIsubGroup <= 64 && (kIsubGroup & (kIsubGroup - 1)) == 0, "a power of two within a wave");

constexpr int64_t kIsubEmpty = -1;   // what the 0xFF fill leaves in a key slot

struct isub_table {
  int64_t* keys;     // cap
  uint32_t* first;   // cap: the lowest position of the slot's key in `nodes` (0xFFFFFFFF = none yet)
  uint64_t mask;     // cap - 1
};

constexpr size_t isub_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

uint64_t isub_capacity(int64_t n)
{
  uint64_t cap = 64;
  while (cap < 2 * static_cast<uint64_t>(n)) cap <<= 1;   // n < 2^31: at most 2^32 slots, which the 32-bit hash still spreads over
  return cap;
}

int64_t isub_blocks(int64_t n) { return (n + kIsubBlock / kIsubGroup - 1) / (kIsubBlock / kIsubGroup); }

// [keys | first] is the table (one 0xFF fill empties it), the per-wave sums of the count come behind it
struct isub_layout {
  isub_table t;
  int64_t* wave_sums;
  int64_t n_waves;
  size_t table_bytes, total;
};

isub_layout isub_plan(void* ws, int64_t n)
{
  isub_layout l;
  const uint64_t cap = isub_capacity(n);
  char* p            = static_cast<char*>(ws);
  size_t o           = 0;
  l.t.keys = reinterpret_cast<int64_t*>(p + o), o += isub_align(sizeof(int64_t) * cap);
  l.t.first = reinterpret_cast<uint32_t*>(p + o), o += isub_align(sizeof(uint32_t) * cap);
  l.t.mask      = cap - 1;
  l.table_bytes = o;
  l.n_waves     = isub_blocks(n) * (kIsubBlock / 64);
  l.wave_sums = reinterpret_cast<int64_t*>(p + o), o += isub_align(sizeof(int64_t) * static_cast<size_t>(l.n_waves > 0 ? l.n_waves : 1));
  l.total = o;
  return l;
}

struct isub_params {
  csr_view g;
  const void* nodes;
  int64_t n;
  isub_table t;
  int* counts;
  int64_t* wave_sums;
  const int* offsets;
  int* out_col;
  int64_t* out_egid;
};

template <typename IdT>
__global__ __launch_bounds__(kIsubBlock) void isub_insert_kernel(const IdT* nodes, int64_t n, int64_t n_nodes, isub_table t)
{
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kIsubBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t v = static_cast<int64_t>(nodes[i]);
  if (v < 0 || v >= n_nodes) return;   // not a member: never matched, whatever col_ind holds
  uint64_t s = au_hash(static_cast<uint64_t>(v)) & t.mask;
  for (uint64_t trip = 0; trip <= t.mask; trip++) {
    int64_t cur = t.keys[s];   // (a plain look first: most positions of a repeated node find its key there)
    if (cur == kIsubEmpty)
      cur = static_cast<int64_t>(atomicCAS(reinterpret_cast<unsigned long long*>(&t.keys[s]), ~0ull, static_cast<unsigned long long>(v)));
    if (cur == kIsubEmpty || cur == v) {   // the slot is v's, now or already
      if (t.first[s] > static_cast<uint32_t>(i)) atomicMin(&t.first[s], static_cast<uint32_t>(i));
      return;
    }
    s = (s + 1) & t.mask;
  }
}

// the slot of c, or false when c is not a member
__device__ __forceinline__ bool isub_find(const isub_table& t, int64_t c, int64_t n_nodes, uint64_t* slot)
{
  if (c < 0 || c >= n_nodes) return false;
  uint64_t s = au_hash(static_cast<uint64_t>(c)) & t.mask;
  for (uint64_t trip = 0; trip <= t.mask; trip++) {
    const int64_t k = t.keys[s];
    if (k == c) {
      *slot = s;
      return true;
    }
    if (k == kIsubEmpty) return false;
    s = (s + 1) & t.mask;
  }
  return false;
}

// the walk of both passes. found(pos, slot, rank): entry pos of the row survives, `rank` survivors of the row stand before it
template <typename IdT, typename ColT, int G, typename F>
__device__ __forceinline__ int isub_walk_row(const isub_params& p, int64_t i, F found)
{
  const int gl    = static_cast<int>(threadIdx.x) & (G - 1);
  const int first = static_cast<int>(threadIdx.x) & 63 & ~(G - 1);   // the group's first lane in its wave
  constexpr unsigned long long kSlice = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
  int64_t s = 0, e = 0;   // a group past the end, a node that is none and bounds that are no row: an empty row
  if (i < p.n) {
    const int64_t u = static_cast<int64_t>(static_cast<const IdT*>(p.nodes)[i]);
    if (u >= 0 && u < p.g.n_nodes) {
      s = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + u);
      e = gref_load<int64_t>(p.g.row_ptr, p.g.row_off + u + 1);
      if (!neg_row_valid(s, e, p.g.n_edges)) s = e = 0;
    }
  }
  int base = 0;   // survivors of the trips so far: below 2^31, as the row is
  for (int64_t r = s; r < e; r += G) {
    const int64_t pos = r + gl;
    bool keep         = false;
    uint64_t slot     = 0;
    if (pos < e) keep = isub_find(p.t, static_cast<int64_t>(gref_load<ColT>(p.g.col_ptr, p.g.col_off + pos)), p.g.n_nodes, &slot);
    const unsigned long long mine = (__ballot(keep) >> first) & kSlice;
    if (keep) found(pos, slot, base + __popcll(mine & ((1ull << gl) - 1ull)));
    base += __popcll(mine);
  }
  return base;
}

template <typename IdT, typename ColT, int G>
__global__ __launch_bounds__(kIsubBlock) void isub_count_kernel(isub_params p)
{
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kIsubBlock + threadIdx.x;
  const int64_t i   = tid / G;
  const int gl      = static_cast<int>(threadIdx.x) & (G - 1);
  const int cnt     = isub_walk_row<IdT, ColT, G>(p, i, [](int64_t, uint64_t, int) {});
  if (gl == 0 && i < p.n) {
    p.counts[i] = cnt;
    if (i == p.n - 1) p.counts[p.n] = 0;   // the scan runs over n + 1 entries
  }
  long long sum = gl == 0 ? cnt : 0;   // (a group past the end counted 0)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if ((threadIdx.x & 63) == 0) p.wave_sums[tid >> 6] = sum;
}

// one wave adds the per-wave sums up: a fixed order, and a word the host may be reading from pinned memory
__global__ __launch_bounds__(64) void isub_total_kernel(const int64_t* wave_sums, int64_t n_waves, int64_t* total)
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

template <typename IdT, typename ColT, int G>
__global__ __launch_bounds__(kIsubBlock) void isub_fill_kernel(isub_params p)
{
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kIsubBlock + threadIdx.x;
  const int64_t i   = tid / G;
  int64_t begin = 0, end = 0;
  if (i < p.n) begin = p.offsets[i], end = p.offsets[i + 1];
  // (k < end: what the count found is what this pass finds; were the graph written to in between, nothing leaves the row's room)
  (void)isub_walk_row<IdT, ColT, G>(p, i, [&](int64_t pos, uint64_t slot, int rank) {
    const int64_t k = begin + rank;
    if (k < end) {
      p.out_col[k] = static_cast<int>(p.t.first[slot]);
      if (p.out_egid != nullptr) p.out_egid[k] = pos;
    }
  });
}

bool isub_args_ok(const wm_isub_args* a)
{
  return a != nullptr && a->n > 0 && a->n < (INT64_C(1) << 31) - 1 && a->n_nodes >= 0 && a->n_edges >= 0 && a->nodes != nullptr &&
         a->workspace != nullptr;
}

isub_params isub_params_of(const wm_isub_args* a, const isub_layout& l)
{
  isub_params p{};
  p.g     = csr_view_of(*a);
  p.nodes = a->nodes, p.n = a->n;
  p.t = l.t, p.wave_sums = l.wave_sums;
  p.counts = a->counts, p.offsets = a->offsets, p.out_col = a->out_col, p.out_egid = a->out_edge_gid;
  return p;
}

}  // namespace

size_t hip_isub_workspace_bytes(int64_t n, size_t* table_bytes)
{
  const isub_layout l = isub_plan(nullptr, n < 0 ? 0 : n);
  if (table_bytes != nullptr) *table_bytes = l.table_bytes;
  return l.total;
}

// what the launchers refuse (-1, nothing queued): the host side has answered all of it before it gets here
int hip_isub_build(const wm_isub_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!isub_args_ok(a)) return -1;
  const isub_layout l   = isub_plan(a->workspace, a->n);
  const unsigned blocks = static_cast<unsigned>((a->n + kIsubBlock - 1) / kIsubBlock);
  if (a->node_dtype == WHOLEMEMORY_DT_INT)
    hipLaunchKernelGGL((isub_insert_kernel<int32_t>), dim3(blocks), dim3(kIsubBlock), 0, stream,
                       static_cast<const int32_t*>(a->nodes), a->n, a->n_nodes, l.t);
  else if (a->node_dtype == WHOLEMEMORY_DT_INT64)
    hipLaunchKernelGGL((isub_insert_kernel<int64_t>), dim3(blocks), dim3(kIsubBlock), 0, stream,
                       static_cast<const int64_t*>(a->nodes), a->n, a->n_nodes, l.t);
  else
    return -1;
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int hip_isub_count(const wm_isub_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!isub_args_ok(a) || a->counts == nullptr || a->total == nullptr) return -1;
  const isub_layout l   = isub_plan(a->workspace, a->n);
  const isub_params p   = isub_params_of(a, l);
  const unsigned blocks = static_cast<unsigned>(isub_blocks(a->n));   // n < 2^31: below 2^28 blocks
  const int rc = dispatch_id_col(a->node_dtype, a->col_dtype, [&](auto id, auto col) {
    hipLaunchKernelGGL((isub_count_kernel<decltype(id), decltype(col), kIsubGroup>), dim3(blocks), dim3(kIsubBlock), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  });
  if (rc != 0) return rc;
  hipLaunchKernelGGL(isub_total_kernel, dim3(1), dim3(64), 0, stream, l.wave_sums, l.n_waves, a->total);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int hip_isub_fill(const wm_isub_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (!isub_args_ok(a) || a->offsets == nullptr || a->out_col == nullptr) return -1;
  const isub_layout l   = isub_plan(a->workspace, a->n);
  const isub_params p   = isub_params_of(a, l);
  const unsigned blocks = static_cast<unsigned>(isub_blocks(a->n));
  return dispatch_id_col(a->node_dtype, a->col_dtype, [&](auto id, auto col) {
    hipLaunchKernelGGL((isub_fill_kernel<decltype(id), decltype(col), kIsubGroup>), dim3(blocks), dim3(kIsubBlock), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  });
}

}  // namespace wm
