// wholegraph_amd — PinSAGE importance neighbourhoods over a CSR graph held in WholeMemory (gfx950 HIP; wholegraph_amd_ext.h
// section 2s): per seed, R random walks with restart of L steps, every arrival counted, and the T most visited nodes with
// their counts, as ONE launch whose only global stores are the [n, T] answer.
//   - One WAVE per seed, one workgroup per wave, one LANE per walk; R > 64 takes ceil(R / 64) passes over the lanes. A lane
//     keeps its walk's generator, its current node and the seed in registers. A step draws twice (restart, neighbour), issues
//     the two row_ptr reads together (walk_common.cuh: walk_row) and then the dependent col_ind read: 64 chains of dependent
//     reads in flight per wave, as many waves per CU as the table's LDS allows.
//   - Visits are counted in an open-addressing table in LDS that belongs to the wave: keys[] holds node ids in col_ind's
//     width (-1: empty), count[] the visits. The slot is au_hash(id) & (SLOTS - 1), then linear probing; a slot is claimed
//     by compare-and-swap on keys[], the count goes up by an atomic add. Integer sums: the table's content does not depend
//     on the order in which the lanes arrive. SLOTS is a template tier, the power of two >= 2 * R * L (128 .. 4096): never
//     more than half full, so a probe always ends; the loop is bounded by SLOTS all the same. The largest tier with 64-bit
//     keys is 48 KB of static LDS.
//   - Selection stays in the wave: the slots are read 64 at a time, an occupied one becomes rwr_pack(count, id) (../rwr.hpp:
//     more visits first, then the lower id), an empty one 0; top_merge (top_merge.cuh) keeps the 64 largest keys, one per
//     lane in descending order; a batch without an occupied slot is skipped by ballot. Lane k < T unpacks its key and stores
//     nodes[i, k] and counts[i, k].
// The three phases of a seed — clear, count, select — are separated by wave_lds_sync(): the wave is the whole workgroup, so
// a workgroup barrier with its LDS fence orders them. No global atomics, no scratch, no waiting on other waves; every loop is
// bounded by L, the passes or SLOTS. An id read from col_ind is range-checked before it is counted or becomes the current
// node, and a row whose bounds do not lie in [0, n_edges] is not stepped from: a damaged graph costs visits, it does not
// read out of bounds. The grid is n workgroups, no cap and no stride loop: seed i is block i, and its walks are the streams
// i * R + r, whatever the launch looks like.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../backend.hpp"
#include "../pcg.hpp"
#include "../rwr.hpp"
#include "id_hash.cuh"
#include "top_merge.cuh"
#include "walk_common.cuh"

namespace wm {
namespace {

constexpr int kRwrWave = 64;   // lanes per workgroup: one wave, which owns the workgroup's LDS

struct rwr_params {
  csr_view g;
  const void* seeds;
  int64_t n;
  int num_walks, walk_length, num_neighbors;
  uint32_t restart_threshold;   // < 2^32 (restart_prob < 1): compared with a 32-bit draw
  uint64_t seed;
  void* out_nodes;   // ColT [n, T]
  int* out_counts;   // [n, T]
};

// the clear must be in LDS before the first insert, the last insert before the scan: a barrier of the (one-wave) workgroup,
// which waits for the wave's outstanding LDS operations and keeps the compiler from moving LDS accesses across it
__device__ __forceinline__ void wave_lds_sync() { __syncthreads(); }

// the table's key type: an unsigned integer of col_ind's width, all ones (the id -1, never a node) for an empty slot
template <typename ColT>
using rwr_key_t = std::conditional_t<sizeof(ColT) == 4, unsigned int, unsigned long long>;

// one visit of node c. SLOTS >= 2 * (visits of the seed): an empty slot or c's own is met before the probe comes round
template <typename KeyT, int SLOTS>
__device__ __forceinline__ void rwr_count_visit(KeyT* keys, unsigned int* count, int64_t c)
{
  const KeyT key = static_cast<KeyT>(c), empty = ~KeyT(0);
  uint32_t slot  = au_hash(static_cast<uint64_t>(c)) & (SLOTS - 1);
  for (int probe = 0; probe < SLOTS; probe++) {
    KeyT seen = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
    if (seen == empty) seen = atomicCAS(&keys[slot], empty, key);   // (another lane may have claimed it in between)
    if (seen == empty || seen == key) {
      atomicAdd(&count[slot], 1u);
      return;
    }
    slot = (slot + 1) & (SLOTS - 1);
  }
}

template <typename IdT, typename ColT, int SLOTS>
__global__ __launch_bounds__(kRwrWave) void rwr_top_kernel(rwr_params p)
{
  using KeyT = rwr_key_t<ColT>;
  __shared__ KeyT keys[SLOTS];
  __shared__ unsigned int count[SLOTS];
  const int64_t i = blockIdx.x;   // the grid is exactly n workgroups
  const int lane  = threadIdx.x;
  const int R = p.num_walks, L = p.walk_length, T = p.num_neighbors;
  int64_t s = static_cast<int64_t>(static_cast<const IdT*>(p.seeds)[i]);
  if (s < 0 || s >= p.g.n_nodes) s = -1;   // the same in every lane: the branches on it below are taken by the whole wave
  uint64_t top = 0;                        // lane k: the k-th largest key so far; 0: none
  if (s >= 0) {
    for (int j = lane; j < SLOTS; j += kRwrWave) keys[j] = ~KeyT(0), count[j] = 0;
    wave_lds_sync();
    for (int r = lane; r < R; r += kRwrWave) {   // pass by pass: lane's walk r of seed i
      pcg32 rng = walk_stream(p.seed, static_cast<uint64_t>(i) * static_cast<uint64_t>(R) + static_cast<uint64_t>(r), 0);
      int64_t v = s;
      for (int t = 0; t < L; t++) {
        const uint32_t a = rng.next_u32();   // step t takes draws 2t and 2t + 1 whether or not it uses them
        const uint32_t b = rng.next_u32();
        int64_t next = s;   // a restart, a row that cannot be stepped from, a damaged entry: back to the seed, nothing counted
        if (a >= p.restart_threshold) {
          int64_t lo;
          int deg;
          if (walk_row(p.g, v, &lo, &deg)) {
            const int64_t pos = lo + walk_uniform_pick(b, static_cast<uint32_t>(deg));
            const int64_t c   = static_cast<int64_t>(gref_load<ColT>(p.g.col_ptr, p.g.col_off + pos));
            if (c >= 0 && c < p.g.n_nodes) {
              next = c;
              if (c != s) rwr_count_visit<KeyT, SLOTS>(keys, count, c);
            }
          }
        }
        v = next;
      }
    }
    wave_lds_sync();
    for (int base = 0; base < SLOTS; base += kRwrWave) {
      const KeyT k   = keys[base + lane];
      const bool occ = k != ~KeyT(0);
      if (__ballot(occ) == 0) continue;
      const uint64_t key = occ ? rwr_pack(count[base + lane], static_cast<uint64_t>(k)) : 0;
      top = top_merge<kRwrWave, uint64_t>(top, key, lane);
    }
  }
  if (lane < T) {
    static_cast<ColT*>(p.out_nodes)[i * T + lane] = top != 0 ? static_cast<ColT>(rwr_key_node(top)) : ColT(-1);
    p.out_counts[i * T + lane]                    = top != 0 ? rwr_key_count(top) : 0;
  }
}

template <typename IdT, typename ColT, int SLOTS>
int launch_tier(const rwr_params& p, hipStream_t stream)
{
  hipLaunchKernelGGL((rwr_top_kernel<IdT, ColT, SLOTS>), dim3(static_cast<unsigned>(p.n)), dim3(kRwrWave), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename IdT, typename ColT>
int launch_rwr(const rwr_params& p, hipStream_t stream)
{
  if (p.n == 0) return 0;
  switch (rwr_table_slots(p.num_walks * p.walk_length)) {
    case 128: return launch_tier<IdT, ColT, 128>(p, stream);
    case 256: return launch_tier<IdT, ColT, 256>(p, stream);
    case 512: return launch_tier<IdT, ColT, 512>(p, stream);
    case 1024: return launch_tier<IdT, ColT, 1024>(p, stream);
    case 2048: return launch_tier<IdT, ColT, 2048>(p, stream);
    case 4096: return launch_tier<IdT, ColT, 4096>(p, stream);
    default: return -1;
  }
}

}  // namespace

int hip_rwr_top(const wm_rwr_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  // what the launcher refuses (-1, nothing queued): the host side has answered all of it before it gets here
  if (a == nullptr || a->n < 0 || a->n_nodes < 0 || a->n_edges < 0 || a->n_nodes > (INT64_C(1) << kRwrNodeBits)) return -1;
  if (!rwr_scalars_ok(a->num_walks, a->walk_length, 0.0, a->num_neighbors) || a->restart_threshold >= (UINT64_C(1) << 32)) return -1;
  if (a->n * a->num_walks >= (INT64_C(1) << 31) || a->n * a->num_neighbors >= (INT64_C(1) << 31)) return -1;
  if (a->n > 0 && (a->seeds == nullptr || a->out_nodes == nullptr || a->out_counts == nullptr)) return -1;
  rwr_params p{};
  p.g     = csr_view_of(*a);
  p.seeds = a->seeds, p.n = a->n;
  p.num_walks = a->num_walks, p.walk_length = a->walk_length, p.num_neighbors = a->num_neighbors;
  p.restart_threshold = static_cast<uint32_t>(a->restart_threshold);
  p.seed = a->random_seed, p.out_nodes = a->out_nodes, p.out_counts = a->out_counts;
  return dispatch_id_col(a->seed_dtype, a->col_dtype,
                         [&](auto id, auto col) { return launch_rwr<decltype(id), decltype(col)>(p, stream); });
}

}  // namespace wm
