// wholegraph_amd — host orchestration helpers shared by the op files (ops.cpp, embedding.cpp, embedding_cache.cpp,
// aggregate.cpp, gat.cpp): scratch from the caller's env functions, the id sort, the id / row exchanges.
#pragma once

#include <atomic>
#include <functional>
#include <vector>

#include <wholememory/wholegraph_amd_ext.h>
#include <wholememory/wholememory_op.h>

#include "backend.hpp"
#include "communicator.hpp"
#include "exchange_plan.hpp"
#include "wm_common.hpp"

namespace wm {

// One scratch allocation obtained through the caller's env functions (reference
// wholememory_ops/temp_memory_handle.hpp:23-93): create ctx -> malloc -> free -> destroy ctx.
class temp_mem {
 public:
  explicit temp_mem(wholememory_env_func_t* env);
  ~temp_mem();
  temp_mem(const temp_mem&)            = delete;
  temp_mem& operator=(const temp_mem&) = delete;
  void* alloc(int64_t elt_count, wholememory_dtype_t dtype, wholememory_memory_allocation_type_t type);
  void* device(int64_t n, wholememory_dtype_t dt) { return alloc(n, dt, WHOLEMEMORY_MA_DEVICE); }
  void* pinned(int64_t n, wholememory_dtype_t dt) { return alloc(n, dt, WHOLEMEMORY_MA_PINNED); }
  void* host(int64_t n, wholememory_dtype_t dt) { return alloc(n, dt, WHOLEMEMORY_MA_HOST); }
  void* get() const { return ptr_; }

 private:
  wholememory_env_func_t* env_;
  void* ctx_ = nullptr;
  void* ptr_ = nullptr;
};

// The id sort every op shares (backend.hpp: dedup_ids) with its scratch, which lives as long as the object: the distinct ids
// in ascending order of their (unsigned) keys, where the run of each one starts in the sorted batch, the stable order that
// sorts the batch, and the number of distinct ids, still on the device.
struct sorted_ids {
  explicit sorted_ids(wholememory_env_func_t* env);
  // allocates unique [n], starts [n + 1], order [n], n_unique_dev [1] and the sort's workspace, in that order, and queues
  // the sort on `stream`. Returns the backend's code as it is (0; -1: an index dtype or an n the sort does not take): what a
  // failure means is the caller's business. Does not ask device_error(), which clears the code it reads.
  int run(const void* ids, wholememory_dtype_t index_dtype, int64_t n, int64_t key_upper_bound, int64_t key_lower_bound,
          void* stream);
  // run(), with -1 thrown as logic_error and any other failure as hip_error
  void run_or_throw(const void* ids, wholememory_dtype_t index_dtype, int64_t n, int64_t key_upper_bound,
                    int64_t key_lower_bound, void* stream);
  void* unique          = nullptr;  // [n] of the index dtype
  int32_t* starts       = nullptr;
  int32_t* order        = nullptr;
  int64_t* n_unique_dev = nullptr;

 private:
  temp_mem unique_mem_, starts_mem_, order_mem_, n_unique_mem_, ws_mem_;
};

// Result of bucket + exchange of lookup ids (reference bucket_and_exchange_ids_func,
// functions/exchange_ids_nccl_func.cu:157-226).
struct id_exchange {
  explicit id_exchange(wholememory_env_func_t* env)
    : bucketed_mem(env), raw_mem(env), recv_mem(env), aux_offsets(env), aux_counts(env), aux_ws(env)
  {
  }
  std::vector<int64_t> send_counts, recv_counts;    // per peer, as they travel (self = 0 when kept local)
  std::vector<int64_t> send_offsets, recv_offsets;  // exclusive prefix of the above, W+1
  std::vector<int64_t> bucket_offsets;              // W+1: where each owner's segment starts in bucketed_ids
  int64_t total_send  = 0;                          // ids that travel
  int64_t total_recv  = 0;                          // ids received from peers
  int64_t total_valid = 0;                          // non-negative ids of this rank (all owners)
  int64_t global_moved = 0;                         // ids that change rank, summed over ALL ranks (same on every rank)
  // one rank and not a single negative id: nothing was moved or dropped — bucketed_ids IS the caller's array and
  // raw_indices (null) stands for the identity. Only produced when the caller asked for it (allow_identity)
  bool identity = false;
  // the ids were handed over sorted and distinct (sorted_unique): bucketed_ids IS that array, owner segments are its
  // contiguous pieces and raw_indices (null) stands for the identity — rows can be received straight into a dense
  // [total_valid, dim] buffer in bucketed order, with no reorder pass
  bool presorted = false;
  // mean over the ranks of the duplicate estimate (permille of the sampled ids), when bucket_and_exchange_ids was asked
  // for it; the same number on every rank
  int64_t dup_permille = 0;
  int64_t self_count  = 0;                          // ids of this rank that it owns itself
  int64_t self_offset = 0;                          // their position in bucketed_ids / raw_indices
  void* bucketed_ids   = nullptr;                   // [n]   ids grouped by owner (index dtype)
  int64_t* raw_indices = nullptr;                   // [n]   original position of each grouped id
  void* recv_ids       = nullptr;                   // [total_recv] ids received, peer-major
  temp_mem bucketed_mem, raw_mem, recv_mem;
  // a deferred exchange (bucket_and_exchange_ids(..., defer_ids) then finish_id_exchange): row offsets on the device and the
  // bucketing workspace with the scanned block counts, kept from the first half for the second; aux_counts: its counts dummy
  temp_mem aux_offsets, aux_counts, aux_ws;
};

// ids that are already sorted (as unsigned keys) and distinct, their number still on the device: what dedup_ids leaves
struct sorted_unique {
  const int64_t* n_dev;  // device: number of ids (<= the n passed to bucket_and_exchange_ids)
  // optional (device): this rank's vote, carried in the spare slot of the counts exchange where the duplicate estimate of a
  // gather rides — id_exchange::dup_permille is then the mean of the ranks' votes, or -1 when any rank voted below zero (a
  // veto: every rank learns it from the same W numbers and takes the same way out)
  const int64_t* vote_dev = nullptr;
};
void bucket_and_exchange_ids(wholememory_comm_t comm, const void* indices, wholememory_dtype_t index_dtype, int64_t n,
                             const std::vector<size_t>& entry_offsets, wholememory_env_func_t* env, void* stream,
                             id_exchange* x, bool keep_self_local = false, bool allow_identity = false,
                             const sorted_unique* sorted = nullptr, bool estimate_duplicates = false,
                             bool defer_ids = false);
void finish_id_exchange(wholememory_comm_t comm, const void* indices, wholememory_dtype_t index_dtype, int64_t n,
                        const std::vector<size_t>& entry_offsets, wholememory_env_func_t* env, void* stream, id_exchange* x);

// all-to-all-v of fixed-size rows with explicit per-peer row offsets on both sides
void exchange_segments(wholememory_comm_t comm, const void* send, const std::vector<int64_t>& send_counts,
                       const std::vector<int64_t>& send_offsets, void* recv, const std::vector<int64_t>& recv_counts,
                       const std::vector<int64_t>& recv_offsets, size_t row_bytes, void* stream);

// all-to-all-v of fixed-size rows: counts in rows, peer-major contiguous on both sides
void exchange_rows(wholememory_comm_t comm, const void* send, const std::vector<int64_t>& send_counts, void* recv,
                   const std::vector<int64_t>& recv_counts, size_t row_bytes, void* stream);

// number of row-chunks the rows all-to-all-v is pipelined in (WM_EXCHANGE_CHUNKS overrides; 1 = no pipelining);
// global_moved = id_exchange::global_moved, so that every rank decides alike
int exchange_chunks(int world_size, int64_t global_moved);

// RAII bundle of backend events
class event_set {
 public:
  explicit event_set(int n);
  ~event_set();
  event_set(event_set&& o) noexcept : events_(std::move(o.events_)) {}
  void* operator[](int i) const { return events_[i]; }

 private:
  std::vector<void*> events_;
};

// ---- the chunked row exchange of the distributed gather, the distributed scatter and the sparse gradient apply ----------
// (exchange_plan.hpp has its index arithmetic; loopback — WM_EXCHANGE_SELF=1 — makes the self segment travel like a peer's)

// One row kernel per PEER, chunk and side (2 (W - 1) C + 1 per call; rounds 2-4) instead of one per chunk and side: backends
// without permute_chunks, more than 16 ranks, one peer (a chunk is one range already), or the knob that asks for it
bool exchange_per_peer(int world_size);

// `src` (raw_indices or recv_ids: the peer-major array of `side`) as the side's row ranges index it: `src` itself unless the
// side is chunk-major and has rows — then a chunk-major copy in `mem`, made by one small kernel that `launches` counts
const void* chunk_major_copy(const void* src, wholememory_dtype_t dtype, const exchange_side& side, temp_mem* mem,
                             std::atomic<int64_t>* launches, void* stream);

// The two-stream pipeline over C chunks. produce(c) fills chunk c of the send buffer on `stream` (HBM), exchange(c, s) is
// its all-to-all-v on stream s (xGMI), consume(c) uses what arrived, on `stream` again (HBM). With one chunk all three run
// on `stream`, without events. Otherwise the exchanges run on the communicator's side stream and the issue order on `stream`
// is P_0 P_1 C_0 P_2 C_1 ... (for the gather G_0 G_1 R_0 G_2 R_1 ...), so that P_{c+1} and C_{c-1} run while chunk c is on the
// links; the wait for the last chunk also orders every side-stream access to the buffers before anything later on `stream`.
// consume may be empty: nothing on `stream` then waits for the rows, and the ONE event recorded behind the last exchange is
// returned for whoever reads them — it must live until that wait is queued. (Empty set: one chunk, or a consume stage.)
using chunk_stage = std::function<void(int)>;
event_set pipeline_chunks(wholememory_comm_t comm, int C, void* stream, const chunk_stage& produce,
                          const std::function<void(int, void*)>& exchange, const chunk_stage& consume);

// Receive layout of the gradient routes: ids and rows of ALL requesters in rank-major order (that order defines the fp32
// summation order of duplicates), this rank's own segment in its slot among the peers'
struct rank_major_recv {
  rank_major_recv(const id_exchange& x, wholememory_comm_t comm);
  // the ids: the peers' segments were received compactly (self cut out) — into `dst` around the self slot, which is filled
  // from the bucketed ids (self_from_bucketed) or from what the loopback exchange delivered
  void place_ids(const id_exchange& x, size_t id_bytes, bool self_from_bucketed, char* dst, void* stream) const;
  std::vector<int64_t> counts, offsets;  // [W], [W+1]
  int64_t n_recv;
  int rank;
};

// row offsets [W+1] of a handle whose rows are entry_bytes wide
std::vector<size_t> entry_offsets_of(wholememory_handle_t handle, size_t entry_bytes);

// flat gref through which GLOBAL row ids address this rank's shard
wholememory_gref_t local_shard_gref(wholememory_handle_t handle);

// gref a kernel should use for a tensor mapped in this process (CONTINUOUS / CHUNKED handle or a plain pointer)
wholememory_error_code_t tensor_mapped_gref(wholememory_tensor_t t, wholememory_gref_t* gref);

struct row_cache;
// gather of an embedding with a device row cache (embedding_cache.hpp)
wholememory_error_code_t gather_cached(wholememory_tensor_t table, wholememory_tensor_t indices_tensor,
                                       wholememory_tensor_t output_tensor, wholememory_env_func_t* env, void* stream,
                                       int gather_sms, row_cache* cache, bool adjust_cache);

// true when a CHUNKED / CONTINUOUS table should be served through the all-to-all-v route (WM_MAPPED_VIA_EXCHANGE=1)
bool mapped_via_exchange(wholememory_tensor_t t, wholememory_memory_type_t mt);

}  // namespace wm
