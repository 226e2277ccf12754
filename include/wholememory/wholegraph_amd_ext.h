/*
 * wholegraph_amd — entry points that do NOT exist in the reference ABI.
 *
 *  (1) external-collective communicators: a communicator whose collectives are supplied by the
 *      host framework instead of RCCL. The product path never needs it on MI355X (RCCL over xGMI
 *      is the transport); it exists so the SAME orchestration code can be driven at world_size > 1
 *      over torch.distributed/gloo in the CPU test-suite, and for hosts that already own a
 *      communicator.
 *  (2) the raw device stages of the distributed path on plain device pointers (id bucketing,
 *      owner-side dedup + optimizer step), so parity tests can check each stage against the oracle
 *      through the C ABI.
 *      (2b) the neighbour aggregation of a sampled CSC block behind the GraphSAGE layer (forward and a deterministic
 *      backward).
 *      (2c) the multi-head graph attention of a sampled CSC block behind the GAT layer (forward and a deterministic
 *      backward).
 *      (2d) the neighbour aggregation of (2b) with a weight per edge (forward, and deterministic gradients into the rows
 *      and into the weights).
 *      (2g) the GATv2 ("dynamic") multi-head graph attention of a sampled CSC block behind the GATv2 layer (forward and a
 *      deterministic backward).
 *      (2h) the relation-typed neighbour aggregation of a sampled CSC block behind the RGCN layer: (2b) with a type per edge
 *      and one output slot per relation (forward and a deterministic backward).
 *      (2i) 8-bit row-quantized tables: a gather that dequantizes the rows it reads and a scatter that quantizes the rows
 *      it writes.
 *      (2j) the neighbour aggregation of (2b) whose rows are read, and dequantized, from a quantized table of (2i) by
 *      global id (forward).
 *      (2k) the scaled dot-product multi-head attention of a sampled CSC block behind the TransformerConv layer (forward
 *      and a deterministic backward).
 *      (2l) the multi-aggregator neighbour aggregation of a sampled CSC block behind the PNAConv layer: sum, mean, min, max
 *      and std of the neighbour rows out of one read of them (forward and a deterministic backward).
 *      (2m) random walks over a CSR graph held in WholeMemory, uniform or by edge weight, as one launch for the whole batch.
 *      (2n) node2vec (p, q) second-order walks over the same graph, with or without edge weights, as one launch.
 *      (2o) negative sampling over the same graph: per source node, K nodes that are not its neighbours, as one launch.
 *      (2p) the dot product of the two endpoint rows of every edge of a sampled CSC block: the score of skip-gram training
 *      over the walks and negatives above and of link prediction (forward and a deterministic backward).
 *      (2q) the node-induced subgraph of a CSR graph held in WholeMemory: all graph edges among a set of nodes as one local
 *      block, the batch of subgraph-wise training (GraphSAINT, ShaDow-GNN, Cluster-GCN).
 *      (2r) temporal neighbour sampling over the same graph with a timestamp per edge: per (node, time) centre, up to M
 *      neighbours whose edge is not in the centre's future, uniformly or the latest (TGN, TGAT).
 *  (3) the testing seam for the device backend (see wholegraph_amd/csrc/backend.hpp).
 */
#ifndef WHOLEMEMORY_WHOLEGRAPH_AMD_EXT_H_
#define WHOLEMEMORY_WHOLEGRAPH_AMD_EXT_H_

#include <wholememory/embedding.h>
#include <wholememory/wholememory_op.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) external collectives ------------------------------------------------------------ */
/* All byte counts/displacements are in BYTES; every function returns 0 on success. `stream` is the
 * hipStream_t the library is working on; a provider that stages through the host must order itself
 * after/before that stream. */
struct wm_ext_collectives_t {
  void* ctx;
  int (*barrier)(void* ctx);
  /* recv[r*bytes .. (r+1)*bytes) = rank r's send; HOST buffers */
  int (*allgather_host)(void* ctx, const void* send, void* recv, size_t bytes);
  /* DEVICE buffers (whatever the installed device backend calls device memory) */
  int (*alltoallv_device)(void* ctx,
                          const void* send,
                          const size_t* send_bytes,
                          const size_t* send_disp,
                          void* recv,
                          const size_t* recv_bytes,
                          const size_t* recv_disp,
                          void* stream);
};
#ifndef __cplusplus
typedef struct wm_ext_collectives_t wm_ext_collectives_t;
#endif

enum wholememory_error_code_t wholememory_create_communicator_ext(
  wholememory_comm_t* comm, int rank, int size, const struct wm_ext_collectives_t* collectives);

/* Which transport carries this communicator's collectives: name = "rccl" | "external" | "external (sub-group)" | "none"
 * (a single-rank communicator needs none); ranks = what the transport itself reports (ncclCommCount for RCCL, -1 when
 * it cannot tell, 0 for "none"). bench.py prints it so that an N-GPU line proves N RCCL ranks. */
enum wholememory_error_code_t wholememory_ext_communicator_transport(wholememory_comm_t comm, const char** name, int* ranks);

/* ---- (2) raw stages ------------------------------------------------------------------------ */
/* Owner bucketing of ids (reference bucket_ids_func.cu:51-87 + the grouping effect of
 * exchange_ids_nccl_func.cu:42-92). entry_offsets: DEVICE uint64[world+1] row offsets. counts:
 * DEVICE int64[world]. bucketed_ids (index dtype) / raw_indices (int64): DEVICE [n] or both NULL for
 * counts only. Scratch comes from p_env_fns. Asynchronous on stream. */
enum wholememory_error_code_t wholememory_ext_bucket_ids(const void* indices,
                                                         enum wholememory_dtype_t index_dtype,
                                                         int64_t n,
                                                         const void* entry_offsets_dev,
                                                         int world_size,
                                                         int64_t* counts_dev,
                                                         void* bucketed_ids_dev,
                                                         int64_t* raw_indices_dev,
                                                         struct wholememory_env_func_t* p_env_fns,
                                                         void* stream);

/* The same with more row ranges than buckets: entry_offsets has owner_count+1 entries (owner_count >= bucket_count) and
 * an id of range o goes to bucket o % bucket_count — the first hop of the HIERARCHY gather (ranges = ranks of every node,
 * buckets = ranks of this node; reference bucket_and_reorder_ids_for_hierarchy_func, gather_op_impl_hierarchy.cu:194-205).
 * counts: DEVICE int64[bucket_count]. */
enum wholememory_error_code_t wholememory_ext_bucket_ids_folded(const void* indices,
                                                                enum wholememory_dtype_t index_dtype,
                                                                int64_t n,
                                                                const void* entry_offsets_dev,
                                                                int owner_count,
                                                                int bucket_count,
                                                                int64_t* counts_dev,
                                                                void* bucketed_ids_dev,
                                                                int64_t* raw_indices_dev,
                                                                struct wholememory_env_func_t* p_env_fns,
                                                                void* stream);

/* Owner-side "dedup + optimizer step" on received (ids, grads): reference
 * exchange_embeddings_nccl_func.cu:76-174 followed by embedding_optimizer_func.cu steps, fused.
 * opt_params: float[6] = {weight_decay, epsilon, beta1, beta2, alpha, adam_w}. State pointers may be
 * NULL when the optimizer has none. Synchronises `stream` before returning the unique count. */
enum wholememory_error_code_t wholememory_ext_dedup_apply(const void* recv_ids,
                                                          enum wholememory_dtype_t index_dtype,
                                                          int64_t n_recv,
                                                          const float* recv_grads,
                                                          int64_t grad_stride,
                                                          int64_t dim,
                                                          float* local_table,
                                                          int64_t table_stride,
                                                          int64_t local_entry_offset,
                                                          int64_t local_entry_count,
                                                          enum wholememory_optimizer_type_t opt_type,
                                                          const float* opt_params,
                                                          float lr,
                                                          float* per_element_state,
                                                          float* per_row_state,
                                                          int64_t* n_unique_host,
                                                          struct wholememory_env_func_t* p_env_fns,
                                                          void* stream);

/* round-robin id remap (reference map_indices_func.cu:26-106) on raw device pointers */
enum wholememory_error_code_t wholememory_ext_round_robin_map(const void* ids,
                                                              void* mapped,
                                                              enum wholememory_dtype_t index_dtype,
                                                              int64_t n,
                                                              int64_t entry_start,
                                                              int world_size,
                                                              int round_robin_size,
                                                              void* stream);

/* name of the installed device backend ("hip-gfx950" in the product) */
const char* wholememory_ext_backend_name();

/* demangled name the HIP runtime holds (hipKernelNameRefByPtr) for the gather / scatter kernel instantiation the calling
 * thread launched last; "" before the first launch */
const char* wholememory_ext_last_rows_kernel();

/* One hop of multi-layer neighbour sampling as one call: unweighted sampling without replacement of every node of
 * `center_nodes_tensor` followed by graph_append_unique(center nodes, sampled neighbours), with ONE host round trip to size
 * the outputs instead of the two of the separate ops (reference: wholegraph_csr_unweighted_sample_without_replacement,
 * include/wholememory/wholegraph_op.h, + graph_append_unique, graph_op.h, driven per hop by
 * python/pylibwholegraph/pylibwholegraph/torch/graph_structure.py:140-196). Outputs, bit-identical to that sequence:
 *   output_sample_offset_tensor  int32 [n_center + 1], caller-allocated (csr_row_ptr of the sampled block)
 *   unique        (memory context)  center nodes ++ new neighbour ids in first-occurrence order
 *   neighbor_pos  (memory context)  int32 [n_samples]: position of each sampled neighbour in `unique`
 *   center_lid    (memory context)  int32 [n_samples]: position of its centre in center_nodes_tensor
 * WHOLEMEMORY_NOT_SUPPORTED (nothing queued, nothing allocated) when the CSR is not mapped into this rank (DISTRIBUTED /
 * HIERARCHY), when column ids and center ids differ in dtype, when max_sample_count <= 0 or the center array is empty:
 * the caller then runs the two ops. */
wholememory_error_code_t wholememory_ext_sample_append_unique(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t center_nodes_tensor, int max_sample_count, unsigned long long random_seed,
  wholememory_tensor_t output_sample_offset_tensor, void* output_unique_memory_context,
  void* output_neighbor_pos_memory_context, void* output_center_localid_memory_context, wholememory_env_func_t* p_env_fns,
  void* stream);

/* wholememory_ext_sample_append_unique with the WEIGHTED sampler (wholegraph_csr_weighted_sample_without_replacement on
 * wm_csr_weight_ptr_tensor: one float or double per edge): same outputs, bit-identical to that sampler followed by
 * graph_append_unique, ONE host round trip. WHOLEMEMORY_NOT_SUPPORTED (nothing queued, nothing allocated) in every case the
 * unweighted call answers it, and when the weight tensor is not mapped into this rank (DISTRIBUTED / HIERARCHY), is not float
 * or double, does not hold one entry per edge, or max_sample_count > 8192: the two-op route then reports what is wrong. */
wholememory_error_code_t wholememory_ext_weighted_sample_append_unique(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t center_nodes_tensor, int max_sample_count,
  unsigned long long random_seed, wholememory_tensor_t output_sample_offset_tensor, void* output_unique_memory_context,
  void* output_neighbor_pos_memory_context, void* output_center_localid_memory_context, wholememory_env_func_t* p_env_fns,
  void* stream);

/* Every hop of a multi-layer unweighted sample (hop = neighbour sample + graph_append_unique, as in
 * wholememory_ext_sample_append_unique) in ONE call with NO host round trip inside. The caller sizes every array for its upper
 * bound: hop h (h = 0 next to the seeds) has at most cap_c[h] centres and cap_s[h] = cap_c[h] * max_sample_counts[h] samples,
 * cap_c[0] = number of seeds, cap_c[h + 1] = cap_c[h] + cap_s[h]:
 *   sample_offsets[h]  int32 [cap_c[h] + 1]        unique[h]       id dtype [cap_c[h] + cap_s[h]]
 *   neighbor_pos[h]    int32 [cap_s[h]]            center_lid[h]   int32 [cap_s[h]]
 * all DEVICE memory; counts_host: PINNED host memory the device can write, 2 * hops ints — the last kernel of hop h leaves
 * {samples, new unique ids} of that hop in counts_host[2h], counts_host[2h + 1]. After ONE stream synchronise the caller
 * trims: with n_c[0] = seeds and n_c[h + 1] = n_c[h] + new[h], hop h's csr_row_ptr is sample_offsets[h][0 .. n_c[h]], its
 * widened frontier unique[h][0 .. n_c[h + 1]), neighbor_pos / center_lid the first samples[h] entries. Bit-identical to `hops`
 * calls of wholememory_ext_sample_append_unique with the same seeds. WHOLEMEMORY_NOT_SUPPORTED (nothing queued) when the CSR is
 * not mapped into this rank, the id dtypes differ, there is no seed, a fan-out is <= 0 or a hop's upper bounds exceed what
 * graph_append_unique's hash-table route takes (the caller then runs hop by hop). With sample_offsets == NULL the call is a QUERY:
 * it answers SUCCESS / NOT_SUPPORTED for these tensors, hops and fan-outs and touches nothing else — ask before allocating the
 * upper-bound buffers. Reference call sequence:
 * python/pylibwholegraph/pylibwholegraph/torch/graph_structure.py:140-196. */
enum wholememory_error_code_t wholememory_ext_multilayer_sample(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor, wholememory_tensor_t seed_nodes_tensor,
  int hops, const int* max_sample_counts, const unsigned long long* random_seeds, void* const* sample_offsets,
  void* const* unique, int* const* neighbor_pos, int* const* center_lid, int* counts_host,
  struct wholememory_env_func_t* p_env_fns, void* stream);

/* wholememory_ext_multilayer_sample with the WEIGHTED sampler on every hop (one weight tensor: a float or double per edge):
 * same arrays, same counts, same QUERY mode (sample_offsets == NULL), bit-identical to `hops` calls of
 * wholememory_ext_weighted_sample_append_unique with the same seeds. WHOLEMEMORY_NOT_SUPPORTED (nothing queued) in every case
 * the unweighted chain answers it, for a weight tensor that call declines, and for a fan-out above 8192. */
enum wholememory_error_code_t wholememory_ext_multilayer_sample_weighted(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t seed_nodes_tensor, int hops, const int* max_sample_counts,
  const unsigned long long* random_seeds, void* const* sample_offsets, void* const* unique, int* const* neighbor_pos,
  int* const* center_lid, int* counts_host, struct wholememory_env_func_t* p_env_fns, void* stream);

/* wholememory_ext_sample_append_unique / wholememory_ext_weighted_sample_append_unique plus the graph EDGE ID of every sample.
 * wm_csr_weight_ptr_tensor == NULL selects the unweighted sampler, a tensor the weighted one. Outputs: those of the fused hop,
 * bit for bit, and
 *   edge_gid      (memory context)  int64 [n_samples]: position in wm_csr_col_ptr_tensor of the edge each sample was drawn
 *                                   from, aligned with neighbor_pos / center_lid — what the one-hop samplers deliver through
 *                                   output_edge_gid_memory_context
 * Still ONE host round trip. WHOLEMEMORY_INVALID_INPUT for a NULL edge id context (as for the other contexts);
 * WHOLEMEMORY_NOT_SUPPORTED (nothing queued, nothing allocated) in every case wholememory_ext_sample_append_unique answers it
 * and, with a weight tensor, in every case wholememory_ext_weighted_sample_append_unique does. */
enum wholememory_error_code_t wholememory_ext_sample_append_unique_edges(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t center_nodes_tensor, int max_sample_count,
  unsigned long long random_seed, wholememory_tensor_t output_sample_offset_tensor, void* output_unique_memory_context,
  void* output_neighbor_pos_memory_context, void* output_center_localid_memory_context, void* output_edge_gid_memory_context,
  struct wholememory_env_func_t* p_env_fns, void* stream);

/* wholememory_ext_multilayer_sample / wholememory_ext_multilayer_sample_weighted (wm_csr_weight_ptr_tensor == NULL: unweighted)
 * plus, per hop, the graph edge ids of the samples and — optionally — attributes of those edges, all still in ONE call with NO
 * host round trip inside:
 *   edge_gid[h]                 int64 [cap_s[h]]   first samples[h] entries defined: position in wm_csr_col_ptr_tensor of the
 *                                                  edge each sample was drawn from, aligned with neighbor_pos[h] / center_lid[h]
 *   attr_out[h * n_attrs + k]   [cap_s[h]] elements of attr_tensors[k]'s dtype, first samples[h] entries defined:
 *                                                  attr_tensors[k][edge_gid[h][i]]   (n_attrs > 0 only)
 * all DEVICE memory sized by the caller like neighbor_pos[h]. The attributes are fetched by one more kernel queued behind hop h
 * (several when n_attrs > 8) that reads the hop's sample count on the device — sample_offsets[h][cap_c[h]], the last entry of the
 * offsets array at its upper-bound size. An attribute tensor the kernel takes is 1-D with 4- or 8-byte elements (float, int32,
 * int64, double; the values are moved as bits), one entry per edge, mapped into this rank (CONTINUOUS / CHUNKED / plain device
 * memory). Every other array, the counts in counts_host and the QUERY mode (sample_offsets == NULL: edge_gid, attr_out, the
 * seeds and counts_host are not looked at, attr_tensors is) are those of wholememory_ext_multilayer_sample; the outputs equal
 * those of `hops` calls of wholememory_ext_sample_append_unique_edges with the same seeds bit for bit.
 * WHOLEMEMORY_INVALID_INPUT, before anything else is looked at: n_attrs < 0, n_attrs > 0 with attr_tensors == NULL or a NULL
 * entry in it, and on a call that is not a query edge_gid == NULL or n_attrs > 0 with attr_out == NULL.
 * WHOLEMEMORY_NOT_SUPPORTED (nothing queued; a query answers the same): every case the chain without edge ids answers it (with a
 * weight tensor: the weighted chain), an attribute tensor that is DISTRIBUTED / HIERARCHY, not 1-D, of another element size or
 * not one entry per edge — the caller leaves that attribute out and gathers it by edge id afterwards — and a device backend
 * without the attribute kernel when n_attrs > 0. */
enum wholememory_error_code_t wholememory_ext_multilayer_sample_edges(
  wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_weight_ptr_tensor, wholememory_tensor_t seed_nodes_tensor, int hops, const int* max_sample_counts,
  const unsigned long long* random_seeds, void* const* sample_offsets, void* const* unique, int* const* neighbor_pos,
  int* const* center_lid, int64_t* const* edge_gid, int n_attrs, const wholememory_tensor_t* attr_tensors,
  void* const* attr_out, int* counts_host, struct wholememory_env_func_t* p_env_fns, void* stream);

/* Number of wholememory_ext_multilayer_sample_edges calls of this process that were not queries and returned
 * WHOLEMEMORY_SUCCESS: how a caller with several sampling routes (GraphStructure.multilayer_sample_with_edge_attributes) shows
 * which one ran. A counter for tests and benchmarks. */
int64_t wholememory_ext_edge_chain_calls(void);

/* Completion semantics of the ops whose reference versions drain the stream before returning (neighbour sampling,
 * graph_append_unique and the fused hop above). Default 0 = the reference's: outputs complete and scratch idle at return,
 * safe with any env functions. 1 = the ops return with their last kernels queued on `stream` (one host round trip fewer
 * per call); only legal when every allocator behind p_env_fns is stream-ordered on that stream and every consumer of the
 * outputs is ordered on it — wholegraph_amd.torch declares it for torch's caching allocator. Process-wide;
 * WM_ASYNC_OPS=0/1 in the environment overrides the call. */
enum wholememory_error_code_t wholememory_ext_set_async_completion(int on);

/* Environment knobs (WM_* / WG_* variables) are read ONCE, the first time the code that consults one runs; no op calls
 * getenv afterwards. A program that changes such a variable later (A/B experiments, tests) calls this to make every knob
 * read its variable again at its next use. Not to be called while ops run on other threads. */
enum wholememory_error_code_t wholememory_ext_reload_knobs(void);

/* Placement probe: milliseconds per GiB of pseudo-random 512-byte rows of [ptr, ptr + bytes) touched by a fixed kernel
 * (kind 0 = zeros written: destroys the contents, 1 = read, 2 = read and written back), averaged over `reps` launches after a
 * warm-up; blocks until done. The level the memory system serves random row accesses at depends on where a large allocation
 * sits in HBM and stays with it for its lifetime. wholememory_malloc makes ONE allocation per device
 * shard, like the reference; WM_MALLOC_PROBE=auto (self-calibrating: candidates are added until two agree with the best seen
 * within 3 %) or =K (exactly K candidates) opts into choosing the shard with this probe — the candidates are alive together,
 * capped at a quarter of the free memory, one prober per device at a time. */
enum wholememory_error_code_t wholememory_ext_probe_memory(void* ptr, size_t bytes, int kind, int reps, float* ms_per_gib);

/* The placement probe of wholememory_malloc (above) without the environment: "auto", "2" ... "8" (that many candidates), "off",
 * or "env" / NULL (follow WM_MALLOC_PROBE again, the initial state). Applies to the device allocations this process makes from
 * now on, until changed; WHOLEMEMORY_INVALID_INPUT for anything else. pylibwholegraph: create_embedding(...,
 * placement_probe="auto") sets it around the one creation. Tables that are written at random — scatter targets, trained
 * embeddings — are what it is for: their speed follows the placement of the shard by up to 20 %. */
enum wholememory_error_code_t wholememory_ext_set_malloc_probe(const char* mode);
/* The mode set by the call above ("env" when none is), written to mode[capacity >= 8]: for callers that set a mode around ONE
 * allocation and restore what was there before. */
enum wholememory_error_code_t wholememory_ext_get_malloc_probe(char* mode, size_t capacity);
/* 1 when the local shard of the handle was chosen among several probed candidates, else 0 */
int wholememory_ext_handle_was_probed(wholememory_handle_t handle);

/* Number of wholememory_gather calls of this process that took the sorted-ids route of HOST-located tables (rows of at most
 * 512 bytes, batches of at least WM_HOST_SORTED_MIN ids: wholememory_op.h / gather_op.cpp:116-120 of the reference).
 * A counter for tests and benchmarks. */
int64_t wholememory_ext_host_sorted_gathers(void);

/* Number of owner-side id sorts (gradient apply, cached gather) of this process that were queued as the two-stage split sort
 * (csrc/kernels/split_sort.cuh: bounded ids, at least WM_DEDUP_SPLIT_MIN of them, a bucket plan that fits) rather than as the
 * generic radix sort. Whether a queued split sort then found a bucket too large and handed the batch to the gated generic path
 * is decided on the device and not visible here. A counter for tests and benchmarks. */
int64_t wholememory_ext_split_sorts(void);

/* Kernel launches of this process since the last call whose grid was sized by the block ops' shared helper (blocks_for() of
 * csrc/kernels/agg_common.cuh: the agg_concat family, agg_concat_pna, the attention ops and their shared backward walk), and
 * how many of them wanted more workgroups than the cap allowed and so run their grid-stride loop more than once
 * ("truncated"). The cap is 2^20 workgroups, or min(WM_AGG_MAX_BLOCKS, 2^20) when that knob is a positive integer. Either
 * pointer may be NULL. Reading resets both counters. A counter for tests. */
void wholememory_ext_agg_grid_stats(int64_t* launches, int64_t* truncated);

/* Duplicate runs of the last finished ORDERED gradient step on the current device that were summed through a dense transposed
 * copy of their gradient rows (csrc/kernels/long_dense.cuh: runs of at least WM_DENSE_FOLD_MIN rows, default 131072, while
 * 3 n / 8 rows of copies last; WM_DENSE_FOLD=0 switches the route off). Read after a synchronise. A counter for tests. */
int64_t wholememory_ext_dense_fold_last(void);

/* Kernels queued so far by the DISTRIBUTED gather route of this process (owner-side row gathers, reorder-on-receive
 * scatters, the two chunk-major copies): with C exchange chunks a call costs at most 2 C + 3 of them whatever the number of
 * ranks (rounds 2-4: 2 (W - 1) C + 1). A counter for tests. */
int64_t wholememory_ext_distributed_gather_launches(void);

/* The same for the DISTRIBUTED scatter route (line-up gathers of the rows to send, owner-side writes, this rank's own rows,
 * the two chunk-major copies): at most 2 C + 3 per call (rounds 1-5: 2 (W - 1) C + 1). A counter for tests. */
int64_t wholememory_ext_distributed_scatter_launches(void);

/* Row kernels queued so far in FRONT of the gradient exchange of wholememory_embedding_gather_gradient_apply (the chunk-major
 * copy of the positions, the line-up gathers of the gradient rows to send, a copy of this rank's own rows when they are not
 * read in place): at most C + 2 per call whatever the number of ranks (rounds 1-5: (W - 1) C + 1). The receive side launches
 * nothing per chunk: rows arrive in rank-major order, which is the order of the fp32 sum of duplicates. A counter for tests. */
int64_t wholememory_ext_gradient_exchange_launches(void);

/* Bytes this process has handed to the all-to-all-v transport for OTHER ranks so far (ids and rows of every distributed op;
 * this rank's own segment counts where it travels like a peer's: WM_EXCHANGE_SELF=1). A counter for tests and for the
 * first-contact report: the sender-side combination of duplicate gradient rows halves it on a Zipf(1.05) batch. */
int64_t wholememory_ext_alltoallv_bytes(void);

/* Calls of wholememory_embedding_gather_gradient_apply that took the COMBINED route: several ranks, a fold that is not bound to
 * the reference's order (optimizer parameter grad_fold = tree / WM_GRAD_FOLD=tree / a 16-bit table) and enough duplicates
 * (decided by all ranks from the duplicate estimates in the counts exchange; WM_GRAD_COMBINE=0|1 forces): every rank folds ITS
 * duplicates of an id into one partial sum before the exchange, the owner folds at most world_size partial rows per id. */
int64_t wholememory_ext_combined_gradient_calls(void);

/* ---- (2b) neighbour aggregation of a sampled CSC block (GraphSAGE `agg_concat`) -------------------------------- */
/* The block as the sampler and graph_append_unique leave it: row_ptr int32 [n_dst + 1] with row_ptr[n_dst] = n_edges,
 * col_ind int32 [n_edges] in [0, n_src) (out-of-range ids are the caller's contract), x fp32 [n_src, x_stride] whose first
 * n_dst rows are the targets themselves. Strides in elements, all arrays DEVICE memory, all work queued on `stream`.
 *
 * forward: out [n_dst, out_stride] fp32, out_stride >= 2 * dim.
 *   out[d, 0:dim]     = A(d). S(d) = fp32 sum of x[col_ind[e]] for e = row_ptr[d] .. row_ptr[d+1] - 1, added left to right
 *                       from the first term. SUM: A = S. MEAN: A = S * fl(1.0f / deg(d)) (one multiply). No edge: +0.0.
 *   out[d, dim:2dim]  = x[d].
 * backward: grad_out [n_dst, grad_out_stride] (2 * dim columns used) -> grad_x [n_src, grad_x_stride], every row written.
 *   t(e) = grad_out[dst(e), 0:dim] (times fl(1.0f / deg(dst(e))) for MEAN). P(s) sums t(e) over the edges with
 *   col_ind[e] = s in ascending edge position: left to right from the first term when s has at most C edges; otherwise the
 *   edges are cut into consecutive chunks of C, each chunk summed left to right and the chunk sums added in chunk order,
 *   ((p0 + p1) + p2) + ... . grad_x[s] = P(s) + grad_out[s, dim:2dim] (the self term added last, only for s < n_dst); with one
 *   part missing the other is copied, with neither the row is +0.0. C = wholememory_ext_csc_aggregate_chunk_edges(). The
 *   order is fixed: results are bitwise reproducible, no atomics. The edge index is built with the library's id sort, scratch
 *   from p_env_fns.
 * n_edges = 0 and n_dst = 0 are valid. INVALID_INPUT, before any device work and under every backend, for null pointers,
 * negative sizes, dim < 1, n_dst > n_src, strides smaller than the row, an unknown aggr; then NOT_SUPPORTED (nothing queued)
 * when the device backend has no such kernels. Every entry point over a sampled block (2b - 2l) answers in this order: the
 * arguments are judged first, then the backend's capability, then (where there is a table) the table's memory type. */
enum wholememory_ext_aggr_t {
  WHOLEMEMORY_EXT_AGGR_SUM  = 0,
  WHOLEMEMORY_EXT_AGGR_MEAN = 1,
};
enum wholememory_error_code_t wholememory_ext_csc_aggregate_forward(const int32_t* row_ptr,
                                                                    const int32_t* col_ind,
                                                                    int64_t n_edges,
                                                                    int64_t n_dst,
                                                                    int64_t n_src,
                                                                    const float* x,
                                                                    int64_t x_stride,
                                                                    int64_t dim,
                                                                    int aggr,
                                                                    float* out,
                                                                    int64_t out_stride,
                                                                    struct wholememory_env_func_t* p_env_fns,
                                                                    void* stream);
enum wholememory_error_code_t wholememory_ext_csc_aggregate_backward(const int32_t* row_ptr,
                                                                     const int32_t* col_ind,
                                                                     int64_t n_edges,
                                                                     int64_t n_dst,
                                                                     int64_t n_src,
                                                                     const float* grad_out,
                                                                     int64_t grad_out_stride,
                                                                     int64_t dim,
                                                                     int aggr,
                                                                     float* grad_x,
                                                                     int64_t grad_x_stride,
                                                                     struct wholememory_env_func_t* p_env_fns,
                                                                     void* stream);
/* C of the backward's chunked sums (a compile-time constant of the library) */
int64_t wholememory_ext_csc_aggregate_chunk_edges(void);

/* (2b, rows of 16-bit floats) The same op with x, out, grad_out and grad_x all of type T = `dtype`: WHOLEMEMORY_DT_HALF
 * (IEEE binary16) or WHOLEMEMORY_DT_BF16; strides in elements of T. Every sum is taken in fp32, in exactly the order
 * stated above, and each output element is rounded to T once, round to nearest even. Widening T -> fp32 is exact, so:
 *   forward: S(d) = fp32 sum of fp32(x[col_ind[e]]), left to right from the first term. A = S (SUM) or
 *     S * fl(1.0f / deg(d)) (MEAN, one fp32 multiply). out[d, 0:dim] = round_T(A); no edge: +0.0. out[d, dim:2dim] = x[d],
 *     copied bit for bit.
 *   backward: t(e) = fp32(grad_out[dst(e), 0:dim]), times fl(1.0f / deg(dst(e))) in fp32 for MEAN. P(s) as above, with the
 *     same chunk size C; the partial rows of chunks stay fp32 in the workspace.
 *     grad_x[s] = round_T(P(s) + fp32(grad_out[s, dim:2dim])) (the self term last, s < n_dst only); only the self term: its
 *     bits are copied; only P: round_T(P); neither: +0.0. No atomics; bitwise reproducible.
 *   fp16 results that leave the fp16 range round to +-inf (IEEE); results in the subnormal range of T are rounded, not
 *     flushed. A NaN stays a NaN (payload not specified).
 * The running sum never lives in T. Hence, for any input, op_T(x) == round_T(op_fp32(fp32(x))) bit for bit: the A half of
 * the forward, and the backward (the copied halves are equal as well, since widening and rounding back is the identity
 * on every value but a NaN's payload).
 * WHOLEMEMORY_DT_FLOAT takes the fp32 entry points above (the same bits); any other dtype is INVALID_INPUT. All other
 * argument checks, and NOT_SUPPORTED, as for the fp32 entry points. */
enum wholememory_error_code_t wholememory_ext_csc_aggregate_forward_typed(const int32_t* row_ptr,
                                                                          const int32_t* col_ind,
                                                                          int64_t n_edges,
                                                                          int64_t n_dst,
                                                                          int64_t n_src,
                                                                          const void* x,
                                                                          int64_t x_stride,
                                                                          int64_t dim,
                                                                          int aggr,
                                                                          void* out,
                                                                          int64_t out_stride,
                                                                          enum wholememory_dtype_t dtype,
                                                                          struct wholememory_env_func_t* p_env_fns,
                                                                          void* stream);
enum wholememory_error_code_t wholememory_ext_csc_aggregate_backward_typed(const int32_t* row_ptr,
                                                                           const int32_t* col_ind,
                                                                           int64_t n_edges,
                                                                           int64_t n_dst,
                                                                           int64_t n_src,
                                                                           const void* grad_out,
                                                                           int64_t grad_out_stride,
                                                                           int64_t dim,
                                                                           int aggr,
                                                                           void* grad_x,
                                                                           int64_t grad_x_stride,
                                                                           enum wholememory_dtype_t dtype,
                                                                           struct wholememory_env_func_t* p_env_fns,
                                                                           void* stream);

/* ---- (2c) multi-head graph attention of a sampled CSC block (GAT `mha_gat_n2n`) ------------------------------ */
/* The block as for (2b): row_ptr int32 [n_dst + 1], col_ind int32 [n_edges] in [0, n_src), h fp32 [n_src, h_stride] with
 * H * F columns used (H = heads, F = dim; the layer's lin(x)), whose first n_dst rows are the targets. Head k owns the
 * columns [k*F, (k+1)*F) of a row. att fp32 [2 * H * F], viewed as (2, H, F): half 0 is the source (neighbour) side, half 1
 * the target side (cugraph-ops' layout). Strides in elements, all arrays DEVICE memory, all work queued on `stream`.
 * Every `*` and `+` below is one fp32 operation, rounded on its own (no fused multiply-add). A sum "left to right" starts
 * from its first term; a sum with no term is +0.0.
 *
 * forward: writes scores [n_src + n_dst, H] (s_src then s_dst), alpha [n_edges, H] and out, all of which the backward
 * reads back.
 *   s_src[j,k] = sum over f of att[0,k,f] * h[j,k,f], left to right (j < n_src); s_dst[d,k] the same with att[1] (d < n_dst).
 *   For each edge e of target d (e = row_ptr[d] .. row_ptr[d+1] - 1): z = s_src[col_ind[e],k] + s_dst[d,k],
 *   l = z > 0 ? z : negative_slope * z. m = max of l over the edges of d; w = expf(l - m) (the device's expf);
 *   den = sum of w over the edges of d, left to right; alpha[e,k] = w / den.
 *   o[d,k,:] = sum of alpha[e,k] * h[col_ind[e],k,:] over the edges of d, left to right; +0.0 for a target without edges.
 *   concat != 0: out [n_dst, out_stride >= H*F] = o. concat == 0: out [n_dst, out_stride >= F] =
 *   ((o[d,0,:] + o[d,1,:]) + ...) * fl(1.0f / H).
 * backward: grad_out G [n_dst, grad_out_stride] (H*F columns with concat, else F) -> grad_h [n_src, grad_h_stride >= H*F]
 * (every row written) and grad_att [2*H*F].
 *   G_k[d,f] = G[d, k*F + f] with concat, else G[d,f] * fl(1.0f / H).
 *   da[e,k] = sum over f of G_k[d,f] * h[col_ind[e],k,f], left to right. c[d,k] = sum of alpha[e,k] * da[e,k] over the
 *   edges of d, left to right. dl = alpha * (da - c); dz = z > 0 ? dl : dl * negative_slope (z recomputed from scores).
 *   ds_dst[d,k] = sum of dz over the edges of d, left to right.
 *   Per source j, over the edges with col_ind[e] = j in ascending edge position: P(j)[k,:] = sum of alpha[e,k] * G_k[d(e),:]
 *   and ds_src[j,k] = sum of dz[e,k]; left to right when j has at most C edges, otherwise cut into consecutive chunks of C
 *   edges, each chunk summed left to right and the chunk sums added in chunk order. C =
 *   wholememory_ext_csc_aggregate_chunk_edges().
 *   grad_h[j,k,:] = (P(j)[k,:] + ds_src[j,k] * att[0,k,:]) + ds_dst[j,k] * att[1,k,:], the last term only for j < n_dst.
 *   grad_att[0,k,f] = sum over j < n_src of ds_src[j,k] * h[j,k,f]; grad_att[1,k,f] the same over j < n_dst with ds_dst.
 *   Both are cut into node chunks of N = wholememory_ext_csc_gat_node_chunk() rows from row 0: each chunk summed left to
 *   right, the chunk sums added in chunk order.
 *   The order is fixed: results are bitwise reproducible, no atomics. The edge index is built with the library's id sort,
 *   scratch from p_env_fns.
 * n_edges = 0 and n_dst = 0 are valid. INVALID_INPUT, before any device work and under every backend, for null pointers,
 * negative sizes, heads < 1, dim < 1, n_dst > n_src, strides smaller than the row; then NOT_SUPPORTED (nothing queued) when
 * the device backend has no such kernels. */
enum wholememory_error_code_t wholememory_ext_csc_gat_forward(const int32_t* row_ptr,
                                                              const int32_t* col_ind,
                                                              int64_t n_edges,
                                                              int64_t n_dst,
                                                              int64_t n_src,
                                                              const float* h,
                                                              int64_t h_stride,
                                                              const float* att,
                                                              int64_t heads,
                                                              int64_t dim,
                                                              float negative_slope,
                                                              int concat,
                                                              float* out,
                                                              int64_t out_stride,
                                                              float* alpha,
                                                              float* scores,
                                                              struct wholememory_env_func_t* p_env_fns,
                                                              void* stream);
enum wholememory_error_code_t wholememory_ext_csc_gat_backward(const int32_t* row_ptr,
                                                               const int32_t* col_ind,
                                                               int64_t n_edges,
                                                               int64_t n_dst,
                                                               int64_t n_src,
                                                               const float* h,
                                                               int64_t h_stride,
                                                               const float* att,
                                                               int64_t heads,
                                                               int64_t dim,
                                                               float negative_slope,
                                                               int concat,
                                                               const float* alpha,
                                                               const float* scores,
                                                               const float* grad_out,
                                                               int64_t grad_out_stride,
                                                               float* grad_h,
                                                               int64_t grad_h_stride,
                                                               float* grad_att,
                                                               struct wholememory_env_func_t* p_env_fns,
                                                               void* stream);
/* N of the backward's grad_att node chunks (a compile-time constant of the library) */
int64_t wholememory_ext_csc_gat_node_chunk(void);

/* ---- (2d) edge-weighted neighbour aggregation of a sampled CSC block (`agg_concat_weighted`) ------------------- */
/* The block as for (2b): row_ptr int32 [n_dst + 1], col_ind int32 [n_edges] in [0, n_src), x fp32 [n_src, x_stride] whose
 * first n_dst rows are the targets; and w fp32 [n_edges], one weight per edge POSITION. fp32 rows only. Strides in elements,
 * all arrays DEVICE memory, all work queued on `stream`. Every `*` and `+` below is one fp32 operation, rounded on its own:
 * a product and the add that follows it are two roundings, never a fused multiply-add. inv(d) = fl(1.0f / deg(d)).
 *
 * forward: out [n_dst, out_stride] fp32, out_stride >= 2 * dim.
 *   S(d) = sum over e = row_ptr[d] .. row_ptr[d+1] - 1, left to right from the first term, of fl(w[e] * x[col_ind[e], c]).
 *   SUM: A = S. MEAN: A = fl(S * inv(d)): the mean over the DEGREE, as (2b), not over the sum of the weights. No edge: +0.0.
 *   out[d, 0:dim] = A(d); out[d, dim:2dim] = x[d], copied bit for bit.
 * backward into x: grad_out [n_dst, grad_out_stride] (2 * dim columns used) -> grad_x [n_src, grad_x_stride], every row
 *   written. t(e) = grad_out[dst(e), 0:dim] (MEAN: fl(t * inv(dst(e))) first), u(e) = fl(w[e] * t(e)). P(s) sums u(e) over
 *   the edges with col_ind[e] = s in ascending edge position, chunked exactly as (2b) with the same
 *   C = wholememory_ext_csc_aggregate_chunk_edges(). grad_x[s] = P(s) + grad_out[s, dim:2dim], the self term last and only
 *   for s < n_dst; the copy / +0.0 rules of (2b).
 * backward into w (only when grad_w is not null): grad_w [n_edges]. For edge e, q[c] = fl(t(e)[c] * x[col_ind[e], c]) for
 *   c < dim and q[c] = +0.0 for dim <= c < Fp, Fp the smallest power of two >= dim. grad_w[e] = the sum of q as a balanced
 *   binary tree of adjacent pairs, level by level: q1[i] = q[2i] + q[2i+1], q2[i] = q1[2i] + q1[2i+1], ... until one value
 *   is left (Fp = 1: q[0] itself). The tree does not depend on how the kernel is launched.
 * A NaN stays a NaN (payload not specified). No atomics; results are bitwise reproducible. The edge index of grad_x is
 * built with the library's id sort, scratch from p_env_fns.
 * grad_x or grad_w may be null (that gradient is then not computed, and nothing is queued for it); both null is
 * INVALID_INPUT. The backward reads x only for grad_w. n_edges = 0 and n_dst = 0 are valid. INVALID_INPUT, before any
 * device work and under every backend, for what (2b) rejects and for a null w with n_edges > 0; then NOT_SUPPORTED (nothing
 * queued) when the device backend has no such kernels. */
enum wholememory_error_code_t wholememory_ext_csc_aggregate_weighted_forward(const int32_t* row_ptr,
                                                                             const int32_t* col_ind,
                                                                             const float* w,
                                                                             int64_t n_edges,
                                                                             int64_t n_dst,
                                                                             int64_t n_src,
                                                                             const float* x,
                                                                             int64_t x_stride,
                                                                             int64_t dim,
                                                                             int aggr,
                                                                             float* out,
                                                                             int64_t out_stride,
                                                                             struct wholememory_env_func_t* p_env_fns,
                                                                             void* stream);
enum wholememory_error_code_t wholememory_ext_csc_aggregate_weighted_backward(const int32_t* row_ptr,
                                                                              const int32_t* col_ind,
                                                                              int64_t n_edges,
                                                                              int64_t n_dst,
                                                                              int64_t n_src,
                                                                              const float* x,
                                                                              int64_t x_stride,
                                                                              const float* w,
                                                                              const float* grad_out,
                                                                              int64_t grad_out_stride,
                                                                              int64_t dim,
                                                                              int aggr,
                                                                              float* grad_x,
                                                                              int64_t grad_x_stride,
                                                                              float* grad_w,
                                                                              struct wholememory_env_func_t* p_env_fns,
                                                                              void* stream);

/* ---- (2e) agg_concat straight from a WholeMemory table (`gather_agg_concat`) ---------------------------------------- */
/* (2b) whose rows are read from a table by global id instead of from a dense x: layer 0 of a GNN without the gathered
 * [n_src, dim] intermediate. `table` is a 2-D WholeMemory tensor [N, dim] of FLOAT, HALF or BF16 with contiguous rows;
 * node_ids [n_src] (WHOLEMEMORY_DT_INT or WHOLEMEMORY_DT_INT64, device memory) holds the global row of every node of the
 * block, the targets first. Define x[i] = fp32(table[node_ids[i]]) for i < n_src; widening is exact. Then, with row_ptr
 * int32 [n_dst + 1] and col_ind int32 [n_edges] in [0, n_src) as for (2b):
 *   out[d, 0:dim]    = A(d) of (2b) over x: S(d) = fp32 sum of x[col_ind[e]] for e = row_ptr[d] .. row_ptr[d+1] - 1, added
 *                      left to right from the first term; SUM: A = S; MEAN: A = S * fl(1.0f / deg(d)); no edge: +0.0.
 *   out[d, dim:2dim] = x[d].
 * out [n_dst, out_stride] is fp32, out_stride >= 2 * dim. Hence the result equals wholememory_ext_csc_aggregate_forward over
 * the rows wholememory_gather would write for node_ids as fp32, bit for bit.
 * Every id must lie in [0, N) (graph_append_unique's output does): the op does not check, and as in wholememory_gather an id
 * out of range is undefined (there is no "skip me" id here). A subtensor view is honoured: storage offset and row stride come
 * from the tensor description, in elements.
 * CONTINUOUS and CHUNKED tables (device- or host-located) and pointer-backed tensors are read through their global
 * reference, by the calling rank alone; DISTRIBUTED and HIERARCHY tables are NOT_SUPPORTED (nothing queued): gather, then
 * (2b). There is no backward entry point: the gradient with respect to x is wholememory_ext_csc_aggregate_backward.
 * INVALID_INPUT, before any device work and under every backend, for what (2b) rejects and for a null table, a table that is not 2-D or whose dtype
 * is not FLOAT / HALF / BF16, a node_id_dtype other than INT / INT64, null node_ids with n_src > 0, out_stride < 2 * dim.
 * Then NOT_SUPPORTED (nothing queued) when the device backend has no such kernel, then for a DISTRIBUTED or HIERARCHY table. */
enum wholememory_error_code_t wholememory_ext_csc_gather_aggregate_forward(wholememory_tensor_t table,
                                                                           const void* node_ids,
                                                                           int node_id_dtype,
                                                                           const int32_t* row_ptr,
                                                                           const int32_t* col_ind,
                                                                           int64_t n_edges,
                                                                           int64_t n_dst,
                                                                           int64_t n_src,
                                                                           int aggr,
                                                                           float* out,
                                                                           int64_t out_stride,
                                                                           struct wholememory_env_func_t* p_env_fns,
                                                                           void* stream);
/* wholememory_ext_csc_gather_aggregate_forward calls that reached the device backend (this process). A counter for tests:
 * it tells the fused route from the gather + (2b) composition. */
int64_t wholememory_ext_gather_aggregate_calls(void);

/* ---- (2f) (2c) with edge features in the attention logit (GAT `mha_gat_n2n(..., edge_feat=...)`) ------------------- */
/* The block, h, H, F and every rule of (2c): row_ptr int32 [n_dst + 1], col_ind int32 [n_edges] in [0, n_src), h fp32
 * [n_src, h_stride] with H * F columns used, head k owning the columns [k*F, (k+1)*F). Every `*` and `+` below is one fp32
 * operation, rounded on its own (no fused multiply-add). A sum "left to right" starts from its first term; a sum with no
 * term is +0.0. New inputs:
 *   att fp32 [3 * H * F], viewed as (3, H, F): half 0 is the source side, half 1 the target side, half 2 the edge side.
 *   edge_feat fp32 [n_edges, ef_stride] with H * F columns used, ef_stride >= H*F (the layer's lin_edge(edge_attr)); row e
 *   belongs to edge POSITION e of col_ind.
 *
 * forward: writes scores, alpha and out as (2c), and edge_scores [n_edges, H], which the backward reads back too.
 *   s_src and s_dst as (2c). s_edge[e,k] = sum over f of att[2,k,f] * edge_feat[e,k,f], left to right; edge_scores = s_edge.
 *   z = (s_src[col_ind[e],k] + s_dst[d,k]) + s_edge[e,k], in that association.
 *   l, m, w, den, alpha, o and out (concat or the mean over heads) are exactly as (2c) from this z. The edge features enter
 *   the logit only: o sums alpha[e,k] * h[col_ind[e],k,:], as cugraph-ops does.
 * backward: grad_out as (2c) -> grad_h [n_src, grad_h_stride >= H*F], grad_att [3*H*F] and grad_edge_feat
 * [n_edges, grad_ef_stride >= H*F] (every used column written).
 *   da, c, dl, dz (z recomputed from scores and edge_scores, associated as above) and ds_dst as (2c); P(j) and ds_src[j]
 *   with the same chunking and the same C; grad_h as (2c); grad_att[0] and grad_att[1] as (2c), in node chunks of N.
 *   grad_edge_feat[e,k,f] = dz[e,k] * att[2,k,f].
 *   grad_att[2,k,f] = sum over e of dz[e,k] * edge_feat[e,k,f] in ascending edge position, cut into chunks of
 *   N = wholememory_ext_csc_gat_node_chunk() edges from edge 0: each chunk summed left to right, the chunk sums added in
 *   chunk order.
 *   No atomics; results are bitwise reproducible.
 * With edge_feat all +0.0 (and no z of (2c) equal to +-0.0), scores, alpha, out, grad_h, grad_att[0] and grad_att[1] are
 * those of (2c) over att[0:2], bit for bit.
 * n_edges = 0 and n_dst = 0 are valid. INVALID_INPUT, before any device work, for everything (2c) rejects, for a null
 * edge_feat, edge_scores or grad_edge_feat with n_edges > 0 and n_dst > 0, and for an ef_stride or grad_ef_stride smaller
 * than H*F, all before any device work and under every backend; then NOT_SUPPORTED (nothing queued) when the device backend
 * has no such kernels. */
enum wholememory_error_code_t wholememory_ext_csc_gat_edge_forward(const int32_t* row_ptr,
                                                                   const int32_t* col_ind,
                                                                   int64_t n_edges,
                                                                   int64_t n_dst,
                                                                   int64_t n_src,
                                                                   const float* h,
                                                                   int64_t h_stride,
                                                                   const float* att,
                                                                   const float* edge_feat,
                                                                   int64_t ef_stride,
                                                                   int64_t heads,
                                                                   int64_t dim,
                                                                   float negative_slope,
                                                                   int concat,
                                                                   float* out,
                                                                   int64_t out_stride,
                                                                   float* alpha,
                                                                   float* scores,
                                                                   float* edge_scores,
                                                                   struct wholememory_env_func_t* p_env_fns,
                                                                   void* stream);
enum wholememory_error_code_t wholememory_ext_csc_gat_edge_backward(const int32_t* row_ptr,
                                                                    const int32_t* col_ind,
                                                                    int64_t n_edges,
                                                                    int64_t n_dst,
                                                                    int64_t n_src,
                                                                    const float* h,
                                                                    int64_t h_stride,
                                                                    const float* att,
                                                                    const float* edge_feat,
                                                                    int64_t ef_stride,
                                                                    int64_t heads,
                                                                    int64_t dim,
                                                                    float negative_slope,
                                                                    int concat,
                                                                    const float* alpha,
                                                                    const float* scores,
                                                                    const float* edge_scores,
                                                                    const float* grad_out,
                                                                    int64_t grad_out_stride,
                                                                    float* grad_h,
                                                                    int64_t grad_h_stride,
                                                                    float* grad_att,
                                                                    float* grad_edge_feat,
                                                                    int64_t grad_ef_stride,
                                                                    struct wholememory_env_func_t* p_env_fns,
                                                                    void* stream);

/* ---- (2g) GATv2 multi-head graph attention of a sampled CSC block (`mha_gat_v2_n2n`) ---------------------------------- */
/* The block as for (2b): row_ptr int32 [n_dst + 1], col_ind int32 [n_edges] in [0, n_src). h_src fp32 [n_src, h_src_stride]
 * with H * F columns used (H = heads, F = dim; the layer's lin_src(x)); h_dst fp32 [n_dst, h_dst_stride] with H * F columns
 * used: row d belongs to target d (the layer's lin_dst(x[:n_dst])). Head k owns the columns [k*F, (k+1)*F) of a row. att
 * fp32 [H * F], viewed as (H, F). Strides in elements, all arrays DEVICE memory, all work queued on `stream`.
 * The contract of (2c): every `*` and `+` below is one fp32 operation, rounded on its own (no fused multiply-add), no
 * atomics, one fixed order for every sum, results bitwise reproducible. A sum "left to right" starts from its first term; a
 * sum with no term is +0.0. "Tree sum over f" of terms q[f] is the balanced binary tree of adjacent pairs of (2d): with Fp
 * the smallest power of two >= F and q[f] = +0.0 for F <= f < Fp, q1[i] = q[2i] + q[2i+1], q2[i] = q1[2i] + q1[2i+1], ...
 * until one value is left (Fp = 1: q[0] itself). The tree does not depend on how the kernel is launched.
 *
 * forward: writes alpha [n_edges, H] and out. For edge e of target d (e = row_ptr[d] .. row_ptr[d+1] - 1), head k,
 * j = col_ind[e]:
 *   u[f] = h_src[j,k,f] + h_dst[d,k,f]; v[f] = u[f] > 0 ? u[f] : negative_slope * u[f].
 *   l[e,k] = tree sum over f of att[k,f] * v[f].
 *   m = max of l over the edges of d; w = expf(l - m) (the device's expf); den = sum of w over the edges of d, left to
 *   right; alpha[e,k] = w / den: exactly as (2c).
 *   o[d,k,:] = sum of alpha[e,k] * h_src[j,k,:] over the edges of d, left to right; +0.0 for a target without edges.
 *   concat != 0: out [n_dst, out_stride >= H*F] = o. concat == 0: out [n_dst, out_stride >= F] =
 *   ((o[d,0,:] + o[d,1,:]) + ...) * fl(1.0f / H).
 * backward: grad_out G [n_dst, grad_out_stride] (H*F columns with concat, else F) -> grad_h_src [n_src, grad_h_src_stride
 * >= H*F] (every row written), grad_h_dst [n_dst, grad_h_dst_stride >= H*F] (every row written) and grad_att [H*F]. Each of
 * the three may be null and is then not computed (nothing is queued for it); all three null is INVALID_INPUT.
 *   G_k[d,f] = G[d, k*F + f] with concat, else G[d,f] * fl(1.0f / H).
 *   da[e,k] = tree sum over f of G_k[d,f] * h_src[j,k,f]. c[d,k] = sum of alpha[e,k] * da[e,k] over the edges of d, left to
 *   right. dl[e,k] = alpha[e,k] * (da[e,k] - c[d,k]).
 *   g[f] = u[f] > 0 ? att[k,f] : att[k,f] * negative_slope (u recomputed); du[e,k,f] = dl[e,k] * g[f].
 *   grad_h_dst[d,k,f] = sum of du[e,k,f] over the edges of d, left to right; +0.0 without edges.
 *   grad_h_src[j,k,:] = sum over the edges with col_ind[e] = j, in ascending edge position, of
 *   (alpha[e,k] * G_k[d(e),:]) + du[e,k,:]: left to right when j has at most C edges, otherwise cut into consecutive chunks
 *   of C edges, each chunk summed left to right and the chunk sums added in chunk order, exactly as (2b), with
 *   C = wholememory_ext_csc_aggregate_chunk_edges(). A source without edges gets +0.0.
 *   grad_att[k,f]: first, per target, A(d)[k,f] = sum over its edges, left to right, of dl[e,k] * v[f] (v of that edge;
 *   +0.0 without edges). Then the A(d) are summed over d in node chunks of N = wholememory_ext_csc_gat_node_chunk() rows
 *   from row 0: each chunk left to right, the chunk sums added in chunk order.
 *   The edge index of grad_h_src is built with the library's id sort, scratch from p_env_fns.
 * n_edges = 0 and n_dst = 0 are valid. INVALID_INPUT, before any device work, for whatever (2c) rejects (null pointers,
 * negative sizes, heads < 1, dim < 1, n_dst > n_src, strides smaller than the row) and for a null h_dst with n_dst > 0;
 * NOT_SUPPORTED (nothing queued) when the device backend has no such kernels. */
enum wholememory_error_code_t wholememory_ext_csc_gatv2_forward(const int32_t* row_ptr,
                                                                const int32_t* col_ind,
                                                                int64_t n_edges,
                                                                int64_t n_dst,
                                                                int64_t n_src,
                                                                const float* h_src,
                                                                int64_t h_src_stride,
                                                                const float* h_dst,
                                                                int64_t h_dst_stride,
                                                                const float* att,
                                                                int64_t heads,
                                                                int64_t dim,
                                                                float negative_slope,
                                                                int concat,
                                                                float* out,
                                                                int64_t out_stride,
                                                                float* alpha,
                                                                struct wholememory_env_func_t* p_env_fns,
                                                                void* stream);
enum wholememory_error_code_t wholememory_ext_csc_gatv2_backward(const int32_t* row_ptr,
                                                                 const int32_t* col_ind,
                                                                 int64_t n_edges,
                                                                 int64_t n_dst,
                                                                 int64_t n_src,
                                                                 const float* h_src,
                                                                 int64_t h_src_stride,
                                                                 const float* h_dst,
                                                                 int64_t h_dst_stride,
                                                                 const float* att,
                                                                 int64_t heads,
                                                                 int64_t dim,
                                                                 float negative_slope,
                                                                 int concat,
                                                                 const float* alpha,
                                                                 const float* grad_out,
                                                                 int64_t grad_out_stride,
                                                                 float* grad_h_src,
                                                                 int64_t grad_h_src_stride,
                                                                 float* grad_h_dst,
                                                                 int64_t grad_h_dst_stride,
                                                                 float* grad_att,
                                                                 struct wholememory_env_func_t* p_env_fns,
                                                                 void* stream);

/* ---- (2h) relation-typed neighbour aggregation of a sampled CSC block (`agg_concat_rel`, RGCN) ----------------------- */
/* The block as for (2b): row_ptr int32 [n_dst + 1], col_ind int32 [n_edges] in [0, n_src), x fp32 [n_src, x_stride] whose
 * first n_dst rows are the targets; and edge_type int32 [n_edges], one relation per edge POSITION, R = num_relations >= 1.
 * fp32 rows only. Strides in elements, all arrays DEVICE memory, all work queued on `stream`. Every `*` and `+` below is one
 * fp32 operation, rounded on its own: a product and the add that follows it are two roundings, never a fused multiply-add.
 * E_r(d) = the edges e in [row_ptr[d], row_ptr[d+1]) with edge_type[e] = r, in ascending e; n_r(d) their number.
 *
 * forward: out [n_dst, out_stride] fp32, out_stride >= (R + 1) * dim: slot r = columns [r * dim, (r + 1) * dim).
 *   S_r(d) = sum of x[col_ind[e]] over E_r(d), left to right from the first term.
 *   SUM: out[d, slot r] = S_r(d). MEAN: out[d, slot r] = fl(S_r(d) * fl(1.0f / n_r(d))), the mean over the edges of THAT
 *   relation (one multiply). E_r(d) empty: the slot is +0.0. out[d, slot R] = x[d], copied bit for bit.
 *   MEAN also writes edge_scale [n_edges]: edge_scale[e] = fl(1.0f / n_r(d)) for d = dst(e), r = edge_type[e]. SUM neither
 *   writes nor reads edge_scale (it may be null).
 * backward: grad_out [n_dst, grad_out_stride] ((R + 1) * dim columns used) and, for MEAN, the edge_scale the forward wrote
 *   -> grad_x [n_src, grad_x_stride], every row written. u(e) = grad_out[dst(e), slot edge_type[e]] for SUM,
 *   fl(edge_scale[e] * grad_out[dst(e), slot edge_type[e]]) for MEAN. P(s) sums u(e) over the edges with col_ind[e] = s in
 *   ascending edge position, chunked exactly as (2b) with the same C = wholememory_ext_csc_aggregate_chunk_edges(): chunks
 *   of C consecutive positions of the source's run, each chunk summed left to right from its first term, the chunk sums added
 *   in chunk order. grad_x[s] = P(s) + grad_out[s, slot R], the self term last and only for s < n_dst; with one part missing
 *   the other is copied, with neither the row is +0.0.
 * An edge_type[e] outside [0, R) contributes no term anywhere: it is counted in no n_r, its edge_scale is +0.0, and in the
 *   backward it still occupies its position when the chunks are cut but adds nothing (a chunk, or a whole P(s), all of whose
 *   edges are such counts as missing). The value is compared, never used to form an address; nothing validates the types on
 *   the host.
 * With R = 1 and every type 0, out, and grad_x from the same grad_out, are those of (2b), bit for bit.
 * No atomics; results are bitwise reproducible. The edge index of the backward is built with the library's id sort, scratch
 * from p_env_fns (the forward needs none). n_edges = 0 and n_dst = 0 are valid. INVALID_INPUT, before any device work and
 * under every backend, for what (2b) rejects (with rows of (R + 1) * dim columns), for num_relations < 1 or >= 2^31 - 1, a
 * null edge_type with n_edges > 0 and, for MEAN, a null edge_scale with n_edges > 0; then NOT_SUPPORTED (nothing queued) when
 * the device backend has no such kernels. */
enum wholememory_error_code_t wholememory_ext_csc_rel_aggregate_forward(const int32_t* row_ptr,
                                                                        const int32_t* col_ind,
                                                                        const int32_t* edge_type,
                                                                        int64_t n_edges,
                                                                        int64_t n_dst,
                                                                        int64_t n_src,
                                                                        int64_t num_relations,
                                                                        const float* x,
                                                                        int64_t x_stride,
                                                                        int64_t dim,
                                                                        int aggr,
                                                                        float* out,
                                                                        int64_t out_stride,
                                                                        float* edge_scale,
                                                                        struct wholememory_env_func_t* p_env_fns,
                                                                        void* stream);
enum wholememory_error_code_t wholememory_ext_csc_rel_aggregate_backward(const int32_t* row_ptr,
                                                                         const int32_t* col_ind,
                                                                         const int32_t* edge_type,
                                                                         int64_t n_edges,
                                                                         int64_t n_dst,
                                                                         int64_t n_src,
                                                                         int64_t num_relations,
                                                                         const float* edge_scale,
                                                                         const float* grad_out,
                                                                         int64_t grad_out_stride,
                                                                         int64_t dim,
                                                                         int aggr,
                                                                         float* grad_x,
                                                                         int64_t grad_x_stride,
                                                                         struct wholememory_env_func_t* p_env_fns,
                                                                         void* stream);

/* ---- (2i) 8-bit row-quantized tables: fused gather + dequantize, quantize + scatter ---------------------------------- */
/* A quantized table of logical shape [N, dim] is an ordinary 2-D INT8 WholeMemory tensor [N, >= row_bytes] whose bytes are
 * read as unsigned. With Q = round_up(dim, 4) and row_bytes = Q + 8, a row is
 *   bytes [0, dim)      the codes c[j] (uint8)
 *   bytes [dim, Q)      zero
 *   bytes [Q, Q + 4)    scale, fp32, little endian
 *   bytes [Q + 4, Q+8)  bias, fp32, little endian
 * The row stride in bytes is >= row_bytes and a multiple of 4, and the view's storage offset is a multiple of 4 bytes:
 * row-range sub-tensors are fine, a column-offset view that breaks the rule is INVALID_INPUT. Being a plain INT8 tensor,
 * the storage works with file I/O, every memory type and every location unchanged.
 *
 * quantize(x[0..dim)), x fp32; every operation below is one fp32 operation rounded on its own (no fused multiply-add):
 *   lo = min(x), hi = max(x), r = hi - lo
 *   r == 0: scale = 1.0f, inv = 1.0f (every code 0); else scale = r / 255.0f, inv = 255.0f / r
 *   c[j] = (uint8) clamp(rintf((x[j] - lo) * inv), 0, 255)          rint: round half to even
 *   bias = lo; a zero minimum is stored as +0.0 whatever the signs of the row's zeros (bias = lo + 0.0f)
 * dequantize: y[j] = (float)c[j] * scale + bias, a multiply then an add (two roundings), then rounded once more, to nearest
 * even, when the output is HALF or BF16. min and max do not depend on the order they are taken in: results are bitwise
 * reproducible. The inputs must be finite with hi - lo finite; anything else is outside the contract (the bytes written are
 * unspecified, no address depends on them).
 *
 * wholememory_ext_gather_dequantize: for indices[i] >= 0, output[i, 0:dim) = dequantize(row indices[i] of q_table); a
 * negative id leaves the output row untouched, as wholememory_gather does. indices NULL: rows 0 .. n-1 with n = the rows of
 * output. output is FLOAT, HALF or BF16, 2-D with dim columns and its own row stride and storage offset.
 * wholememory_ext_quantize_scatter: for indices[i] >= 0, row indices[i] of q_table = quantize(input[i, :]) — codes, the
 * zero bytes and the trailer; bytes of the row past row_bytes are left alone. input is FLOAT, 2-D with dim columns.
 * Duplicate ids have no defined winner, as in wholememory_scatter. indices NULL: rows 0 .. n-1 with n = the rows of input.
 * Ids at or past the rows of q_table are the caller's contract, as for gather and scatter.
 *
 * Routes. CONTINUOUS and CHUNKED tables (device or host located) and a handle-less tensor
 * (wholememory_make_tensor_from_pointer: a local buffer) are read / written by one kernel that addresses the rows through
 * the table's global reference. DISTRIBUTED and HIERARCHY tables, and mapped tables served through the exchange
 * (WM_MAPPED_VIA_EXCHANGE=1), take two steps — collective like wholememory_gather / wholememory_scatter on such tables, and
 * needing indices: the raw rows move with wholememory_gather into a [n, row_bytes] temporary that is then dequantized in
 * place order (the ids only marking the rows to skip), or are quantized into such a temporary that wholememory_scatter then
 * moves; the links carry quantized bytes. A gather of a batch large enough for the sorted-ids gather of HOST-located tables
 * (WM_HOST_SORTED_MIN ids, rows of at most 512 bytes) from such a table takes the same two steps, for the sake of that
 * gather's row order. Scratch comes from p_env_fns only. gather_sms / scatter_sms cap the grid as for
 * gather and scatter (-1: default).
 *
 * Before any device work, and under every backend: INVALID_INPUT for a null q_table / output / input, dim < 1, a q_table
 * that is not 2-D INT8 with unit inner stride, sizes[1] < row_bytes, a row stride below row_bytes or no multiple of 4, a
 * storage offset that is no multiple of 4, an output / input that is not 2-D with dim columns and unit inner stride or whose
 * dtype is a floating type other than the ones named above, indices that are not 1-D INT / INT64 or outnumber the rows of
 * output / input, null indices with more rows than q_table has (or on an exchange-served table), and a null data pointer
 * where rows are to be moved; LOGIC_ERROR for an output / input of an integer dtype (the float <-> integer mix
 * wholememory_gather refuses the same way). Then NOT_SUPPORTED (nothing queued) when the device backend has no such
 * kernels, then success without a launch for n = 0 on a mapped table. */
int64_t wholememory_ext_quantized_row_bytes(int64_t dim); /* Q + 8; -1 for dim < 1 */
enum wholememory_error_code_t wholememory_ext_gather_dequantize(wholememory_tensor_t q_table,
                                                                int64_t dim,
                                                                wholememory_tensor_t indices /* may be NULL */,
                                                                wholememory_tensor_t output,
                                                                struct wholememory_env_func_t* p_env_fns,
                                                                void* stream,
                                                                int gather_sms);
enum wholememory_error_code_t wholememory_ext_quantize_scatter(wholememory_tensor_t input,
                                                               wholememory_tensor_t indices /* may be NULL */,
                                                               wholememory_tensor_t q_table,
                                                               int64_t dim,
                                                               struct wholememory_env_func_t* p_env_fns,
                                                               void* stream,
                                                               int scatter_sms);
/* wholememory_ext_gather_dequantize calls served by the fused kernel that reads the table itself (this process): a counter
 * for tests, it tells that route from the two steps. */
int64_t wholememory_ext_gather_dequantize_calls(void);

/* ---- (2j) agg_concat straight from a quantized table (`gather_agg_concat` over a quantized source) ------------------- */
/* (2e) over a table of (2i): layer 0 of a GNN over 8-bit row-quantized features without the dequantized [n_src, dim]
 * intermediate. `table` is the 2-D INT8 tensor [N, >= row_bytes] of (2i) — Q = round_up(dim, 4) code bytes, fp32 scale, fp32
 * bias per row; row stride >= row_bytes = Q + 8 and a multiple of 4 bytes, storage offset a multiple of 4 bytes — and `dim`
 * its logical width. node_ids [n_src] (WHOLEMEMORY_DT_INT or WHOLEMEMORY_DT_INT64, device memory) holds the global row of
 * every node of the block, the targets first. Define, for i < n_src and j < dim,
 *   x[i][j] = (float)c[j] * scale + bias    of table row node_ids[i]: the dequantize of (2i), a multiply then an add, each
 *                                           one fp32 operation rounded on its own (no fused multiply-add).
 * Then, with row_ptr int32 [n_dst + 1] and col_ind int32 [n_edges] in [0, n_src) as for (2b):
 *   out[d, 0:dim]    = A(d) of (2b) over x: S(d) = fp32 sum of x[col_ind[e]] for e = row_ptr[d] .. row_ptr[d+1] - 1, started
 *                      at -0.0f and added in ascending edge position; SUM: A = S; MEAN: A = S * fl(1.0f / (float)deg(d)); a
 *                      target without edges: +0.0.
 *   out[d, dim:2dim] = x[d].
 * out [n_dst, out_stride] is fp32, out_stride >= 2 * dim; columns at and past 2 * dim are left alone, and neither the zero
 * bytes behind column dim of a row nor its trailer reach out. Hence the result equals
 * wholememory_ext_csc_aggregate_forward over the FLOAT rows wholememory_ext_gather_dequantize writes for node_ids, bit for
 * bit. Every id must lie in [0, N): the op does not check, an id out of range is undefined (there is no "skip me" id here).
 * A row-range sub-tensor is honoured. There is no backward entry point: a quantized table holds frozen features.
 *
 * In this order: INVALID_INPUT, before any device work and under every backend, for a null table, a table that is not 2-D,
 * not INT8 or whose inner stride is not 1, dim < 1, rows of fewer than row_bytes bytes, a row stride below row_bytes or no
 * multiple of 4, a storage offset that is no multiple of 4, a node_id_dtype other than INT / INT64, what (2b) rejects (null
 * pointers, negative counts, n_dst > n_src, out_stride < 2 * dim, an unknown aggr) and node ids into a table without rows.
 * Then NOT_SUPPORTED when the device backend has no such kernel. Then NOT_SUPPORTED for a table whose handle is neither
 * CONTINUOUS nor CHUNKED (DISTRIBUTED, HIERARCHY) or that is served through the exchange (WM_MAPPED_VIA_EXCHANGE=1): gather
 * with (2i), then (2b). Nothing is queued in any refused case. CONTINUOUS and CHUNKED tables (device- or host-located) and
 * handle-less tensors are read through their global reference, by the calling rank alone. */
enum wholememory_error_code_t wholememory_ext_csc_gather_dequantize_aggregate_forward(wholememory_tensor_t table,
                                                                                      int64_t dim,
                                                                                      const void* node_ids,
                                                                                      int node_id_dtype,
                                                                                      const int32_t* row_ptr,
                                                                                      const int32_t* col_ind,
                                                                                      int64_t n_edges,
                                                                                      int64_t n_dst,
                                                                                      int64_t n_src,
                                                                                      int aggr,
                                                                                      float* out,
                                                                                      int64_t out_stride,
                                                                                      struct wholememory_env_func_t* p_env_fns,
                                                                                      void* stream);
/* wholememory_ext_csc_gather_dequantize_aggregate_forward calls that launched on the device backend (this process). A
 * counter for tests: it tells the fused route from the (2i) gather + (2b) composition. */
int64_t wholememory_ext_gather_dequantize_aggregate_calls(void);

/* ---- (2k) scaled dot-product multi-head attention of a sampled CSC block (`mha_simple_n2n`) -------------------------- */
/* The block as for (2b): row_ptr int32 [n_dst + 1], col_ind int32 [n_edges] in [0, n_src). key fp32 [n_src, key_stride],
 * value fp32 [n_src, value_stride] and query fp32 [n_dst, query_stride], row d of query belonging to target d (the layer's
 * lin_key(x), lin_value(x) and lin_query(x[:n_dst])); each row uses H * F columns (H = heads, F = dim) and head h owns the
 * columns [h*F, (h+1)*F). Strides in elements, all arrays DEVICE memory, all work queued on `stream`.
 * The contract of (2c) / (2g): every `*` and `+` below is one fp32 operation, rounded on its own (no fused multiply-add), no
 * atomics, one fixed order for every sum, results bitwise reproducible. A sum "left to right" starts from its first term; a
 * sum with no term is +0.0. "Tree sum over f" is the balanced binary tree of adjacent pairs of (2d) / (2g), padded to the
 * next power of two Fp >= F with +0.0; it does not depend on how the kernel is launched.
 * The scale is s = fl(1.0f / fl(sqrtf((float)F))), computed once on the host, both operations correctly rounded. It applies
 * only when norm_by_dim != 0; with norm_by_dim == 0 no multiplication takes place.
 *
 * forward: writes alpha [n_edges, H] and out. For edge e of target d (e = row_ptr[d] .. row_ptr[d+1] - 1), head h,
 * j = col_ind[e]:
 *   t[e,h] = tree sum over f of query[d,h,f] * key[j,h,f]. l[e,h] = t[e,h] * s (norm_by_dim), else l[e,h] = t[e,h].
 *   m = max of l over the edges of d; w = expf(l - m) (the device's expf); den = sum of w over the edges of d, left to
 *   right; alpha[e,h] = w / den: exactly as (2c).
 *   o[d,h,:] = sum of alpha[e,h] * value[j,h,:] over the edges of d, left to right; +0.0 for a target without edges.
 *   concat != 0: out [n_dst, out_stride >= H*F] = o. concat == 0: out [n_dst, out_stride >= F] =
 *   ((o[d,0,:] + o[d,1,:]) + ...) * fl(1.0f / H), as (2g).
 * backward: grad_out G [n_dst, grad_out_stride] (H*F columns with concat, else F) -> grad_query [n_dst, grad_query_stride],
 * grad_key [n_src, grad_key_stride] and grad_value [n_src, grad_value_stride], each with a stride >= H*F and every row of a
 * requested gradient written. Each of the three may be null and is then not computed (nothing is queued for it); all three
 * null is INVALID_INPUT.
 *   G_h[d,f] = G[d, h*F + f] with concat, else G[d,f] * fl(1.0f / H), as (2g).
 *   da[e,h] = tree sum over f of G_h[d,f] * value[j,h,f]. c[d,h] = sum of alpha[e,h] * da[e,h] over the edges of d, left to
 *   right. dl[e,h] = alpha[e,h] * (da[e,h] - c[d,h]). ds[e,h] = dl[e,h] * s (norm_by_dim), else ds[e,h] = dl[e,h].
 *   grad_query[d,h,f] = sum of ds[e,h] * key[j,h,f] over the edges of d, left to right; +0.0 without edges.
 *   grad_key[j,h,:] = sum over the edges with col_ind[e] = j, in ascending edge position, of ds[e,h] * query[d(e),h,:].
 *   grad_value[j,h,:] = the same edges in the same order, of alpha[e,h] * G_h[d(e),:].
 *   Both per-source sums: left to right when j has at most C edges, otherwise cut into consecutive chunks of C edges, each
 *   chunk summed left to right and the chunk sums added in chunk order, exactly as (2b), with
 *   C = wholememory_ext_csc_aggregate_chunk_edges(). A source without edges gets +0.0.
 *   The edge index of grad_key and grad_value is built with the library's id sort, scratch from p_env_fns, and only when
 *   one of the two is asked for.
 * n_edges = 0 and n_dst = 0 are valid. INVALID_INPUT, before any device work and under every backend, for whatever (2g)
 * rejects: null pointers (a null query with n_dst > 0 among them), negative sizes, heads < 1, dim < 1, n_dst > n_src and any
 * stride smaller than its row (for out and grad_out the row is F without concat). NOT_SUPPORTED (nothing queued) when the
 * device backend has no such kernels. */
enum wholememory_error_code_t wholememory_ext_csc_mha_simple_forward(const int32_t* row_ptr,
                                                                     const int32_t* col_ind,
                                                                     int64_t n_edges,
                                                                     int64_t n_dst,
                                                                     int64_t n_src,
                                                                     const float* key,
                                                                     int64_t key_stride,
                                                                     const float* query,
                                                                     int64_t query_stride,
                                                                     const float* value,
                                                                     int64_t value_stride,
                                                                     int64_t heads,
                                                                     int64_t dim,
                                                                     int norm_by_dim,
                                                                     int concat,
                                                                     float* out,
                                                                     int64_t out_stride,
                                                                     float* alpha,
                                                                     struct wholememory_env_func_t* p_env_fns,
                                                                     void* stream);
enum wholememory_error_code_t wholememory_ext_csc_mha_simple_backward(const int32_t* row_ptr,
                                                                      const int32_t* col_ind,
                                                                      int64_t n_edges,
                                                                      int64_t n_dst,
                                                                      int64_t n_src,
                                                                      const float* key,
                                                                      int64_t key_stride,
                                                                      const float* query,
                                                                      int64_t query_stride,
                                                                      const float* value,
                                                                      int64_t value_stride,
                                                                      int64_t heads,
                                                                      int64_t dim,
                                                                      int norm_by_dim,
                                                                      int concat,
                                                                      const float* alpha,
                                                                      const float* grad_out,
                                                                      int64_t grad_out_stride,
                                                                      float* grad_key,
                                                                      int64_t grad_key_stride,
                                                                      float* grad_query,
                                                                      int64_t grad_query_stride,
                                                                      float* grad_value,
                                                                      int64_t grad_value_stride,
                                                                      struct wholememory_env_func_t* p_env_fns,
                                                                      void* stream);

/* ---- (2l) multi-aggregator neighbour aggregation of a sampled CSC block (`agg_concat_pna`) --------------------------- */
/* The block as for (2b): row_ptr int32 [n_dst + 1], col_ind int32 [n_edges] in [0, n_src), x fp32 [n_src, x_stride] whose
 * first n_dst rows are the targets themselves. Strides in elements, all arrays DEVICE memory, all work queued on `stream`.
 * `aggregators` is a non-empty mask of the bits of wholememory_ext_pna_aggr_t, A of them set. A row of out, and of grad_out,
 * has one slot of dim columns per selected aggregator, in the order SUM, MEAN, MIN, MAX, STD, and then the slot of the
 * target's own row: (A + 1) * dim columns.
 * Every `*`, `+`, `-` and `/` below is one fp32 operation, rounded on its own (no fused multiply-add); the square root is
 * correctly rounded; no atomics, one fixed order for every sum, results bitwise reproducible.
 *
 * forward, for target d with the edges e0 = row_ptr[d] .. e1 - 1 = row_ptr[d+1] - 1, t_i = x[col_ind[e0 + i]], r = fl(1.0f /
 * deg(d)), per column:
 *   SUM   S = ((t_0 + t_1) + t_2) + ... , left to right from the first term: the S of (2b).
 *   MEAN  S * r: the MEAN of (2b).
 *   MIN   acc = t_0, arg = e0; then for i = 1, 2, ...: if t_i < acc then acc = t_i, arg = e0 + i. MAX the same with `>`.
 *         Only a strict comparison replaces: among equal values, duplicate edges and -0.0 / +0.0 (which compare equal) the
 *         lowest edge position wins and its bits are the result. A NaN compares false: a NaN in t_0 stays (acc = NaN,
 *         arg = e0), a NaN in a later term is passed over.
 *   STD   Q = ((t_0 * t_0 + t_1 * t_1) + t_2 * t_2) + ... , each square rounded, added left to right from the first one.
 *         m = S * r. v = Q * r - m * m. std = sqrtf((v > 0 ? v : 0) + eps) (so a NaN v counts as 0).
 *   A target without edges gets +0.0 in every aggregator slot, arg = -1, m = 0 and c = 0.
 *   The last slot is x[d].
 *   Saved for the backward, each [n_dst, dim] dense (row d at d * dim), each written only when its pointer is not null and
 *   its aggregator is selected: arg_min, arg_max int32 (global edge positions), std_mean = m, std_coef = c =
 *   (v > 0) ? r / std : 0.
 * backward: grad_out G [n_dst, grad_out_stride] -> grad_x [n_src, grad_x_stride], every row written. With G_sum, G_mean,
 * G_min, G_max, G_std and G_self the slots of a row of G, the term of edge e = (s -> d), per column f, is the sum of its
 * parts in this order, starting from the first part that is present:
 *   G_sum[d,f]; G_mean[d,f] * r(d); G_min[d,f] if arg_min[d,f] == e; G_max[d,f] if arg_max[d,f] == e;
 *   (G_std[d,f] * c[d,f]) * (x[s,f] - m[d,f]).
 *   A part whose aggregator is not selected, or whose arg is another edge, is absent: it is not added as a zero. An edge
 *   with no part adds nothing.
 *   P(s) = +0.0 + t(e_0) + t(e_1) + ... over the edges with col_ind[e] = s in ascending edge position, left to right, when s
 *   has at most C edges; otherwise the edges are cut into consecutive chunks of C, each chunk summed in that way from its own
 *   +0.0 and the chunk sums added in chunk order, with C = wholememory_ext_csc_aggregate_chunk_edges(). (Unlike (2b) the sums
 *   start from +0.0, since an edge may add nothing.) grad_x[s] = P(s) + G_self[s] (the self term added last, only for
 *   s < n_dst); with one side missing the other is copied, with neither the row is +0.0. No per-target pre-pass: the d-only
 *   factors are read per edge as they stand. The edge index is built with the library's id sort, scratch from p_env_fns.
 *   The backward reads x only when STD is selected, and arg_min / arg_max / std_mean / std_coef only for their aggregator.
 * n_edges = 0 and n_dst = 0 are valid. INVALID_INPUT, before any device work and under every backend, for what (2b) rejects
 * (null pointers, negative sizes, dim < 1, n_dst > n_src, a stride of out / grad_out below (A + 1) * dim or of x / grad_x
 * below dim), a mask that is 0 or has other bits, eps < 0 or NaN, and in the backward a selected aggregator whose saved
 * buffer is null (n_dst > 0), a selected STD with a null x (n_src > 0) and a null p_env_fns. NOT_SUPPORTED (nothing queued)
 * when the device backend has no such kernels. */
enum wholememory_ext_pna_aggr_t {
  WHOLEMEMORY_EXT_PNA_SUM  = 1,
  WHOLEMEMORY_EXT_PNA_MEAN = 2,
  WHOLEMEMORY_EXT_PNA_MIN  = 4,
  WHOLEMEMORY_EXT_PNA_MAX  = 8,
  WHOLEMEMORY_EXT_PNA_STD  = 16,
};
enum wholememory_error_code_t wholememory_ext_csc_pna_aggregate_forward(const int32_t* row_ptr,
                                                                        const int32_t* col_ind,
                                                                        int64_t n_edges,
                                                                        int64_t n_dst,
                                                                        int64_t n_src,
                                                                        const float* x,
                                                                        int64_t x_stride,
                                                                        int64_t dim,
                                                                        int aggregators,
                                                                        float eps, /* 1e-5f in the Python op */
                                                                        float* out,
                                                                        int64_t out_stride,
                                                                        int32_t* arg_min,
                                                                        int32_t* arg_max,
                                                                        float* std_mean,
                                                                        float* std_coef,
                                                                        struct wholememory_env_func_t* p_env_fns,
                                                                        void* stream);
enum wholememory_error_code_t wholememory_ext_csc_pna_aggregate_backward(const int32_t* row_ptr,
                                                                         const int32_t* col_ind,
                                                                         int64_t n_edges,
                                                                         int64_t n_dst,
                                                                         int64_t n_src,
                                                                         const float* x,
                                                                         int64_t x_stride,
                                                                         int64_t dim,
                                                                         int aggregators,
                                                                         const int32_t* arg_min,
                                                                         const int32_t* arg_max,
                                                                         const float* std_mean,
                                                                         const float* std_coef,
                                                                         const float* grad_out,
                                                                         int64_t grad_out_stride,
                                                                         float* grad_x,
                                                                         int64_t grad_x_stride,
                                                                         struct wholememory_env_func_t* p_env_fns,
                                                                         void* stream);

/* ---- (2m) random walks over a CSR graph held in WholeMemory ------------------------------------------------------------ */
/* n walks of walk_length = L >= 1 steps over the graph row_ptr (int64, [n_nodes + 1]; n_nodes is its size minus one),
 * col_ind (int32 or int64, [n_edges]) and, for the weighted form, one weight per edge position (float or double); start
 * nodes int32 or int64, [n]; a 64-bit seed. The graph tensors are CONTINUOUS or CHUNKED WholeMemory tensors in device or host
 * memory, or plain device arrays wrapped with wholememory_make_tensor_from_pointer; start nodes and outputs are device
 * arrays. One launch on `stream`; nothing is allocated, nothing is read back and the call does not synchronise.
 *
 * Outputs. walks [n, L + 1] in col_ind's dtype and, optionally, edge_ids [n, L] int64 (positions in col_ind), each a dense
 * block given as a 2-D tensor of that shape or a 1-D one of as many entries. Column 0 of walk w is its start node, or -1 when
 * the start is outside [0, n_nodes). A walk ends when a step is not taken; from that step on walks and edge_ids hold -1. A
 * step from v is not taken when
 *   - deg(v) = row_ptr[v + 1] - row_ptr[v] is <= 0 or >= 2^31 (or the row's bounds do not lie in [0, n_edges]: a valid
 *     graph has no such row);
 *   - the weighted form finds no eligible neighbour;
 *   - the chosen col_ind entry is outside [0, n_nodes): an id read from col_ind indexes row_ptr in the next step, so a
 *     damaged graph ends a walk, it does not read out of bounds;
 *   - the walk has already ended.
 *
 * Random streams. mix(z), all modulo 2^64:  z += 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31.  stream(seed, a, b) is the PCG-XSH-RR 64/32 generator of the
 * samplers initialised as init(seed' = mix(mix(seed + a) + b), subsequence = a, offset = 0): state = 0, inc = (a << 1) | 1,
 * one step, state += seed', one step. mix(0) = 0xe220a8397b1dcdaf; stream(42, 3, 0) starts 2748719185, 1404529248,
 * 2891244060, 1914411027 and stream(42, 3, 5) starts 2746596618, 1305647937, 1544306493. (Streams told apart by the
 * increment alone, without mix, gave correlated picks two steps apart in one walk.)
 *
 * Uniform step. Walk w has one generator, stream(seed, w, 0); step t (0-based) uses its t-th 32-bit output r, whether or
 * not earlier steps were taken. The chosen neighbour is k = (uint64(r) * uint64(deg)) >> 32, the edge row_ptr[v] + k.
 *
 * Weighted step. A weight is converted to fp32 first; neighbour j is eligible when that value is > 0 (zero, negative and NaN
 * weights are never chosen; +inf is not specified). The key of neighbour j at step t of walk w is the A-Res key of the
 * weighted sampler, log2(u) * (1.0f / weight) with log2(u) from three draws of stream(seed, w * L + t, j + 1) (a 24-bit
 * mantissa from the first, the exponent from the leading zeros of the 64 bits of the next two, low word first). The chosen
 * neighbour is the eligible j with the largest key in an fp32 `>` comparison; ties go to the lowest j.
 *
 * The result depends on (seed, w, t, j) only, not on the launch geometry and not on n: the first 100 walks of a batch of 512
 * equal a batch of those 100.
 *
 * INVALID_INPUT for a null row_ptr, col_ind, start nodes or walks tensor, a tensor among the first three that is not 1-D,
 * walk_length < 1, n * (walk_length + 1) >= 2^31, an output of the wrong size, a weight tensor that is not one entry per edge,
 * and HIERARCHY tensors. LOGIC_ERROR for a row_ptr that is not int64, col_ind or start nodes that are not int32 / int64,
 * walks not in col_ind's dtype, edge ids not int64, weights not float / double. NOT_IMPLEMENTED for a DISTRIBUTED tensor.
 * NOT_SUPPORTED, nothing queued, when the device backend has no walk kernels. n = 0 succeeds and queues nothing. Every
 * answer other than SUCCESS comes before any device work. */
enum wholememory_error_code_t wholememory_ext_csr_random_walk(wholememory_tensor_t wm_csr_row_ptr_tensor,
                                                              wholememory_tensor_t wm_csr_col_ptr_tensor,
                                                              wholememory_tensor_t wm_csr_weight_ptr_tensor, /* NULL: uniform */
                                                              wholememory_tensor_t start_nodes_tensor,
                                                              int walk_length,
                                                              unsigned long long random_seed,
                                                              wholememory_tensor_t output_walks_tensor,
                                                              wholememory_tensor_t output_edge_ids_tensor, /* may be NULL */
                                                              void* stream);

/* ---- (2n) node2vec (p, q) second-order walks over a CSR graph held in WholeMemory ----------------------------------------- */
/* n walks of walk_length = L >= 1 steps whose step depends on the previous node. Tensors and dtypes, memory types and
 * locations, the outputs walks [n, L + 1] and edge_ids [n, L] with -1 behind a walk's end, when a step is not taken, and the
 * random streams are as (2m), word for word; wm_csr_weight_ptr_tensor may be NULL, and then every edge has weight 1.0f. One
 * launch on `stream`; nothing is allocated, nothing is read back and the call does not synchronise. Only the step rule is new.
 *
 * Step rule. inv_p = 1.0f / p and inv_q = 1.0f / q, one fp32 division each, done on the host. At step t of walk w the walker
 * stands on v; the previous node is u = walks[w, t - 1] for t >= 1, and there is none at t = 0. Neighbour j of v is
 * x = col_ind[row_ptr[v] + j]. Its bias a is
 *   - 1.0f at t = 0;
 *   - else inv_p when x == u;
 *   - else 1.0f when x occurs in col_ind[row_ptr[u] : row_ptr[u + 1]];
 *   - else inv_q.
 * Only ids are compared: x is never used as an index before it is chosen and range-checked, so a damaged col_ind entry gets
 * some class and causes no out-of-bounds read. The effective weight is ew = w32 * a, a single fp32 multiply with no
 * contraction, w32 the edge weight converted to fp32 (1.0f without a weight tensor). Neighbour j is eligible when ew > 0; its
 * key is the A-Res key of (2m) from stream(seed, w * L + t, j + 1) with ew as the weight, log2(u) * (1.0f / ew). The chosen
 * neighbour is the eligible j with the largest key in an fp32 `>` comparison; ties go to the lowest j.
 *
 * Two consequences. With p = q = 1, ew == w32 bit for bit, and the walks equal wholememory_ext_csr_random_walk with the same
 * weight tensor. Without a weight tensor, p = q = 1 gives the walks that wholememory_ext_csr_random_walk gives over a
 * weight tensor of ones.
 *
 * The result depends on (seed, w, t, j) and the graph only: not on n, not on the launch geometry, and not on which search
 * route answered the adjacency question.
 *
 * col_sorted. 0: the rows of col_ind may be in any order; membership in u's row is found by scanning it, which is right on
 * every graph and costs deg(u) compares per neighbour. Non-zero: the caller promises that every row of col_ind is ascending,
 * and membership is found by a binary search. On a graph whose rows are ascending both settings give identical outputs. If
 * the promise is broken the walks still only follow edges and nothing is read out of bounds, but the class of a neighbour
 * is not specified.
 *
 * Errors, all answered before any device work: everything (2m) lists, unchanged; INVALID_INPUT unless p, q, 1.0f / p and
 * 1.0f / q are all finite and > 0 (that refuses 0, negatives, NaN, inf, and a subnormal p or q whose reciprocal overflows);
 * NOT_IMPLEMENTED for a DISTRIBUTED tensor; NOT_SUPPORTED, nothing queued, when the device backend has no such kernel.
 * n = 0 succeeds and queues nothing. */
enum wholememory_error_code_t wholememory_ext_csr_node2vec_walk(wholememory_tensor_t wm_csr_row_ptr_tensor,
                                                                wholememory_tensor_t wm_csr_col_ptr_tensor,
                                                                wholememory_tensor_t wm_csr_weight_ptr_tensor, /* NULL: 1.0f */
                                                                wholememory_tensor_t start_nodes_tensor,
                                                                int walk_length,
                                                                float p,
                                                                float q,
                                                                int col_sorted,
                                                                unsigned long long random_seed,
                                                                wholememory_tensor_t output_walks_tensor,
                                                                wholememory_tensor_t output_edge_ids_tensor, /* may be NULL */
                                                                void* stream);

/* ---- (2o) negative sampling over a CSR graph held in WholeMemory ---------------------------------------------------------- */
/* For each of n source nodes, num_negatives = K nodes drawn at random that are not the source and not in its row — the
 * negatives of skip-gram training over the walks above, and of link prediction. Graph tensors are as (2m): row_ptr int64
 * [n_nodes + 1], col_ind int32 or int64 [n_edges], both CONTINUOUS or CHUNKED, in device or host memory, or plain device
 * arrays wrapped with wholememory_make_tensor_from_pointer. src_nodes is int32 or int64 [n], on the device.
 * output_negatives is [n, K] in col_ind's dtype, given as 2-D or as 1-D with n * K entries. One launch on `stream`; nothing
 * is allocated, nothing is read back and the call does not synchronise.
 *
 * Sample (i, k), with source u = src_nodes[i]. Its generator is stream(seed, i * K + k, 0) of (2m). Attempt a (0-based,
 * a < max_tries = T) uses r, the a-th 64-bit draw of that generator, made of two 32-bit outputs, low word first, as
 * pcg32::next_u64 does; attempt a takes that draw whether or not earlier attempts were rejected. The candidate c is
 *   - mode 0 (uniform): c = (r * n_nodes) >> 64, a 128-bit product;
 *   - mode 1 (by degree): pos = (r * n_edges) >> 64 and c = col_ind[pos], so that a node is drawn in proportion to how often
 *     it occurs in col_ind. With n_edges = 0 every attempt is rejected.
 * Attempt a is rejected when
 *   - c is outside [0, n_nodes) (a damaged col_ind entry), or
 *   - exclude & 2 is set and c == u, or
 *   - exclude & 1 is set and c occurs in col_ind[row_ptr[u] : row_ptr[u + 1]].
 * The first attempt that is not rejected is the output; if all T attempts are rejected the output is -1. All K outputs of a
 * source are -1 when u is outside [0, n_nodes). A source whose row bounds are not a valid row excludes no edge; a row is valid
 * when 0 <= s <= e <= n_edges and e - s < 2^31. Samples are drawn with replacement: the K negatives of one source may repeat.
 *
 * col_sorted. 0: the rows of col_ind may be in any order; membership in u's row is found by scanning it, which is right on
 * every graph. Non-zero: the caller promises that every row of col_ind is ascending, and membership is found by a binary
 * search. On a graph whose rows are ascending both settings give identical outputs. If the promise is broken nothing is read
 * outside the row, but the class of a candidate is not specified. Only ids are compared: a candidate is never used as an
 * index before it is range-checked.
 *
 * The result depends on (seed, i, k, a), K and the graph only: not on n, not on the launch geometry, and not on which search
 * route answered.
 *
 * Errors, all answered before any device work. INVALID_INPUT: a NULL row_ptr, col_ind, src_nodes or output; one of the first
 * three not 1-D; num_negatives < 1; max_tries outside [1, 64]; mode not 0 or 1; exclude outside [0, 3]; n * K >= 2^31; an
 * output of the wrong size; a HIERARCHY tensor. LOGIC_ERROR, the dtype cases of (2m): row_ptr not int64, col_ind or src_nodes
 * not int32 / int64, the output not in col_ind's dtype. NOT_IMPLEMENTED for a DISTRIBUTED tensor. NOT_SUPPORTED, nothing
 * queued, when the device backend has no such kernel. n = 0 succeeds and queues nothing. */
enum wholememory_error_code_t wholememory_ext_csr_negative_sample(wholememory_tensor_t wm_csr_row_ptr_tensor,
                                                                  wholememory_tensor_t wm_csr_col_ptr_tensor,
                                                                  wholememory_tensor_t src_nodes_tensor,
                                                                  int num_negatives,
                                                                  int mode,    /* 0: uniform, 1: by degree */
                                                                  int exclude, /* bit 0: neighbours, bit 1: the source */
                                                                  int max_tries,
                                                                  int col_sorted,
                                                                  unsigned long long random_seed,
                                                                  wholememory_tensor_t output_negatives_tensor,
                                                                  void* stream);

/* ---- (2p) edge dot product of a sampled CSC block (`edge_dot_n2n`) ---------------------------------------------------- */
/* The block: row_ptr int32 [n_dst + 1], col_ind int32 [n_edges] in [0, n_src). x_src fp32 [n_src, x_src_stride] and x_dst fp32
 * [n_dst, x_dst_stride], row d of x_dst belonging to target d; each row uses F = dim columns. Unlike (2b) .. (2l) the targets
 * are not among the source rows: n_dst may exceed n_src (the centre positions of a batch of walks against the distinct
 * context nodes). Strides in elements, all arrays DEVICE memory, all work queued on `stream`.
 * The contract of (2k): every `*` and `+` below is one fp32 operation, rounded on its own (no fused multiply-add), no atomics,
 * one fixed order for every sum, results bitwise reproducible. "Tree sum over f" is the balanced binary tree of adjacent pairs
 * of (2g) / (2k), padded to the next power of two Fp >= F with +0.0; it does not depend on how the kernel is launched. There
 * are no heads and no scale.
 *
 * forward: writes score [n_edges]. For edge e of target d (e = row_ptr[d] .. row_ptr[d+1] - 1), j = col_ind[e]:
 *   score[e] = tree sum over f of x_dst[d,f] * x_src[j,f].
 * backward: grad_score g [n_edges] -> grad_dst [n_dst, grad_dst_stride] and grad_src [n_src, grad_src_stride], each with a
 * stride >= F and every row of a requested gradient written. Either may be null and is then not computed (nothing is queued
 * for it); both null is INVALID_INPUT.
 *   grad_dst[d,:] = sum of g[e] * x_src[j,:] over the edges of d, left to right from the first term; +0.0 without edges.
 *   grad_src[j,:] = sum over the edges with col_ind[e] = j, in ascending edge position, of g[e] * x_dst[d(e),:]: left to right
 *   when j has at most C edges, otherwise cut into consecutive chunks of C edges, each chunk summed left to right and the
 *   chunk sums added in chunk order, exactly as (2b), with C = wholememory_ext_csc_aggregate_chunk_edges(). A source without
 *   edges gets +0.0.
 *   The edge index of grad_src is built with the library's id sort, scratch from p_env_fns, and only when grad_src is asked
 *   for and n_src > 0.
 * n_edges = 0 and n_dst = 0 are valid: what there is to write (the rows of the requested gradients, +0.0) is written. A
 * col_ind entry outside [0, n_src) is treated as by (2k): it is not looked for. INVALID_INPUT, before any device work and
 * under every backend: null pointers (row_ptr; col_ind, score and grad_score when there are edges; x_src with n_src > 0; x_dst
 * with n_dst > 0; p_env_fns), negative sizes, 2^31 or more edges, targets or source rows, dim outside [1, 2^31 / 4) and any
 * stride smaller than dim. NOT_SUPPORTED (nothing queued) when the device backend has no such kernels. */
enum wholememory_error_code_t wholememory_ext_csc_edge_dot_forward(const int32_t* row_ptr,
                                                                   const int32_t* col_ind,
                                                                   int64_t n_edges,
                                                                   int64_t n_dst,
                                                                   int64_t n_src,
                                                                   const float* x_src,
                                                                   int64_t x_src_stride,
                                                                   const float* x_dst,
                                                                   int64_t x_dst_stride,
                                                                   int64_t dim,
                                                                   float* score,
                                                                   struct wholememory_env_func_t* p_env_fns,
                                                                   void* stream);
enum wholememory_error_code_t wholememory_ext_csc_edge_dot_backward(const int32_t* row_ptr,
                                                                    const int32_t* col_ind,
                                                                    int64_t n_edges,
                                                                    int64_t n_dst,
                                                                    int64_t n_src,
                                                                    const float* x_src,
                                                                    int64_t x_src_stride,
                                                                    const float* x_dst,
                                                                    int64_t x_dst_stride,
                                                                    int64_t dim,
                                                                    const float* grad_score,
                                                                    float* grad_src,
                                                                    int64_t grad_src_stride,
                                                                    float* grad_dst,
                                                                    int64_t grad_dst_stride,
                                                                    struct wholememory_env_func_t* p_env_fns,
                                                                    void* stream);

/* ---- (2q) node-induced subgraph of a CSR graph held in WholeMemory -------------------------------------------------------- */
/* The block of subgraph-wise training: for a list of n nodes, every graph edge whose two ends are in the list, as local CSR
 * arrays that the block ops of (2b) .. (2p) take with n_dst = n_src = n. Graph tensors are as (2m): row_ptr int64
 * [n_nodes + 1], col_ind int32 or int64 [n_edges], both CONTINUOUS or CHUNKED, in device or host memory, or plain device
 * arrays wrapped with wholememory_make_tensor_from_pointer. nodes is int32 or int64 [n], on the device. The shape of the
 * samplers: output_offset_tensor is the caller's, int32 with at least n + 1 entries, on the device; col int32 [m] and, with a
 * context for them, edge_gid int64 [m] are allocated through p_env_fns once m is known.
 *
 * Definition. A node v is a member when 0 <= v < n_nodes and v occurs in nodes. Its local id is first(v), the lowest i with
 * nodes[i] == v. Duplicates in nodes are allowed: every position gets a row. Row i, with u = nodes[i]:
 *   - the row is empty when u is outside [0, n_nodes);
 *   - the row is empty when (s, e) = (row_ptr[u], row_ptr[u + 1]) does not satisfy 0 <= s <= e <= n_edges and e - s < 2^31
 *     (a valid graph has no such row);
 *   - otherwise, for pos = s .. e - 1 ascending with c = col_ind[pos]: if c is a member, the row gets the entry
 *     (first(c), pos).
 * Multi-edges and self-loops are kept, and the graph's order within a row is kept. offsets is the exclusive prefix of the row
 * lengths, offsets[n] = m. col[k] is the local id of entry k, edge_gid[k] its position in col_ind. A col_ind value is only
 * ever compared, never used as an index: damaged entries (-1, n_nodes, 2^31 - 1) never match, even when nodes holds those
 * same values, because such values are not members. The result is a function of the graph and nodes alone: it does not
 * depend on the launch geometry, on the capacity of the membership table, on the order of the inserts or on the memory type.
 *
 * The call makes one host round trip, for m: table and count are queued, the stream is synchronised, the outputs are
 * allocated, the fill is queued. It then returns with the outputs complete, or, after
 * wholememory_ext_set_async_completion(1), with the fill queued on `stream`, exactly as the samplers do.
 *
 * Errors, in this order; all but the last are answered before any device work. INVALID_INPUT: a NULL row_ptr, col_ind, nodes,
 * offset tensor, p_env_fns or output_col_memory_context; one of the four tensors not 1-D; n >= 2^31 - 1; an offset tensor
 * with fewer than n + 1 entries. LOGIC_ERROR, the dtype cases of (2m): row_ptr not int64, col_ind or nodes not int32 / int64,
 * offsets not int32. INVALID_INPUT for a HIERARCHY tensor. NOT_IMPLEMENTED for a DISTRIBUTED tensor: every membership probe
 * would be a collective gather. NOT_SUPPORTED, nothing queued, when the device backend has no such kernels. INVALID_INPUT when
 * m >= 2^31: answered after the count, with no output allocated. n = 0 succeeds: it writes offsets[0] = 0 and allocates empty
 * outputs. */
enum wholememory_error_code_t wholememory_ext_csr_induced_subgraph(
  wholememory_tensor_t wm_csr_row_ptr_tensor,
  wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t nodes_tensor,         /* [n] int32 / int64, device */
  wholememory_tensor_t output_offset_tensor, /* int32, at least n + 1 entries, device */
  void* output_col_memory_context,           /* int32 [m]: local positions */
  void* output_edge_gid_memory_context,      /* int64 [m] or NULL: positions in csr_col_ptr */
  wholememory_env_func_t* p_env_fns,
  void* stream);

/* ---- (2r) temporal neighbour sampling over a CSR graph held in WholeMemory ------------------------------------------------- */
/* The sampler of a model that trains on an interaction graph (TGN, TGAT; PyG's NeighborLoader with time_attr): a centre is a
 * node WITH a time, and only edges that are not in that time's future may be aggregated. For centre i the op returns the
 * neighbours of center_nodes[i] whose edge time passes the rule below against center_times[i], at most max_sample_count of
 * them. Graph tensors are as (2m): row_ptr int64 [n_nodes + 1], col_ind int32 or int64 [n_edges], and edge_time int64
 * [n_edges], one entry per edge position; all three CONTINUOUS or CHUNKED, in device or host memory, or plain device arrays
 * wrapped with wholememory_make_tensor_from_pointer. center_nodes is int32 or int64 [n], center_times int64 [n], both on the
 * device. The outputs follow the samplers: output_offset_tensor is the caller's, int32 with at least n + 1 entries, on the
 * device; dest (col_ind's dtype) and, with a context for them, center_localid int32 and edge_gid int64 are allocated through
 * p_env_fns once the total is known.
 *
 * Row of centre i, with u = center_nodes[i] and t = center_times[i]:
 *   - the row is empty when u is outside [0, n_nodes);
 *   - the row is empty when (s, e) = (row_ptr[u], row_ptr[u + 1]) does not satisfy 0 <= s <= e <= n_edges and e - s < 2^31
 *     (the rule of (2o) and (2q));
 *   - a col_ind entry is copied, never used as an index.
 * Eligibility. Neighbour j sits at position s + j, with ts = edge_time[s + j]. It is eligible when both hold:
 *   - ts <= t when inclusive != 0, ts < t when inclusive == 0;
 *   - time_window < 0, or (uint64)t - (uint64)ts <= (uint64)time_window. With ts <= t that difference is the exact distance
 *     of any two int64 values: there is no overflow case.
 * E_i is the number of eligible neighbours of centre i.
 * Counts. c_i = E_i when max_sample_count <= 0 (every eligible neighbour), else c_i = min(E_i, M) with M = max_sample_count.
 * M > 64 is INVALID_INPUT: the selection holds its M candidates in the registers of one wave. offsets is the exclusive prefix
 * of the c_i, offsets[n] the total.
 * Selection when E_i > M.
 *   - strategy 0 (uniform without replacement): r(i, j) is the first 32-bit output of stream(seed, i, j + 1) of (2m). The M
 *     eligible neighbours with the largest composite (uint64(r) << 32) | (0xFFFFFFFF - j) are chosen: the largest draws, ties to
 *     the lowest j. An ineligible neighbour draws nothing and shifts no one else's draw.
 *   - strategy 1 (last): the M eligible neighbours with the largest ts, ties to the lowest j.
 * Output order. Within a centre the output is in ascending j, whatever the strategy and whether or not a selection took place;
 * for a row stored in time order that is chronological order. center_localid[k] = i, edge_gid[k] = s + j. The result depends
 * on (seed, i, j), the graph and the times only, not on n or on the launch geometry: the rows of the first 100 centres of a
 * batch of 512 equal a batch of those 100.
 *
 * The call makes one host round trip, for the total: the count is queued, the stream is synchronised, the outputs are
 * allocated, the selection is queued. It then returns with the outputs complete, or, after
 * wholememory_ext_set_async_completion(1), with the selection queued on `stream`, exactly as the samplers do.
 *
 * Errors, in this order; all but the last are answered before any device work. INVALID_INPUT: a NULL row_ptr, col_ind,
 * edge_time, center_nodes, center_times, offset tensor, p_env_fns or output_dest_memory_context; one of the six tensors not
 * 1-D; max_sample_count > 64; strategy not 0 or 1; n >= 2^31 - 1; edge_time not one entry per edge; center_times not n
 * entries; an offset tensor with fewer than n + 1 entries. LOGIC_ERROR: row_ptr not int64, col_ind or center_nodes not int32 /
 * int64, edge_time or center_times not int64, offsets not int32. INVALID_INPUT for a HIERARCHY tensor. NOT_IMPLEMENTED for a
 * DISTRIBUTED tensor: Python composes that route (the all-neighbour sampler brings the centres' rows with their edge ids, a
 * gather their times, and this op runs on them as a device CSR with centres 0 .. n - 1, which preserves i and j and so the
 * samples). NOT_SUPPORTED, nothing queued, when the device backend has no such kernels. INVALID_INPUT when the total is
 * >= 2^31, reachable with max_sample_count <= 0 only: answered after the count, with no output allocated. n = 0 succeeds: it
 * writes offsets[0] = 0 and allocates empty outputs. */
enum wholememory_error_code_t wholememory_ext_csr_temporal_sample(
  wholememory_tensor_t wm_csr_row_ptr_tensor,
  wholememory_tensor_t wm_csr_col_ptr_tensor,
  wholememory_tensor_t wm_csr_edge_time_tensor, /* int64, one entry per edge */
  wholememory_tensor_t center_nodes_tensor,     /* [n] int32 / int64, device */
  wholememory_tensor_t center_times_tensor,     /* [n] int64, device */
  int max_sample_count,                         /* <= 0: every eligible neighbour, else at most 64 */
  int strategy,                                 /* 0: uniform, 1: last */
  int inclusive,
  long long time_window,                        /* < 0: none */
  unsigned long long random_seed,
  wholememory_tensor_t output_offset_tensor,    /* int32, at least n + 1 entries, device */
  void* output_dest_memory_context,             /* col_ind's dtype [total] */
  void* output_center_localid_memory_context,   /* int32 [total] or NULL */
  void* output_edge_gid_memory_context,         /* int64 [total] or NULL: positions in csr_col_ptr */
  wholememory_env_func_t* p_env_fns,
  void* stream);

/* ---- (3) testing seam ---------------------------------------------------------------------- */
/* Replaces the device backend. Refuses (WHOLEMEMORY_NOT_SUPPORTED) unless the environment has
 * WHOLEGRAPH_AMD_TESTING=1. `backend` is a const wm_device_backend* (wholegraph_amd/csrc/backend.hpp);
 * NULL restores the HIP backend. Never called by product code. */
enum wholememory_error_code_t wm_testing_install_backend(const void* backend);

/* Occupancy / effectiveness of an embedding's device row cache: slots, occupied slots, modified slots, lookups served
 * from the cache and lookups seen so far (this rank). A lookup is an id the cache was asked for: the cache of a rank's own
 * shard (cache communicator = the embedding's) is asked for the ids that reach this owner — an id that addresses no row, the
 * negative "skip" ids among them, reaches none and is not counted —, a local cache of the whole table for every id of the
 * caller's batch. INVALID_INPUT for an embedding without cache. */
enum wholememory_error_code_t wholememory_ext_embedding_cache_info(wholememory_embedding_t embedding, int64_t* slots,
                                                                   int64_t* occupied, int64_t* dirty, int64_t* hits,
                                                                   int64_t* lookups);

#ifdef __cplusplus
}
#endif
#endif
