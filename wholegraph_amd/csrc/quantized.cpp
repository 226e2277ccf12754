// wholegraph_amd — host side of the 8-bit row-quantized tables (wholegraph_amd_ext.h, section 2i): validation and the two
// routes of the gather that dequantizes and of the scatter that quantizes. Tables mapped into this process (CONTINUOUS,
// CHUNKED, a plain pointer) are read / written by kernels/qrows.hip through their global reference; tables served by the
// exchange (DISTRIBUTED, HIERARCHY, WM_MAPPED_VIA_EXCHANGE) move their raw INT8 rows with wholememory_gather /
// wholememory_scatter, unchanged, and the kernels work on a local [n, row_bytes] temporary in place order.
#include <atomic>

#include <wholememory/wholegraph_amd_ext.h>
#include <wholememory/wholememory_tensor.h>

#include "ops_internal.hpp"

namespace {

using namespace wm;

std::atomic<int64_t> g_gather_dequantize_calls{0};   // gathers served by the kernel that reads the table itself

int64_t row_bytes_of(int64_t dim) { return (dim + 3) / 4 * 4 + 8; }

struct qcall {
  wm_qrows_args a{};
  bool via_exchange = false;
  int64_t row_bytes = 0;
};

// Everything both entry points check before any device work; `plain` is the gather's output / the scatter's input.
// Throws invalid_input / logic_error; fills the kernel arguments except the gref.
qcall check_call(wholememory_tensor_t q_table, int64_t dim, wholememory_tensor_t indices, wholememory_tensor_t plain,
                 const char* plain_name, bool gather, int max_blocks)
{
  auto bad = [](const std::string& what) { throw invalid_input(what); };
  if (q_table == nullptr) bad("q_table is null");
  if (plain == nullptr) bad(format_string("%s is null", plain_name));
  if (dim < 1) bad("dim must be >= 1");
  qcall q;
  q.row_bytes = row_bytes_of(dim);
  const wholememory_tensor_description_t td = *wholememory_tensor_get_tensor_description(q_table);
  if (td.dim != 2) bad("q_table must be a 2-D tensor");
  if (td.dtype != WHOLEMEMORY_DT_INT8) bad("q_table must be INT8");
  if (td.strides[1] != 1) bad("q_table rows must be contiguous");
  if (td.sizes[1] < q.row_bytes) bad(format_string("q_table rows hold %ld bytes, dim %ld needs %ld", static_cast<long>(td.sizes[1]), static_cast<long>(dim), static_cast<long>(q.row_bytes)));
  if (td.strides[0] < q.row_bytes || td.strides[0] % 4 != 0) bad("q_table row stride must be >= the row's bytes and a multiple of 4");
  if (td.storage_offset % 4 != 0) bad("q_table storage offset must be a multiple of 4 bytes");
  const wholememory_tensor_description_t pd = *wholememory_tensor_get_tensor_description(plain);
  if (pd.dim != 2) bad(format_string("%s must be a 2-D tensor", plain_name));
  if (!wholememory_dtype_is_floating_number(pd.dtype))
    throw logic_error(format_string("%s must be floating point (a quantized table holds floating-point values)", plain_name));
  if (gather ? (pd.dtype != WHOLEMEMORY_DT_FLOAT && pd.dtype != WHOLEMEMORY_DT_HALF && pd.dtype != WHOLEMEMORY_DT_BF16)
             : pd.dtype != WHOLEMEMORY_DT_FLOAT)
    bad(format_string("%s must be %s", plain_name, gather ? "FLOAT, HALF or BF16" : "FLOAT"));
  if (pd.strides[1] != 1) bad(format_string("%s rows must be contiguous", plain_name));
  if (pd.sizes[1] != dim) bad(format_string("%s has %ld columns, dim is %ld", plain_name, static_cast<long>(pd.sizes[1]), static_cast<long>(dim)));
  if (pd.strides[0] < dim) bad(format_string("%s row stride smaller than its row", plain_name));
  if (pd.sizes[0] < 0) bad("negative size");
  const bool has_handle = wholememory_tensor_has_handle(q_table);
  if (has_handle) {
    const auto mt = wholememory_get_memory_type(wholememory_tensor_get_memory_handle(q_table));
    q.via_exchange = mt == WHOLEMEMORY_MT_DISTRIBUTED || mt == WHOLEMEMORY_MT_HIERARCHY || mapped_via_exchange(q_table, mt);
    if (!q.via_exchange && mt != WHOLEMEMORY_MT_CONTINUOUS && mt != WHOLEMEMORY_MT_CHUNKED) bad("q_table has no memory type");
  }
  int64_t n = pd.sizes[0];
  if (indices != nullptr) {
    const wholememory_tensor_description_t id = *wholememory_tensor_get_tensor_description(indices);
    if (id.dim != 1) bad("indices must be a 1-D tensor");
    if (id.dtype != WHOLEMEMORY_DT_INT && id.dtype != WHOLEMEMORY_DT_INT64) bad("indices must be INT or INT64");
    if (id.sizes[0] < 0 || id.sizes[0] > pd.sizes[0]) bad(format_string("more indices than %s has rows", plain_name));
    n               = id.sizes[0];
    q.a.indices     = wholememory_tensor_get_data_pointer(indices);
    q.a.index_dtype = id.dtype;
    if (n > 0 && q.a.indices == nullptr) bad("indices have no data");
  } else {
    if (q.via_exchange) bad("a table served through the exchange needs indices");
    if (n > td.sizes[0]) bad(format_string("%s has more rows than q_table", plain_name));
    q.a.index_dtype = WHOLEMEMORY_DT_INT64;
  }
  q.a.plain = wholememory_tensor_get_data_pointer(plain);
  if (n > 0 && q.a.plain == nullptr) bad(format_string("%s has no data", plain_name));
  q.a.positions            = indices == nullptr ? 1 : 0;
  q.a.table_stride         = td.strides[0];
  q.a.table_storage_offset = td.storage_offset;
  q.a.dim                  = dim;
  q.a.n                    = n;
  q.a.plain_dtype          = pd.dtype;
  q.a.plain_stride         = pd.strides[0];
  q.a.max_blocks           = max_blocks;
  return q;
}

// the exchange route's local [n, stride] byte rows and the two tensors wholememory_gather / _scatter take: the table's
// columns [0, row_bytes) and the temporary
struct raw_rows {
  raw_rows(wholememory_env_func_t* env, wholememory_tensor_t q_table, const qcall& q) : mem(env)
  {
    stride = (q.row_bytes + 15) / 16 * 16;
    ptr    = mem.device(q.a.n * stride, WHOLEMEMORY_DT_INT8);
    wholememory_tensor_description_t d;
    wholememory_initialize_tensor_desc(&d);
    d.dim        = 2;
    d.dtype      = WHOLEMEMORY_DT_INT8;
    d.sizes[0]   = q.a.n;
    d.sizes[1]   = q.row_bytes;
    d.strides[0] = stride;
    d.strides[1] = 1;
    WM_CHECK(wholememory_make_tensor_from_pointer(&local, ptr, &d) == WHOLEMEMORY_SUCCESS, "temporary rows");
    int64_t starts[2] = {0, 0}, ends[2] = {-1, q.row_bytes};
    WM_CHECK(wholememory_tensor_get_subtensor(q_table, starts, ends, &columns) == WHOLEMEMORY_SUCCESS, "row columns");
  }
  ~raw_rows()
  {
    if (local != nullptr) wholememory_destroy_tensor(local);
    if (columns != nullptr) wholememory_destroy_tensor(columns);
  }
  // the kernel arguments of the call over the temporary: entry i is row i, the ids only say "skip"
  wm_qrows_args in_place(const qcall& q) const
  {
    wm_qrows_args a        = q.a;
    a.gref                 = wholememory_create_continuous_global_reference(ptr);
    a.positions            = 1;
    a.table_stride         = stride;
    a.table_storage_offset = 0;
    return a;
  }
  temp_mem mem;
  void* ptr                    = nullptr;
  int64_t stride               = 0;
  wholememory_tensor_t local   = nullptr;
  wholememory_tensor_t columns = nullptr;
};

// Large batches from a HOST-located mapped table take the two steps as well: wholememory_gather then reads the raw rows in
// ascending row order (ops.cpp: the sorted-ids gather of host tables, same condition), which PCIe serves several times
// faster than the same rows in random order, and the second step is local. Measured on the C1 shape (10 M x 64 in host
// memory): the table-reading kernel 4.13 ms / 41.4 ms for 1 M / 10 M ids, the two steps 3.70 / 14.9 ms.
bool host_sorted_route(wholememory_tensor_t q_table, wholememory_tensor_t indices, const qcall& q, wholememory_env_func_t* env)
{
  if (indices == nullptr || env == nullptr || !wholememory_tensor_has_handle(q_table)) return false;
  if (backend()->sort_ids == nullptr || host_sorted_gather_min() <= 0 || q.a.n < host_sorted_gather_min()) return false;
  return wholememory_get_memory_location(wholememory_tensor_get_memory_handle(q_table)) == WHOLEMEMORY_ML_HOST &&
         q.row_bytes <= 512;
}

}  // namespace

extern "C" {

int64_t wholememory_ext_quantized_row_bytes(int64_t dim) { return dim < 1 ? -1 : row_bytes_of(dim); }

wholememory_error_code_t wholememory_ext_gather_dequantize(wholememory_tensor_t q_table, int64_t dim,
                                                           wholememory_tensor_t indices, wholememory_tensor_t output,
                                                           wholememory_env_func_t* p_env_fns, void* stream, int gather_sms)
{
  WM_API_BEGIN
  qcall q        = check_call(q_table, dim, indices, output, "output", true, gather_sms);
  const auto* bk = backend();
  if (bk->qrows_gather_dequant == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (q.via_exchange || host_sorted_route(q_table, indices, q, p_env_fns)) {
    if (p_env_fns == nullptr) throw invalid_input("the exchange route needs env functions for its scratch");
    raw_rows rows(p_env_fns, q_table, q);
    WHOLEMEMORY_RETURN_ON_FAIL(wholememory_gather(rows.columns, indices, rows.local, p_env_fns, stream, gather_sms));
    const wm_qrows_args a = rows.in_place(q);
    WM_BK(bk->qrows_gather_dequant(&a, stream));
  } else {
    if (q.a.n == 0) return WHOLEMEMORY_SUCCESS;
    WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(q_table, &q.a.gref));
    WM_BK(bk->qrows_gather_dequant(&q.a, stream));
    g_gather_dequantize_calls.fetch_add(1, std::memory_order_relaxed);
  }
  if (debug_sync_enabled()) WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

wholememory_error_code_t wholememory_ext_quantize_scatter(wholememory_tensor_t input, wholememory_tensor_t indices,
                                                          wholememory_tensor_t q_table, int64_t dim,
                                                          wholememory_env_func_t* p_env_fns, void* stream, int scatter_sms)
{
  WM_API_BEGIN
  qcall q        = check_call(q_table, dim, indices, input, "input", false, scatter_sms);
  const auto* bk = backend();
  if (bk->qrows_quantize_scatter == nullptr) return WHOLEMEMORY_NOT_SUPPORTED;
  if (q.via_exchange) {
    if (p_env_fns == nullptr) throw invalid_input("the exchange route needs env functions for its scratch");
    raw_rows rows(p_env_fns, q_table, q);
    const wm_qrows_args a = rows.in_place(q);
    WM_BK(bk->qrows_quantize_scatter(&a, stream));
    WHOLEMEMORY_RETURN_ON_FAIL(wholememory_scatter(rows.local, indices, rows.columns, p_env_fns, stream, scatter_sms));
  } else {
    if (q.a.n == 0) return WHOLEMEMORY_SUCCESS;
    WHOLEMEMORY_RETURN_ON_FAIL(tensor_mapped_gref(q_table, &q.a.gref));
    WM_BK(bk->qrows_quantize_scatter(&q.a, stream));
  }
  if (debug_sync_enabled()) WM_BK(bk->stream_sync(stream));
  return WHOLEMEMORY_SUCCESS;
  WM_API_END
}

int64_t wholememory_ext_gather_dequantize_calls(void) { return g_gather_dequantize_calls.load(std::memory_order_relaxed); }

}  // extern "C"
