// wholegraph_amd — 8-bit row-quantized tables on gfx950 (wholegraph_amd_ext.h section 2i): the fused gather + dequantize
// and the quantize + scatter.
//
// A quantized row of `dim` values is Q = round_up(dim, 4) code bytes (the bytes past dim are zero), then fp32 scale and fp32
// bias: Q + 8 bytes, 4-byte aligned. y[j] = float(c[j]) * scale + bias — one multiply and one add, rounded separately (the
// file is built with -ffp-contract=off), then rounded once more to the output's fp16 / bf16.
//
// qrows_gather_dequant_kernel — the hot one; byte movement like kernels/rows.hip, and built the same way:
//  * a wave owns a tile of 64 consecutive entries: one coalesced id load, each lane resolves ITS entry's row address once
//    (continuous base, or the owner of a chunked table's row by multiply-high / the search over the rank offsets), and the
//    addresses then travel between lanes with ds_bpermute;
//  * one lane owns one dword = 4 codes of a row: a 128-wide row is 32 lanes, one coalesced 128-byte read, four
//    v_cvt_f32_ubyte, and one coalesced 512-byte write of 16 bytes per lane. Rows of up to 4 * 64 codes take a power-of-two
//    group of lanes (64 / lanes rows per wave step), longer rows are walked 64 dwords at a time;
//  * a lane has only 4 code bytes in flight per row, so the loads of KU (up to 8) steps — codes, scale and bias, the last two
//    at one address for the whole group — are issued back to back before the first conversion, as a straight-line batch with
//    nothing predicated: a skipped entry (negative id, or past n) takes the addresses of a valid entry of its tile and
//    repeats that entry's work (the same bytes to the same place), a lane past the row's last dword repeats the last dword;
//  * the output is written once: non-temporal stores, which leaves L2 / Infinity Cache to the table rows (they repeat);
//  * rows whose width is no multiple of 4, and outputs whose rows are not aligned to a lane's 4 elements, take the
//    element-wise instantiation (WIDE = false): the same batch of loads, stores of single elements under the column bound —
//    the bytes behind column dim of the last dword (zeros, and in the trailer's dword scale) are never stored;
//  * capped, persistent grid (grid-stride over tiles): 32 workgroups per CU at the most, fewer when the caller says so.
//
// qrows_quantize_kernel — not hot: one wave per row. Sweep 1 reduces min and max over the wave (shuffles), sweep 2 reads the
// row again and writes one dword of four codes per lane and step, then lane 0 the trailer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../backend.hpp"
#include "device_common.cuh"

namespace wm {
namespace {

constexpr int kBlock = 256;
constexpr int kWave  = 64;

struct qrows_params {
  // table side
  char* base;                      // continuous: flat base
  char* const* rank_ptrs;          // chunked: per-rank bases (device array)
  const size_t* rank_offsets;      // chunked, !same_chunk: byte offsets [world + 1] (device array)
  size_t chunk_stride;             // 0 = continuous; else bytes per rank
  uint64_t chunk_magic;            // same_chunk: rank = off / chunk_stride as umulhi(off, magic) >> shift; 0: stride 1
  int chunk_shift;
  int world_size;
  int same_chunk;
  int positions;                   // 1: entry i IS row i (ids, when given, only say "skip")
  int ids64;
  int64_t table_stride_bytes;
  int64_t table_offset_bytes;
  const void* indices;             // [n] or nullptr (positions mode only)
  int64_t n;
  // plain side (already offset by its storage offset)
  char* plain;
  int64_t plain_stride_bytes;
  int64_t dim;
  int words;                       // dwords of codes per row: Q / 4
  int lpr_log2;                    // log2(lanes per row)
};

// byte address of table row `row` (kernels/rows.hip: resolve_row)
__device__ __forceinline__ char* qrow_address(const qrows_params& p, int64_t row)
{
  const size_t off = static_cast<size_t>(p.table_offset_bytes) + static_cast<size_t>(row) * static_cast<size_t>(p.table_stride_bytes);
  if (p.chunk_stride == 0) return p.base + off;
  int rank;
  size_t rank_start;
  if (p.same_chunk) {
    rank       = static_cast<int>(p.chunk_magic == 0 ? off : (__umul64hi(off, p.chunk_magic) >> p.chunk_shift));
    rank       = rank < p.world_size ? rank : p.world_size - 1;
    rank_start = static_cast<size_t>(rank) * p.chunk_stride;
  } else {
    rank = 0;
    for (int r = 1; r < p.world_size; r++)
      if (off >= p.rank_offsets[r]) rank = r;
    rank_start = p.rank_offsets[rank];
  }
  return p.rank_ptrs[rank] + (off - rank_start);
}

// table row of entry `entry`, or nullptr when the entry is skipped (past n, or a negative id)
__device__ __forceinline__ char* entry_row(const qrows_params& p, int64_t entry)
{
  if (entry >= p.n) return nullptr;
  int64_t id = entry;
  if (p.indices != nullptr) {
    id = p.ids64 ? static_cast<const int64_t*>(p.indices)[entry] : static_cast<int64_t>(static_cast<const int32_t*>(p.indices)[entry]);
    if (id < 0) return nullptr;
    if (p.positions) id = entry;
  }
  return qrow_address(p, id);
}

__device__ __forceinline__ char* shfl_ptr(char* p, int src_lane)
{
  const uint64_t v  = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), src_lane, kWave);
  const uint32_t hi = __shfl(static_cast<uint32_t>(v >> 32), src_lane, kWave);
  return reinterpret_cast<char*>((static_cast<uint64_t>(hi) << 32) | lo);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <typename OutT>
__device__ __forceinline__ OutT narrow(float y);
template <>
__device__ __forceinline__ float narrow<float>(float y) { return y; }
template <>
__device__ __forceinline__ half_t narrow<half_t>(float y) { return static_cast<half_t>(y); }
template <>
__device__ __forceinline__ bf16_t narrow<bf16_t>(float y) { return float_to_bf16(y); }

template <typename OutT>
__device__ __forceinline__ uint32_t bits_of(OutT v)
{
  if constexpr (sizeof(OutT) == 4) {
    return __float_as_uint(v);
  } else {
    uint16_t s;
    __builtin_memcpy(&s, &v, 2);
    return s;
  }
}

// element k of the dword `w` of codes, dequantized
template <typename OutT>
__device__ __forceinline__ OutT dequant(uint32_t w, int k, float scale, float bias)
{
  const float c = static_cast<float>((w >> (8 * k)) & 0xffu);
  return narrow<OutT>(c * scale + bias);
}

// OutT: float, half_t or bf16_t. KU: steps per batch (KU * 64 >> lpr_log2 rows a wave loads before it converts the first;
// KU <= lanes per row, so that a batch never leaves the tile). WIDE: a lane stores its 4 elements as one vector.
template <typename OutT, int KU, bool WIDE>
__global__ __launch_bounds__(kBlock) void qrows_gather_dequant_kernel(qrows_params p)
{
  const int lane        = threadIdx.x & (kWave - 1);
  const int64_t wave    = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int lpr         = 1 << p.lpr_log2;
  const int rps         = kWave >> p.lpr_log2;
  const int sub         = lane >> p.lpr_log2;
  const int col         = lane & (lpr - 1);
  const int64_t tiles   = (p.n + kWave - 1) / kWave;
  const int64_t q_bytes = static_cast<int64_t>(p.words) * 4;

  for (int64_t tile = wave; tile < tiles; tile += n_waves) {
    const int64_t entry = tile * kWave + lane;
    char* my_tab        = entry_row(p, entry);
    char* my_plain      = p.plain + entry * p.plain_stride_bytes;
    // skipped entries repeat a valid entry of the tile: every lane of the batches below has a row to read and to write
    const uint64_t live = __ballot(my_tab != nullptr);
    if (live == 0) continue;
    if ((~live) != 0) {
      const int donor = __ffsll(static_cast<unsigned long long>(live)) - 1;
      char* dt        = shfl_ptr(my_tab, donor);
      char* dp        = shfl_ptr(my_plain, donor);
      if (my_tab == nullptr) my_tab = dt, my_plain = dp;
    }
    // both bases are complete HERE (kernels/rows.hip: load_tile_entry)
    asm volatile("" : "+v"(my_tab), "+v"(my_plain));
    for (int cbase = 0; cbase < p.words; cbase += lpr) {
      const int c  = cbase + col;
      const int cc = min(c, p.words - 1);
      for (int s0 = 0; s0 < kWave; s0 += rps * KU) {
        uint32_t w[KU], sc[KU], bi[KU];
        char* dst[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
          const int el = s0 + u * rps + sub;
          char* t      = shfl_ptr(my_tab, el);
          dst[u]       = shfl_ptr(my_plain, el) + static_cast<int64_t>(cc) * 4 * sizeof(OutT);
          w[u]         = ld_global<uint32_t>(t + static_cast<int64_t>(cc) * 4);
          sc[u]        = ld_global<uint32_t>(t + q_bytes);
          bi[u]        = ld_global<uint32_t>(t + q_bytes + 4);
        }
#pragma unroll
        for (int u = 0; u < KU; u++) {
          const float scale = __uint_as_float(sc[u]), bias = __uint_as_float(bi[u]);
          if constexpr (WIDE) {
            if constexpr (sizeof(OutT) == 4) {
              u32x4 o;
#pragma unroll
              for (int k = 0; k < 4; k++) o[k] = bits_of(dequant<OutT>(w[u], k, scale, bias));
              st_global_nt<u32x4>(dst[u], o);
            } else {
              u32x2 o;
#pragma unroll
              for (int k = 0; k < 2; k++)
                o[k] = bits_of(dequant<OutT>(w[u], 2 * k, scale, bias)) | (bits_of(dequant<OutT>(w[u], 2 * k + 1, scale, bias)) << 16);
              st_global_nt<u32x2>(dst[u], o);
            }
          } else {
            using store_t = typename std::conditional<sizeof(OutT) == 4, uint32_t, uint16_t>::type;
#pragma unroll
            for (int k = 0; k < 4; k++)
              if (c < p.words && static_cast<int64_t>(c) * 4 + k < p.dim)
                st_global_nt<store_t>(dst[u] + k * sizeof(OutT), static_cast<store_t>(bits_of(dequant<OutT>(w[u], k, scale, bias))));
          }
        }
      }
    }
  }
}

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) v = fminf(v, __shfl_xor(v, m, kWave));
  return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
  return v;
}

// one wave per entry; `plain` is the fp32 input, plain_stride_bytes its row stride
__global__ __launch_bounds__(kBlock) void qrows_quantize_kernel(qrows_params p)
{
  const int lane        = threadIdx.x & (kWave - 1);
  const int64_t wave    = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t entry = wave; entry < p.n; entry += n_waves) {
    char* row = entry_row(p, entry);   // (wave-uniform)
    if (row == nullptr) continue;
    const float* x = reinterpret_cast<const float*>(p.plain + entry * p.plain_stride_bytes);
    float lo = x[0], hi = x[0];
    for (int64_t j = lane; j < p.dim; j += kWave) {
      const float v = x[j];
      lo = fminf(lo, v), hi = fmaxf(hi, v);
    }
    lo = wave_min(lo) + 0.0f;   // (a zero minimum is stored as +0.0 whatever the signs of the row's zeros)
    hi = wave_max(hi);
    const float r     = hi - lo;
    const float scale = r == 0.0f ? 1.0f : r / 255.0f;
    const float inv   = r == 0.0f ? 1.0f : 255.0f / r;
    for (int wd = lane; wd < p.words; wd += kWave) {
      uint32_t packed = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int64_t j = static_cast<int64_t>(wd) * 4 + k;
        if (j < p.dim) {
          const float q = fminf(fmaxf(rintf((x[j] - lo) * inv), 0.0f), 255.0f);
          packed |= static_cast<uint32_t>(q) << (8 * k);
        }
      }
      st_global<uint32_t>(row + static_cast<int64_t>(wd) * 4, packed);
    }
    if (lane == 0) {
      st_global<uint32_t>(row + static_cast<int64_t>(p.words) * 4, __float_as_uint(scale));
      st_global<uint32_t>(row + static_cast<int64_t>(p.words) * 4 + 4, __float_as_uint(lo));
    }
  }
}

// rank = off / chunk_stride as multiply-high + shift (kernels/rows.hip: magic_for)
void magic_for(uint64_t d, uint64_t* m, int* shift)
{
  if (d <= 1) {
    *m = 0, *shift = 0;
    return;
  }
  int l = 0;
  while (l < 63 && (uint64_t(1) << l) < d) l++;
  const unsigned __int128 num = static_cast<unsigned __int128>(1) << (63 + l);
  *m     = static_cast<uint64_t>((num + d - 1) / d);
  *shift = l - 1;
}

// the cap of every launch here: 32 workgroups per CU (kernels/rows.hip: default_max_blocks)
int max_blocks_default()
{
  static int cus = 0;
  if (cus == 0) {
    hipDeviceProp_t prop;
    int dev = 0;
    cus = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  return cus * 32;
}

int blocks_for(int64_t waves_of_work, int max_blocks)
{
  int64_t b = (waves_of_work + (kBlock / kWave) - 1) / (kBlock / kWave);
  b         = std::min<int64_t>(std::max<int64_t>(b, 1), max_blocks_default());
  if (max_blocks > 0) b = std::min<int64_t>(b, max_blocks);
  return static_cast<int>(b);
}

// 0, or -1 for arguments no kernel here takes
int fill_params(const wm_qrows_args* a, int64_t plain_elt_bytes, qrows_params* p)
{
  if (a->dim < 1 || a->n < 0 || a->table_stride % 4 != 0 || a->table_storage_offset % 4 != 0) return -1;
  if (a->index_dtype != WHOLEMEMORY_DT_INT && a->index_dtype != WHOLEMEMORY_DT_INT64 && a->indices != nullptr) return -1;
  if (a->indices == nullptr && !a->positions) return -1;
  const int64_t words = (a->dim + 3) / 4;
  if (words * 4 + 8 > a->table_stride || words >= (int64_t(1) << 29)) return -1;
  p->chunk_stride = a->gref.stride;
  p->world_size   = a->gref.world_size;
  p->same_chunk   = a->gref.same_chunk ? 1 : 0;
  if (a->gref.stride == 0) {
    p->base = static_cast<char*>(a->gref.pointer);
  } else {
    p->rank_ptrs    = static_cast<char* const*>(a->gref.pointer);
    p->rank_offsets = a->gref.rank_memory_offsets;
    magic_for(p->chunk_stride, &p->chunk_magic, &p->chunk_shift);
  }
  p->positions          = a->positions ? 1 : 0;
  p->ids64              = a->index_dtype == WHOLEMEMORY_DT_INT64 ? 1 : 0;
  p->table_stride_bytes = a->table_stride;
  p->table_offset_bytes = a->table_storage_offset;
  p->indices            = a->indices;
  p->n                  = a->n;
  p->plain              = static_cast<char*>(a->plain);
  p->plain_stride_bytes = a->plain_stride * plain_elt_bytes;
  p->dim                = a->dim;
  p->words              = static_cast<int>(words);
  int l = 0;
  while (l < 6 && (1 << l) < words) l++;
  p->lpr_log2 = l;
  return 0;
}

template <typename OutT, bool WIDE>
void launch_gather(const qrows_params& p, int blocks, hipStream_t stream)
{
  switch (p.lpr_log2) {   // KU = min(8, lanes per row)
    case 0: hipLaunchKernelGGL((qrows_gather_dequant_kernel<OutT, 1, WIDE>), dim3(blocks), dim3(kBlock), 0, stream, p); break;
    case 1: hipLaunchKernelGGL((qrows_gather_dequant_kernel<OutT, 2, WIDE>), dim3(blocks), dim3(kBlock), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((qrows_gather_dequant_kernel<OutT, 4, WIDE>), dim3(blocks), dim3(kBlock), 0, stream, p); break;
    default: hipLaunchKernelGGL((qrows_gather_dequant_kernel<OutT, 8, WIDE>), dim3(blocks), dim3(kBlock), 0, stream, p); break;
  }
}

template <typename OutT>
void launch_gather_out(const qrows_params& p, int blocks, hipStream_t stream)
{
  // a lane's 4 elements as one store: whole dwords of codes only, and every row of the output aligned to those 4 elements
  const int64_t piece = 4 * static_cast<int64_t>(sizeof(OutT));
  const bool wide     = p.dim % 4 == 0 && p.plain_stride_bytes % piece == 0 && reinterpret_cast<uintptr_t>(p.plain) % piece == 0;
  if (wide) launch_gather<OutT, true>(p, blocks, stream);
  else launch_gather<OutT, false>(p, blocks, stream);
}

}  // namespace

int hip_qrows_gather_dequant(const wm_qrows_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const auto dt      = a->plain_dtype;
  if (dt != WHOLEMEMORY_DT_FLOAT && dt != WHOLEMEMORY_DT_HALF && dt != WHOLEMEMORY_DT_BF16) return -1;
  qrows_params p{};
  if (fill_params(a, dt == WHOLEMEMORY_DT_FLOAT ? 4 : 2, &p) != 0) return -1;
  if (a->n == 0) return 0;
  const int blocks = blocks_for((a->n + kWave - 1) / kWave, a->max_blocks);
  if (dt == WHOLEMEMORY_DT_FLOAT) launch_gather_out<float>(p, blocks, stream);
  else if (dt == WHOLEMEMORY_DT_HALF) launch_gather_out<half_t>(p, blocks, stream);
  else launch_gather_out<bf16_t>(p, blocks, stream);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int hip_qrows_quantize_scatter(const wm_qrows_args* a, void* stream_v)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  if (a->plain_dtype != WHOLEMEMORY_DT_FLOAT) return -1;
  qrows_params p{};
  if (fill_params(a, 4, &p) != 0) return -1;
  if (a->n == 0) return 0;
  hipLaunchKernelGGL(qrows_quantize_kernel, dim3(blocks_for(a->n, a->max_blocks)), dim3(kBlock), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace wm
