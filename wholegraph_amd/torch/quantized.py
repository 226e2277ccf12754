"""8-bit row-quantized WholeMemory tables (``include/wholememory/wholegraph_amd_ext.h`` section 2i, kernels in
``csrc/kernels/qrows.hip``): a read-mostly feature table kept as one uint8 code per value plus an fp32 ``(scale, bias)`` pair
per row, gathered and dequantized by ONE kernel — a 128-wide row is 136 bytes in memory and on the links instead of 512.

The storage is an ordinary int8 ``WholeMemoryTensor`` of shape ``[N, row_bytes]`` (``quantized_row_bytes(dim)``: the codes,
zero bytes up to a multiple of 4, then scale and bias), so files, every memory type and every location work on it
unchanged; ``WholeMemoryQuantizedTensor`` wraps it with the logical shape ``[N, dim]``:

    table = create_quantized_tensor(comm, "chunked", "cuda", [n_rows, dim])
    table.scatter(values, ids)                    # quantizes as it writes
    x = table.gather(ids)                         # float32 [n, dim]; force_dtype=torch.float16 / torch.bfloat16

CONTINUOUS and CHUNKED tables (and local buffers) take the fused kernels; DISTRIBUTED and HIERARCHY tables move their raw
rows through the usual exchange and are (de)quantized on the local side of it. ``calls()`` counts the fused gathers.
``quantize_rows`` / ``dequantize_rows`` are the same arithmetic on local tensors. The arithmetic is fixed and bitwise
reproducible: the header states it."""
import ctypes as C

import torch

from .. import binding as wmb
from .tensor import WholeMemoryTensor, create_wholememory_tensor
from .wholegraph_env import get_stream, get_wholegraph_env_fns, op_device, wrap_torch_tensor

_OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_ID_DTYPES = (torch.int32, torch.int64)


def quantized_row_bytes(dim: int) -> int:
    """bytes of one quantized row of `dim` values: round_up(dim, 4) + 8"""
    dim = int(dim)
    if dim < 1:
        raise ValueError("dim must be >= 1 (got %d)" % dim)
    return int(wmb.lib().wholememory_ext_quantized_row_bytes(dim))


def calls() -> int:
    """gathers served by the fused kernel that reads the table itself, in this process"""
    return int(wmb.lib().wholememory_ext_gather_dequantize_calls())


def _check_out_dtype(dtype):
    if dtype not in _OUT_DTYPES:
        raise TypeError("the output dtype must be float32, float16 or bfloat16 (got %s)" % dtype)


def _check_ids(indice):
    if indice.dim() != 1:
        raise ValueError("indice must be 1-D")
    if indice.dtype not in _ID_DTYPES:
        raise TypeError("indice must be int32 or int64 (got %s)" % indice.dtype)


def _values_f32(values, dim):
    if not isinstance(values, torch.Tensor):
        raise TypeError("values must be a torch tensor (got %s)" % type(values).__name__)
    if values.dtype in (torch.float16, torch.bfloat16):
        values = values.float()
    if values.dtype != torch.float32:
        raise TypeError("values must be float32, float16 or bfloat16 (got %s)" % values.dtype)
    if values.dim() != 2:
        raise ValueError("values must be 2-D")
    if dim is not None and values.shape[1] != dim:
        raise ValueError("values have %d columns, the table has %d" % (values.shape[1], dim))
    if values.shape[1] < 1:
        raise ValueError("values need at least one column")
    return values if values.stride(1) == 1 or values.numel() == 0 else values.contiguous()


def _on_device(t):
    dev = torch.device(op_device())
    return t if t.device == dev else t.to(dev)


def quantize_rows(values: torch.Tensor) -> torch.Tensor:
    """int8 [n, quantized_row_bytes(dim)]: the quantized rows of `values` [n, dim] (float32; float16 / bfloat16 are widened),
    on the device"""
    values = _on_device(_values_f32(values, None))
    n, dim = values.shape
    raw = torch.empty((n, quantized_row_bytes(dim)), dtype=torch.int8, device=values.device)
    wmb.check(wmb.lib().wholememory_ext_quantize_scatter(wrap_torch_tensor(values), None, wrap_torch_tensor(raw), dim,
                                                         get_wholegraph_env_fns(), C.c_void_p(get_stream()), -1),
              "quantize_scatter")
    return raw


def dequantize_rows(raw: torch.Tensor, dim: int, dtype=torch.float32) -> torch.Tensor:
    """`dtype` [n, dim]: the values of the quantized rows `raw` (int8 [n, >= quantized_row_bytes(dim)], row stride and offset
    multiples of 4 bytes), on the device"""
    _check_out_dtype(dtype)
    if not isinstance(raw, torch.Tensor) or raw.dtype != torch.int8:
        raise TypeError("raw must be an int8 tensor")
    if raw.dim() != 2:
        raise ValueError("raw must be 2-D")
    if raw.shape[1] < quantized_row_bytes(dim):
        raise ValueError("raw rows hold %d bytes, dim %d needs %d" % (raw.shape[1], dim, quantized_row_bytes(dim)))
    raw = _on_device(raw)
    if raw.numel() > 0 and raw.stride(1) != 1:
        raw = raw.contiguous()
    out = torch.empty((raw.shape[0], int(dim)), dtype=dtype, device=raw.device)
    wmb.check(wmb.lib().wholememory_ext_gather_dequantize(wrap_torch_tensor(raw), int(dim), None, wrap_torch_tensor(out),
                                                          get_wholegraph_env_fns(), C.c_void_p(get_stream()), -1),
              "gather_dequantize")
    return out


class WholeMemoryQuantizedTensor(object):
    """The logical [N, dim] face of an int8 WholeMemoryTensor [N, >= quantized_row_bytes(dim)] of quantized rows (one made
    by create_quantized_tensor, or any other — a table loaded from files, a row-range sub-tensor)."""

    def __init__(self, storage: WholeMemoryTensor, dim: int):
        if not isinstance(storage, WholeMemoryTensor):
            raise TypeError("storage must be a WholeMemoryTensor (got %s)" % type(storage).__name__)
        if storage.dtype != torch.int8:
            raise TypeError("storage must be int8 (got %s)" % storage.dtype)
        if storage.dim() != 2:
            raise ValueError("storage must be 2-D")
        row_bytes = quantized_row_bytes(dim)
        if storage.shape[1] < row_bytes:
            raise ValueError("storage rows hold %d bytes, dim %d needs %d" % (storage.shape[1], dim, row_bytes))
        if storage.stride()[0] % 4 != 0 or storage.storage_offset() % 4 != 0:
            raise ValueError("the row stride and the storage offset of the storage must be multiples of 4 bytes")
        self.storage = storage
        self.dim_ = int(dim)

    @property
    def shape(self):
        return (self.storage.shape[0], self.dim_)

    def get_comm(self):
        return self.storage.get_comm()

    def gather(self, indice: torch.Tensor, *, force_dtype=None) -> torch.Tensor:
        """[n, dim] of float32 (or force_dtype: float16 / bfloat16): the dequantized rows `indice`; rows of negative ids are
        left as torch.empty made them"""
        out_dtype = torch.float32 if force_dtype is None else force_dtype
        _check_out_dtype(out_dtype)
        _check_ids(indice)
        output = torch.empty((indice.shape[0], self.dim_), device=op_device(), dtype=out_dtype, requires_grad=False)
        wmb.check(wmb.lib().wholememory_ext_gather_dequantize(self.storage.wmb_tensor, self.dim_, wrap_torch_tensor(indice),
                                                              wrap_torch_tensor(output), get_wholegraph_env_fns(),
                                                              C.c_void_p(get_stream()), -1), "gather_dequantize")
        return output

    def scatter(self, values: torch.Tensor, indice: torch.Tensor):
        """rows `indice` of the table = the quantized rows of `values` [n, dim]"""
        values = _values_f32(values, self.dim_)
        _check_ids(indice)
        if indice.shape[0] != values.shape[0]:
            raise ValueError("%d ids for %d rows of values" % (indice.shape[0], values.shape[0]))
        wmb.check(wmb.lib().wholememory_ext_quantize_scatter(wrap_torch_tensor(values), wrap_torch_tensor(indice),
                                                             self.storage.wmb_tensor, self.dim_, get_wholegraph_env_fns(),
                                                             C.c_void_p(get_stream()), -1), "quantize_scatter")


def create_quantized_tensor(comm, memory_type, memory_location, sizes, *, row_align=16) -> WholeMemoryQuantizedTensor:
    """Collective. A quantized table of logical shape sizes = [N, dim]; the storage's row stride is
    quantized_row_bytes(dim) rounded up to `row_align` bytes (a multiple of 4)."""
    if len(sizes) != 2:
        raise ValueError("sizes must be [rows, dim]")
    row_align = int(row_align)
    if row_align < 4 or row_align % 4 != 0:
        raise ValueError("row_align must be a positive multiple of 4 (got %d)" % row_align)
    rows, dim = int(sizes[0]), int(sizes[1])
    row_bytes = quantized_row_bytes(dim)
    stride = (row_bytes + row_align - 1) // row_align * row_align
    storage = create_wholememory_tensor(comm, memory_type, memory_location, [rows, row_bytes], torch.int8, [stride, 1])
    return WholeMemoryQuantizedTensor(storage, dim)
