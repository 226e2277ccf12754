"""Value sets on which a dtype conversion goes wrong if it can: built on the host, deterministic, no random tolerances.
Shared by tests/test_cast_values_gpu.py (row kernels vs the oracle) and tests/test_oracle_pinning.py (oracle vs torch's CPU
casts).

Carriers: every dtype travels as a numpy array of its own dtype, except bf16, which numpy does not have: raw bits in uint16
(what oracle.DT_BF16 takes). Every set holds a known number of NaNs (NAN_COUNT): for a NaN input a test asks only for a NaN
output — hardware and C disagree on payload bits — and asserts that count, so that the exclusion cannot grow silently.
The two 16-bit sources are ALL 65 536 bit patterns, so their NaN counts are the formats' own (2 x 1023 and 2 x 127)."""
import functools

import numpy as np

import oracle

FLOAT_NAMES = ("f32", "f16", "f64", "bf16")
INT_NAMES = ("i8", "i16", "i32", "i64")
FLOAT_PAIRS = [(a, b) for a in FLOAT_NAMES for b in FLOAT_NAMES if a != b]
INT_PAIRS = [(a, b) for a in INT_NAMES for b in INT_NAMES if a != b]

CARRIER = {"f32": np.float32, "f16": np.float16, "f64": np.float64, "bf16": np.uint16,
           "i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64}
ORACLE_DT = {"f32": oracle.DT_FLOAT, "f16": oracle.DT_HALF, "f64": oracle.DT_DOUBLE, "bf16": oracle.DT_BF16,
             "i8": oracle.DT_INT8, "i16": oracle.DT_INT16, "i32": oracle.DT_INT, "i64": oracle.DT_INT64}
# NaNs in each source set (see the module docstring)
NAN_COUNT = {"f16": 2 * 1023, "bf16": 2 * 127, "f32": 8, "f64": 8}

_F32_NANS = np.array([0x7fc00000, 0xffc00000, 0x7fc12345, 0xffc12345,      # quiet, both signs, with and without payload
                      0x7f800001, 0xff800001, 0x7fa00000, 0xffa00000],     # signalling (top mantissa bit clear)
                     dtype=np.uint32)
_F64_NANS = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000012345678, 0xfff8000012345678,
                      0x7ff0000000000001, 0xfff0000000000001, 0x7ff4000000000000, 0xfff4000000000000], dtype=np.uint64)


def torch_dtype(name):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "f64": torch.float64, "bf16": torch.bfloat16, "i8": torch.int8,
            "i16": torch.int16, "i32": torch.int32, "i64": torch.int64}[name]


def to_torch(arr, name):
    """carrier array -> torch tensor of dtype `name` over the same bits"""
    import torch
    if name == "bf16":
        return torch.from_numpy(arr.view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(arr)


def from_torch(t, name):
    """torch tensor (any device) -> carrier array, bits unchanged"""
    import torch
    t = t.cpu().contiguous()
    if name == "bf16":
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def bits_of(arr):
    """the array as unsigned integers of its element width (for bit-for-bit compares)"""
    return arr.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[arr.dtype.itemsize])


def isnan(arr, name):
    if name == "bf16":
        return (arr & 0x7fff) > 0x7f80
    return np.isnan(arr)


def sentinel(name):
    """one element that no conversion here produces by accident: -7 in the dtype"""
    if name == "bf16":
        return np.uint16(0xc0e0)
    return CARRIER[name](-7)


def _finite_16(name):
    """every non-negative finite value of a 16-bit format, ascending, exact in float64"""
    if name == "f16":
        return np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)
    return (np.arange(0x7f80, dtype=np.uint32) << 16).view(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def ties(name):
    """every midpoint between two neighbouring non-negative finite values of the 16-bit format `name`, as float32. Exact:
    a midpoint needs one more significand bit than the format (12 or 9) and is at least 2^-25 (f16) or 2^-134 (bf16), above
    float32's smallest subnormal 2^-149. The first one is half the smallest subnormal, the tie to zero."""
    v = _finite_16(name)
    mid = (v[:-1] + v[1:]) / 2
    out = mid.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), mid)
    out.setflags(write=False)
    return out


def _both_signs(a):
    return np.concatenate([a, -a])


def _with_neighbours(a):
    """a, and the next representable value of a's dtype below and above each element"""
    inf = a.dtype.type(np.inf)
    return np.concatenate([a, np.nextafter(a, -inf), np.nextafter(a, inf)])


def _bulk(n, seed, dtype):
    rng = np.random.default_rng(seed)
    with np.errstate(over="ignore"):   # 1e39 overflows float32 on purpose
        return (rng.standard_normal(n) * rng.choice([1e-42, 1e-8, 1e-6, 1e-4, 1, 300, 7e4, 1e39], n)).astype(dtype)


@functools.lru_cache(maxsize=None)
def f32_values():
    """float32 sources, without the NaNs: for both 16-bit targets every tie with its two float32 neighbours (2 x ~190 k with
    the signs), the overflow boundary (largest finite target value, the first value that rounds to infinity — the midpoint
    between it and the next power of two — and their neighbours), float32's own subnormals and limits, zeros, infinities, and
    2 k random values over eight magnitudes, 1e-42 (float32 subnormals) and 1e39 (infinity) among them."""
    parts = []
    for name, top, to_inf in (("f16", 65504.0, 65520.0),
                              ("bf16", float(np.uint32(0x7f7f0000).view(np.float32)), float(np.uint32(0x7f7f8000).view(np.float32)))):
        parts.append(_with_neighbours(ties(name)))
        parts.append(_with_neighbours(np.array([top, to_inf], dtype=np.float32)))
    sub = np.array([1, 2, 3, 0x400000, 0x7fffff, 0x800000, 0x800001, 0x7f7fffff], dtype=np.uint32).view(np.float32)
    parts.append(sub)
    parts.append(np.array([0.0, np.inf, 1.0, 0.5, 1.5, 2.0 ** -24, 2.0 ** -14, 2.0 ** -126, 2.0 ** -133], dtype=np.float32))
    parts.append(np.abs(_bulk(2048, 20, np.float32)))
    out = _both_signs(np.concatenate(parts))
    assert not np.isnan(out).any()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def f64_values():
    """float64 sources, without the NaNs: the float32 set widened; ties of float32 itself (the midpoint above 16 mantissas in
    each of its 254 binades and among its subnormals — all of them is 2^31 values) with their float64 neighbours; float32's
    overflow and underflow boundaries with their neighbours; +-1e300; and the double-rounding set: m (1 +- 2^-40) for every f16
    and bf16 tie m. float64 -> float32 rounds those onto the tie (2^-40 is far inside half a float32 ulp, also where m is a
    float32 subnormal: m 2^-40 <= 2^-166 against a spacing of 2^-149), and the tie then goes to even, whereas one rounding
    from float64 would follow the side the value is on."""
    parts = [f32_values().astype(np.float64)]
    mant = np.array([0, 1, 2, 3, 0x2aaaaa, 0x3fffff, 0x400000, 0x400001, 0x555555, 0x7ffffc, 0x7ffffd, 0x7ffffe, 0x7fffff,
                     0x123456, 0x654321, 0x0f0f0f], dtype=np.uint32)
    lo = ((np.arange(0, 255, dtype=np.uint32)[:, None] << 23) | mant[None, :]).ravel()   # exponent field 0: subnormals
    lo = lo[lo < 0x7f7fffff]
    a, b = lo.view(np.float32).astype(np.float64), (lo + 1).view(np.float32).astype(np.float64)
    parts.append(_with_neighbours((a + b) / 2))       # (the first one is 2^-150, float32's tie to zero)
    f32_max = float(np.finfo(np.float32).max)
    parts.append(_with_neighbours(np.array([f32_max, f32_max + 2.0 ** 103, 2.0 ** 128, 2.0 ** -150, 2.0 ** -149, 2.0 ** -126,
                                            2.0 ** -126 - 2.0 ** -150, 1e300, 1e-300, 2.0 ** -1074], dtype=np.float64)))
    for name in ("f16", "bf16"):
        m = ties(name).astype(np.float64)
        parts.append(m * (1 + 2.0 ** -40))
        parts.append(m * (1 - 2.0 ** -40))
    out = np.concatenate(parts)
    out = _both_signs(out[out >= 0])          # (nextafter below zero went negative: the mirror brings it back)
    assert not np.isnan(out).any()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def float_source(name):
    """all values of source dtype `name` as a flat carrier array (read-only), NaNs spread through it"""
    if name in ("f16", "bf16"):
        out = np.arange(65536, dtype=np.uint16)
        if name == "f16":
            out = out.view(np.float16)
    else:
        vals = f32_values() if name == "f32" else f64_values()
        nans = _F32_NANS.view(np.float32) if name == "f32" else _F64_NANS.view(np.float64)
        at = np.linspace(0, vals.size, len(nans), endpoint=False).astype(np.int64)
        out = np.insert(vals, at, nans)   # (memory copies: signalling NaNs keep their bits)
        assert out.size < 1 << 20 and len(nans) * 100 < out.size
    assert int(isnan(out, name).sum()) == NAN_COUNT[name]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def int_source(src, dst):
    """source values for the integer pair src -> dst: both types' limits and their neighbours where src holds them, -1, 0,
    and 8 k random values over src's whole range (enough rows for tiles with and without a skipped entry). Narrowing wraps,
    widening sign-extends."""
    si, di = np.iinfo(CARRIER[src]), np.iinfo(CARRIER[dst])
    edge = [si.min, si.min + 1, si.max, si.max - 1, -1, 0, 1, di.min - 1, di.min, di.min + 1, di.max - 1, di.max, di.max + 1,
            2 * di.max + 1, 2 * di.max + 2, 2 * di.min, 2 * di.min - 1]
    edge = np.array([v for v in edge if si.min <= v <= si.max], dtype=CARRIER[src])
    rnd = np.random.default_rng(30).integers(si.min, si.max, 8192, dtype=CARRIER[src], endpoint=True)
    out = np.concatenate([edge, rnd])
    out.setflags(write=False)
    return out


def as_table(values, dim, name):
    """the flat value set as a [rows, dim] table of its carrier dtype, the last row padded with 1"""
    rows = (values.size + dim - 1) // dim
    one = np.uint16(0x3f80) if name == "bf16" else values.dtype.type(1)
    table = np.full(rows * dim, one, dtype=values.dtype)
    table[:values.size] = values
    return table.reshape(rows, dim)


def rows_kernel(name):
    """(family, template arguments as text) of the row kernel named by wholememory_ext_last_rows_kernel(): e.g.
    ("rows_convert_kernel", ["float", "wm::bf16_t", "long", "4", "true"])"""
    import re
    m = re.search(r"(rows_\w+)<([^>]*)>", name)
    assert m, "not the demangled name of a row kernel: %r" % name
    return m.group(1), [a.strip() for a in m.group(2).split(",")]
