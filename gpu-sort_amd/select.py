"""Partial sort: the first k elements of the stable sort, by radix select (gs_topk_u32 in include/gpusort.h).

DeviceTopK is two-phase like DeviceRadixSort (d_temp_storage=None returns the size); topk() is the convenience form that
allocates outputs and workspace.  DeviceTopK16 is DeviceTopK for a flat array of 2-byte keys (gs_topk_u16: int16 / uint16 /
float16 / bfloat16) and DeviceTopK64 for 8-byte keys (gs_topk_u64: int64 / uint64 / float64); topk() sends such tensors there.  DeviceTopKSegmented / topk_segmented() are the same for every ragged segment given by device offsets
(gs_topk_segmented_u32, and gs_topk_segmented_u16 for int16 / uint16 / float16 / bfloat16 keys); DeviceTopKSegmented64 /
topk_segmented64() are the segmented form for 8-byte keys (gs_topk_segmented_u64: int64 / uint64 / float64).  DeviceTopKRows / topk_rows() are the same for every row of a matrix (gs_topk_rows_u32, and
gs_topk_rows_u16 for int16 / uint16 / float16 / bfloat16 keys, in the order of GS_KEY_F16 / BF16 at the enum); DeviceTopKRows64 /
topk_rows64() are the rows form for 8-byte keys (gs_topk_rows_u64: int64 / uint64 / float64); DeviceTopKRowsAnyK /
topk_rows_anyk() are the rows form for 32-bit keys and any k up to the row length (gs_topk_rows_anyk_u32).  The result is exactly the first k elements of DeviceRadixSort.SortKeys / SortPairs
(descending for the Max forms) on the same input: stable, keys in the caller's bit patterns, floats in the order of
GS_KEY_F32 (negative NaNs first, positive NaNs last ascending; -0.0 before +0.0).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import lib, check
from .lsb import _KEY_TYPES, _stream_ptr, _check_buf


def _key_type_of(t, key_type):
    if key_type is not None:
        return key_type
    kt = _KEY_TYPES.get(t.dtype, _lib.GS_KEY_U32)
    if kt not in (_lib.GS_KEY_U32, _lib.GS_KEY_I32, _lib.GS_KEY_F32):
        raise TypeError(f"DeviceTopK: 32-bit keys only (int32, float32, or uint32 by key_type), not {t.dtype}")
    return kt


_NARROW16 = (_lib.GS_KEY_U16, _lib.GS_KEY_I16, _lib.GS_KEY_F16, _lib.GS_KEY_BF16)     # what gs_topk_u16 / gs_topk_rows_u16 take


def _key_type16_of(t, key_type, who="DeviceTopKRows"):
    if key_type is None:
        key_type = _KEY_TYPES.get(t.dtype)
    if key_type not in _NARROW16:
        raise TypeError(f"{who}: no 16-bit key category for {t.dtype} (int16, uint16, float16, bfloat16, or GS_KEY_U16 / "
                        "I16 / F16 / BF16 by key_type)")
    return key_type


# what the key width changes at the flat front end: the name in messages, the entry point, its size query and status function,
# the key-type resolver, the key's bytes, and the explicit key types refused before anything else (None: the entry point's own
# refusal serves)
_WIDE64 = (_lib.GS_KEY_U64, _lib.GS_KEY_I64, _lib.GS_KEY_F64)                          # what gs_topk_u64 takes


def _key_type64_of(t, key_type, who="DeviceTopK64"):
    if key_type is None:
        key_type = _KEY_TYPES.get(t.dtype)
    if key_type not in _WIDE64:
        raise TypeError(f"{who}: no 64-bit key category for {t.dtype} (int64, float64, uint64, or GS_KEY_U64 / I64 / F64 by "
                        "key_type)")
    return key_type


_FLAT_BY_WIDTH = {
    32: ("DeviceTopK", "gs_topk_u32", "gs_topk_temp_bytes", "gs_topk_status", _key_type_of, 4, None, ""),
    16: ("DeviceTopK16", "gs_topk_u16", "gs_topk_u16_temp_bytes", "gs_topk_u16_status",
         lambda t, key_type: _key_type16_of(t, key_type, "DeviceTopK16"), 2, _NARROW16, "GS_KEY_U16 / I16 / F16 / BF16"),
    64: ("DeviceTopK64", "gs_topk_u64", "gs_topk_u64_temp_bytes", "gs_topk_u64_status", _key_type64_of, 8, _WIDE64,
         "GS_KEY_U64 / I64 / F64"),
}


class DeviceTopK:
    """MinKeys / MaxKeys / MinPairs / MaxPairs: the k smallest (largest) keys, sorted, with their values.

    d_values_in=None in the pairs forms writes the elements' input indices (u32 bit patterns in d_values_out): an argsort of
    the top k.  The inputs are never written; d_keys_out / d_values_out need k elements and must not overlap anything."""

    _width = 32

    @classmethod
    def _run(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_items, k, descending,
             has_values, stream, key_type):
        who, entry, size_query, _, resolve, elem, explicit, names = _FLAT_BY_WIDTH[cls._width]
        if key_type is not None and explicit is not None and key_type not in explicit:
            raise TypeError(f"{who}: key_type must be {names}")
        need = getattr(lib, size_query)(num_items, k, int(has_values))
        if d_temp_storage is None:
            return need
        if not isinstance(d_keys_in, torch.Tensor) or d_keys_in.element_size() != elem:
            raise TypeError(f"{who}: {8 * elem}-bit keys only")
        key_type = resolve(d_keys_in, key_type)
        _check_buf(d_keys_in, num_items, "d_keys_in", elem)
        _check_buf(d_keys_out, k, "d_keys_out", elem)
        if has_values:
            if d_values_in is not None:
                _check_buf(d_values_in, num_items, "d_values_in")
            _check_buf(d_values_out, k, "d_values_out")
        err = getattr(lib, entry)(C.c_void_p(d_temp_storage.data_ptr()),
                                  min(temp_storage_bytes, d_temp_storage.numel() * d_temp_storage.element_size()),
                                  d_keys_in.data_ptr(), d_values_in.data_ptr() if d_values_in is not None else None,
                                  d_keys_out.data_ptr(), d_values_out.data_ptr() if has_values else None,
                                  num_items, k, int(descending), key_type, _stream_ptr(stream))
        check(err, entry)
        return need

    @classmethod
    def MinKeys(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_items, k, stream=None, key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_items, k, False, False, stream,
                        key_type)

    @classmethod
    def MaxKeys(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_items, k, stream=None, key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_items, k, True, False, stream,
                        key_type)

    @classmethod
    def MinPairs(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_items, k, stream=None,
                 key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_items, k, False,
                        True, stream, key_type)

    @classmethod
    def MaxPairs(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_items, k, stream=None,
                 key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_items, k, True,
                        True, stream, key_type)

    @classmethod
    def Status(cls, d_temp_storage, num_items, k, has_values, stream=None):
        """gs_topk_status / gs_topk_u16_status: [route, image of the k-th element (16 bits wide for 16-bit keys), elements before
        it, taken from its tie run, elements sharing its top byte, 0, 0, 0] of the last call on d_temp_storage.  Synchronises
        the stream."""
        status = _FLAT_BY_WIDTH[cls._width][3]
        out = (C.c_uint32 * 8)()
        check(getattr(lib, status)(C.c_void_p(d_temp_storage.data_ptr()), num_items, k, int(has_values), out, _stream_ptr(stream)),
              status)
        return [int(x) for x in out]


class DeviceTopK16(DeviceTopK):
    """DeviceTopK for a flat array of 16-bit keys (gs_topk_u16): MinKeys / MaxKeys / MinPairs / MaxPairs / Status.

    The key type comes from the tensor's dtype (int16, uint16, float16, bfloat16) or from an explicit 16-bit key_type; the
    result is the first k of DeviceRadixSort on the same keys, in the order of GS_KEY_F16 / BF16 at the enum for the float
    types.  Values and indices are 4 bytes, as in DeviceTopK.  Keys of any other width raise TypeError."""

    _width = 16


class DeviceTopK64(DeviceTopK):
    """DeviceTopK for a flat array of 64-bit keys (gs_topk_u64): MinKeys / MaxKeys / MinPairs / MaxPairs / Status.

    The key type comes from the tensor's dtype (int64, float64, uint64) or from an explicit 64-bit key_type; the result is the
    first k of DeviceRadixSort on the same keys, float64 in the order of GS_KEY_F32 at the enum.  Values and indices are 4
    bytes, as in DeviceTopK.  Status() is [route, low and high word of the k-th image, elements before it, taken from its tie
    run, D, passes over the input, elements of the bucket or tie run].  Keys of any other width raise TypeError."""

    _width = 64


def topk(keys, k, largest=False, values=None, indices=False, stream=None):
    """The k smallest (largest=True: largest) of `keys`, sorted, as (keys_out, values_out).

    2-byte keys (int16, uint16, float16, bfloat16) take gs_topk_u16 through DeviceTopK16, 8-byte keys (int64, float64, uint64)
    gs_topk_u64 through DeviceTopK64, 4-byte keys gs_topk_u32.

    values: a 4-byte tensor of the same length, carried with the keys.  indices=True (without values): values_out holds the
    input positions as int32 bit patterns of u32 indices.  Neither: values_out is None.  Allocates outputs and workspace."""
    if values is not None and indices:
        raise ValueError("topk: give values or indices=True, not both")
    n = keys.numel()
    if not 0 <= k <= n:
        raise ValueError(f"topk: need 0 <= k <= {n}")
    has_values = values is not None or indices
    keys_out = torch.empty(k, dtype=keys.dtype, device=keys.device)
    values_out = None
    if has_values:
        values_out = torch.empty(k, dtype=values.dtype if values is not None else torch.int32, device=keys.device)
    front = {2: DeviceTopK16, 8: DeviceTopK64}.get(keys.element_size(), DeviceTopK)
    if front is DeviceTopK16:
        _key_type16_of(keys, None, "topk")
    elif front is DeviceTopK64:
        _key_type64_of(keys, None, "topk")
    if k == 0:
        return keys_out, values_out
    nbytes = front._run(None, 0, None, None, None, None, n, k, largest, has_values, stream, None)
    temp = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
    if stream is not None:
        temp.record_stream(stream)   # the workspace is freed on return: keep it until the stream has used it
    front._run(temp, nbytes, keys, keys_out, values, values_out, n, k, largest, has_values, stream, None)
    return keys_out, values_out


def _check_rows_in(t, what, elem=4):
    """An input matrix: a device tensor of `elem`-byte elements whose data_ptr() is row 0 (it may be a strided view, so its
    extent is the caller's statement: (num_rows - 1) * row_stride + num_cols elements)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.element_size() != elem:
        raise ValueError(f"{what}: expected a device tensor of {elem}-byte elements")


# what the key width changes at the front end: the entry point, its size query, the key-type resolver, the key's bytes
_ROWS_BY_WIDTH = {
    32: ("gs_topk_rows_u32", "gs_topk_rows_temp_bytes", _key_type_of, 4),
    16: ("gs_topk_rows_u16", "gs_topk_rows_u16_temp_bytes", _key_type16_of, 2),
}


class DeviceTopKRows:
    """MinKeys / MaxKeys / MinPairs / MaxPairs for every row of a matrix: row r is d_keys_in[r * row_stride .. + num_cols)
    (flat element offsets), and its k smallest (largest), sorted, go to d_keys_out[r * k .. + k) with their values.

    d_values_in=None in the pairs forms writes the elements' column indices (u32 bit patterns).  Each row's result is what
    DeviceTopK gives for that row alone.  The size query is 0 for a shape the entry point refuses (k > MaxK(), ...).

    2-byte key tensors (int16, uint16, float16, bfloat16, or an explicit 16-bit key_type) go to gs_topk_rows_u16: the same
    definition on the 16-bit image, values still 4 bytes.  The size query (d_temp_storage=None) sees no tensor: with a 16-bit
    key_type it answers for gs_topk_rows_u16, without one for gs_topk_rows_u32, which is never the smaller of the two."""

    @staticmethod
    def _run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols, row_stride,
             k, descending, has_values, stream, key_type):
        narrow = key_type in _NARROW16 if d_temp_storage is None or key_type is not None else d_keys_in.element_size() == 2
        entry, size_query, resolve, elem = _ROWS_BY_WIDTH[16 if narrow else 32]
        need = getattr(lib, size_query)(num_rows, num_cols, k, int(has_values))
        if d_temp_storage is None:
            return need
        if d_keys_in.element_size() != elem:
            raise TypeError("DeviceTopKRows: 32-bit keys, or 2-byte keys with a 16-bit key type")
        key_type = resolve(d_keys_in, key_type)
        _check_rows_in(d_keys_in, "d_keys_in", elem)
        _check_buf(d_keys_out, num_rows * k, "d_keys_out", elem)
        if has_values:
            if d_values_in is not None:
                _check_rows_in(d_values_in, "d_values_in")
            _check_buf(d_values_out, num_rows * k, "d_values_out")
        err = getattr(lib, entry)(C.c_void_p(d_temp_storage.data_ptr()),
                                  min(temp_storage_bytes, d_temp_storage.numel() * d_temp_storage.element_size()),
                                  d_keys_in.data_ptr(), d_values_in.data_ptr() if d_values_in is not None else None,
                                  d_keys_out.data_ptr(), d_values_out.data_ptr() if has_values else None,
                                  num_rows, num_cols, row_stride, k, int(descending), key_type, _stream_ptr(stream))
        check(err, entry)
        return need

    @staticmethod
    def MinKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_rows, num_cols, row_stride, k, stream=None,
                key_type=None):
        return DeviceTopKRows._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_rows, num_cols,
                                   row_stride, k, False, False, stream, key_type)

    @staticmethod
    def MaxKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_rows, num_cols, row_stride, k, stream=None,
                key_type=None):
        return DeviceTopKRows._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_rows, num_cols,
                                   row_stride, k, True, False, stream, key_type)

    @staticmethod
    def MinPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                 row_stride, k, stream=None, key_type=None):
        return DeviceTopKRows._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows,
                                   num_cols, row_stride, k, False, True, stream, key_type)

    @staticmethod
    def MaxPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                 row_stride, k, stream=None, key_type=None):
        return DeviceTopKRows._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows,
                                   num_cols, row_stride, k, True, True, stream, key_type)

    @staticmethod
    def MaxK():
        return int(lib.gs_topk_rows_max_k())

    @staticmethod
    def Plan(num_rows, num_cols, k, has_values=False):
        """gs_topk_rows_plan: [path, select levels, CH, chunks per row at level 0, candidates per row after level 0, max k,
        0, 0]; a pure host function.  Raises for a refused shape."""
        out = (C.c_uint32 * 8)()
        check(lib.gs_topk_rows_plan(num_rows, num_cols, k, int(has_values), out), "gs_topk_rows_plan")
        return [int(x) for x in out]


def topk_rows(keys, k, largest=False, values=None, indices=False, stream=None):
    """The k smallest (largest=True: largest) of every row of the 2-D tensor `keys`, sorted, as (keys_out, values_out) of shape
    [rows, k].

    The last dimension must be contiguous; the rows may sit at any stride >= cols (a column slice of a wider matrix).
    values: a 4-byte tensor of the same shape and strides, carried with the keys.  indices=True (without values): values_out
    holds the column indices as int32 bit patterns of u32.  Neither: values_out is None.  Allocates outputs and workspace.
    A k above DeviceTopKRows.MaxK() is served by gs_topk_u32 row by row.  2-byte keys (int16, uint16, float16, bfloat16) take
    gs_topk_rows_u16; for them a k above MaxK() raises ValueError: such callers loop topk() over the rows."""
    if values is not None and indices:
        raise ValueError("topk_rows: give values or indices=True, not both")
    if keys.dim() != 2:
        raise ValueError("topk_rows: a 2-D tensor, not %d-D" % keys.dim())
    rows, cols = keys.shape
    if cols > 1 and keys.stride(1) != 1:
        raise ValueError("topk_rows: the last dimension must be contiguous")
    if not 0 <= k <= cols:
        raise ValueError(f"topk_rows: need 0 <= k <= {cols}")
    stride = keys.stride(0) if rows > 1 else cols
    if rows > 1 and stride < cols:
        raise ValueError("topk_rows: rows overlap (stride %d < %d columns)" % (stride, cols))
    if values is not None and (values.shape != keys.shape or values.element_size() != 4 or
                               (cols > 1 and values.stride(1) != 1) or (rows > 1 and values.stride(0) != stride)):
        raise ValueError("topk_rows: values must have the keys' shape and strides and 4-byte elements")
    narrow = keys.element_size() == 2
    if narrow:
        _key_type16_of(keys, None)
        if k > lib.gs_topk_rows_max_k():
            raise ValueError("topk_rows: 16-bit keys need k <= %d; loop topk() over the rows for more" % lib.gs_topk_rows_max_k())
    elif keys.element_size() != 4:
        raise TypeError("topk_rows: 32-bit or 16-bit keys only")
    has_values = values is not None or indices
    keys_out = torch.empty((rows, k), dtype=keys.dtype, device=keys.device)
    values_out = None
    if has_values:
        values_out = torch.empty((rows, k), dtype=values.dtype if values is not None else torch.int32, device=keys.device)
    if k == 0 or rows == 0:
        return keys_out, values_out
    nbytes = getattr(lib, _ROWS_BY_WIDTH[16 if narrow else 32][1])(rows, cols, k, int(has_values))
    if nbytes == 0 and not narrow and k > lib.gs_topk_rows_max_k() and rows * stride < (1 << 32) and rows * k < (1 << 32):
        # refused for k alone: the flat top k of every row, one call each on one workspace
        nbytes = lib.gs_topk_temp_bytes(cols, k, int(has_values))
        temp = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
        if stream is not None:
            temp.record_stream(stream)
        for r in range(rows):
            DeviceTopK._run(temp, nbytes, keys[r], keys_out[r], None if values is None else values[r],
                            values_out[r] if has_values else None, cols, k, largest, has_values, stream, None)
        return keys_out, values_out
    if nbytes == 0:
        raise ValueError("topk_rows: the entry point refuses this shape (rows * stride and rows * k must be below 2^32)")
    temp = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
    if stream is not None:
        temp.record_stream(stream)   # the workspace is freed on return: keep it until the stream has used it
    DeviceTopKRows._run(temp, nbytes, keys, keys_out, values, values_out, rows, cols, stride, k, largest, has_values, stream, None)
    return keys_out, values_out


class DeviceTopKRows64:
    """DeviceTopKRows for a matrix of 64-bit keys (gs_topk_rows_u64): MinKeys / MaxKeys / MinPairs / MaxPairs / MaxK / Plan.

    The key type comes from the tensor's dtype (int64, float64, uint64) or from an explicit GS_KEY_U64 / I64 / F64; each row's
    result is what DeviceTopK64 gives for that row alone, float64 in the order of GS_KEY_F32 at the enum.  Values and column
    indices are 4 bytes.  Two-phase: d_temp_storage=None returns the size, 0 for a shape the entry point refuses.  Keys of
    any other width and any other key_type raise TypeError.  The geometry is DeviceTopKRows': Plan() is the same answer."""

    @staticmethod
    def _run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols, row_stride,
             k, descending, has_values, stream, key_type):
        if key_type is not None and key_type not in _WIDE64:
            raise TypeError("DeviceTopKRows64: key_type must be GS_KEY_U64 / I64 / F64")
        need = lib.gs_topk_rows_u64_temp_bytes(num_rows, num_cols, k, int(has_values))
        if d_temp_storage is None:
            return need
        if not isinstance(d_keys_in, torch.Tensor) or d_keys_in.element_size() != 8:
            raise TypeError("DeviceTopKRows64: 64-bit keys only")
        key_type = _key_type64_of(d_keys_in, key_type, "DeviceTopKRows64")
        _check_rows_in(d_keys_in, "d_keys_in", 8)
        _check_buf(d_keys_out, num_rows * k, "d_keys_out", 8)
        if has_values:
            if d_values_in is not None:
                _check_rows_in(d_values_in, "d_values_in")
            _check_buf(d_values_out, num_rows * k, "d_values_out")
        err = lib.gs_topk_rows_u64(C.c_void_p(d_temp_storage.data_ptr()),
                                   min(temp_storage_bytes, d_temp_storage.numel() * d_temp_storage.element_size()),
                                   d_keys_in.data_ptr(), d_values_in.data_ptr() if d_values_in is not None else None,
                                   d_keys_out.data_ptr(), d_values_out.data_ptr() if has_values else None,
                                   num_rows, num_cols, row_stride, k, int(descending), key_type, _stream_ptr(stream))
        check(err, "gs_topk_rows_u64")
        return need

    @staticmethod
    def MinKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_rows, num_cols, row_stride, k, stream=None,
                key_type=None):
        return DeviceTopKRows64._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_rows, num_cols,
                                     row_stride, k, False, False, stream, key_type)

    @staticmethod
    def MaxKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_rows, num_cols, row_stride, k, stream=None,
                key_type=None):
        return DeviceTopKRows64._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_rows, num_cols,
                                     row_stride, k, True, False, stream, key_type)

    @staticmethod
    def MinPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                 row_stride, k, stream=None, key_type=None):
        return DeviceTopKRows64._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows,
                                     num_cols, row_stride, k, False, True, stream, key_type)

    @staticmethod
    def MaxPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                 row_stride, k, stream=None, key_type=None):
        return DeviceTopKRows64._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows,
                                     num_cols, row_stride, k, True, True, stream, key_type)

    MaxK = staticmethod(DeviceTopKRows.MaxK)
    Plan = staticmethod(DeviceTopKRows.Plan)


def topk_rows64(keys, k, largest=False, values=None, indices=False, stream=None):
    """topk_rows() for a 2-D tensor of 8-byte keys (int64, float64, uint64): the k smallest (largest=True: largest) of every row,
    sorted, as (keys_out, values_out) of shape [rows, k], through gs_topk_rows_u64.

    The checks and the return shapes are topk_rows()': the last dimension contiguous, rows at any stride >= cols, values a
    4-byte tensor of the same shape and strides, indices=True for the column indices as int32 bit patterns of u32.  A k above
    DeviceTopKRows64.MaxK() is served by gs_topk_u64 row by row on one workspace.  Any other key width raises TypeError."""
    if values is not None and indices:
        raise ValueError("topk_rows64: give values or indices=True, not both")
    if keys.dim() != 2:
        raise ValueError("topk_rows64: a 2-D tensor, not %d-D" % keys.dim())
    rows, cols = keys.shape
    if cols > 1 and keys.stride(1) != 1:
        raise ValueError("topk_rows64: the last dimension must be contiguous")
    if not 0 <= k <= cols:
        raise ValueError(f"topk_rows64: need 0 <= k <= {cols}")
    stride = keys.stride(0) if rows > 1 else cols
    if rows > 1 and stride < cols:
        raise ValueError("topk_rows64: rows overlap (stride %d < %d columns)" % (stride, cols))
    if values is not None and (values.shape != keys.shape or values.element_size() != 4 or
                               (cols > 1 and values.stride(1) != 1) or (rows > 1 and values.stride(0) != stride)):
        raise ValueError("topk_rows64: values must have the keys' shape and strides and 4-byte elements")
    if keys.element_size() != 8:
        raise TypeError("topk_rows64: 64-bit keys only (int64, float64, uint64)")
    _key_type64_of(keys, None, "topk_rows64")
    has_values = values is not None or indices
    keys_out = torch.empty((rows, k), dtype=keys.dtype, device=keys.device)
    values_out = None
    if has_values:
        values_out = torch.empty((rows, k), dtype=values.dtype if values is not None else torch.int32, device=keys.device)
    if k == 0 or rows == 0:
        return keys_out, values_out
    nbytes = lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, int(has_values))
    if nbytes == 0 and k > lib.gs_topk_rows_max_k() and rows * stride < (1 << 32) and rows * k < (1 << 32):
        # refused for k alone: the flat top k of every row, one call each on one workspace
        nbytes = lib.gs_topk_u64_temp_bytes(cols, k, int(has_values))
        temp = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
        if stream is not None:
            temp.record_stream(stream)
        for r in range(rows):
            DeviceTopK64._run(temp, nbytes, keys[r], keys_out[r], None if values is None else values[r],
                              values_out[r] if has_values else None, cols, k, largest, has_values, stream, None)
        return keys_out, values_out
    if nbytes == 0:
        raise ValueError("topk_rows64: the entry point refuses this shape (rows * stride and rows * k must be below 2^32)")
    temp = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
    if stream is not None:
        temp.record_stream(stream)   # the workspace is freed on return: keep it until the stream has used it
    DeviceTopKRows64._run(temp, nbytes, keys, keys_out, values, values_out, rows, cols, stride, k, largest, has_values, stream, None)
    return keys_out, values_out


class DeviceTopKRowsAnyK:
    """DeviceTopKRows without the cap at MaxK() (gs_topk_rows_anyk_u32): MinKeys / MaxKeys / MinPairs / MaxPairs / Plan / Status
    for 32-bit keys and any 1 <= k <= num_cols.

    Each row's result is what DeviceTopK gives for that row alone; for k <= DeviceTopKRows.MaxK() it is DeviceTopKRows' result,
    and that class remains the faster one there.  Two-phase: d_temp_storage=None returns the size, 0 for a shape the entry
    point refuses (k > num_cols, num_rows * k >= 2^31, ...).  Keys of any other width raise TypeError."""

    @staticmethod
    def _run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols, row_stride,
             k, descending, has_values, stream, key_type):
        need = lib.gs_topk_rows_anyk_temp_bytes(num_rows, num_cols, k, int(has_values))
        if d_temp_storage is None:
            return need
        if not isinstance(d_keys_in, torch.Tensor) or d_keys_in.element_size() != 4:
            raise TypeError("DeviceTopKRowsAnyK: 32-bit keys only")
        key_type = _key_type_of(d_keys_in, key_type)
        _check_rows_in(d_keys_in, "d_keys_in")
        _check_buf(d_keys_out, num_rows * k, "d_keys_out")
        if has_values:
            if d_values_in is not None:
                _check_rows_in(d_values_in, "d_values_in")
            _check_buf(d_values_out, num_rows * k, "d_values_out")
        err = lib.gs_topk_rows_anyk_u32(C.c_void_p(d_temp_storage.data_ptr()),
                                        min(temp_storage_bytes, d_temp_storage.numel() * d_temp_storage.element_size()),
                                        d_keys_in.data_ptr(), d_values_in.data_ptr() if d_values_in is not None else None,
                                        d_keys_out.data_ptr(), d_values_out.data_ptr() if has_values else None,
                                        num_rows, num_cols, row_stride, k, int(descending), key_type, _stream_ptr(stream))
        check(err, "gs_topk_rows_anyk_u32")
        return need

    @staticmethod
    def MinKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_rows, num_cols, row_stride, k, stream=None,
                key_type=None):
        return DeviceTopKRowsAnyK._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_rows, num_cols,
                                       row_stride, k, False, False, stream, key_type)

    @staticmethod
    def MaxKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_rows, num_cols, row_stride, k, stream=None,
                key_type=None):
        return DeviceTopKRowsAnyK._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_rows, num_cols,
                                       row_stride, k, True, False, stream, key_type)

    @staticmethod
    def MinPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                 row_stride, k, stream=None, key_type=None):
        return DeviceTopKRowsAnyK._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out,
                                       num_rows, num_cols, row_stride, k, False, True, stream, key_type)

    @staticmethod
    def MaxPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                 row_stride, k, stream=None, key_type=None):
        return DeviceTopKRowsAnyK._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out,
                                       num_rows, num_cols, row_stride, k, True, True, stream, key_type)

    @staticmethod
    def Plan(num_rows, num_cols, k, has_values=False):
        """gs_topk_rows_anyk_plan: [path, kernel launches before the finish, CH, tile, tiles per slab, slabs per row, tiles per
        row, 0]; a pure host function.  Raises for a refused shape."""
        out = (C.c_uint32 * 8)()
        check(lib.gs_topk_rows_anyk_plan(num_rows, num_cols, k, int(has_values), out), "gs_topk_rows_anyk_plan")
        return [int(x) for x in out]

    @staticmethod
    def Status(d_temp_storage, num_rows, num_cols, k, has_values, row, stream=None):
        """gs_topk_rows_anyk_status: [path, image of row `row`'s k-th element, elements before it, taken from its tie run,
        elements that matched the prefix after round one, after round two, 0, 0] of the last call on d_temp_storage.
        Synchronises the stream."""
        out = (C.c_uint32 * 8)()
        check(lib.gs_topk_rows_anyk_status(C.c_void_p(d_temp_storage.data_ptr()), num_rows, num_cols, k, int(has_values), row, out,
                                           _stream_ptr(stream)), "gs_topk_rows_anyk_status")
        return [int(x) for x in out]


def topk_rows_anyk(keys, k, largest=False, values=None, indices=False, stream=None):
    """topk_rows() for any 0 <= k <= cols in one batched call (gs_topk_rows_anyk_u32): the k smallest (largest=True: largest)
    of every row of the 2-D tensor `keys` of 4-byte elements, sorted, as (keys_out, values_out) of shape [rows, k].

    The checks and the return shapes are topk_rows()': the last dimension contiguous, rows at any stride >= cols, values a
    4-byte tensor of the same shape and strides, indices=True for the column indices as int32 bit patterns of u32.  Any other
    key width raises TypeError.  For k <= DeviceTopKRows.MaxK() topk_rows() gives the same result faster."""
    if values is not None and indices:
        raise ValueError("topk_rows_anyk: give values or indices=True, not both")
    if keys.dim() != 2:
        raise ValueError("topk_rows_anyk: a 2-D tensor, not %d-D" % keys.dim())
    rows, cols = keys.shape
    if cols > 1 and keys.stride(1) != 1:
        raise ValueError("topk_rows_anyk: the last dimension must be contiguous")
    if not 0 <= k <= cols:
        raise ValueError(f"topk_rows_anyk: need 0 <= k <= {cols}")
    stride = keys.stride(0) if rows > 1 else cols
    if rows > 1 and stride < cols:
        raise ValueError("topk_rows_anyk: rows overlap (stride %d < %d columns)" % (stride, cols))
    if values is not None and (values.shape != keys.shape or values.element_size() != 4 or
                               (cols > 1 and values.stride(1) != 1) or (rows > 1 and values.stride(0) != stride)):
        raise ValueError("topk_rows_anyk: values must have the keys' shape and strides and 4-byte elements")
    if keys.element_size() != 4:
        raise TypeError("topk_rows_anyk: 32-bit keys only (int32, float32, uint32)")
    has_values = values is not None or indices
    keys_out = torch.empty((rows, k), dtype=keys.dtype, device=keys.device)
    values_out = None
    if has_values:
        values_out = torch.empty((rows, k), dtype=values.dtype if values is not None else torch.int32, device=keys.device)
    if k == 0 or rows == 0:
        return keys_out, values_out
    nbytes = lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, int(has_values))
    if nbytes == 0 or rows * stride >= (1 << 32):
        raise ValueError("topk_rows_anyk: the entry point refuses this shape (rows * stride below 2^32, rows * k below 2^31)")
    temp = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
    if stream is not None:
        temp.record_stream(stream)   # the workspace is freed on return: keep it until the stream has used it
    DeviceTopKRowsAnyK._run(temp, nbytes, keys, keys_out, values, values_out, rows, cols, stride, k, largest, has_values, stream, None)
    return keys_out, values_out


# the same table for the ragged segments
_SEG_BY_WIDTH = {
    32: ("gs_topk_segmented_u32", "gs_topk_segmented_temp_bytes", _key_type_of, 4),
    16: ("gs_topk_segmented_u16", "gs_topk_segmented_u16_temp_bytes",
         lambda t, key_type: _key_type16_of(t, key_type, "DeviceTopKSegmented"), 2),
}


class DeviceTopKSegmented:
    """MinKeys / MaxKeys / MinPairs / MaxPairs for every segment of a flat array (gs_topk_segmented_u32): segment s is
    d_keys_in[d_begin_offsets[s] .. d_end_offsets[s]) (int32 offsets on the device, clamped to [0, num_items] there), and its
    min(k, length) smallest (largest), sorted, go to d_keys_out[s * k ..) with their values; d_counts_out[s] (may be None) gets
    that number, and the slots behind it are not written.

    d_values_in=None in the pairs forms writes the elements' positions within their segment (u32 bit patterns).  Each
    segment's result is what DeviceTopK gives for that segment alone.  Two-phase like DeviceTopKRows: d_temp_storage=None
    returns the size, which is 0 for a shape the entry point refuses (k > MaxK(), num_items >= 2^31, ...).

    2-byte key tensors (int16, uint16, float16, bfloat16, or an explicit 16-bit key_type) go to gs_topk_segmented_u16: the same
    definition on the 16-bit image, values, counts and offsets still 4 bytes.  The size query (d_temp_storage=None) sees no
    tensor: with a 16-bit key_type it answers for gs_topk_segmented_u16, without one for gs_topk_segmented_u32, which is never
    the smaller of the two.  Plan() and Status() serve both widths."""

    @staticmethod
    def _run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
             num_segments, d_begin_offsets, d_end_offsets, k, descending, has_values, stream, key_type):
        if d_temp_storage is None or key_type is not None:
            narrow = key_type in _NARROW16
        else:
            narrow = isinstance(d_keys_in, torch.Tensor) and d_keys_in.element_size() == 2
        entry, size_query, resolve, elem = _SEG_BY_WIDTH[16 if narrow else 32]
        need = getattr(lib, size_query)(num_items, num_segments, k, int(has_values))
        if d_temp_storage is None:
            return need
        if not isinstance(d_keys_in, torch.Tensor) or d_keys_in.element_size() != elem:
            raise TypeError("DeviceTopKSegmented: 32-bit keys, or 2-byte keys with a 16-bit key type")
        key_type = resolve(d_keys_in, key_type)
        _check_buf(d_keys_in, num_items, "d_keys_in", elem)
        _check_buf(d_keys_out, num_segments * k, "d_keys_out", elem)
        _check_buf(d_begin_offsets, num_segments, "d_begin_offsets")
        _check_buf(d_end_offsets, num_segments, "d_end_offsets")
        if d_counts_out is not None:
            _check_buf(d_counts_out, num_segments, "d_counts_out")
        if has_values:
            if d_values_in is not None:
                _check_buf(d_values_in, num_items, "d_values_in")
            _check_buf(d_values_out, num_segments * k, "d_values_out")
        err = getattr(lib, entry)(C.c_void_p(d_temp_storage.data_ptr()),
                                  min(temp_storage_bytes, d_temp_storage.numel() * d_temp_storage.element_size()),
                                  d_keys_in.data_ptr(), d_values_in.data_ptr() if d_values_in is not None else None,
                                  d_keys_out.data_ptr(), d_values_out.data_ptr() if has_values else None,
                                  d_counts_out.data_ptr() if d_counts_out is not None else None, num_items, num_segments,
                                  d_begin_offsets.data_ptr(), d_end_offsets.data_ptr(), k, int(descending), key_type,
                                  _stream_ptr(stream))
        check(err, entry)
        return need

    @staticmethod
    def MinKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_counts_out, num_items, num_segments, d_begin_offsets,
                d_end_offsets, k, stream=None, key_type=None):
        return DeviceTopKSegmented._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, d_counts_out, num_items,
                                        num_segments, d_begin_offsets, d_end_offsets, k, False, False, stream, key_type)

    @staticmethod
    def MaxKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_counts_out, num_items, num_segments, d_begin_offsets,
                d_end_offsets, k, stream=None, key_type=None):
        return DeviceTopKSegmented._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, d_counts_out, num_items,
                                        num_segments, d_begin_offsets, d_end_offsets, k, True, False, stream, key_type)

    @staticmethod
    def MinPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
                 num_segments, d_begin_offsets, d_end_offsets, k, stream=None, key_type=None):
        return DeviceTopKSegmented._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out,
                                        d_counts_out, num_items, num_segments, d_begin_offsets, d_end_offsets, k, False, True, stream,
                                        key_type)

    @staticmethod
    def MaxPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
                 num_segments, d_begin_offsets, d_end_offsets, k, stream=None, key_type=None):
        return DeviceTopKSegmented._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out,
                                        d_counts_out, num_items, num_segments, d_begin_offsets, d_end_offsets, k, True, True, stream,
                                        key_type)

    @staticmethod
    def MaxK():
        return int(lib.gs_topk_rows_max_k())

    @staticmethod
    def Plan(num_items, num_segments, k, has_values=False):
        """gs_topk_segmented_plan: [launch groups (bit 0 wave, 1 workgroup, 2 long), kernel launches, CH, Lmax, Tmax, max k, 0,
        0]; a pure host function.  Raises for a refused shape."""
        out = (C.c_uint32 * 8)()
        check(lib.gs_topk_segmented_plan(num_items, num_segments, k, int(has_values), out), "gs_topk_segmented_plan")
        return [int(x) for x in out]

    @staticmethod
    def Status(d_temp_storage, num_items, num_segments, k, has_values, stream=None):
        """gs_topk_segmented_status: [segments in the four wave lists, the workgroup list, the long list, chunk tasks, dropped
        segments] of the last call on d_temp_storage.  Synchronises the stream."""
        out = (C.c_uint32 * 8)()
        check(lib.gs_topk_segmented_status(C.c_void_p(d_temp_storage.data_ptr()), num_items, num_segments, k, int(has_values), out,
                                           _stream_ptr(stream)), "gs_topk_segmented_status")
        return [int(x) for x in out]


def topk_segmented(keys, offsets, k, largest=False, values=None, indices=False, stream=None, end_offsets=None):
    """The k smallest (largest=True: largest) of every segment of the 1-D tensor `keys`, sorted, as (keys_out [S, k],
    values_out [S, k] or None, counts [S] int32).

    offsets: an int32 device tensor of S + 1 elements, segment s being keys[offsets[s] : offsets[s + 1]]; or, with end_offsets
    given, the S begins, segment s being keys[offsets[s] : end_offsets[s]] (any order, gaps, repeats; see gs_topk_segmented_u32
    for overlaps).  counts[s] = min(k, length of segment s); the slots of row s past counts[s] are unspecified.
    values: a 4-byte tensor of the keys' length, carried with the keys.  indices=True (without values): values_out holds the
    positions within the segment as int32 bit patterns of u32.  Neither: values_out is None.  Allocates outputs and workspace.
    2-byte keys (int16, uint16, float16, bfloat16) take gs_topk_segmented_u16 and come back in the input dtype."""
    if values is not None and indices:
        raise ValueError("topk_segmented: give values or indices=True, not both")
    if keys.dim() != 1 or keys.element_size() not in (2, 4):
        raise TypeError("topk_segmented: a 1-D tensor of 32-bit or 16-bit keys")
    narrow = keys.element_size() == 2
    if narrow:
        _key_type16_of(keys, None, "topk_segmented")
    if offsets.dtype != torch.int32 or (end_offsets is not None and end_offsets.dtype != torch.int32):
        raise TypeError("topk_segmented: int32 offsets")
    if end_offsets is None:
        if offsets.numel() < 1:
            raise ValueError("topk_segmented: offsets needs S + 1 elements")
        begins, ends, segs = offsets[:-1], offsets[1:], offsets.numel() - 1
    else:
        if end_offsets.numel() != offsets.numel():
            raise ValueError("topk_segmented: as many ends as begins")
        begins, ends, segs = offsets, end_offsets, offsets.numel()
    n = keys.numel()
    if k < 0:
        raise ValueError("topk_segmented: need k >= 0")
    if values is not None and (values.numel() != n or values.element_size() != 4 or values.dim() != 1):
        raise ValueError("topk_segmented: values must have the keys' length and 4-byte elements")
    has_values = values is not None or indices
    keys_out = torch.empty((segs, k), dtype=keys.dtype, device=keys.device)
    values_out = None
    if has_values:
        values_out = torch.empty((segs, k), dtype=values.dtype if values is not None else torch.int32, device=keys.device)
    counts = torch.zeros(segs, dtype=torch.int32, device=keys.device)
    if k == 0 or segs == 0 or n == 0:
        return keys_out, values_out, counts
    nbytes = getattr(lib, _SEG_BY_WIDTH[16 if narrow else 32][1])(n, segs, k, int(has_values))
    if nbytes == 0:
        raise ValueError("topk_segmented: the entry point refuses this shape (k <= %d, fewer than 2^31 keys, segments * k below 2^32)"
                         % lib.gs_topk_rows_max_k())
    temp = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
    if stream is not None:
        temp.record_stream(stream)   # the workspace is freed on return: keep it until the stream has used it
    DeviceTopKSegmented._run(temp, nbytes, keys.contiguous(), keys_out, values, values_out, counts, n, segs, begins, ends, k, largest,
                             has_values, stream, None)
    return keys_out, values_out, counts


class DeviceTopKSegmented64:
    """DeviceTopKSegmented for a flat array of 64-bit keys (gs_topk_segmented_u64): MinKeys / MaxKeys / MinPairs / MaxPairs /
    MaxK / Plan / Status.

    The key type comes from the tensor's dtype (int64, float64, uint64) or from an explicit GS_KEY_U64 / I64 / F64; each
    segment's result is what DeviceTopK64 gives for that segment alone, float64 in the order of GS_KEY_F32 at the enum.
    Values, positions, counts and offsets are 4 bytes.  Two-phase: d_temp_storage=None returns the size, 0 for a shape the
    entry point refuses.  Keys of any other width and any other key_type raise TypeError.  The geometry is
    DeviceTopKSegmented's: Plan() is the same answer, and Status() reads a workspace of either class."""

    @staticmethod
    def _run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
             num_segments, d_begin_offsets, d_end_offsets, k, descending, has_values, stream, key_type):
        if key_type is not None and key_type not in _WIDE64:
            raise TypeError("DeviceTopKSegmented64: key_type must be GS_KEY_U64 / I64 / F64")
        need = lib.gs_topk_segmented_u64_temp_bytes(num_items, num_segments, k, int(has_values))
        if d_temp_storage is None:
            return need
        if not isinstance(d_keys_in, torch.Tensor) or d_keys_in.element_size() != 8:
            raise TypeError("DeviceTopKSegmented64: 64-bit keys only")
        key_type = _key_type64_of(d_keys_in, key_type, "DeviceTopKSegmented64")
        _check_buf(d_keys_in, num_items, "d_keys_in", 8)
        _check_buf(d_keys_out, num_segments * k, "d_keys_out", 8)
        _check_buf(d_begin_offsets, num_segments, "d_begin_offsets")
        _check_buf(d_end_offsets, num_segments, "d_end_offsets")
        if d_counts_out is not None:
            _check_buf(d_counts_out, num_segments, "d_counts_out")
        if has_values:
            if d_values_in is not None:
                _check_buf(d_values_in, num_items, "d_values_in")
            _check_buf(d_values_out, num_segments * k, "d_values_out")
        err = lib.gs_topk_segmented_u64(C.c_void_p(d_temp_storage.data_ptr()),
                                        min(temp_storage_bytes, d_temp_storage.numel() * d_temp_storage.element_size()),
                                        d_keys_in.data_ptr(), d_values_in.data_ptr() if d_values_in is not None else None,
                                        d_keys_out.data_ptr(), d_values_out.data_ptr() if has_values else None,
                                        d_counts_out.data_ptr() if d_counts_out is not None else None, num_items, num_segments,
                                        d_begin_offsets.data_ptr(), d_end_offsets.data_ptr(), k, int(descending), key_type,
                                        _stream_ptr(stream))
        check(err, "gs_topk_segmented_u64")
        return need

    @staticmethod
    def MinKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_counts_out, num_items, num_segments, d_begin_offsets,
                d_end_offsets, k, stream=None, key_type=None):
        return DeviceTopKSegmented64._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, d_counts_out,
                                          num_items, num_segments, d_begin_offsets, d_end_offsets, k, False, False, stream, key_type)

    @staticmethod
    def MaxKeys(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_counts_out, num_items, num_segments, d_begin_offsets,
                d_end_offsets, k, stream=None, key_type=None):
        return DeviceTopKSegmented64._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, d_counts_out,
                                          num_items, num_segments, d_begin_offsets, d_end_offsets, k, True, False, stream, key_type)

    @staticmethod
    def MinPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
                 num_segments, d_begin_offsets, d_end_offsets, k, stream=None, key_type=None):
        return DeviceTopKSegmented64._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out,
                                          d_counts_out, num_items, num_segments, d_begin_offsets, d_end_offsets, k, False, True,
                                          stream, key_type)

    @staticmethod
    def MaxPairs(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
                 num_segments, d_begin_offsets, d_end_offsets, k, stream=None, key_type=None):
        return DeviceTopKSegmented64._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out,
                                          d_counts_out, num_items, num_segments, d_begin_offsets, d_end_offsets, k, True, True,
                                          stream, key_type)

    MaxK = staticmethod(DeviceTopKSegmented.MaxK)
    Plan = staticmethod(DeviceTopKSegmented.Plan)
    Status = staticmethod(DeviceTopKSegmented.Status)


def topk_segmented64(keys, offsets, k, largest=False, values=None, indices=False, stream=None, end_offsets=None):
    """topk_segmented() for a 1-D tensor of 8-byte keys (int64, float64, uint64): the k smallest (largest=True: largest) of
    every segment, sorted, as (keys_out [S, k], values_out [S, k] or None, counts [S] int32), through gs_topk_segmented_u64.

    The arguments, the checks and the return shapes are topk_segmented()'s: int32 device offsets of S + 1 elements, or begins
    and end_offsets; values a 4-byte tensor of the keys' length; indices=True for the positions within the segment as int32
    bit patterns of u32.  The keys come back in the input dtype.  Any other key width raises TypeError."""
    if values is not None and indices:
        raise ValueError("topk_segmented64: give values or indices=True, not both")
    if keys.dim() != 1 or keys.element_size() != 8:
        raise TypeError("topk_segmented64: a 1-D tensor of 64-bit keys (int64, float64, uint64)")
    _key_type64_of(keys, None, "topk_segmented64")
    if offsets.dtype != torch.int32 or (end_offsets is not None and end_offsets.dtype != torch.int32):
        raise TypeError("topk_segmented64: int32 offsets")
    if end_offsets is None:
        if offsets.numel() < 1:
            raise ValueError("topk_segmented64: offsets needs S + 1 elements")
        begins, ends, segs = offsets[:-1], offsets[1:], offsets.numel() - 1
    else:
        if end_offsets.numel() != offsets.numel():
            raise ValueError("topk_segmented64: as many ends as begins")
        begins, ends, segs = offsets, end_offsets, offsets.numel()
    n = keys.numel()
    if k < 0:
        raise ValueError("topk_segmented64: need k >= 0")
    if values is not None and (values.numel() != n or values.element_size() != 4 or values.dim() != 1):
        raise ValueError("topk_segmented64: values must have the keys' length and 4-byte elements")
    has_values = values is not None or indices
    keys_out = torch.empty((segs, k), dtype=keys.dtype, device=keys.device)
    values_out = None
    if has_values:
        values_out = torch.empty((segs, k), dtype=values.dtype if values is not None else torch.int32, device=keys.device)
    counts = torch.zeros(segs, dtype=torch.int32, device=keys.device)
    if k == 0 or segs == 0 or n == 0:
        return keys_out, values_out, counts
    nbytes = lib.gs_topk_segmented_u64_temp_bytes(n, segs, k, int(has_values))
    if nbytes == 0:
        raise ValueError("topk_segmented64: the entry point refuses this shape (k <= %d, fewer than 2^31 keys, segments * k below "
                         "2^32)" % lib.gs_topk_rows_max_k())
    temp = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
    if stream is not None:
        temp.record_stream(stream)   # the workspace is freed on return: keep it until the stream has used it
    DeviceTopKSegmented64._run(temp, nbytes, keys.contiguous(), keys_out, values, values_out, counts, n, segs, begins, ends, k,
                               largest, has_values, stream, None)
    return keys_out, values_out, counts
