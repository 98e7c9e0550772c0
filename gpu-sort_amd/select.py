"""Partial sort: the first k elements of the stable sort, by radix select (the gs_topk_* entry points of include/gpusort.h).

    class                   entry point               keys
    DeviceTopK              gs_topk_u32               int32, float32, uint32
    DeviceTopK16            gs_topk_u16               int16, uint16, float16, bfloat16
    DeviceTopK64            gs_topk_u64               int64, float64, uint64
    DeviceTopKRows          gs_topk_rows_u32          int32, float32, uint32
                            gs_topk_rows_u16          int16, uint16, float16, bfloat16
    DeviceTopKRows64        gs_topk_rows_u64          int64, float64, uint64
    DeviceTopKRowsAnyK      gs_topk_rows_anyk_u32     int32, float32, uint32; any k up to the row length
    DeviceTopKRowsAnyK16    gs_topk_rows_anyk_u16     int16, uint16, float16, bfloat16; any k up to the row length
    DeviceTopKRowsAnyK64    gs_topk_rows_anyk_u64     int64, float64, uint64; any k up to the row length
    DeviceTopKSegmented     gs_topk_segmented_u32     int32, float32, uint32
                            gs_topk_segmented_u16     int16, uint16, float16, bfloat16
    DeviceTopKSegmented64   gs_topk_segmented_u64     int64, float64, uint64
    DeviceTopKSegmentedAnyK gs_topk_segmented_anyk_u32  int32, float32, uint32; any k

The classes are two-phase like DeviceRadixSort (d_temp_storage=None returns the size); topk(), topk_rows(), topk_rows64(),
topk_rows_anyk(), topk_rows_anyk16(), topk_rows_anyk64(), topk_segmented(), topk_segmented64() and topk_segmented_anyk() allocate outputs and workspace, topk() for any of the three widths.
The result is exactly the first k elements of DeviceRadixSort.SortKeys / SortPairs (descending for the Max forms) on the same
input (the whole array, every row of a matrix, every ragged segment given by device offsets): stable, keys in the caller's bit
patterns, floats in the order of GS_KEY_F32 (negative NaNs first, positive NaNs last ascending; -0.0 before +0.0), float16 /
bfloat16 in the order of GS_KEY_F16 / BF16 at the enum.
"""
import collections
import ctypes as C

import torch

from . import _lib
from ._lib import lib, check
from .lsb import _KEY_TYPES, _stream_ptr, _check_buf


# A key width, for all three call shapes: the key's bytes, the GS_KEY_* the width's entry points take, their names and the
# dtypes behind them as the messages state them, and how an unknown key type is met.  strict: a foreign explicit key_type is a
# TypeError before anything else, and a tensor needs a dtype of the width's own.  Not strict (32 bits): the entry point's own
# refusal of a foreign key_type serves, and a 4-byte tensor of any other dtype is sorted as GS_KEY_U32.
_Width = collections.namedtuple("_Width", "elem key_types names dtypes strict")
_W16 = _Width(2, (_lib.GS_KEY_U16, _lib.GS_KEY_I16, _lib.GS_KEY_F16, _lib.GS_KEY_BF16), "GS_KEY_U16 / I16 / F16 / BF16",
              "int16, uint16, float16, bfloat16", True)
_W32 = _Width(4, (_lib.GS_KEY_U32, _lib.GS_KEY_I32, _lib.GS_KEY_F32), "GS_KEY_U32 / I32 / F32", "int32, float32, uint32", False)
_W64 = _Width(8, (_lib.GS_KEY_U64, _lib.GS_KEY_I64, _lib.GS_KEY_F64), "GS_KEY_U64 / I64 / F64", "int64, float64, uint64", True)


def _key_type_of(t, key_type, w, who):
    """The key type of a call at width `w`: the explicit one, or the category of the tensor's dtype."""
    if key_type is not None:
        return key_type
    key_type = _KEY_TYPES.get(t.dtype, None if w.strict else _lib.GS_KEY_U32)
    if key_type not in w.key_types:
        raise TypeError(f"{who}: no {8 * w.elem}-bit key category for {t.dtype} ({w.dtypes}, or {w.names} by key_type)")
    return key_type


def _eight_words(name, *args, stream=()):
    """A plan or status function of the library: eight u32 behind `args` (and in front of the stream, where it takes one)."""
    out = (C.c_uint32 * 8)()
    check(getattr(lib, name)(*args, out, *stream), name)
    return [int(x) for x in out]


class _Front:
    """What the call shapes share: the entry points by key width, the choice among them, and the key checks."""

    _entries = {}      # {width: (entry point, its size query)}

    @classmethod
    def _accepts(cls):
        """The keys the class takes, for the messages of the convenience forms: (which widths, which dtypes in brackets)."""
        w = next(iter(cls._entries))
        return (f"{8 * w.elem}-bit keys", f" ({w.dtypes})") if len(cls._entries) == 1 else ("32-bit or 16-bit keys", "")

    @classmethod
    def _query(cls, d_temp_storage, d_keys_in, key_type, *shape):
        """(width, entry point, the answer of its size query for `shape`).  A class of one width has no choice.  The others
        take 16 or 32 bits from key_type when it is given, answer a size query without one for 32 bits (it sees no tensor, and
        that answer is never the smaller one), and otherwise go by the tensor's element size."""
        if len(cls._entries) == 1:
            w = next(iter(cls._entries))
        elif d_temp_storage is None or key_type is not None:
            w = _W16 if key_type in _W16.key_types else _W32
        else:
            w = _W16 if isinstance(d_keys_in, torch.Tensor) and d_keys_in.element_size() == 2 else _W32
        if key_type is not None and w.strict and key_type not in w.key_types:
            raise TypeError(f"{cls.__name__}: key_type must be {w.names}")
        entry, size_query = cls._entries[w]
        return w, entry, getattr(lib, size_query)(*shape)

    @classmethod
    def _keys(cls, w, d_keys_in, key_type):
        """The key type of a call that goes on behind the size query: the key tensor must have the width chosen."""
        if not isinstance(d_keys_in, torch.Tensor) or d_keys_in.element_size() != w.elem:
            only = f"{8 * w.elem}-bit keys only" if len(cls._entries) == 1 else "32-bit keys, or 2-byte keys with a 16-bit key type"
            raise TypeError(f"{cls.__name__}: {only}")
        return _key_type_of(d_keys_in, key_type, w, cls.__name__)


class DeviceTopK(_Front):
    """MinKeys / MaxKeys / MinPairs / MaxPairs: the k smallest (largest) keys, sorted, with their values.

    d_values_in=None in the pairs forms writes the elements' input indices (u32 bit patterns in d_values_out): an argsort of
    the top k.  The inputs are never written; d_keys_out / d_values_out need k elements and must not overlap anything."""

    _entries = {_W32: ("gs_topk_u32", "gs_topk_temp_bytes")}
    _status = "gs_topk_status"

    @classmethod
    def _run(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_items, k, descending,
             has_values, stream, key_type):
        w, entry, need = cls._query(d_temp_storage, d_keys_in, key_type, num_items, k, int(has_values))
        if d_temp_storage is None:
            return need
        key_type = cls._keys(w, d_keys_in, key_type)
        _check_buf(d_keys_in, num_items, "d_keys_in", w.elem)
        _check_buf(d_keys_out, k, "d_keys_out", w.elem)
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
        return _eight_words(cls._status, C.c_void_p(d_temp_storage.data_ptr()), num_items, k, int(has_values),
                            stream=(_stream_ptr(stream),))


class DeviceTopK16(DeviceTopK):
    """DeviceTopK for a flat array of 16-bit keys (gs_topk_u16): MinKeys / MaxKeys / MinPairs / MaxPairs / Status.

    The key type comes from the tensor's dtype (int16, uint16, float16, bfloat16) or from an explicit 16-bit key_type; the
    result is the first k of DeviceRadixSort on the same keys, in the order of GS_KEY_F16 / BF16 at the enum for the float
    types.  Values and indices are 4 bytes, as in DeviceTopK.  Keys of any other width raise TypeError."""

    _entries = {_W16: ("gs_topk_u16", "gs_topk_u16_temp_bytes")}
    _status = "gs_topk_u16_status"


class DeviceTopK64(DeviceTopK):
    """DeviceTopK for a flat array of 64-bit keys (gs_topk_u64): MinKeys / MaxKeys / MinPairs / MaxPairs / Status.

    The key type comes from the tensor's dtype (int64, float64, uint64) or from an explicit 64-bit key_type; the result is the
    first k of DeviceRadixSort on the same keys, float64 in the order of GS_KEY_F32 at the enum.  Values and indices are 4
    bytes, as in DeviceTopK.  Status() is [route, low and high word of the k-th image, elements before it, taken from its tie
    run, D, passes over the input, elements of the bucket or tie run].  Keys of any other width raise TypeError."""

    _entries = {_W64: ("gs_topk_u64", "gs_topk_u64_temp_bytes")}
    _status = "gs_topk_u64_status"


def _outputs(shape, keys, values, indices):
    """(has_values, keys_out, values_out) of a convenience form: values_out in the values' dtype, int32 for indices, or None."""
    has_values = values is not None or indices
    keys_out = torch.empty(shape, dtype=keys.dtype, device=keys.device)
    values_dtype = values.dtype if values is not None else torch.int32
    return has_values, keys_out, torch.empty(shape, dtype=values_dtype, device=keys.device) if has_values else None


def _workspace(nbytes, device, stream):
    temp = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if stream is not None:
        temp.record_stream(stream)   # the workspace is freed on return: keep it until the stream has used it
    return temp


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
    has_values, keys_out, values_out = _outputs(k, keys, values, indices)
    front = {2: DeviceTopK16, 8: DeviceTopK64}.get(keys.element_size(), DeviceTopK)
    w = next(iter(front._entries))
    if w.strict:
        _key_type_of(keys, None, w, "topk")
    if k == 0:
        return keys_out, values_out
    nbytes = front._run(None, 0, None, None, None, None, n, k, largest, has_values, stream, None)
    temp = _workspace(nbytes, keys.device, stream)
    front._run(temp, nbytes, keys, keys_out, values, values_out, n, k, largest, has_values, stream, None)
    return keys_out, values_out


def _check_rows_in(t, what, elem=4):
    """An input matrix: a device tensor of `elem`-byte elements whose data_ptr() is row 0 (it may be a strided view, so its
    extent is the caller's statement: (num_rows - 1) * row_stride + num_cols elements)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.element_size() != elem:
        raise ValueError(f"{what}: expected a device tensor of {elem}-byte elements")


class _TopKRows(_Front):
    """The rows shape: the call and its four forms, for the classes that state the entry points."""

    @classmethod
    def _run(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols, row_stride,
             k, descending, has_values, stream, key_type):
        w, entry, need = cls._query(d_temp_storage, d_keys_in, key_type, num_rows, num_cols, k, int(has_values))
        if d_temp_storage is None:
            return need
        key_type = cls._keys(w, d_keys_in, key_type)
        _check_rows_in(d_keys_in, "d_keys_in", w.elem)
        _check_buf(d_keys_out, num_rows * k, "d_keys_out", w.elem)
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

    @classmethod
    def MinKeys(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_rows, num_cols, row_stride, k, stream=None,
                key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_rows, num_cols, row_stride, k,
                        False, False, stream, key_type)

    @classmethod
    def MaxKeys(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, num_rows, num_cols, row_stride, k, stream=None,
                key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, num_rows, num_cols, row_stride, k,
                        True, False, stream, key_type)

    @classmethod
    def MinPairs(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                 row_stride, k, stream=None, key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                        row_stride, k, False, True, stream, key_type)

    @classmethod
    def MaxPairs(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                 row_stride, k, stream=None, key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, num_rows, num_cols,
                        row_stride, k, True, True, stream, key_type)


class DeviceTopKRows(_TopKRows):
    """MinKeys / MaxKeys / MinPairs / MaxPairs for every row of a matrix: row r is d_keys_in[r * row_stride .. + num_cols)
    (flat element offsets), and its k smallest (largest), sorted, go to d_keys_out[r * k .. + k) with their values.

    d_values_in=None in the pairs forms writes the elements' column indices (u32 bit patterns).  Each row's result is what
    DeviceTopK gives for that row alone.  The size query is 0 for a shape the entry point refuses (k > MaxK(), ...).

    2-byte key tensors (int16, uint16, float16, bfloat16, or an explicit 16-bit key_type) go to gs_topk_rows_u16: the same
    definition on the 16-bit image, values still 4 bytes.  The size query (d_temp_storage=None) sees no tensor: with a 16-bit
    key_type it answers for gs_topk_rows_u16, without one for gs_topk_rows_u32, which is never the smaller of the two."""

    _entries = {_W32: ("gs_topk_rows_u32", "gs_topk_rows_temp_bytes"), _W16: ("gs_topk_rows_u16", "gs_topk_rows_u16_temp_bytes")}

    @staticmethod
    def MaxK():
        return int(lib.gs_topk_rows_max_k())

    @staticmethod
    def Plan(num_rows, num_cols, k, has_values=False):
        """gs_topk_rows_plan: [path, select levels, CH, chunks per row at level 0, candidates per row after level 0, max k,
        0, 0]; a pure host function.  Raises for a refused shape."""
        return _eight_words("gs_topk_rows_plan", num_rows, num_cols, k, int(has_values))


class DeviceTopKRows64(DeviceTopKRows):
    """DeviceTopKRows for a matrix of 64-bit keys (gs_topk_rows_u64): MinKeys / MaxKeys / MinPairs / MaxPairs / MaxK / Plan.

    The key type comes from the tensor's dtype (int64, float64, uint64) or from an explicit GS_KEY_U64 / I64 / F64; each row's
    result is what DeviceTopK64 gives for that row alone, float64 in the order of GS_KEY_F32 at the enum.  Values and column
    indices are 4 bytes.  Two-phase: d_temp_storage=None returns the size, 0 for a shape the entry point refuses.  Keys of
    any other width and any other key_type raise TypeError.  The geometry is DeviceTopKRows': Plan() is the same answer."""

    _entries = {_W64: ("gs_topk_rows_u64", "gs_topk_rows_u64_temp_bytes")}


class DeviceTopKRowsAnyK(_TopKRows):
    """DeviceTopKRows without the cap at MaxK() (gs_topk_rows_anyk_u32): MinKeys / MaxKeys / MinPairs / MaxPairs / Plan / Status
    for 32-bit keys and any 1 <= k <= num_cols.

    Each row's result is what DeviceTopK gives for that row alone; for k <= DeviceTopKRows.MaxK() it is DeviceTopKRows' result,
    and that class remains the faster one there.  Two-phase: d_temp_storage=None returns the size, 0 for a shape the entry
    point refuses (k > num_cols, num_rows * k >= 2^31, ...).  Keys of any other width raise TypeError."""

    _entries = {_W32: ("gs_topk_rows_anyk_u32", "gs_topk_rows_anyk_temp_bytes")}
    _plan, _status = "gs_topk_rows_anyk_plan", "gs_topk_rows_anyk_status"

    @classmethod
    def Plan(cls, num_rows, num_cols, k, has_values=False):
        """gs_topk_rows_anyk_plan: [path, kernel launches before the finish, CH, tile, tiles per slab, slabs per row, tiles per
        row, 0]; a pure host function.  Raises for a refused shape."""
        return _eight_words(cls._plan, num_rows, num_cols, k, int(has_values))

    @classmethod
    def Status(cls, d_temp_storage, num_rows, num_cols, k, has_values, row, stream=None):
        """gs_topk_rows_anyk_status: [path, image of row `row`'s k-th element, elements before it, taken from its tie run,
        elements that matched the prefix after round one, after round two, 0, 0] of the last call on d_temp_storage.
        Synchronises the stream."""
        return _eight_words(cls._status, C.c_void_p(d_temp_storage.data_ptr()), num_rows, num_cols, k, int(has_values), row,
                            stream=(_stream_ptr(stream),))


class DeviceTopKRowsAnyK16(DeviceTopKRowsAnyK):
    """DeviceTopKRowsAnyK for a matrix of 16-bit keys (gs_topk_rows_anyk_u16): MinKeys / MaxKeys / MinPairs / MaxPairs / Plan /
    Status for any 1 <= k <= num_cols.

    The key type comes from the tensor's dtype (int16, uint16, float16, bfloat16) or from an explicit 16-bit key_type; each
    row's result is what DeviceTopK16 gives for that row alone, and for k <= DeviceTopKRows.MaxK() it is DeviceTopKRows' result
    on the same keys, that class remaining the faster one there.  Values and column indices are 4 bytes.  Plan() is
    gs_topk_rows_anyk_u16_plan (two counting rounds: 9 launches before the finish on path 2, the geometry words those of
    DeviceTopKRowsAnyK), Status() gs_topk_rows_anyk_u16_status: [path, 16-bit image of the k-th element, elements before it,
    taken from its tie run, elements sharing its top byte, 0, 0, 0].  Keys of any other width and any other key_type raise
    TypeError."""

    _entries = {_W16: ("gs_topk_rows_anyk_u16", "gs_topk_rows_anyk_u16_temp_bytes")}
    _plan, _status = "gs_topk_rows_anyk_u16_plan", "gs_topk_rows_anyk_u16_status"


class DeviceTopKRowsAnyK64(DeviceTopKRowsAnyK):
    """DeviceTopKRowsAnyK for a matrix of 64-bit keys (gs_topk_rows_anyk_u64): MinKeys / MaxKeys / MinPairs / MaxPairs / Plan /
    Status for any 1 <= k <= num_cols.

    The key type comes from the tensor's dtype (int64, float64, uint64) or from an explicit GS_KEY_U64 / I64 / F64; each row's
    result is what DeviceTopK64 gives for that row alone, float64 in the order of GS_KEY_F32 at the enum, and for
    k <= DeviceTopKRows64.MaxK() it is DeviceTopKRows64's result, that class remaining the faster one there.  Values and column
    indices are 4 bytes.  Keys of any other width and any other key_type raise TypeError."""

    _entries = {_W64: ("gs_topk_rows_anyk_u64", "gs_topk_rows_anyk_u64_temp_bytes")}
    _plan, _status = "gs_topk_rows_anyk_u64_plan", "gs_topk_rows_anyk_u64_status"

    @classmethod
    def Plan(cls, num_rows, num_cols, k, has_values=False):
        """gs_topk_rows_anyk_u64_plan: [path, kernel launches before the finish (2 on path 1, 19 on path 2), CH, tile, tiles
        per slab, slabs per row, tiles per row, L: the capacity of a row's list (0 on path 1)]; a pure host function.  Raises
        for a refused shape."""
        return _eight_words(cls._plan, num_rows, num_cols, k, int(has_values))

    @classmethod
    def Status(cls, d_temp_storage, num_rows, num_cols, k, has_values, row, stream=None):
        """gs_topk_rows_anyk_u64_status: [path, low word of the image of row `row`'s k-th element, its high word, elements
        before it, taken from its tie run, D: the counting rounds the row took (0 on path 1), how its descent ended (0 path 1,
        1 from the row's list, 2 a tie run), elements put on the list (0 otherwise)] of the last call on d_temp_storage.
        Synchronises the stream."""
        return _eight_words(cls._status, C.c_void_p(d_temp_storage.data_ptr()), num_rows, num_cols, k, int(has_values), row,
                            stream=(_stream_ptr(stream),))


def _rows_call(who, front, keys, k, values, indices, stream):
    """The argument checks of the topk_rows*() forms, in the name of `who`, the [rows, k] outputs and the answer of `front`'s
    size query (None where k or the number of rows is 0 and the outputs are the whole result), as (key_type, rows, cols,
    stride, has_values, keys_out, values_out, nbytes)."""
    if values is not None and indices:
        raise ValueError(f"{who}: give values or indices=True, not both")
    if keys.dim() != 2:
        raise ValueError("%s: a 2-D tensor, not %d-D" % (who, keys.dim()))
    rows, cols = keys.shape
    if cols > 1 and keys.stride(1) != 1:
        raise ValueError(f"{who}: the last dimension must be contiguous")
    if not 0 <= k <= cols:
        raise ValueError(f"{who}: need 0 <= k <= {cols}")
    stride = keys.stride(0) if rows > 1 else cols
    if rows > 1 and stride < cols:
        raise ValueError("%s: rows overlap (stride %d < %d columns)" % (who, stride, cols))
    if values is not None and (values.shape != keys.shape or values.element_size() != 4 or
                               (cols > 1 and values.stride(1) != 1) or (rows > 1 and values.stride(0) != stride)):
        raise ValueError(f"{who}: values must have the keys' shape and strides and 4-byte elements")
    w = next((w for w in front._entries if w.elem == keys.element_size()), None)
    if w is None:
        raise TypeError("%s: %s only%s" % ((who,) + front._accepts()))
    key_type = _key_type_of(keys, None, w, who)
    if w is _W16 and hasattr(front, "MaxK") and k > lib.gs_topk_rows_max_k():   # (a front without a cap takes any k)
        raise ValueError("%s: 16-bit keys need k <= %d; topk_rows_anyk16() serves more" % (who, lib.gs_topk_rows_max_k()))
    has_values, keys_out, values_out = _outputs((rows, k), keys, values, indices)
    nbytes = None
    if k != 0 and rows != 0:
        nbytes = front._run(None, 0, None, None, None, None, rows, cols, stride, k, False, has_values, stream, key_type)
    return key_type, rows, cols, stride, has_values, keys_out, values_out, nbytes


def _topk_rows(who, front, flat, keys, k, largest, values, indices, stream):
    """topk_rows() and topk_rows64(): `front` in one call, or, for a k above its MaxK(), `flat` row by row."""
    key_type, rows, cols, stride, has_values, keys_out, values_out, nbytes = _rows_call(who, front, keys, k, values, indices, stream)
    if nbytes is None:
        return keys_out, values_out
    if nbytes == 0 and k > lib.gs_topk_rows_max_k() and rows * stride < (1 << 32) and rows * k < (1 << 32):
        # refused for k alone: the flat top k of every row, one call each on one workspace
        nbytes = flat._run(None, 0, None, None, None, None, cols, k, largest, has_values, stream, key_type)
        temp = _workspace(nbytes, keys.device, stream)
        for r in range(rows):
            flat._run(temp, nbytes, keys[r], keys_out[r], None if values is None else values[r],
                      values_out[r] if has_values else None, cols, k, largest, has_values, stream, key_type)
        return keys_out, values_out
    if nbytes == 0:
        raise ValueError(f"{who}: the entry point refuses this shape (rows * stride and rows * k must be below 2^32)")
    temp = _workspace(nbytes, keys.device, stream)
    front._run(temp, nbytes, keys, keys_out, values, values_out, rows, cols, stride, k, largest, has_values, stream, key_type)
    return keys_out, values_out


def topk_rows(keys, k, largest=False, values=None, indices=False, stream=None):
    """The k smallest (largest=True: largest) of every row of the 2-D tensor `keys`, sorted, as (keys_out, values_out) of shape
    [rows, k].

    The last dimension must be contiguous; the rows may sit at any stride >= cols (a column slice of a wider matrix).
    values: a 4-byte tensor of the same shape and strides, carried with the keys.  indices=True (without values): values_out
    holds the column indices as int32 bit patterns of u32.  Neither: values_out is None.  Allocates outputs and workspace.
    A k above DeviceTopKRows.MaxK() is served by gs_topk_u32 row by row.  2-byte keys (int16, uint16, float16, bfloat16) take
    gs_topk_rows_u16; for them a k above MaxK() raises ValueError: such callers use topk_rows_anyk16()."""
    return _topk_rows("topk_rows", DeviceTopKRows, DeviceTopK, keys, k, largest, values, indices, stream)


def topk_rows64(keys, k, largest=False, values=None, indices=False, stream=None):
    """topk_rows() for a 2-D tensor of 8-byte keys (int64, float64, uint64): the k smallest (largest=True: largest) of every row,
    sorted, as (keys_out, values_out) of shape [rows, k], through gs_topk_rows_u64.

    The checks and the return shapes are topk_rows()': the last dimension contiguous, rows at any stride >= cols, values a
    4-byte tensor of the same shape and strides, indices=True for the column indices as int32 bit patterns of u32.  A k above
    DeviceTopKRows64.MaxK() is served by gs_topk_u64 row by row on one workspace.  Any other key width raises TypeError."""
    return _topk_rows("topk_rows64", DeviceTopKRows64, DeviceTopK64, keys, k, largest, values, indices, stream)


def topk_rows_anyk(keys, k, largest=False, values=None, indices=False, stream=None):
    """topk_rows() for any 0 <= k <= cols in one batched call (gs_topk_rows_anyk_u32): the k smallest (largest=True: largest)
    of every row of the 2-D tensor `keys` of 4-byte elements, sorted, as (keys_out, values_out) of shape [rows, k].

    The checks and the return shapes are topk_rows()': the last dimension contiguous, rows at any stride >= cols, values a
    4-byte tensor of the same shape and strides, indices=True for the column indices as int32 bit patterns of u32.  Any other
    key width raises TypeError.  For k <= DeviceTopKRows.MaxK() topk_rows() gives the same result faster."""
    return _topk_rows_anyk("topk_rows_anyk", DeviceTopKRowsAnyK, keys, k, largest, values, indices, stream)


def topk_rows_anyk16(keys, k, largest=False, values=None, indices=False, stream=None):
    """topk_rows_anyk() for a 2-D tensor of 2-byte keys (int16, uint16, float16, bfloat16): the k smallest (largest=True:
    largest) of every row for any 0 <= k <= cols in one batched call, sorted, as (keys_out, values_out) of shape [rows, k],
    through gs_topk_rows_anyk_u16.

    The checks and the return shapes are topk_rows()': the last dimension contiguous, rows at any stride >= cols, values a
    4-byte tensor of the same shape and strides, indices=True for the column indices as int32 bit patterns of u32.  The keys
    come back in the input dtype, float16 / bfloat16 in the order of GS_KEY_F16 / BF16 at the enum.  Any other key width raises
    TypeError.  For k <= DeviceTopKRows.MaxK() topk_rows() gives the same result faster."""
    return _topk_rows_anyk("topk_rows_anyk16", DeviceTopKRowsAnyK16, keys, k, largest, values, indices, stream)


def topk_rows_anyk64(keys, k, largest=False, values=None, indices=False, stream=None):
    """topk_rows_anyk() for a 2-D tensor of 8-byte keys (int64, float64, uint64): the k smallest (largest=True: largest) of
    every row for any 0 <= k <= cols in one batched call, sorted, as (keys_out, values_out) of shape [rows, k], through
    gs_topk_rows_anyk_u64.

    The checks and the return shapes are topk_rows()': the last dimension contiguous, rows at any stride >= cols, values a
    4-byte tensor of the same shape and strides, indices=True for the column indices as int32 bit patterns of u32.  float64 is
    in the order of GS_KEY_F32 at the enum.  Any other key width raises TypeError.  For k <= DeviceTopKRows64.MaxK()
    topk_rows64() gives the same result faster."""
    return _topk_rows_anyk("topk_rows_anyk64", DeviceTopKRowsAnyK64, keys, k, largest, values, indices, stream)


def _topk_rows_anyk(who, front, keys, k, largest, values, indices, stream):
    """topk_rows_anyk(), topk_rows_anyk16() and topk_rows_anyk64(): the argument checks in the name of `who`, the outputs, and `front`'s call."""
    key_type, rows, cols, stride, has_values, keys_out, values_out, nbytes = _rows_call(who, front, keys, k, values, indices, stream)
    if nbytes is None:
        return keys_out, values_out
    if nbytes == 0 or rows * stride >= (1 << 32):
        raise ValueError(f"{who}: the entry point refuses this shape (rows * stride below 2^32, rows * k below 2^31)")
    temp = _workspace(nbytes, keys.device, stream)
    front._run(temp, nbytes, keys, keys_out, values, values_out, rows, cols, stride, k, largest, has_values, stream, key_type)
    return keys_out, values_out


class _TopKSegmented(_Front):
    """The ragged shape: the call and its four forms, for the classes that state the entry points."""

    @classmethod
    def _run(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
             num_segments, d_begin_offsets, d_end_offsets, k, descending, has_values, stream, key_type):
        w, entry, need = cls._query(d_temp_storage, d_keys_in, key_type, num_items, num_segments, k, int(has_values))
        if d_temp_storage is None:
            return need
        key_type = cls._keys(w, d_keys_in, key_type)
        _check_buf(d_keys_in, num_items, "d_keys_in", w.elem)
        _check_buf(d_keys_out, num_segments * k, "d_keys_out", w.elem)
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

    @classmethod
    def MinKeys(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_counts_out, num_items, num_segments, d_begin_offsets,
                d_end_offsets, k, stream=None, key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, d_counts_out, num_items, num_segments,
                        d_begin_offsets, d_end_offsets, k, False, False, stream, key_type)

    @classmethod
    def MaxKeys(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_counts_out, num_items, num_segments, d_begin_offsets,
                d_end_offsets, k, stream=None, key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, None, None, d_counts_out, num_items, num_segments,
                        d_begin_offsets, d_end_offsets, k, True, False, stream, key_type)

    @classmethod
    def MinPairs(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
                 num_segments, d_begin_offsets, d_end_offsets, k, stream=None, key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
                        num_segments, d_begin_offsets, d_end_offsets, k, False, True, stream, key_type)

    @classmethod
    def MaxPairs(cls, d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
                 num_segments, d_begin_offsets, d_end_offsets, k, stream=None, key_type=None):
        return cls._run(d_temp_storage, temp_storage_bytes, d_keys_in, d_keys_out, d_values_in, d_values_out, d_counts_out, num_items,
                        num_segments, d_begin_offsets, d_end_offsets, k, True, True, stream, key_type)


class DeviceTopKSegmented(_TopKSegmented):
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

    _entries = {_W32: ("gs_topk_segmented_u32", "gs_topk_segmented_temp_bytes"),
                _W16: ("gs_topk_segmented_u16", "gs_topk_segmented_u16_temp_bytes")}

    MaxK = staticmethod(DeviceTopKRows.MaxK)

    @staticmethod
    def Plan(num_items, num_segments, k, has_values=False):
        """gs_topk_segmented_plan: [launch groups (bit 0 wave, 1 workgroup, 2 long), kernel launches, CH, Lmax, Tmax, max k, 0,
        0]; a pure host function.  Raises for a refused shape."""
        return _eight_words("gs_topk_segmented_plan", num_items, num_segments, k, int(has_values))

    @staticmethod
    def Status(d_temp_storage, num_items, num_segments, k, has_values, stream=None):
        """gs_topk_segmented_status: [segments in the four wave lists, the workgroup list, the long list, chunk tasks, dropped
        segments] of the last call on d_temp_storage.  Synchronises the stream."""
        return _eight_words("gs_topk_segmented_status", C.c_void_p(d_temp_storage.data_ptr()), num_items, num_segments, k,
                            int(has_values), stream=(_stream_ptr(stream),))


class DeviceTopKSegmented64(DeviceTopKSegmented):
    """DeviceTopKSegmented for a flat array of 64-bit keys (gs_topk_segmented_u64): MinKeys / MaxKeys / MinPairs / MaxPairs /
    MaxK / Plan / Status.

    The key type comes from the tensor's dtype (int64, float64, uint64) or from an explicit GS_KEY_U64 / I64 / F64; each
    segment's result is what DeviceTopK64 gives for that segment alone, float64 in the order of GS_KEY_F32 at the enum.
    Values, positions, counts and offsets are 4 bytes.  Two-phase: d_temp_storage=None returns the size, 0 for a shape the
    entry point refuses.  Keys of any other width and any other key_type raise TypeError.  The geometry is
    DeviceTopKSegmented's: Plan() is the same answer, and Status() reads a workspace of either class."""

    _entries = {_W64: ("gs_topk_segmented_u64", "gs_topk_segmented_u64_temp_bytes")}


class DeviceTopKSegmentedAnyK(_TopKSegmented):
    """DeviceTopKSegmented without the cap at MaxK() (gs_topk_segmented_anyk_u32): MinKeys / MaxKeys / MinPairs / MaxPairs /
    Plan / Status for 32-bit keys and any k >= 1, which may exceed every segment's length.

    Each segment's result is what DeviceTopK gives for that segment alone at min(k, length); for k <= DeviceTopKSegmented.MaxK()
    it is DeviceTopKSegmented's result.  d_counts_out[s] (may be None) gets min(k, length), and the slots behind it are not
    written.  Two-phase: d_temp_storage=None returns the size, 0 for a shape the entry point refuses (num_items >= 2^31,
    num_segments * k >= 2^31).  Keys of any other width raise TypeError."""

    _entries = {_W32: ("gs_topk_segmented_anyk_u32", "gs_topk_segmented_anyk_temp_bytes")}

    @staticmethod
    def Plan(num_items, num_segments, k, has_values=False):
        """gs_topk_segmented_anyk_plan: [launch groups (bit 0 wave, 1 workgroup, 2 long), kernel launches before the finish, CH,
        tile, tiles per slab, Lmax, Tmax, 0]; a pure host function.  Raises for a refused shape."""
        return _eight_words("gs_topk_segmented_anyk_plan", num_items, num_segments, k, int(has_values))

    @staticmethod
    def Status(d_temp_storage, num_items, num_segments, k, has_values, stream=None):
        """gs_topk_segmented_anyk_status: [segments in the four wave lists, the workgroup list, the long list, tile tasks,
        dropped segments] of the last call on d_temp_storage.  Synchronises the stream."""
        return _eight_words("gs_topk_segmented_anyk_status", C.c_void_p(d_temp_storage.data_ptr()), num_items, num_segments, k,
                            int(has_values), stream=(_stream_ptr(stream),))


def _topk_segmented(who, front, keys, offsets, k, largest, values, indices, stream, end_offsets):
    """topk_segmented(), topk_segmented64() and topk_segmented_anyk(): the argument checks in the name of `who`, the outputs, and `front`'s call."""
    if values is not None and indices:
        raise ValueError(f"{who}: give values or indices=True, not both")
    w = next((w for w in front._entries if w.elem == keys.element_size()), None)
    if keys.dim() != 1 or w is None:
        raise TypeError("%s: a 1-D tensor of %s%s" % ((who,) + front._accepts()))
    key_type = _key_type_of(keys, None, w, who)
    if offsets.dtype != torch.int32 or (end_offsets is not None and end_offsets.dtype != torch.int32):
        raise TypeError(f"{who}: int32 offsets")
    if end_offsets is None:
        if offsets.numel() < 1:
            raise ValueError(f"{who}: offsets needs S + 1 elements")
        begins, ends, segs = offsets[:-1], offsets[1:], offsets.numel() - 1
    else:
        if end_offsets.numel() != offsets.numel():
            raise ValueError(f"{who}: as many ends as begins")
        begins, ends, segs = offsets, end_offsets, offsets.numel()
    n = keys.numel()
    if k < 0:
        raise ValueError(f"{who}: need k >= 0")
    if values is not None and (values.numel() != n or values.element_size() != 4 or values.dim() != 1):
        raise ValueError(f"{who}: values must have the keys' length and 4-byte elements")
    has_values, keys_out, values_out = _outputs((segs, k), keys, values, indices)
    counts = torch.zeros(segs, dtype=torch.int32, device=keys.device)
    if k == 0 or segs == 0 or n == 0:
        return keys_out, values_out, counts
    nbytes = front._run(None, 0, None, None, None, None, None, n, segs, None, None, k, largest, has_values, stream, key_type)
    if nbytes == 0 and not hasattr(front, "MaxK"):   # (a front without a cap takes any k)
        raise ValueError(f"{who}: the entry point refuses this shape (fewer than 2^31 keys, segments * k below 2^31)")
    if nbytes == 0:
        raise ValueError("%s: the entry point refuses this shape (k <= %d, fewer than 2^31 keys, segments * k below 2^32)"
                         % (who, lib.gs_topk_rows_max_k()))
    temp = _workspace(nbytes, keys.device, stream)
    front._run(temp, nbytes, keys.contiguous(), keys_out, values, values_out, counts, n, segs, begins, ends, k, largest, has_values,
               stream, key_type)
    return keys_out, values_out, counts


def topk_segmented(keys, offsets, k, largest=False, values=None, indices=False, stream=None, end_offsets=None):
    """The k smallest (largest=True: largest) of every segment of the 1-D tensor `keys`, sorted, as (keys_out [S, k],
    values_out [S, k] or None, counts [S] int32).

    offsets: an int32 device tensor of S + 1 elements, segment s being keys[offsets[s] : offsets[s + 1]]; or, with end_offsets
    given, the S begins, segment s being keys[offsets[s] : end_offsets[s]] (any order, gaps, repeats; see gs_topk_segmented_u32
    for overlaps).  counts[s] = min(k, length of segment s); the slots of row s past counts[s] are unspecified.
    values: a 4-byte tensor of the keys' length, carried with the keys.  indices=True (without values): values_out holds the
    positions within the segment as int32 bit patterns of u32.  Neither: values_out is None.  Allocates outputs and workspace.
    2-byte keys (int16, uint16, float16, bfloat16) take gs_topk_segmented_u16 and come back in the input dtype."""
    return _topk_segmented("topk_segmented", DeviceTopKSegmented, keys, offsets, k, largest, values, indices, stream, end_offsets)


def topk_segmented64(keys, offsets, k, largest=False, values=None, indices=False, stream=None, end_offsets=None):
    """topk_segmented() for a 1-D tensor of 8-byte keys (int64, float64, uint64): the k smallest (largest=True: largest) of
    every segment, sorted, as (keys_out [S, k], values_out [S, k] or None, counts [S] int32), through gs_topk_segmented_u64.

    The arguments, the checks and the return shapes are topk_segmented()'s: int32 device offsets of S + 1 elements, or begins
    and end_offsets; values a 4-byte tensor of the keys' length; indices=True for the positions within the segment as int32
    bit patterns of u32.  The keys come back in the input dtype.  Any other key width raises TypeError."""
    return _topk_segmented("topk_segmented64", DeviceTopKSegmented64, keys, offsets, k, largest, values, indices, stream, end_offsets)


def topk_segmented_anyk(keys, offsets, k, largest=False, values=None, indices=False, stream=None, end_offsets=None):
    """topk_segmented() for any k >= 0 in one call (gs_topk_segmented_anyk_u32): the k smallest (largest=True: largest) of every
    segment of the 1-D tensor `keys` of 4-byte elements, sorted, as (keys_out [S, k], values_out [S, k] or None, counts [S]
    int32).  k may exceed every segment's length: counts[s] = min(k, length of segment s), and the slots of row s past
    counts[s] are unspecified.

    The arguments, the checks and the return shapes are topk_segmented()'s: int32 device offsets of S + 1 elements, or begins
    and end_offsets; values a 4-byte tensor of the keys' length; indices=True for the positions within the segment as int32
    bit patterns of u32.  2- and 8-byte keys raise TypeError."""
    return _topk_segmented("topk_segmented_anyk", DeviceTopKSegmentedAnyK, keys, offsets, k, largest, values, indices, stream,
                           end_offsets)
