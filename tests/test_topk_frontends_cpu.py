"""The top-k front ends of gpu_sort_amd.select as keyword callers see them, without a device: every public callable keeps its
parameter names and defaults, every class its set of public attributes, and every form of every class answers the size query
(d_temp_storage=None, no tensors) with its width's gs_*_temp_bytes.  The names and defaults are written out here, not read
from the module."""
import inspect

import pytest

ROWS, COLS, K = 40, 30000, 200

_CONV = "keys k largest=False values=None indices=False stream=None"
FUNCTIONS = {
    "topk": _CONV,
    "topk_rows": _CONV,
    "topk_rows64": _CONV,
    "topk_rows_anyk": _CONV,
    "topk_segmented": "keys offsets k largest=False values=None indices=False stream=None end_offsets=None",
    "topk_segmented64": "keys offsets k largest=False values=None indices=False stream=None end_offsets=None",
}

_FLAT = {
    "MinKeys": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out num_items k stream=None key_type=None",
    "MaxKeys": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out num_items k stream=None key_type=None",
    "MinPairs": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out d_values_in d_values_out num_items k stream=None key_type=None",
    "MaxPairs": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out d_values_in d_values_out num_items k stream=None key_type=None",
    "Status": "d_temp_storage num_items k has_values stream=None",
}
_ROWS = {
    "MinKeys": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out num_rows num_cols row_stride k stream=None key_type=None",
    "MaxKeys": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out num_rows num_cols row_stride k stream=None key_type=None",
    "MinPairs": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out d_values_in d_values_out num_rows num_cols row_stride k "
                "stream=None key_type=None",
    "MaxPairs": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out d_values_in d_values_out num_rows num_cols row_stride k "
                "stream=None key_type=None",
    "Plan": "num_rows num_cols k has_values=False",
}
_ROWS_CAPPED = dict(_ROWS, MaxK="")
_ROWS_ANYK = dict(_ROWS, Status="d_temp_storage num_rows num_cols k has_values row stream=None")
_SEG = {
    "MinKeys": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out d_counts_out num_items num_segments d_begin_offsets "
               "d_end_offsets k stream=None key_type=None",
    "MaxKeys": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out d_counts_out num_items num_segments d_begin_offsets "
               "d_end_offsets k stream=None key_type=None",
    "MinPairs": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out d_values_in d_values_out d_counts_out num_items num_segments "
                "d_begin_offsets d_end_offsets k stream=None key_type=None",
    "MaxPairs": "d_temp_storage temp_storage_bytes d_keys_in d_keys_out d_values_in d_values_out d_counts_out num_items num_segments "
                "d_begin_offsets d_end_offsets k stream=None key_type=None",
    "MaxK": "",
    "Plan": "num_items num_segments k has_values=False",
    "Status": "d_temp_storage num_items num_segments k has_values stream=None",
}
CLASSES = {
    "DeviceTopK": _FLAT,
    "DeviceTopK16": _FLAT,
    "DeviceTopK64": _FLAT,
    "DeviceTopKRows": _ROWS_CAPPED,
    "DeviceTopKRows64": _ROWS_CAPPED,
    "DeviceTopKRowsAnyK": _ROWS_ANYK,
    "DeviceTopKSegmented": _SEG,
    "DeviceTopKSegmented64": _SEG,
}


def _written(text):
    """'a b=None c=False' as [(name, default)], inspect.Parameter.empty for none."""
    out = []
    for word in text.split():
        name, _, default = word.partition("=")
        out.append((name, {"": inspect.Parameter.empty, "None": None, "False": False}[default]))
    return out


def _found(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


@pytest.mark.parametrize("name", sorted(FUNCTIONS))
def test_function_keeps_its_parameters(gs, name):
    assert name in gs.__all__
    assert _found(getattr(gs, name)) == _written(FUNCTIONS[name])


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_class_keeps_its_public_attributes_and_their_parameters(gs, name):
    assert name in gs.__all__
    cls = getattr(gs, name)
    assert sorted(a for a in dir(cls) if not a.startswith("_")) == sorted(CLASSES[name])
    for attr, text in CLASSES[name].items():
        assert _found(getattr(cls, attr)) == _written(text), attr
        kinds = {p.kind for p in inspect.signature(getattr(cls, attr)).parameters.values()}
        assert kinds <= {inspect.Parameter.POSITIONAL_OR_KEYWORD}, attr     # no *args pass-through: keyword callers work


def test_the_classes_stay_distinct(gs):
    classes = [getattr(gs, name) for name in CLASSES]
    assert len(set(classes)) == len(classes) and all(inspect.isclass(c) for c in classes)
    assert not hasattr(gs.DeviceTopKRowsAnyK, "MaxK")
    assert gs.DeviceTopKRows64.MaxK() == gs.DeviceTopKRows.MaxK() == gs.DeviceTopKSegmented64.MaxK() == gs.DeviceTopKSegmented.MaxK()
    for k in (K, 1, gs.DeviceTopKRows.MaxK()):
        for has_values in (False, True):
            assert gs.DeviceTopKRows64.Plan(ROWS, COLS, k, has_values) == gs.DeviceTopKRows.Plan(ROWS, COLS, k, has_values)
            assert (gs.DeviceTopKSegmented64.Plan(ROWS * COLS, ROWS, k, has_values=has_values)
                    == gs.DeviceTopKSegmented.Plan(ROWS * COLS, ROWS, k, has_values=has_values))
    assert gs.DeviceTopKRowsAnyK.Plan(ROWS, COLS, K) != gs.DeviceTopKRows.Plan(ROWS, COLS, K)
    with pytest.raises(gs.GpuSortError):
        gs.DeviceTopKRows64.Plan(ROWS, COLS, 2000)
    assert len(gs.DeviceTopKRowsAnyK.Plan(ROWS, COLS, 2000)) == 8


# (class, key_type of the query: a GS_KEY_* name or None, the width's size query, the call shape, a k the shape accepts, a k it
#  refuses: above MaxK() where there is one, above the row length for DeviceTopKRowsAnyK, none for the flat shape, which has no
#  cap and is asked at k = 2000 as a second accepted shape)
N = ROWS * COLS
QUERIES = [
    ("DeviceTopK", None, "gs_topk_temp_bytes", "flat", K, None),
    ("DeviceTopK", "GS_KEY_F32", "gs_topk_temp_bytes", "flat", K, None),
    ("DeviceTopK16", None, "gs_topk_u16_temp_bytes", "flat", K, None),
    ("DeviceTopK16", "GS_KEY_BF16", "gs_topk_u16_temp_bytes", "flat", K, None),
    ("DeviceTopK64", None, "gs_topk_u64_temp_bytes", "flat", K, None),
    ("DeviceTopK64", "GS_KEY_I64", "gs_topk_u64_temp_bytes", "flat", K, None),
    ("DeviceTopKRows", None, "gs_topk_rows_temp_bytes", "rows", K, 2000),
    ("DeviceTopKRows", "GS_KEY_I32", "gs_topk_rows_temp_bytes", "rows", K, 2000),
    ("DeviceTopKRows", "GS_KEY_U16", "gs_topk_rows_u16_temp_bytes", "rows", K, 2000),
    ("DeviceTopKRows64", None, "gs_topk_rows_u64_temp_bytes", "rows", K, 2000),
    ("DeviceTopKRows64", "GS_KEY_F64", "gs_topk_rows_u64_temp_bytes", "rows", K, 2000),
    ("DeviceTopKRowsAnyK", None, "gs_topk_rows_anyk_temp_bytes", "rows", 2000, COLS + 1),
    ("DeviceTopKRowsAnyK", "GS_KEY_U32", "gs_topk_rows_anyk_temp_bytes", "rows", 2000, COLS + 1),
    ("DeviceTopKSegmented", None, "gs_topk_segmented_temp_bytes", "segmented", K, 2000),
    ("DeviceTopKSegmented", "GS_KEY_F32", "gs_topk_segmented_temp_bytes", "segmented", K, 2000),
    ("DeviceTopKSegmented", "GS_KEY_F16", "gs_topk_segmented_u16_temp_bytes", "segmented", K, 2000),
    ("DeviceTopKSegmented64", None, "gs_topk_segmented_u64_temp_bytes", "segmented", K, 2000),
    ("DeviceTopKSegmented64", "GS_KEY_U64", "gs_topk_segmented_u64_temp_bytes", "segmented", K, 2000),
]


@pytest.mark.parametrize("name,key_type,query,shape,k_ok,k_refused", QUERIES)
def test_size_query_without_tensors_is_the_widths_own(gs, name, key_type, query, shape, k_ok, k_refused):
    cls = getattr(gs, name)
    kt = None if key_type is None else getattr(gs, key_type)
    for k, refused in ((k_ok, False), (2000, False) if k_refused is None else (k_refused, True)):
        if shape == "flat":
            keys, pairs, lib_args = (None, None, N, k), (None, None, None, None, N, k), (N, k)
        elif shape == "rows":
            keys, pairs, lib_args = (None, None, ROWS, COLS, COLS, k), (None, None, None, None, ROWS, COLS, COLS, k), (ROWS, COLS, k)
        else:
            keys = (None, None, None, N, ROWS, None, None, k)
            pairs, lib_args = (None, None, None, None, None, N, ROWS, None, None, k), (N, ROWS, k)
        want0, want1 = getattr(gs.lib, query)(*lib_args, 0), getattr(gs.lib, query)(*lib_args, 1)
        assert (want0 == want1 == 0) if refused else (want1 > want0 > 0)
        assert cls.MinKeys(None, 0, *keys, key_type=kt) == want0
        assert cls.MaxKeys(None, 0, *keys, key_type=kt) == want0
        assert cls.MinPairs(None, 0, *pairs, key_type=kt) == want1
        assert cls.MaxPairs(None, 0, *pairs, key_type=kt) == want1
    # by keyword, as a caller who names every argument writes it
    names = [n for n, _ in _found(cls.MinPairs)][2:-2]
    by_name = dict(zip(names, pairs))
    assert cls.MaxPairs(d_temp_storage=None, temp_storage_bytes=0, stream=None, key_type=kt, **by_name) == want1
