"""MI355X-native radix sort: Python host mirror of the reference's entry points.

The compute path is hand-written HIP for gfx950 behind the C ABI of
include/gpusort.h (libgpusort.so); this package only carries device pointers
and streams to it.  torch is used for device memory, streams and
torch.distributed -- plumbing, not the product.

Names follow the reference:
  DoubleBuffer, DeviceRadixSort.SortKeys/SortPairs/SortKeysDescending/
  SortPairsDescending           (lsb/cub/cub/device/device_radix_sort.cuh)
  DeviceRadixSortLarge          (the same four, stable, for 2^32 elements and more)
  DeviceTopK, topk              (the first k elements of the stable sort, by radix select; no reference counterpart)
  DeviceTopK16                  (DeviceTopK for a flat array of int16 / uint16 / float16 / bfloat16 keys; topk() routes them)
  DeviceTopK64                  (DeviceTopK for a flat array of int64 / uint64 / float64 keys: gs_topk_u64; topk() routes them)
  DeviceTopKRows, topk_rows     (the same for every row of a matrix; 32-bit keys, and int16 / uint16 / float16 / bfloat16)
  DeviceTopKRows64, topk_rows64 (the same for every row of a matrix of int64 / uint64 / float64 keys: gs_topk_rows_u64)
  DeviceTopKRowsAnyK, topk_rows_anyk   (every row of a matrix of 32-bit keys for any k <= columns: gs_topk_rows_anyk_u32)
  DeviceTopKRowsAnyK16, topk_rows_anyk16   (the same for int16 / uint16 / float16 / bfloat16 keys: gs_topk_rows_anyk_u16)
  DeviceTopKRowsAnyK64, topk_rows_anyk64   (the same for int64 / uint64 / float64 keys: gs_topk_rows_anyk_u64)
  DeviceTopKSegmented, topk_segmented   (the same for every ragged segment given by device offsets; 32-bit keys, and int16 / uint16 / float16 / bfloat16)
  DeviceTopKSegmented64, topk_segmented64   (the same for ragged segments of int64 / uint64 / float64 keys: gs_topk_segmented_u64)
  DeviceTopKSegmentedAnyK, topk_segmented_anyk   (ragged segments of 32-bit keys for any k: gs_topk_segmented_anyk_u32)
  sortKeysGPU / sortPairsGPU    (lsb/sort.cu:25-76)
  rdxsrt_unstable_sort, rdxsrt_unstable_sort_keys/_pairs, RDXSRT_SortedSequence
                                (msb/src/sort/gpu_radix_sort.h:31-34,197,511,544)
"""
from ._lib import (GpuSortError, GS_KEY_U32, GS_KEY_I32, GS_KEY_F32, GS_KEY_U64, GS_KEY_I64, GS_KEY_F64, GS_KEY_U8, GS_KEY_I8, GS_KEY_U16, GS_KEY_I16, GS_KEY_F16, GS_KEY_BF16,
                   GS_KEY_F8, GS_GEN_UNIFORM, GS_GEN_ZIPF,
                   GS_GEN_ENTROPY_AND, GS_GEN_ENUMERATED, LIB_PATH, lib, KernelProfile)
from .lsb import DoubleBuffer, DeviceRadixSort, DeviceRadixSortLarge, DeviceSegmentedRadixSort, sortKeysGPU, sortPairsGPU, lsb_pass_kernels
from .select import (DeviceTopK, DeviceTopK16, DeviceTopK64, DeviceTopKRows, DeviceTopKRows64, DeviceTopKRowsAnyK, DeviceTopKRowsAnyK16,
                     DeviceTopKRowsAnyK64, topk_rows_anyk64,
                     DeviceTopKSegmented, DeviceTopKSegmented64, topk, topk_rows, topk_rows64, topk_rows_anyk, topk_rows_anyk16, topk_segmented,
                     topk_segmented64, DeviceTopKSegmentedAnyK, topk_segmented_anyk)
from .datagen import (generate_random_keys, generate_uniform_keys, generate_zipf_keys, generate_enumerated_values,
                      check_sorted, check_pairs_enumerated)
from .msb import (RDXSRT_SortedSequence, rdxsrt_unstable_sort, rdxsrt_unstable_sort_keys, rdxsrt_unstable_sort_pairs,
                  rdxsrt_unstable_sort_large, rdxsrt_unstable_sort_large_wide)

__all__ = [n for n in dir() if not n.startswith("_")]
