"""Torch-facing ops of the MI355X kernels (GPU) with host C fallbacks for CPU tensors."""
from .gemm import sgemm, sgemm_naive_host, sgemm_out, sgemm_simt
from .halo import pack_edges, unpack_halo_
from .image import (SEED_3D, Camera, apply_region_mask, corner_seeds, create_volume, default_camera, histeq, pad1,
                    raycast, region2d, region2d_grow_padded_, region3d)
from .sparse import CSR, SlicedCSR, banded_csr, create_vector, powerlaw_csr, spmm, spmv, spmv_banded
from .stencil import init_grid, stencil5_reference, stencil5_step_, stencil5x2_step_, stencil5_fused_step_, stencil5_fused_spans_
# sort_keys / sort / argsort / sort_by_key / topk / kth_value take dim=int for the row-wise forms (one wave or one block
# per row, csrc/kernels/rowsort.hip); their route constants (ROWSORT_*, ROW_TOPK_*) live in .vector. reduce / scan take
# dim=int for the forms along a dimension (csrc/kernels/axis.hip); their route constants (AXIS_*) live there too.
# segment_reduce / segment_scan take ragged segments by offsets (csrc/kernels/ragged.hip; RAGGED_TILE, RAGGED_LANE_ITEMS)
from .vector import (CMP_CODES, OP_CODES, argsort, axpy_, bincount, bucketize, compact, compact_indices, compact_where, copy_, dot, fill_,
                     gather_, histc, histogram, kth_value, merge, merge_by_key, merge_keys, rand_uniform_, reduce, reduce_by_key, run_length_encode, run_positions, scan,
                     scan_by_key, scan_check, searchsorted, segment_reduce, segment_scan, segmented_scan, select, select_indices, sort, sort_by_key, sort_keys, sum_by_key,
                     topk, unique, unique_consecutive, vadd, vmul)
# segment_sort_keys / segment_sort / segment_argsort / segment_sort_by_key sort inside the same ragged segments
# (csrc/kernels/segsort.hip; SEGSORT_CLASS_LIMITS, SEGSORT_MAX_LEN, SEGSORT_GRID_MULT)
from .vector import segment_argsort, segment_sort, segment_sort_by_key, segment_sort_keys
# arg_reduce / argmax / argmin (flat or dim=int) and segment_arg_reduce / segment_argmax / segment_argmin say where the
# extremum is (csrc/kernels/argreduce.hip; ARG_BLOCK, ARG_MAX_BLOCKS)
from .vector import arg_reduce, argmax, argmin, segment_arg_reduce, segment_argmax, segment_argmin
# set operations on SORTED tensors (multiset rule of std::set_*, csrc/kernels/setops.hip; SETOP_TILE, SET_OP_CODES) and
# their numpy-style forms for unsorted input
from .vector import (intersect1d, set_compact, set_compact_by_key, set_difference, set_intersection, set_op_by_key,
                     set_symmetric_difference, set_union, setdiff1d, setxor1d, union1d)

__all__ = [
    "sgemm", "sgemm_out", "sgemm_simt", "sgemm_naive_host",
    "vmul", "vadd", "axpy_", "copy_", "gather_", "dot", "reduce", "scan", "scan_check", "fill_", "rand_uniform_", "OP_CODES",
    "histeq", "region2d", "region2d_grow_padded_", "region3d", "corner_seeds", "pad1", "apply_region_mask",
    "create_volume", "raycast", "default_camera", "Camera", "SEED_3D",
    "stencil5_step_", "stencil5x2_step_", "stencil5_fused_step_", "stencil5_fused_spans_", "stencil5_reference", "init_grid",
    "CSR", "SlicedCSR", "banded_csr", "create_vector", "powerlaw_csr", "spmm", "spmv", "spmv_banded",
    "pack_edges", "unpack_halo_",
    "compact", "select", "compact_indices", "select_indices", "compact_where", "CMP_CODES",
    "sort_keys", "sort", "argsort", "sort_by_key", "topk", "kth_value",
    "run_length_encode", "reduce_by_key", "unique_consecutive", "unique", "sum_by_key",
    "scan_by_key", "segmented_scan", "run_positions",
    "bincount", "histc", "histogram",
    "merge_keys", "merge", "merge_by_key", "searchsorted", "bucketize",
    "segment_reduce", "segment_scan",
    "segment_sort_keys", "segment_sort", "segment_argsort", "segment_sort_by_key",
    "arg_reduce", "argmax", "argmin", "segment_arg_reduce", "segment_argmax", "segment_argmin",
    "set_compact", "set_compact_by_key", "set_intersection", "set_union", "set_difference", "set_symmetric_difference",
    "set_op_by_key", "intersect1d", "union1d", "setdiff1d", "setxor1d",
]
