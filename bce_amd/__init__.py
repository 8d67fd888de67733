"""bce_amd -- MI355X-native (gfx950) implementation of the `bce -c` hot path of akamiru/bce.

The product is bce_amd/lib/libbcehip.so (hand-written HIP kernels behind the C ABI of
include/bce_hip.h) plus the `bce` command line (bce_amd/bin/bce).  This package is the thin Python
binding used by tests and bench.py; it mirrors the reference's own interface names
(RankFile, BCE.encode, `bce -c archive file [config]`, bce.cpp:932-984,1117-1167,1403-1427).
There is no CPU fallback: every compute call goes through the HIP library and fails loudly
when it is missing or when no GPU is present.
"""
from .api import (BCE, BceError, ContextPool, RankFile, compress, compress_device, compress_many, decompress, decompress_device, decompress_to_device,  # noqa: F401
                  library_path, load_library, scan, synth_rand, synth_text, stats, stats_of, archive_of, plane_stream, set_plane_mask, set_plane_stream,
                  verify, verify_device, ChecksumError, crc32, crc32_combine, crc32_device, decode_crc32, input_crc32, Estimate, estimate, estimate_device, cost_q24, count, seam_count, linear_counts, count_near, locate_near, near_linear_counts, NEAR_MAX_K, NEAR_MAX_LEN, count_edit, locate_edit, EDIT_MAX_K, EDIT_MAX_LEN, EDIT_MAX_PATTERNS, count_classes, locate_classes, compile_classes, class_linear_counts, CLASS_MAX_LEN, CLASS_MAX_WIDE, CLASS_DEFAULT_NODES, CLASS_MAX_NODES, parse, patch, delta, apply_delta, ParseInfo, Op, OP_LITERAL, OP_DTYPE, parse_of_lengths_device, locate, match, coverage, KGram, kgrams, TopKGram, TopKGrams, top_kgrams, top_classes_of_lcp_device, TOP_MAX, TOP_DTYPE, MaxRepInfo, maximal_repeats, maxrep_of_arrays_device, MAXREP_DTYPE, MAXREP_ORDERS, entropy_profile, entropy_from_sums, longest_repeat, lpf, self_parse, nsv_device, self_parse_of_lpf_device, suffix_array, sufcheck, suffix_array_device, sufcheck_device, SUFCHECK_REASONS)
from .build import build as build_native  # noqa: F401


_TENSOR_NAMES = ("compress_tensor", "estimate_tensor", "decompress_tensor", "verify_tensor", "compress_tensor_blocks", "decompress_container_tensor", "test_container", "count_tensor", "count_in_archive", "locate_tensor", "parse_tensor", "patch_tensor", "locate_in_archive", "count_near_tensor", "count_near_in_archive", "locate_near_tensor", "locate_near_in_archive", "count_edit_tensor", "count_edit_in_archive", "locate_edit_tensor", "locate_edit_in_archive", "count_classes_tensor", "count_classes_in_archive", "locate_classes_tensor", "locate_classes_in_archive", "match_tensor", "coverage_tensor", "coverage_in_archive", "lcp_tensor", "kgrams_tensor", "entropy_profile_tensor", "entropy_profile_in_archive", "top_kgrams_tensor", "top_kgrams_in_archive", "maximal_repeats_tensor", "maximal_repeats_in_archive", "lpf_tensor", "self_parse_tensor", "self_parse_in_archive", "suffix_array_tensor", "sufcheck_tensor")


def __getattr__(name):
    # the torch plumbing (bce_amd/tensor.py) is imported when it is first asked for: the binding itself needs no torch
    if name in _TENSOR_NAMES:
        from . import tensor
        return getattr(tensor, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
