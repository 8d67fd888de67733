"""ctypes binding of include/bce_hip.h, shaped like the reference's own objects.

reference                                   here
------------------------------------------  ---------------------------------------------
RankFile(name)  (bce.cpp:932-984)           RankFile(data)      rotate+BWT (K1), planes (K2)
  .size() .offset() .status() .ranks          .size() .offset() .status() .zeros / .rank1()
BCE<AdaptiveCoder<31>,...>::encode(file)    BCE(config).encode(rank_file) -> archive bytes
  (bce.cpp:1117-1167)
AdaptiveCoder::load_config (bce.cpp:626)    BCE(config=288 bytes) / BCE.load_config(path)
main -c (bce.cpp:1403-1427)                 compress(data, config) ; bce_amd/bin/bce
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("BCE_HIP_LIB") or os.path.join(_HERE, "lib", "libbcehip.so")   # (BCE_HIP_LIB: kernel-variant experiments)
_lib = None

CONFIG_BYTES = 288


class BceError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__("%s failed: status %d (%s)%s" % (where, status, _strerror(status), (" -- " + detail) if detail else ""))


class ChecksumError(BceError):
    """A block of a version-2 container decoded to bytes whose CRC-32 is not the table's."""

    def __init__(self, block, expected, actual):
        self.status, self.block, self.expected, self.actual = -6, block, expected, actual
        RuntimeError.__init__(self, "Checksum mismatch in block %d: table %08X, decoded %08X" % (block, expected, actual))


class Stats(C.Structure):
    _fields_ = [("n", C.c_uint64), ("nodes", C.c_uint64), ("symbols", C.c_uint64), ("rounds", C.c_uint32),
                ("sort_rounds", C.c_uint32), ("flushes", C.c_uint32), ("spine_levels", C.c_uint32),
                ("t_load", C.c_double), ("t_bwt", C.c_double), ("t_planes", C.c_double), ("t_enum", C.c_double),
                ("t_model", C.c_double), ("t_coder", C.c_double), ("t_total", C.c_double),
                ("k3_ms", C.c_double), ("k3_launches", C.c_double), ("t_coder_busy", C.c_double),
                ("list_grows", C.c_double), ("list_nodes", C.c_double), ("split_rounds", C.c_double),
                ("reg_maps", C.c_double), ("reg_unmaps", C.c_double), ("dec_restarts", C.c_double), ("t_model_kernels", C.c_double),
                ("dec_list_grows", C.c_double), ("dec_split_rounds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ParseInfo(C.Structure):
    """bce_hip_parse_info: what a parse holds (RankFile.parse): nlits + copied == q, nops - ncopies literal runs."""
    _fields_ = [("nops", C.c_uint64), ("nlits", C.c_uint64), ("ncopies", C.c_uint64), ("copied", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class MaxRepInfo(C.Structure):
    """bce_hip_maxrep_info: what a list of maximal repeats comes with (RankFile.maximal_repeats): `total` repeats of min_len bytes or
    more, `capped` of them at the bound, the runs of the BWT, and the entries written."""
    _fields_ = [("total", C.c_uint64), ("capped", C.c_uint64), ("bwt_runs", C.c_uint64), ("found", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


class Op(C.Structure):
    """bce_hip_op: src == OP_LITERAL: the next len bytes of the literal stream; else text[src : src + len]."""
    _fields_ = [("len", C.c_uint32), ("src", C.c_uint32)]


# every symbol include/bce_hip.h declares: (name, restype, argtypes)
_u8p, _u32p, _vp = C.c_void_p, C.c_void_p, C.c_void_p
SYMBOLS = [
    ("bce_hip_create", C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    ("bce_hip_create_sized", C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_uint64]),
    ("bce_hip_destroy", None, [C.c_void_p]),
    ("bce_hip_strerror", C.c_char_p, [C.c_int]),
    ("bce_hip_last_error", C.c_char_p, [C.c_void_p]),
    ("bce_hip_set_config", C.c_int, [C.c_void_p, _u8p]),
    ("bce_hip_set_symbol_capacity", C.c_int, [C.c_void_p, C.c_uint64]),
    ("bce_hip_set_gated", C.c_int, [C.c_void_p, C.c_int]),
    ("bce_hip_set_progress", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("bce_hip_debug_set", C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    ("bce_hip_load_host", C.c_int, [C.c_void_p, _u8p, C.c_uint32]),
    ("bce_hip_load_device", C.c_int, [C.c_void_p, _vp, C.c_uint32]),
    ("bce_hip_bwt", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("bce_hip_set_bwt", C.c_int, [C.c_void_p, _u8p, C.c_uint32, C.c_uint32]),
    ("bce_hip_get_bwt", C.c_int, [C.c_void_p, _u8p]),
    ("bce_hip_divbwt", C.c_int, [C.c_void_p, _u8p, _u8p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("bce_hip_inverse_bwt", C.c_int, [C.c_void_p, _u8p, _u8p, C.c_uint32, C.c_uint32]),
    ("bce_hip_build_planes", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("bce_hip_get_plane_bits", C.c_int, [C.c_void_p, C.c_int, _u8p]),
    ("bce_hip_rank1", C.c_int, [C.c_void_p, C.c_int, _u32p, C.c_uint32, _u32p]),
    ("bce_hip_encode", C.c_int, [C.c_void_p]),
    ("bce_hip_archive_size", C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    ("bce_hip_archive_copy", C.c_int, [C.c_void_p, _u8p, C.c_size_t]),
    ("bce_hip_set_plane_mask", C.c_int, [C.c_void_p, C.c_uint32]),
    ("bce_hip_plane_stream_size", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    ("bce_hip_plane_stream_copy", C.c_int, [C.c_void_p, C.c_int, _vp, C.c_size_t]),
    ("bce_hip_plane_stream_set", C.c_int, [C.c_void_p, C.c_int, _vp, C.c_size_t]),
    ("bce_hip_compress", C.c_int, [C.c_void_p, _u8p, C.c_uint32, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("bce_hip_compress_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("bce_hip_enum_begin", C.c_int, [C.c_void_p]),
    ("bce_hip_enum_nodes", C.c_int, [C.c_void_p, C.c_int, _u32p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("bce_hip_enum_round", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("bce_hip_enum_symbols", C.c_int, [C.c_void_p, _u32p, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_enum_model", C.c_int, [C.c_void_p, _u32p, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_model_begin", C.c_int, [C.c_void_p]),
    ("bce_hip_model_flush", C.c_int, [C.c_void_p, _u32p, _u32p, C.c_uint64, _vp, C.POINTER(C.c_uint32)]),
    ("bce_hip_scan", C.c_int, [C.c_void_p, _u8p, C.POINTER(C.c_double)]),
    ("bce_hip_scan_records", C.c_int, [C.c_void_p, _u32p, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_decompress", C.c_int, [_u8p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("bce_hip_decompress_device", C.c_int, [C.c_void_p, _u8p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("bce_hip_decompress_to_device", C.c_int, [C.c_void_p, _u8p, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("bce_hip_verify_device", C.c_int, [C.c_void_p, _u8p, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_uint64)]),
    ("bce_hip_verify_host", C.c_int, [C.c_void_p, _u8p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(C.c_uint64)]),
    ("bce_hip_crc32", C.c_uint32, [C.c_uint32, _u8p, C.c_size_t]),
    ("bce_hip_crc32_combine", C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint64]),
    ("bce_hip_crc32_device", C.c_int, [C.c_void_p, _vp, C.c_size_t, C.POINTER(C.c_uint32)]),
    ("bce_hip_input_crc32", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("bce_hip_decode_crc32", C.c_int, [C.c_void_p, _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    ("bce_hip_decompress_device_crc32", C.c_int, [C.c_void_p, _u8p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    ("bce_hip_estimate", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]),
    ("bce_hip_estimate_host", C.c_int, [C.c_void_p, _u8p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]),
    ("bce_hip_estimate_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]),
    ("bce_hip_cost_q24", C.c_uint32, [C.c_uint32, C.c_uint32]),
    ("bce_hip_sort_pairs_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("bce_hip_sort_wide_device", C.c_int, [C.c_void_p, _vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("bce_hip_compare_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_size_t, C.POINTER(C.c_uint64)]),
    ("bce_hip_planes_from_ranks_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, _vp, _vp, _vp]),
    ("bce_hip_unbwt_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, C.c_uint32, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("bce_hip_lcp_reduce_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, _vp, _vp, C.c_uint32, _vp, _vp]),
    ("bce_hip_top_classes_of_lcp_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, _vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), _vp]),
    ("bce_hip_coverage_of_lengths_device", C.c_int, [C.c_void_p, _vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("bce_hip_count", C.c_int, [C.c_void_p, _u8p, _vp, C.c_uint32, _vp]),
    ("bce_hip_count_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, _vp]),
    ("bce_hip_input_bytes", C.c_int, [C.c_void_p, C.c_uint64, C.c_size_t, _u8p]),
    ("bce_hip_locate", C.c_int, [C.c_void_p, _u8p, _vp, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_locate_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_count_near", C.c_int, [C.c_void_p, _u8p, _vp, C.c_uint32, C.c_uint32, _vp]),
    ("bce_hip_count_near_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, _vp]),
    ("bce_hip_locate_near", C.c_int, [C.c_void_p, _u8p, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_locate_near_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_count_edit", C.c_int, [C.c_void_p, _u8p, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp]),
    ("bce_hip_count_edit_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp]),
    ("bce_hip_locate_edit", C.c_int, [C.c_void_p, _u8p, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_locate_edit_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_count_classes", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    ("bce_hip_count_classes_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    ("bce_hip_locate_classes", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_locate_classes_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_match", C.c_int, [C.c_void_p, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, _vp, _vp]),
    ("bce_hip_match_device", C.c_int, [C.c_void_p, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, _vp]),
    ("bce_hip_coverage", C.c_int, [C.c_void_p, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("bce_hip_coverage_device", C.c_int, [C.c_void_p, _vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("bce_hip_lcp", C.c_int, [C.c_void_p, C.c_uint32, _vp]),
    ("bce_hip_lcp_device", C.c_int, [C.c_void_p, C.c_uint32, _vp]),
    ("bce_hip_kgrams", C.c_int, [C.c_void_p, _vp, C.c_uint32, _vp]),
    ("bce_hip_longest_repeat", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("bce_hip_top_kgrams", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), _vp]),
    ("bce_hip_top_kgrams_device", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), _vp]),
    ("bce_hip_maximal_repeats", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint32, C.c_uint64, C.POINTER(MaxRepInfo)]),
    ("bce_hip_maximal_repeats_device", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint32, C.c_uint64, C.POINTER(MaxRepInfo)]),
    ("bce_hip_maxrep_of_arrays_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.POINTER(MaxRepInfo)]),
    ("bce_hip_parse", C.c_int, [C.c_void_p, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint64, _u8p, C.c_uint64, C.POINTER(ParseInfo)]),
    ("bce_hip_parse_device", C.c_int, [C.c_void_p, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(ParseInfo)]),
    ("bce_hip_patch", C.c_int, [C.c_void_p, _vp, C.c_uint64, _u8p, C.c_uint64, _u8p, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_patch_device", C.c_int, [C.c_void_p, _vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("bce_hip_parse_of_lengths_device", C.c_int, [C.c_void_p, _vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(ParseInfo)]),
    ("bce_hip_lpf", C.c_int, [C.c_void_p, C.c_uint32, _vp, _vp]),
    ("bce_hip_lpf_device", C.c_int, [C.c_void_p, C.c_uint32, _vp, _vp]),
    ("bce_hip_self_parse", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _vp, C.c_uint64, _u8p, C.c_uint64, C.POINTER(ParseInfo)]),
    ("bce_hip_self_parse_device", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(ParseInfo)]),
    ("bce_hip_nsv_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, _vp, _vp]),
    ("bce_hip_self_parse_of_lpf_device", C.c_int, [C.c_void_p, _vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(ParseInfo)]),
    ("bce_hip_suffix_array", C.c_int, [C.c_void_p, _u8p, C.c_uint32, _vp, _vp]),
    ("bce_hip_suffix_array_device", C.c_int, [C.c_void_p, _vp, C.c_uint32, _vp, _vp]),
    ("bce_hip_sufcheck", C.c_int, [C.c_void_p, _u8p, _vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("bce_hip_sufcheck_device", C.c_int, [C.c_void_p, _vp, _vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("bce_hip_get_stats", C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    ("bce_hip_synth_text", None, [C.c_uint64, _u8p, C.c_size_t]),
    ("bce_hip_synth_rand", None, [C.c_uint64, _u8p, C.c_size_t]),
]


def library_path():
    return _LIB_PATH


def load_library():
    """Load libbcehip.so (no fallback: raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or make -C bce_amd/csrc) first; there is no CPU fallback" % _LIB_PATH)
        lib = C.CDLL(_LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _strerror(status):
    try:
        return load_library().bce_hip_strerror(status).decode()
    except Exception:  # pragma: no cover
        return "?"


def _as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


LOCATE_LINEAR = 1                               # BCE_HIP_LOCATE_LINEAR
NEAR_MAX_K = 2                                  # BCE_HIP_NEAR_MAX_K: mismatches allowed at most; a work bound, not a format limit
NEAR_MAX_LEN = 4096                             # BCE_HIP_NEAR_MAX_LEN: bytes of a pattern searched with mismatches
EDIT_MAX_K = 2                                  # BCE_HIP_EDIT_MAX_K: edits allowed at most; a work bound, as NEAR_MAX_K
EDIT_MAX_LEN = 4096                             # BCE_HIP_EDIT_MAX_LEN: bytes of a pattern searched with edits
EDIT_MAX_PATTERNS = 1 << 28                     # BCE_HIP_EDIT_MAX_PATTERNS: patterns of one call
CLASS_MAX_LEN = 4096                            # BCE_HIP_CLASS_MAX_LEN: classes of a pattern searched by byte classes
CLASS_MAX_WIDE = 64                             # BCE_HIP_CLASS_MAX_WIDE: of them, those with two members or more
CLASS_DEFAULT_NODES = 1 << 16                   # BCE_HIP_CLASS_DEFAULT_NODES: the budget of search nodes per pattern when none is given
CLASS_MAX_NODES = 1 << 16                       # BCE_HIP_CLASS_MAX_NODES: the largest budget a call takes
CLASS_OVER = 1                                  # BCE_HIP_CLASS_OVER: status of a pattern whose search ran out of its budget
MATCH_LINEAR = 1                                # BCE_HIP_MATCH_LINEAR
MATCH_MAX_LEN = 4096                            # BCE_HIP_MATCH_MAX_LEN: a work bound per end position, not a format limit
KGRAMS_MAX = 64                                 # BCE_HIP_KGRAMS_MAX: values of k in one bce_hip_kgrams call
TOP_MAX = 1 << 20                               # BCE_HIP_TOP_MAX: the longest list of one bce_hip_top_kgrams call
TOP_DTYPE = np.dtype([("count", "<u4"), ("row", "<u4"), ("pos", "<u4")])   # bce_hip_top_kgram as a numpy record
MAXREP_DTYPE = np.dtype([("len", "<u4"), ("count", "<u4"), ("row", "<u4"), ("pos", "<u4")])   # bce_hip_maxrep as a numpy record
MAXREP_ORDERS = {"len": 0, "count": 1, "gain": 2}   # BCE_HIP_MAXREP_BY_LEN / _BY_COUNT / _BY_GAIN
MAXREP_BYTES_MAX = 4096                         # the most bytes of one repeat a call hands out
E_OVERFLOW = -5                                 # BCE_HIP_E_OVERFLOW
OP_LITERAL = 0xFFFFFFFF                         # BCE_HIP_OP_LITERAL: bce_hip_op::src of a literal run
PARSE_MAX_LEN = 256                             # the default length bound of a parse: the search costs up to q * max_len lane steps
OP_DTYPE = np.dtype([("len", "<u4"), ("src", "<u4")])   # bce_hip_op as a numpy record


def _positions_buffer(total):
    """Host room for `total` located positions (RankFile.locate makes it only after the sizing call has passed max_hits)."""
    return np.empty(max(total, 1), dtype=np.uint32)


def _is_one_pattern(patterns):
    return isinstance(patterns, (bytes, bytearray, memoryview, np.ndarray))


def seam_count(head, tail, pattern) -> int:
    """The occurrences of `pattern` (m bytes) in a circular text that straddle its end: those of the seam tail + head, where
    `tail` is the text's last m - 1 bytes and `head` its first m - 1 (overlapping matches counted).  Every match inside the
    2 (m - 1) bytes of the seam crosses their middle.  A cyclic count minus this is the linear count, for m <= n."""
    seam, pattern = bytes(tail) + bytes(head), bytes(pattern)
    found, at = 0, seam.find(pattern)
    while at >= 0:
        found += 1
        at = seam.find(pattern, at + 1)
    return found


def linear_counts(cyclic, patterns, n, ends):
    """Cyclic counts -> the counts an overlapping `bytes` scan of the n-byte text gives.  ends(k) -> (the text's first k bytes,
    its last k), k <= n.  A pattern longer than the text occurs nowhere; otherwise the matches across the seam come off."""
    out = np.array(cyclic, dtype=np.uint64)
    longest = max([len(p) for p in patterns if len(p) <= n] + [1])
    head, tail = ends(longest - 1)
    for i, p in enumerate(patterns):
        m = len(p)
        if m > n:
            out[i] = 0
        elif m > 1:
            out[i] -= seam_count(head[:m - 1], tail[len(tail) - (m - 1):], p)
    return out


def near_linear_counts(cyclic, patterns, n, ends):
    """Cyclic counts per distance (rows of k + 1: RankFile.count_near) -> the counts a sliding window over the n-byte text gives.
    ends: as for linear_counts.  A pattern longer than the text is nowhere; otherwise each of the m - 1 windows that start in the
    text's last m - 1 bytes and run into its first comes off at its own distance, where that is within k."""
    out = np.array(cyclic, dtype=np.uint64).reshape(len(patterns), -1)
    k = out.shape[1] - 1
    longest = max([len(p) for p in patterns if len(p) <= n] + [1])
    head, tail = ends(longest - 1)
    for i, p in enumerate(patterns):
        m = len(p)
        if m > n:
            out[i] = 0
        elif m > 1:
            seam = np.frombuffer(bytes(tail[len(tail) - (m - 1):]) + bytes(head[:m - 1]), dtype=np.uint8)
            d = (np.lib.stride_tricks.sliding_window_view(seam, m)[:m - 1] != np.frombuffer(bytes(p), dtype=np.uint8)).sum(axis=1)
            out[i] -= np.bincount(d[d <= k], minlength=k + 1)[:k + 1].astype(np.uint64)
    return out


_CLASS_ESCAPES = b"\\.[]^-{}"


def compile_classes(expr, ignore_case=False):
    """An expression over bytes (bytes-like, or str taken as UTF-8) -> its classes: a numpy uint32 array of shape (m, 8), one
    256-bit set per position, byte c being bit c & 31 of word c >> 5 -- what the class searches take (bce_amd/csrc/class_expr.h
    is the same grammar for `bce -ge`).
      .        any byte
      [...]    a set: bytes and ranges a-b (a > b is an error); a leading ^ negates.  Inside a set only ] \\ and - are special (and
               ^ in front); a - that is not between the two ends of a range, and the empty set, are errors
      \\xHH    the byte HH; \\ before one of \\ . [ ] ^ - { } is that byte; both inside and outside sets; any other escape is an error
      {N}      after an atom: the atom N times in all, 1 <= N <= 4096
    Every other byte is itself; outside a set ] { } must be escaped.  More than CLASS_MAX_LEN classes, or anything malformed:
    ValueError.  ignore_case adds the other ASCII case of every letter of a literal or a set, before the set is negated."""
    s = expr.encode("utf-8") if isinstance(expr, str) else bytes(expr)
    out, at, atom = [], 0, False

    def escape(at):
        if at >= len(s):
            raise ValueError("a backslash at the end")
        if s[at] == 0x78:
            digits = s[at + 1:at + 3]
            if len(digits) != 2 or any(d not in b"0123456789abcdefABCDEF" for d in digits):
                raise ValueError("\\x wants two hex digits")
            return int(digits, 16), at + 3
        if s[at] in _CLASS_ESCAPES:
            return s[at], at + 1
        raise ValueError("an escape that is not one of \\xHH \\\\ \\. \\[ \\] \\^ \\- \\{ \\}")

    def item(at):
        return escape(at + 1) if s[at] == 0x5C else (s[at], at + 1)

    while at < len(s):
        ch = s[at]
        at += 1
        if ch == 0x7B:                                          # {N}
            end = at
            while end < len(s) and end - at < 8 and 0x30 <= s[end] <= 0x39:
                end += 1
            if not atom or end == at or end >= len(s) or s[end] != 0x7D:
                raise ValueError("{N} wants an atom before it, decimal digits and its }")
            count, at = int(s[at:end]), end + 1
            if not 1 <= count <= CLASS_MAX_LEN:
                raise ValueError("a repeat count outside 1 .. %d" % CLASS_MAX_LEN)
            if len(out) + count - 1 > CLASS_MAX_LEN:
                raise ValueError("more than %d classes" % CLASS_MAX_LEN)
            out += [out[-1]] * (count - 1)
            atom = False
            continue
        if ch in (0x5D, 0x7D):
            raise ValueError("] or } outside a set or a repeat")
        member, fold, negate = np.zeros(256, dtype=bool), True, False
        if ch == 0x2E:
            member[:], fold = True, False
        elif ch == 0x5B:
            if at < len(s) and s[at] == 0x5E:
                negate, at = True, at + 1
            while True:
                if at >= len(s):
                    raise ValueError("a set without its ]")
                if s[at] == 0x5D:
                    at += 1
                    break
                if s[at] == 0x2D:
                    raise ValueError("a - that is not inside a range")
                a, at = item(at)
                b = a
                if at < len(s) and s[at] == 0x2D:
                    at += 1
                    if at >= len(s):
                        raise ValueError("a set without its ]")
                    if s[at] in (0x5D, 0x2D):
                        raise ValueError("a - that is not inside a range")
                    b, at = item(at)
                    if a > b:
                        raise ValueError("a range whose first byte is above its last")
                member[a:b + 1] = True
            if not member.any():
                raise ValueError("an empty set")
        else:
            c, at = escape(at) if ch == 0x5C else (ch, at)
            member[c] = True
        if fold and ignore_case:
            both = member[0x41:0x5B] | member[0x61:0x7B]
            member[0x41:0x5B] = member[0x61:0x7B] = both
        if negate:
            member = ~member
        if len(out) >= CLASS_MAX_LEN:
            raise ValueError("more than %d classes" % CLASS_MAX_LEN)
        out.append(np.packbits(member, bitorder="little").view("<u4").astype(np.uint32))
        atom = True
    return np.array(out, dtype=np.uint32).reshape(len(out), 8)


def _class_member(masks, data):
    """masks: (m, 8) classes; data: uint8 array whose last axis has m bytes -> which of them lie in their position's class"""
    at = np.arange(masks.shape[0])
    return ((masks[at, data >> 5] >> (data & 31).astype(np.uint32)) & 1).astype(bool)


def class_linear_counts(cyclic, patterns, n, ends, over=None):
    """Cyclic counts of patterns of byte classes (RankFile.count_classes; `patterns`: their (m, 8) mask arrays) -> the counts a
    sliding window over the n-byte text gives.  ends: as for linear_counts.  A pattern longer than the text is nowhere; otherwise
    the windows that start in the text's last m - 1 bytes and match come off.  `over`: the patterns whose search ran out of its
    budget -- they have no count and stay at 0."""
    out = np.array(cyclic, dtype=np.uint64)
    longest = max([len(p) for p in patterns if len(p) <= n] + [1])
    head, tail = ends(longest - 1)
    for i, p in enumerate(patterns):
        m = len(p)
        if m > n or (over is not None and over[i]):
            out[i] = 0
        elif m > 1:
            seam = np.frombuffer(bytes(tail[len(tail) - (m - 1):]) + bytes(head[:m - 1]), dtype=np.uint8)
            inside = _class_member(np.asarray(p, dtype=np.uint32), np.lib.stride_tricks.sliding_window_view(seam, m)[:m - 1])
            out[i] -= np.uint64(inside.all(axis=1).sum())
    return out


def _is_one_class_pattern(patterns):
    return isinstance(patterns, (bytes, bytearray, memoryview, str)) or (isinstance(patterns, np.ndarray) and patterns.dtype != object and patterns.ndim == 2)


def _as_classes(pattern, ignore_case):
    """one pattern of a class search: an expression is compiled, an array of masks is taken as it stands"""
    if isinstance(pattern, (bytes, bytearray, memoryview, str)):
        return compile_classes(pattern, ignore_case=ignore_case)
    masks = np.ascontiguousarray(pattern, dtype=np.uint32)
    if masks.ndim != 2 or masks.shape[1] != 8:
        raise ValueError("a pattern of classes is an expression or an array of shape (m, 8), not %r" % (masks.shape,))
    return masks


class KGram(C.Structure):
    """bce_hip_kgram: the cyclic k-grams of a text for one k (RankFile.kgrams)."""
    _fields_ = [("distinct", C.c_uint64), ("once", C.c_uint64), ("nlogn_q24", C.c_uint64), ("max_count", C.c_uint32), ("max_pos", C.c_uint32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}

    def __repr__(self):
        return "KGram(%s)" % ", ".join("%s=%d" % kv for kv in self.as_dict().items())


class TopKGram(C.Structure):
    """bce_hip_top_kgram: one entry of the list of the most frequent k-grams (RankFile.top_kgrams)."""
    _fields_ = [("count", C.c_uint32), ("row", C.c_uint32), ("pos", C.c_uint32)]


class TopKGrams(list):
    """What RankFile.top_kgrams returns: a list of (count, pos, row, bytes), most frequent first and equal counts in the order of
    their bytes, with `distinct` (the number of distinct k-grams) and `size_hist` (32 ints: the k-grams whose count N has
    floor(log2 N) = b) beside it."""

    def __init__(self, entries, distinct, size_hist):
        super().__init__(entries)
        self.distinct = int(distinct)
        self.size_hist = [int(v) for v in size_hist]


def _top_limit(k, limit):
    k, limit = int(k), int(limit)
    if k < 0 or k > 0xFFFFFFFF:
        raise ValueError("k is 0 .. %d" % MATCH_MAX_LEN)
    if limit < 0 or limit > 0xFFFFFFFF:
        raise ValueError("limit is 1 .. %d" % TOP_MAX)
    return k, limit


def _maxrep_args(min_len, max_len, order, limit, bytes_per):
    """The arguments of a maximal_repeats call as the library takes them (`order` a name of MAXREP_ORDERS or its number)."""
    if isinstance(order, str):
        if order not in MAXREP_ORDERS:
            raise ValueError("order is one of %s" % ", ".join(sorted(MAXREP_ORDERS)))
        order = MAXREP_ORDERS[order]
    vals = [int(min_len), int(max_len), int(order), int(limit), int(bytes_per)]
    if any(v < 0 or v > 0xFFFFFFFF for v in vals):
        raise ValueError("min_len, max_len, order, limit and bytes_per are unsigned 32-bit numbers")
    return vals


def entropy_from_sums(n, s_k, s_k1) -> float:
    """H_k of the circular text of n bytes from S_k and S_(k+1) (KGram.nlogn_q24), in bits per byte: the double expression
    `bce -gk` prints, max(0, S_k - S_(k+1)) / (n * 2^24)."""
    return max(0, int(s_k) - int(s_k1)) / (int(n) * 16777216.0)


class _Ctx:
    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.bce_hip_create(C.byref(h), device)
        if rc != 0:
            raise BceError(rc, "bce_hip_create", "no usable HIP device %d (a GPU is required; there is no CPU path)" % device)
        self.h = h

    def check(self, rc, where):
        if rc != 0:
            raise BceError(rc, where, self.lib.bce_hip_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.bce_hip_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class RankFile:
    """The reference's RankFile (bce.cpp:932-984) on the GPU: input -> rotate + BWT (K1) -> 8 planes (K2).

    `data` may be bytes / a numpy u8 array (host) or an int device pointer with `n` (input resident in HBM).
    """

    def __init__(self, data=None, n=None, device=0, device_ptr=None, bwt=None, offset=None, ctx=None, build=True, index=True):
        self._c = ctx or _Ctx(device)
        lib = self._c.lib
        self._status = 0
        self._text = None                        # the host input, when there is one: count() cuts the text's two ends from it
        self._ends = (b"", b"")                  # of an input that came from device memory: its first and last bytes, as far as count() has fetched them
        self._has_text = bwt is None
        if bwt is not None:                      # test hook: inject a BWT, skip K1
            a = _as_u8(bwt)
            self._c.check(lib.bce_hip_set_bwt(self._c.h, a.ctypes.data, len(a), int(offset)), "bce_hip_set_bwt")
            self._n, self._offset = len(a), int(offset)
        else:
            if device_ptr is not None:
                self._c.check(lib.bce_hip_load_device(self._c.h, int(device_ptr), int(n)), "bce_hip_load_device")
                self._n = int(n)
            else:
                a = _as_u8(data)
                if len(a) == 0:
                    self._status = 1               # reference: `Error loading file` path; (empty input crashes it, Q12)
                    raise BceError(-1, "RankFile", "empty input")
                self._c.check(lib.bce_hip_load_host(self._c.h, a.ctypes.data, len(a)), "bce_hip_load_host")
                self._n = len(a)
                self._text = a
            self._offset = None
            if index:                            # (index=False: the text is loaded and nothing more -- all that patch() reads)
                off = C.c_uint32()
                self._c.check(lib.bce_hip_bwt(self._c.h, C.byref(off)), "bce_hip_bwt")
                self._offset = off.value
        self.zeros = None
        if build and index:
            z = (C.c_uint32 * 8)()
            self._c.check(lib.bce_hip_build_planes(self._c.h, z), "bce_hip_build_planes")
            self.zeros = list(z)

    def size(self):
        return self._n

    def offset(self):
        return self._offset

    def status(self):
        return self._status

    def bwt(self):
        out = np.empty(self._n, dtype=np.uint8)
        self._c.check(self._c.lib.bce_hip_get_bwt(self._c.h, out.ctypes.data), "bce_hip_get_bwt")
        return out

    def plane_bits(self, plane):
        out = np.empty(self._n, dtype=np.uint8)
        self._c.check(self._c.lib.bce_hip_get_plane_bits(self._c.h, plane, out.ctypes.data), "bce_hip_get_plane_bits")
        return out

    def rank1(self, plane, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        out = np.empty(len(idx), dtype=np.uint32)
        self._c.check(self._c.lib.bce_hip_rank1(self._c.h, plane, idx.ctypes.data, len(idx), out.ctypes.data), "bce_hip_rank1")
        return out

    def _text_ends(self, k):
        """(the first k bytes of the text, its last k), k <= n: from the host input, or 2 k bytes fetched from the context's copy."""
        if self._text is not None:
            return self._text[:k].tobytes(), self._text[self._n - k:].tobytes()
        if k > len(self._ends[0]):
            head, tail = np.empty(k, dtype=np.uint8), np.empty(k, dtype=np.uint8)
            self._c.check(self._c.lib.bce_hip_input_bytes(self._c.h, 0, k, head.ctypes.data), "bce_hip_input_bytes")
            self._c.check(self._c.lib.bce_hip_input_bytes(self._c.h, self._n - k, k, tail.ctypes.data), "bce_hip_input_bytes")
            self._ends = (head.tobytes(), tail.tobytes())
        head, tail = self._ends
        return head[:k], tail[len(tail) - k:]

    def count(self, patterns, cyclic=False):
        """How often byte strings occur in the text, counted on the GPU from the planes (bce_hip_count: backward search, the text
        is not read).  `patterns`: one bytes-like -> an int; a sequence of them -> a numpy uint64 array.
        cyclic=False: the count an overlapping scan of the text gives (what bytes.count would, if it counted overlapping
        matches); 0 for a pattern longer than the text; an empty pattern raises ValueError.
        cyclic=True: the matches in the circular text, those that run across its end included -- defined for every length (the
        empty pattern: n).  The only count a RankFile built from an injected BWT can give: it has no text for the correction."""
        one = _is_one_pattern(patterns)
        pats = [_as_u8(patterns)] if one else [_as_u8(p) for p in patterns]
        if not cyclic:
            if not self._has_text:
                raise ValueError("a RankFile built from an injected BWT holds no text: only cyclic=True counts are defined")
            if any(len(p) == 0 for p in pats):
                raise ValueError("an empty pattern has no linear count (cyclic=True: n)")
        out = np.zeros(len(pats), dtype=np.uint64)
        if pats:
            offsets = np.zeros(len(pats) + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
            flat = np.concatenate(pats) if int(offsets[-1]) else np.zeros(1, dtype=np.uint8)
            self._c.check(self._c.lib.bce_hip_count(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), out.ctypes.data), "bce_hip_count")
            if not cyclic:
                out = linear_counts(out, pats, self._n, self._text_ends)
        return int(out[0]) if one else out

    def count_device(self, patterns_ptr, offsets_ptr, npat, counts_ptr):
        """bce_hip_count_device: the cyclic counts of `npat` patterns that lie concatenated in device memory (int pointers: the
        bytes, npat + 1 uint64 offsets, npat uint64 counts out).  Stream rule: as decompress_to_device."""
        self._c.check(self._c.lib.bce_hip_count_device(self._c.h, None if patterns_ptr is None else int(patterns_ptr),
                                                       None if offsets_ptr is None else int(offsets_ptr), int(npat),
                                                       None if counts_ptr is None else int(counts_ptr)), "bce_hip_count_device")

    def locate(self, patterns, cyclic=False, limit=None, max_hits=1 << 26):
        """Where byte strings occur in the text: their byte offsets, ascending, gathered on the GPU from K1's suffix array at the
        rows backward search ends at (bce_hip_locate; the text is not read).  `patterns`: one bytes-like -> one numpy uint32 array;
        a sequence of them -> a list of arrays, in input order.
        cyclic=False: the hits an overlapping scan of the text finds (as many as count() says); none for a pattern longer than the
        text; an empty pattern raises ValueError.  cyclic=True: the hits in the circular text, those that run across its end
        included, defined for every length (the empty pattern: every position).  A RankFile built from an injected BWT has no
        suffix array: cyclic=False raises ValueError as count() does, cyclic=True BceError.
        A sizing call comes first: more than `max_hits` hits in all -> ValueError naming the total, before any room for positions
        is made.  `limit` keeps the first `limit` hits of each pattern in text order; it bounds the result, NOT the work (every
        hit is gathered and sorted first) nor what max_hits is compared with.  The sizing call and the full call each run the
        search (and, cyclic=False, the pass that counts the hits across the end): a request searches twice and gathers once."""
        one = _is_one_pattern(patterns)
        pats = [_as_u8(patterns)] if one else [_as_u8(p) for p in patterns]
        if not cyclic:
            if not self._has_text:
                raise ValueError("a RankFile built from an injected BWT holds no text: only cyclic=True hits are defined")
            if any(len(p) == 0 for p in pats):
                raise ValueError("an empty pattern has no linear hits (cyclic=True: every position)")
        if limit is not None and limit < 0:
            raise ValueError("limit must not be negative")
        if not pats:
            return []
        lib, flags = self._c.lib, 0 if cyclic else LOCATE_LINEAR
        offsets = np.zeros(len(pats) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
        flat = np.concatenate(pats) if int(offsets[-1]) else np.zeros(1, dtype=np.uint8)
        hits, total = np.zeros(len(pats) + 1, dtype=np.uint64), C.c_uint64(0)
        rc = lib.bce_hip_locate(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), flags, hits.ctypes.data, None, 0, C.byref(total))
        if rc in (0, E_OVERFLOW) and total.value > max_hits:        # (a batch beyond the call's row limit is sized exactly too)
            raise ValueError("%d hits in all, more than max_hits = %d" % (total.value, max_hits))
        self._c.check(rc, "bce_hip_locate")
        pos = _positions_buffer(total.value)
        self._c.check(lib.bce_hip_locate(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), flags, hits.ctypes.data, pos.ctypes.data,
                                         total.value, C.byref(total)), "bce_hip_locate")
        out = [pos[int(hits[i]):int(hits[i + 1])][:limit].copy() for i in range(len(pats))]
        return out[0] if one else out

    def locate_device(self, patterns_ptr, offsets_ptr, npat, hit_offsets_ptr, positions_ptr, cap, cyclic=False) -> int:
        """bce_hip_locate_device: the hits of `npat` patterns that lie concatenated in device memory (int pointers: the bytes,
        npat + 1 uint64 offsets; out: npat + 1 uint64 hit offsets, up to `cap` uint32 positions) -> the total.  positions_ptr None
        with cap 0 only sizes; a total above cap raises BceError (BCE_HIP_E_OVERFLOW) with the hit offsets written and the
        positions untouched.  Stream rule: as count_device."""
        total = C.c_uint64(0)
        ptr = lambda v: None if v is None else int(v)  # noqa: E731
        self._c.check(self._c.lib.bce_hip_locate_device(self._c.h, ptr(patterns_ptr), ptr(offsets_ptr), int(npat), 0 if cyclic else LOCATE_LINEAR,
                                                        ptr(hit_offsets_ptr), ptr(positions_ptr), int(cap), C.byref(total)), "bce_hip_locate_device")
        return total.value

    def _near_args(self, patterns, k, cyclic, what):
        """-> (one, pats, flat, offsets) of a search with mismatches, judged as count() and locate() judge theirs"""
        if not 0 <= int(k) <= NEAR_MAX_K:
            raise ValueError("k = %r, outside 0 .. %d" % (k, NEAR_MAX_K))
        one = _is_one_pattern(patterns)
        pats = [_as_u8(patterns)] if one else [_as_u8(p) for p in patterns]
        if not cyclic:
            if not self._has_text:
                raise ValueError("a RankFile built from an injected BWT holds no text: only cyclic=True %s are defined" % what)
            if any(len(p) == 0 for p in pats):
                raise ValueError("an empty pattern has no linear %s (cyclic=True: every position, at distance 0)" % what)
        if any(len(p) > NEAR_MAX_LEN for p in pats):
            raise ValueError("a pattern of more than %d bytes" % NEAR_MAX_LEN)
        offsets = np.zeros(len(pats) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
        flat = np.concatenate(pats) if pats and int(offsets[-1]) else np.zeros(1, dtype=np.uint8)
        return one, pats, flat, offsets

    def count_near(self, patterns, k, cyclic=False):
        """How often something occurs in the text that differs from a pattern in at most k bytes (Hamming distance, k = 0 ..
        NEAR_MAX_K), counted on the GPU by backward search that branches (bce_hip_count_near).  `patterns`: one bytes-like -> a
        numpy uint64 array of k + 1 counts, the hits at distance exactly 0 .. k; a sequence -> shape (npat, k + 1).
        cyclic=False: what a sliding window over the text finds; zeros for a pattern longer than the text; an empty pattern
        raises ValueError.  cyclic=True: the hits in the circular text, defined for every length (the empty pattern: n at
        distance 0; k >= m: every position).  Patterns of more than NEAR_MAX_LEN bytes: ValueError."""
        one, pats, flat, offsets = self._near_args(patterns, k, cyclic, "counts")
        out = np.zeros((len(pats), int(k) + 1), dtype=np.uint64)
        if pats:
            self._c.check(self._c.lib.bce_hip_count_near(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), int(k), out.ctypes.data),
                          "bce_hip_count_near")
            if not cyclic:
                out = near_linear_counts(out, pats, self._n, self._text_ends)
        return out[0] if one else out

    def count_near_device(self, patterns_ptr, offsets_ptr, npat, k, counts_ptr):
        """bce_hip_count_near_device: the cyclic counts per distance of `npat` patterns that lie concatenated in device memory (int
        pointers: the bytes, npat + 1 uint64 offsets, npat * (k + 1) uint64 counts out).  Stream rule: as count_device."""
        ptr = lambda v: None if v is None else int(v)  # noqa: E731
        self._c.check(self._c.lib.bce_hip_count_near_device(self._c.h, ptr(patterns_ptr), ptr(offsets_ptr), int(npat), int(k), ptr(counts_ptr)),
                      "bce_hip_count_near_device")

    def locate_near(self, patterns, k, cyclic=False, limit=None, max_hits=1 << 26):
        """Where something occurs that differs from a pattern in at most k bytes: (positions uint32 ascending, dists uint8, the
        distance of each) for one bytes-like, a list of such pairs for a sequence (bce_hip_locate_near).  cyclic, the empty
        pattern and an injected BWT: as locate(), with count_near()'s distances.  `max_hits` and `limit`: locate()'s rules -- a
        sizing call first, ValueError above max_hits before any room is made; limit keeps each pattern's first hits in text
        order and bounds the result, not the work."""
        one, pats, flat, offsets = self._near_args(patterns, k, cyclic, "hits")
        if limit is not None and limit < 0:
            raise ValueError("limit must not be negative")
        if not pats:
            return []
        lib, flags = self._c.lib, 0 if cyclic else LOCATE_LINEAR
        hits, total = np.zeros(len(pats) + 1, dtype=np.uint64), C.c_uint64(0)
        rc = lib.bce_hip_locate_near(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), int(k), flags, hits.ctypes.data, None, None, 0,
                                     C.byref(total))
        if rc in (0, E_OVERFLOW) and total.value > max_hits:
            raise ValueError("%d hits in all, more than max_hits = %d" % (total.value, max_hits))
        self._c.check(rc, "bce_hip_locate_near")
        pos, dist = _positions_buffer(total.value), np.empty(max(total.value, 1), dtype=np.uint8)
        self._c.check(lib.bce_hip_locate_near(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), int(k), flags, hits.ctypes.data,
                                              pos.ctypes.data, dist.ctypes.data, total.value, C.byref(total)), "bce_hip_locate_near")
        out = [(pos[int(hits[i]):int(hits[i + 1])][:limit].copy(), dist[int(hits[i]):int(hits[i + 1])][:limit].copy()) for i in range(len(pats))]
        return out[0] if one else out

    def locate_near_device(self, patterns_ptr, offsets_ptr, npat, k, hit_offsets_ptr, positions_ptr, dists_ptr, cap, cyclic=False) -> int:
        """bce_hip_locate_near_device: locate_device with mismatches (out, beside the positions: up to `cap` uint8 distances) -> the
        total.  positions_ptr and dists_ptr None with cap 0 only sizes.  Stream rule: as count_device."""
        total = C.c_uint64(0)
        ptr = lambda v: None if v is None else int(v)  # noqa: E731
        self._c.check(self._c.lib.bce_hip_locate_near_device(self._c.h, ptr(patterns_ptr), ptr(offsets_ptr), int(npat), int(k),
                                                             0 if cyclic else LOCATE_LINEAR, ptr(hit_offsets_ptr), ptr(positions_ptr), ptr(dists_ptr),
                                                             int(cap), C.byref(total)), "bce_hip_locate_near_device")
        return total.value

    def _edit_args(self, patterns, k, cyclic, what):
        """-> (one, pats, flat, offsets) of a search with edits, judged as _near_args judges its own"""
        if not 0 <= int(k) <= EDIT_MAX_K:
            raise ValueError("k = %r, outside 0 .. %d" % (k, EDIT_MAX_K))
        one = _is_one_pattern(patterns)
        pats = [_as_u8(patterns)] if one else [_as_u8(p) for p in patterns]
        if not cyclic:
            if not self._has_text:
                raise ValueError("a RankFile built from an injected BWT holds no text: only cyclic=True %s are defined" % what)
            if any(len(p) == 0 for p in pats):
                raise ValueError("an empty pattern has no linear %s (cyclic=True: every position, at distance 0)" % what)
        if any(len(p) > EDIT_MAX_LEN for p in pats):
            raise ValueError("a pattern of more than %d bytes" % EDIT_MAX_LEN)
        offsets = np.zeros(len(pats) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
        flat = np.concatenate(pats) if pats and int(offsets[-1]) else np.zeros(1, dtype=np.uint8)
        return one, pats, flat, offsets

    def count_edit(self, patterns, k, cyclic=False):
        """How often something occurs in the text within k edits of a pattern -- substitutions, insertions and deletions, the
        anchored edit distance of include/bce_hip.h, k = 0 .. EDIT_MAX_K -- searched and reduced on the GPU (bce_hip_count_edit).
        `patterns`: one bytes-like -> a numpy uint64 array of k + 1 counts, the positions whose least distance is exactly
        0 .. k; a sequence -> shape (npat, k + 1).  cyclic=False: over the alignments that end inside the text; an empty pattern
        raises ValueError.  cyclic=True: in the circular text, defined for every length.  Needs the suffix array, so a RankFile
        built from an injected BWT is refused (BceError) in either mode.  Patterns of more than EDIT_MAX_LEN bytes: ValueError."""
        one, pats, flat, offsets = self._edit_args(patterns, k, cyclic, "counts")
        out = np.zeros((len(pats), int(k) + 1), dtype=np.uint64)
        if pats:
            self._c.check(self._c.lib.bce_hip_count_edit(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), int(k),
                                                         0 if cyclic else LOCATE_LINEAR, out.ctypes.data), "bce_hip_count_edit")
        return out[0] if one else out

    def count_edit_device(self, patterns_ptr, offsets_ptr, npat, k, counts_ptr, cyclic=False):
        """bce_hip_count_edit_device: the counts per distance of `npat` patterns that lie concatenated in device memory (int
        pointers: the bytes, npat + 1 uint64 offsets, npat * (k + 1) uint64 counts out).  Stream rule: as count_device."""
        ptr = lambda v: None if v is None else int(v)  # noqa: E731
        self._c.check(self._c.lib.bce_hip_count_edit_device(self._c.h, ptr(patterns_ptr), ptr(offsets_ptr), int(npat), int(k),
                                                            0 if cyclic else LOCATE_LINEAR, ptr(counts_ptr)), "bce_hip_count_edit_device")

    def locate_edit(self, patterns, k, cyclic=False, limit=None, max_hits=1 << 26):
        """Where something occurs within k edits of a pattern: (positions uint32 ascending, lens uint16, dists uint8: the length
        and the distance of the best alignment that starts at each) for one bytes-like, a list of such triples for a sequence
        (bce_hip_locate_edit).  cyclic and the empty pattern: as count_edit().  `max_hits` and `limit`: locate()'s rules -- a
        sizing call first (here a whole search), ValueError above max_hits before any room is made; limit keeps each pattern's
        first hits in text order and bounds the result, not the work."""
        one, pats, flat, offsets = self._edit_args(patterns, k, cyclic, "hits")
        if limit is not None and limit < 0:
            raise ValueError("limit must not be negative")
        if not pats:
            return []
        lib, flags = self._c.lib, 0 if cyclic else LOCATE_LINEAR
        hits, total = np.zeros(len(pats) + 1, dtype=np.uint64), C.c_uint64(0)
        rc = lib.bce_hip_locate_edit(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), int(k), flags, hits.ctypes.data, None, None, None, 0,
                                     C.byref(total))
        if rc in (0, E_OVERFLOW) and total.value > max_hits:
            raise ValueError("%d hits in all, more than max_hits = %d" % (total.value, max_hits))
        self._c.check(rc, "bce_hip_locate_edit")
        room = max(total.value, 1)
        pos, lens, dist = _positions_buffer(total.value), np.empty(room, dtype=np.uint16), np.empty(room, dtype=np.uint8)
        self._c.check(lib.bce_hip_locate_edit(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), int(k), flags, hits.ctypes.data,
                                              pos.ctypes.data, lens.ctypes.data, dist.ctypes.data, total.value, C.byref(total)), "bce_hip_locate_edit")
        out = [tuple(a[int(hits[i]):int(hits[i + 1])][:limit].copy() for a in (pos, lens, dist)) for i in range(len(pats))]
        return out[0] if one else out

    def locate_edit_device(self, patterns_ptr, offsets_ptr, npat, k, hit_offsets_ptr, positions_ptr, lens_ptr, dists_ptr, cap, cyclic=False) -> int:
        """bce_hip_locate_edit_device: locate_near_device with edits (out, beside the positions: up to `cap` uint16 lengths and uint8
        distances) -> the total.  positions_ptr, lens_ptr and dists_ptr None with cap 0 only sizes.  Stream rule: as count_device."""
        total = C.c_uint64(0)
        ptr = lambda v: None if v is None else int(v)  # noqa: E731
        self._c.check(self._c.lib.bce_hip_locate_edit_device(self._c.h, ptr(patterns_ptr), ptr(offsets_ptr), int(npat), int(k),
                                                             0 if cyclic else LOCATE_LINEAR, ptr(hit_offsets_ptr), ptr(positions_ptr), ptr(lens_ptr),
                                                             ptr(dists_ptr), int(cap), C.byref(total)), "bce_hip_locate_edit_device")
        return total.value

    def _class_args(self, patterns, cyclic, max_nodes, ignore_case, what):
        """-> (one, pats, flat, offsets, budget) of a search by byte classes, judged as count() and locate() judge theirs"""
        budget = 0 if max_nodes is None else int(max_nodes)
        if max_nodes is not None and not 1 <= budget <= CLASS_MAX_NODES:
            raise ValueError("max_nodes = %r, outside 1 .. %d" % (max_nodes, CLASS_MAX_NODES))
        one = _is_one_class_pattern(patterns)
        pats = [_as_classes(p, ignore_case) for p in ([patterns] if one else patterns)]
        if not cyclic:
            if not self._has_text:
                raise ValueError("a RankFile built from an injected BWT holds no text: only cyclic=True %s are defined" % what)
            if any(len(p) == 0 for p in pats):
                raise ValueError("an empty pattern has no linear %s (cyclic=True: every position)" % what)
        if any(len(p) > CLASS_MAX_LEN for p in pats):
            raise ValueError("a pattern of more than %d classes" % CLASS_MAX_LEN)
        if any(int((np.unpackbits(p.view(np.uint8), axis=1).sum(axis=1) > 1).sum()) > CLASS_MAX_WIDE for p in pats if len(p)):
            raise ValueError("a pattern with more than %d classes of two bytes or more" % CLASS_MAX_WIDE)
        offsets = np.zeros(len(pats) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
        flat = np.concatenate(pats).reshape(-1) if pats and int(offsets[-1]) else np.zeros(8, dtype=np.uint32)
        return one, pats, np.ascontiguousarray(flat, dtype=np.uint32), offsets, budget

    def count_classes(self, patterns, cyclic=False, max_nodes=None, ignore_case=False, return_work=False):
        """How often something occurs in the text that a pattern of byte CLASSES describes: every position of the pattern is a set of
        bytes (bce_hip_count_classes: backward search that branches at every set of two bytes or more, on the GPU).  `patterns`:
        one expression (bytes or str: compile_classes) or one (m, 8) uint32 array of masks -> (count, over); a sequence of them ->
        (counts uint64[npat], over bool[npat]).  over: the pattern's search tree has more than `max_nodes` nodes (None:
        CLASS_DEFAULT_NODES; at most CLASS_MAX_NODES) and the search gave up -- its count is 0, not a part of the answer.
        return_work adds a third value, the nodes counted: exactly the tree's size within budget, something above max_nodes over it.
        cyclic=False: what a sliding window over the text finds; 0 for a pattern longer than the text; an empty pattern raises
        ValueError.  cyclic=True: the hits in the circular text, defined for every length (the empty pattern: n).  ignore_case is
        for expressions (masks are taken as they stand).  More than CLASS_MAX_LEN classes, or more than CLASS_MAX_WIDE of them
        with two bytes or more: ValueError."""
        one, pats, flat, offsets, budget = self._class_args(patterns, cyclic, max_nodes, ignore_case, "counts")
        out, work, status = np.zeros(len(pats), dtype=np.uint64), np.zeros(len(pats), dtype=np.uint64), np.zeros(len(pats), dtype=np.uint32)
        if pats:
            self._c.check(self._c.lib.bce_hip_count_classes(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), budget, out.ctypes.data,
                                                            work.ctypes.data, status.ctypes.data), "bce_hip_count_classes")
        over = status != 0
        if pats and not cyclic:
            out = class_linear_counts(out, pats, self._n, self._text_ends, over)
        res = (int(out[0]), bool(over[0])) if one else (out, over)
        return res + ((int(work[0]) if one else work),) if return_work else res

    def count_classes_device(self, masks_ptr, offsets_ptr, npat, counts_ptr, status_ptr, work_ptr=None, max_nodes=None):
        """bce_hip_count_classes_device: the cyclic counts of `npat` patterns of classes that lie concatenated in device memory (int
        pointers: 8 uint32 words per class, npat + 1 uint64 offsets counted in classes; out: npat uint64 counts, npat uint32
        verdicts and, unless None, npat uint64 node counts).  Stream rule: as count_device."""
        ptr = lambda v: None if v is None else int(v)  # noqa: E731
        self._c.check(self._c.lib.bce_hip_count_classes_device(self._c.h, ptr(masks_ptr), ptr(offsets_ptr), int(npat), int(max_nodes or 0),
                                                               ptr(counts_ptr), ptr(work_ptr), ptr(status_ptr)), "bce_hip_count_classes_device")

    def locate_classes(self, patterns, cyclic=False, limit=None, max_hits=1 << 26, max_nodes=None, ignore_case=False):
        """Where something occurs that a pattern of byte classes describes: (positions uint32 ascending, over) for one pattern,
        (a list of such arrays, over bool[npat]) for a sequence (bce_hip_locate_classes).  Patterns, max_nodes, over and
        ignore_case: as count_classes -- a pattern over budget has no positions.  cyclic, the empty pattern and an injected BWT: as
        locate().  `max_hits` and `limit`: locate()'s rules."""
        one, pats, flat, offsets, budget = self._class_args(patterns, cyclic, max_nodes, ignore_case, "hits")
        if limit is not None and limit < 0:
            raise ValueError("limit must not be negative")
        if not pats:
            return [], np.zeros(0, dtype=bool)
        lib, flags = self._c.lib, 0 if cyclic else LOCATE_LINEAR
        hits, status, total = np.zeros(len(pats) + 1, dtype=np.uint64), np.zeros(len(pats), dtype=np.uint32), C.c_uint64(0)
        rc = lib.bce_hip_locate_classes(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), budget, flags, hits.ctypes.data, status.ctypes.data,
                                        None, 0, C.byref(total))
        if rc in (0, E_OVERFLOW) and total.value > max_hits:
            raise ValueError("%d hits in all, more than max_hits = %d" % (total.value, max_hits))
        self._c.check(rc, "bce_hip_locate_classes")
        pos = _positions_buffer(total.value)
        self._c.check(lib.bce_hip_locate_classes(self._c.h, flat.ctypes.data, offsets.ctypes.data, len(pats), budget, flags, hits.ctypes.data,
                                                 status.ctypes.data, pos.ctypes.data, total.value, C.byref(total)), "bce_hip_locate_classes")
        out = [pos[int(hits[i]):int(hits[i + 1])][:limit].copy() for i in range(len(pats))]
        over = status != 0
        return (out[0], bool(over[0])) if one else (out, over)

    def locate_classes_device(self, masks_ptr, offsets_ptr, npat, hit_offsets_ptr, status_ptr, positions_ptr, cap, cyclic=False, max_nodes=None) -> int:
        """bce_hip_locate_classes_device: locate_device for patterns of classes (in: as count_classes_device; out: npat + 1 uint64 hit
        offsets, npat uint32 verdicts, up to `cap` uint32 positions) -> the total.  positions_ptr None with cap 0 only sizes.
        Stream rule: as count_device."""
        total = C.c_uint64(0)
        ptr = lambda v: None if v is None else int(v)  # noqa: E731
        self._c.check(self._c.lib.bce_hip_locate_classes_device(self._c.h, ptr(masks_ptr), ptr(offsets_ptr), int(npat), int(max_nodes or 0),
                                                                0 if cyclic else LOCATE_LINEAR, ptr(hit_offsets_ptr), ptr(status_ptr),
                                                                ptr(positions_ptr), int(cap), C.byref(total)), "bce_hip_locate_classes_device")
        return total.value

    def _match_flags(self, cyclic, what):
        if not cyclic and not self._has_text:
            raise ValueError("a RankFile built from an injected BWT holds no text: only cyclic=True %s are defined" % what)
        return 0 if cyclic else MATCH_LINEAR

    def match(self, query, max_len, cyclic=False, positions=True):
        """The matching statistics of `query` (a bytes-like, a second buffer) against the text, from the index on the GPU
        (bce_hip_match: backward search from every end position, one lane each) -> (lens, pos), numpy uint32 arrays as long as the
        query.  lens[i]: the length of the longest string that ends at query[i] and occurs in the text, at most min(max_len, i + 1);
        max_len (1 .. 4096) bounds the work per position, a match cut short there is reported as max_len.  pos[i]: where one such
        occurrence starts in the text (which one is not specified), 0xFFFFFFFF where lens[i] == 0; positions=False -> pos is None.
        cyclic=False: occurrences inside the text, pos[i] + lens[i] <= n.  cyclic=True: in the circular text, those across its end
        included -- without positions the only answer a RankFile built from an injected BWT can give (cyclic=False there:
        ValueError, as count(); positions there: BceError, there is no suffix array)."""
        flags = self._match_flags(cyclic, "matches")
        q = _as_u8(query)
        lens = np.zeros(len(q), dtype=np.uint32)
        pos = np.full(len(q), 0xFFFFFFFF, dtype=np.uint32) if positions else None
        self._c.check(self._c.lib.bce_hip_match(self._c.h, q.ctypes.data if len(q) else None, len(q), int(max_len), flags,
                                                lens.ctypes.data if len(q) else None, pos.ctypes.data if positions and len(q) else None), "bce_hip_match")
        return lens, pos

    def match_device(self, query_ptr, q, max_len, lens_ptr, pos_ptr, cyclic=False):
        """bce_hip_match_device: the same for a query of `q` bytes that lies in device memory (int pointers: the bytes; out: q uint32
        lengths and, unless pos_ptr is None, q uint32 positions).  Stream rule: as count_device."""
        ptr = lambda v: None if v is None else int(v)  # noqa: E731
        self._c.check(self._c.lib.bce_hip_match_device(self._c.h, ptr(query_ptr), int(q), int(max_len), self._match_flags(cyclic, "matches"),
                                                       ptr(lens_ptr), ptr(pos_ptr)), "bce_hip_match_device")

    def coverage(self, query, min_len, cyclic=False) -> int:
        """How many bytes of `query` lie in strings of min_len bytes or more (1 .. 4096) that occur in the text: the size of the
        union of all such matches (bce_hip_coverage: searched and reduced on the GPU, 8 bytes come back).  cyclic: as match()."""
        flags = self._match_flags(cyclic, "coverage figures")
        q = _as_u8(query)
        out = C.c_uint64(0)
        self._c.check(self._c.lib.bce_hip_coverage(self._c.h, q.ctypes.data if len(q) else None, len(q), int(min_len), flags, C.byref(out)),
                      "bce_hip_coverage")
        return out.value

    def coverage_device(self, query_ptr, q, min_len, cyclic=False) -> int:
        """bce_hip_coverage_device: coverage() of a query of `q` bytes in device memory (an int pointer).  Stream rule: as count_device."""
        out = C.c_uint64(0)
        self._c.check(self._c.lib.bce_hip_coverage_device(self._c.h, None if query_ptr is None else int(query_ptr), int(q), int(min_len),
                                                          self._match_flags(cyclic, "coverage figures"), C.byref(out)), "bce_hip_coverage_device")
        return out.value

    def lcp(self, max_len):
        """The LCP array of the sorted rotations of the CIRCULAR text (bce_hip_lcp: one lane per row, on the GPU) -> a numpy uint32
        array of n words: lcp[0] = 0, lcp[r] = the bytes on which the rotations in rows r - 1 and r agree, at most max_len
        (1 .. 4096, a work bound).  Not capped at n: equal rotations of a periodic text give max_len.  Needs the suffix array and
        the text: a RankFile built from an injected BWT raises BceError."""
        out = np.zeros(self._n, dtype=np.uint32)
        self._c.check(self._c.lib.bce_hip_lcp(self._c.h, int(max_len), out.ctypes.data), "bce_hip_lcp")
        return out

    def lcp_device(self, max_len, ptr):
        """bce_hip_lcp_device: the same into n uint32 words of device memory (an int pointer).  Stream rule: as count_device."""
        self._c.check(self._c.lib.bce_hip_lcp_device(self._c.h, int(max_len), None if ptr is None else int(ptr)), "bce_hip_lcp_device")

    def kgrams(self, ks):
        """The cyclic k-grams of the text (bce_hip_kgrams: one LCP pass, reduced on the GPU): one k -> a KGram record, a sequence
        of up to 64 -> a list of them.  Fields: distinct (k-grams), once (those that occur once), nlogn_q24 (S_k, the sum of
        N * log2(N) over them in Q24 integers), max_count (the most frequent one's occurrences), max_pos (where one of its
        occurrences starts).  k: 0 .. 4096; k > n wraps around the text."""
        one = isinstance(ks, (int, np.integer))
        karr = np.array([ks] if one else list(ks), dtype=np.int64)
        if len(karr) and (karr.min() < 0 or karr.max() > 0xFFFFFFFF):
            raise ValueError("k is 0 .. %d" % MATCH_MAX_LEN)
        karr = karr.astype(np.uint32)
        out = (KGram * max(len(karr), 1))()
        self._c.check(self._c.lib.bce_hip_kgrams(self._c.h, karr.ctypes.data if len(karr) else None, len(karr), C.addressof(out)), "bce_hip_kgrams")
        recs = [out[i] for i in range(len(karr))]
        return recs[0] if one else recs

    def entropy_profile(self, K):
        """[H_0 .. H_K], the order-k empirical entropies of the circular text in bits per byte, K <= 62: from kgrams(range(K + 2)),
        H_k = max(0, S_k - S_(k+1)) / (n * 2^24)."""
        K = int(K)
        if K < 0 or K + 2 > KGRAMS_MAX:
            raise ValueError("K is 0 .. %d" % (KGRAMS_MAX - 2))
        recs = self.kgrams(range(K + 2))
        return [entropy_from_sums(self._n, recs[k].nlogn_q24, recs[k + 1].nlogn_q24) for k in range(K + 1)]

    def longest_repeat(self, max_len=MATCH_MAX_LEN):
        """(len, pos_a, pos_b): the longest repeat of the circular text -- two rotations that agree on len bytes, len the largest
        such number up to max_len (len == max_len: that many or more).  len == 0: no byte occurs twice, both positions are
        0xFFFFFFFF."""
        ln, a, b = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._c.check(self._c.lib.bce_hip_longest_repeat(self._c.h, int(max_len), C.byref(ln), C.byref(a), C.byref(b)), "bce_hip_longest_repeat")
        return ln.value, a.value, b.value

    def top_kgrams(self, k, limit, with_bytes=True):
        """The `limit` (1 .. 2^20) most frequent cyclic k-grams of the text (bce_hip_top_kgrams: selected, sorted and gathered on the
        GPU) -> a TopKGrams list of (count, pos, row, bytes): by count descending and, among equal counts, in the order of the
        bytes; pos is where one occurrence starts, row the first row of the k-gram among the sorted rotations, bytes the k-gram
        (None with with_bytes=False).  `.distinct` and `.size_hist` come with it.  k: 0 .. 4096; k > n wraps around the text."""
        k, limit = _top_limit(k, limit)
        sound = 1 <= limit <= TOP_MAX and k <= MATCH_MAX_LEN             # (otherwise the library refuses: no room is made)
        out = np.zeros(limit if sound else 1, dtype=TOP_DTYPE)
        raw = np.zeros(max(1, limit * k) if sound else 1, dtype=np.uint8) if with_bytes else None
        found, distinct, hist = C.c_uint32(0), C.c_uint64(0), (C.c_uint64 * 32)()
        self._c.check(self._c.lib.bce_hip_top_kgrams(self._c.h, k, limit, out.ctypes.data, raw.ctypes.data if with_bytes else None,
                                                     limit * k if with_bytes else 0, C.byref(found), C.byref(distinct), C.addressof(hist)), "bce_hip_top_kgrams")
        ents = [(int(e["count"]), int(e["pos"]), int(e["row"]), raw[i * k:(i + 1) * k].tobytes() if with_bytes else None) for i, e in enumerate(out[:found.value])]
        return TopKGrams(ents, distinct.value, hist)

    def top_kgrams_device(self, k, limit, out_ptr, bytes_ptr=None, bytes_cap=0):
        """bce_hip_top_kgrams_device: the same into device memory (int pointers: room for `limit` entries of three uint32 -- count,
        row, pos -- and, unless bytes_ptr is None, for bytes_cap >= limit * k bytes) -> (found, distinct, size_hist).  Stream rule:
        as count_device."""
        k, limit = _top_limit(k, limit)
        found, distinct, hist = C.c_uint32(0), C.c_uint64(0), (C.c_uint64 * 32)()
        self._c.check(self._c.lib.bce_hip_top_kgrams_device(self._c.h, k, limit, None if out_ptr is None else int(out_ptr),
                                                            None if bytes_ptr is None else int(bytes_ptr), int(bytes_cap), C.byref(found), C.byref(distinct),
                                                            C.addressof(hist)), "bce_hip_top_kgrams_device")
        return found.value, distinct.value, [int(v) for v in hist]

    def maximal_repeats(self, min_len=1, max_len=MATCH_MAX_LEN, order="len", limit=100, bytes_per=64):
        """The maximal repeats of the circular text (bce_hip_maximal_repeats: found, weighed, selected, sorted and gathered on the
        GPU): the strings of min_len bytes or more that occur twice or more and can be extended neither to the right nor to the left
        without losing an occurrence -> (entries, strings, info).  entries: a numpy record array (len, count, row, pos), heaviest
        first -- order "len": longest first, the most frequent among equal lengths; "count": most frequent first; "gain":
        len * (count - 1) -- and equal weights in row order; len == max_len means "max_len bytes or more".  strings: the first
        min(len, bytes_per) bytes of every entry (None with bytes_per=0).  info: a dict (total, capped, bwt_runs, found)."""
        min_len, max_len, order, limit, bytes_per = _maxrep_args(min_len, max_len, order, limit, bytes_per)
        sound = 1 <= limit <= TOP_MAX and bytes_per <= MAXREP_BYTES_MAX  # (otherwise the library refuses: no room is made)
        out = np.zeros(limit if sound else 1, dtype=MAXREP_DTYPE)
        raw = np.zeros(max(1, limit * bytes_per) if sound else 1, dtype=np.uint8) if bytes_per else None
        info = MaxRepInfo()
        self._c.check(self._c.lib.bce_hip_maximal_repeats(self._c.h, min_len, max_len, order, limit, out.ctypes.data, raw.ctypes.data if bytes_per else None,
                                                          bytes_per, limit * bytes_per if bytes_per else 0, C.byref(info)), "bce_hip_maximal_repeats")
        ents = out[:info.found].copy()
        strs = [raw[i * bytes_per:i * bytes_per + min(int(e["len"]), bytes_per)].tobytes() for i, e in enumerate(ents)] if bytes_per else None
        return ents, strs, info.as_dict()

    def maximal_repeats_device(self, min_len, max_len, order, limit, out_ptr, bytes_ptr=None, bytes_per=0, bytes_cap=0):
        """bce_hip_maximal_repeats_device: the same into device memory (int pointers: room for `limit` entries of four uint32 -- len,
        count, row, pos -- and, unless bytes_ptr is None, for bytes_cap >= limit * bytes_per bytes, a slot of bytes_per per entry,
        zero behind the repeat) -> the info dict.  Stream rule: as count_device."""
        min_len, max_len, order, limit, bytes_per = _maxrep_args(min_len, max_len, order, limit, bytes_per)
        info = MaxRepInfo()
        self._c.check(self._c.lib.bce_hip_maximal_repeats_device(self._c.h, min_len, max_len, order, limit, None if out_ptr is None else int(out_ptr),
                                                                 None if bytes_ptr is None else int(bytes_ptr), bytes_per, int(bytes_cap), C.byref(info)),
                      "bce_hip_maximal_repeats_device")
        return info.as_dict()

    def parse(self, query, min_len, max_len=PARSE_MAX_LEN):
        """`query` (a bytes-like, a second buffer) written as copies out of the text plus the bytes that are new (bce_hip_parse: the
        linear matching statistics at bound max_len, then from the query's end a copy of lens[e] bytes wherever lens[e] >= min_len,
        else a literal byte; on the GPU) -> (ops, lits, info): ops a numpy record array (len, src) in query order, src == OP_LITERAL
        for a run of literal bytes -- the next len bytes of lits (uint8) -- else text[src : src + len]; info a dict (nops, nlits,
        ncopies, copied).  A sizing call, then the full call; each runs the search."""
        q = _as_u8(query)
        info = ParseInfo()
        qp = q.ctypes.data if len(q) else None
        self._c.check(self._c.lib.bce_hip_parse(self._c.h, qp, len(q), int(min_len), int(max_len), None, 0, None, 0, C.byref(info)), "bce_hip_parse")
        ops, lits = np.zeros(info.nops, dtype=OP_DTYPE), np.zeros(info.nlits, dtype=np.uint8)
        if len(q):
            self._c.check(self._c.lib.bce_hip_parse(self._c.h, qp, len(q), int(min_len), int(max_len), ops.ctypes.data, len(ops),
                                                    lits.ctypes.data if len(lits) else None, len(lits), C.byref(info)), "bce_hip_parse")
        return ops, lits, info.as_dict()

    def parse_device(self, query_ptr, q, min_len, max_len=PARSE_MAX_LEN, ops_ptr=None, ops_cap=0, lits_ptr=None, lits_cap=0):
        """bce_hip_parse_device: the same for a query of `q` bytes in device memory, into `ops_cap` ops (8 bytes each, 4-byte
        aligned) at ops_ptr and `lits_cap` bytes at lits_ptr (int pointers; both None with caps 0: a sizing call) -> the info dict.
        More ops or literal bytes than room: BceError with status E_OVERFLOW, nothing written.  Stream rule: as count_device."""
        info = ParseInfo()
        self._c.check(self._c.lib.bce_hip_parse_device(self._c.h, _ptr(query_ptr), int(q), int(min_len), int(max_len), _ptr(ops_ptr), int(ops_cap),
                                                       _ptr(lits_ptr), int(lits_cap), C.byref(info)), "bce_hip_parse_device")
        return info.as_dict()

    def lpf(self, max_len=PARSE_MAX_LEN, sources=True):
        """The longest previous factors of the LINEAR text (bce_hip_lpf: all nearest smaller values over the suffix array, then two
        compares per row, on the GPU) -> (lpf, src), numpy uint32 arrays of n words: lpf[i] = the most bytes, at most
        min(max_len, n - i), that text[i:] shares with text[j:] for some j < i (overlap allowed), src[i] = one such j, OP_LITERAL
        (0xFFFFFFFF) where lpf[i] == 0.  sources=False: src is None.  Needs the suffix array and the text, as lcp()."""
        out = np.zeros(self._n, dtype=np.uint32)
        src = np.zeros(self._n, dtype=np.uint32) if sources else None
        self._c.check(self._c.lib.bce_hip_lpf(self._c.h, int(max_len), out.ctypes.data, src.ctypes.data if sources else None), "bce_hip_lpf")
        return out, src

    def lpf_device(self, max_len=PARSE_MAX_LEN, lpf_ptr=None, src_ptr=None):
        """bce_hip_lpf_device: the same into n uint32 words each of device memory (int pointers; src_ptr may be None).  Stream
        rule: as count_device."""
        self._c.check(self._c.lib.bce_hip_lpf_device(self._c.h, int(max_len), _ptr(lpf_ptr), _ptr(src_ptr)), "bce_hip_lpf_device")

    def self_parse(self, min_len, max_len=PARSE_MAX_LEN):
        """The text written as copies of its OWN earlier bytes plus the bytes that are new (bce_hip_self_parse: from position 0 a
        copy of lpf[s] bytes from src[s] wherever lpf[s] >= min_len, else a literal byte; the greedy LZ77 factorisation, on the
        GPU) -> (ops, lits, info) as parse() gives them, in text order.  Every copy's src lies in front of its destination, so the
        list decodes from left to right without the text; patch(ops, lits) gives the text back as well.  With min_len 1,
        info["ncopies"] + info["nlits"] is z, the number of LZ77 phrases."""
        info = ParseInfo()
        self._c.check(self._c.lib.bce_hip_self_parse(self._c.h, int(min_len), int(max_len), None, 0, None, 0, C.byref(info)), "bce_hip_self_parse")
        ops, lits = np.zeros(info.nops, dtype=OP_DTYPE), np.zeros(info.nlits, dtype=np.uint8)
        self._c.check(self._c.lib.bce_hip_self_parse(self._c.h, int(min_len), int(max_len), ops.ctypes.data, len(ops),
                                                     lits.ctypes.data if len(lits) else None, len(lits), C.byref(info)), "bce_hip_self_parse")
        return ops, lits, info.as_dict()

    def self_parse_device(self, min_len, max_len=PARSE_MAX_LEN, ops_ptr=None, ops_cap=0, lits_ptr=None, lits_cap=0):
        """bce_hip_self_parse_device: the same into `ops_cap` ops (8 bytes each, 4-byte aligned) at ops_ptr and `lits_cap` bytes at
        lits_ptr (int pointers; both None with caps 0: a sizing call) -> the info dict.  More ops or literal bytes than room:
        BceError with status E_OVERFLOW, nothing written.  Stream rule: as count_device."""
        info = ParseInfo()
        self._c.check(self._c.lib.bce_hip_self_parse_device(self._c.h, int(min_len), int(max_len), _ptr(ops_ptr), int(ops_cap), _ptr(lits_ptr),
                                                            int(lits_cap), C.byref(info)), "bce_hip_self_parse_device")
        return info.as_dict()

    def patch(self, ops, lits):
        """The bytes that `ops` (a record array as parse() gives, or an (nops, 2) uint32 array of (len, src)) and `lits` describe
        over the text (bce_hip_patch: validated and copied on the GPU) -> a numpy uint8 array.  Any well-formed list is taken; one
        that is not raises BceError (status -1) with the reason."""
        ops, lits = _as_ops(ops), _as_u8(lits)
        total = C.c_uint64(0)
        args = (self._c.h, ops.ctypes.data if len(ops) else None, len(ops), lits.ctypes.data if len(lits) else None, len(lits))
        self._c.check(self._c.lib.bce_hip_patch(*(args + (None, 0, C.byref(total)))), "bce_hip_patch")
        out = np.zeros(total.value, dtype=np.uint8)
        if total.value:
            self._c.check(self._c.lib.bce_hip_patch(*(args + (out.ctypes.data, len(out), C.byref(total)))), "bce_hip_patch")
        return out

    def patch_device(self, ops_ptr, nops, lits_ptr, nlits, out_ptr=None, cap=0) -> int:
        """bce_hip_patch_device: the same with the ops, the literal bytes and the result in device memory (int pointers; out_ptr
        None with cap 0 validates and sizes) -> the result's bytes.  Stream rule: as count_device."""
        total = C.c_uint64(0)
        self._c.check(self._c.lib.bce_hip_patch_device(self._c.h, _ptr(ops_ptr), int(nops), _ptr(lits_ptr), int(nlits), _ptr(out_ptr), int(cap),
                                                       C.byref(total)), "bce_hip_patch_device")
        return total.value

    def close(self):
        self._c.close()


def _as_ops(ops):
    """ops as contiguous (len, src) pairs of little-endian uint32: a record array of OP_DTYPE, or anything of shape (nops, 2)."""
    if isinstance(ops, np.ndarray) and ops.dtype == OP_DTYPE:
        return np.ascontiguousarray(ops)
    a = np.ascontiguousarray(np.asarray(ops, dtype=np.uint32).reshape(-1, 2))
    return a.view(OP_DTYPE).reshape(-1)


def _archive_into(c, out=None):
    """The archive of context `c`'s last encode: into `out` where that is a large enough uint8 array, else a new bytearray."""
    lib, h = c.lib, c.h
    n = C.c_size_t()
    c.check(lib.bce_hip_archive_size(h, C.byref(n)), "bce_hip_archive_size")
    if out is not None and isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable and out.size >= n.value:
        c.check(lib.bce_hip_archive_copy(h, out.ctypes.data, out.size), "bce_hip_archive_copy")
        return memoryview(out.reshape(-1))[:n.value]
    # the library lays the archive out straight into this buffer (one copy of the coded streams, none in Python):
    # a bytearray compares, hashes, slices and writes like bytes
    out = bytearray(n.value)
    view = (C.c_uint8 * n.value).from_buffer(out)
    c.check(lib.bce_hip_archive_copy(h, C.addressof(view), n.value), "bce_hip_archive_copy")
    del view
    return out


class BCE:
    """The reference's BCE<AdaptiveCoder<31>, ...> (bce.cpp:1111-1374), encode side."""

    max = 31

    def __init__(self, config=None, symbol_capacity=0):
        if config is not None and len(config) != CONFIG_BYTES:
            raise ValueError("Config not found or wrong size.")   # bce.cpp:629-631
        self.config = None if config is None else bytes(config)
        self.symbol_capacity = symbol_capacity

    @staticmethod
    def load_config(path):
        with open(path, "rb") as f:
            return f.read()

    def _apply(self, rf):
        self._apply_ctx(rf._c)

    def _apply_ctx(self, c):
        lib, h = c.lib, c.h
        cfg = None
        if self.config is not None:
            cfg = _as_u8(self.config)
        c.check(lib.bce_hip_set_config(h, cfg.ctypes.data if cfg is not None else None), "bce_hip_set_config")
        c.check(lib.bce_hip_set_symbol_capacity(h, self.symbol_capacity), "bce_hip_set_symbol_capacity")

    def encode(self, rf: RankFile, out=None):
        """-> the archive (a bytearray).  With `out` (a writable C-contiguous uint8 numpy array that is large enough) the
        library lays the archive out there -- the C ABI's own shape: the caller's buffer, e.g. pinned memory a collective
        sends from -- and a memoryview of its first len(archive) bytes comes back; too small an `out` is ignored."""
        self._apply(rf)
        rf._c.check(rf._c.lib.bce_hip_encode(rf._c.h), "bce_hip_encode")
        return _archive_into(rf._c, out)

    def compress_loaded(self, c, load, out=None):
        """The one-shot entry points (bce_hip_compress / bce_hip_compress_device: `load(ctx handle, length pointer)` calls one of
        them): the library runs the stages in the order it likes best -- the enumeration's early rounds before K1 has finished.
        -> the archive, as encode()."""
        self._apply_ctx(c)
        n = C.c_size_t()
        load(c.h, C.byref(n))
        return _archive_into(c, out)

    # --- BCE::code one round at a time (parity tests) ---
    def code_begin(self, rf: RankFile):
        self._apply(rf)
        rf._c.check(rf._c.lib.bce_hip_enum_begin(rf._c.h), "bce_hip_enum_begin")

    def code_nodes(self, rf: RankFile, plane):
        cap = rf.size() // 2 + 2
        out = np.empty((cap, 3), dtype=np.uint32)
        cnt = C.c_uint32()
        rf._c.check(rf._c.lib.bce_hip_enum_nodes(rf._c.h, plane, out.ctypes.data, cap, C.byref(cnt)), "bce_hip_enum_nodes")
        return out[:cnt.value].copy()

    def code_round(self, rf: RankFile):
        nxt = C.c_uint64()
        rf._c.check(rf._c.lib.bce_hip_enum_round(rf._c.h, C.byref(nxt)), "bce_hip_enum_round")
        return nxt.value

    def code_symbols(self, rf: RankFile, cap):
        out = np.empty((max(cap, 1), 6), dtype=np.uint32)
        cnt = C.c_uint64()
        rf._c.check(rf._c.lib.bce_hip_enum_symbols(rf._c.h, out.ctypes.data, cap, C.byref(cnt)), "bce_hip_enum_symbols")
        return out[:cnt.value].copy()

    def code_model(self, rf: RankFile, cap):
        out = np.empty((max(cap, 1), 3), dtype=np.uint32)
        cnt = C.c_uint64()
        rf._c.check(rf._c.lib.bce_hip_enum_model(rf._c.h, out.ctypes.data, cap, C.byref(cnt)), "bce_hip_enum_model")
        return out[:cnt.value].copy()


class Model:
    """Test hook: K4 (the adaptive model's kernels) alone, on symbol records of the caller's choosing (bce_hip_model_begin /
    bce_hip_model_flush).  Needs no input; counters persist from flush to flush until the next begin()."""

    def __init__(self, config=None, device=0, ctx=None):
        if config is not None and len(config) != CONFIG_BYTES:
            raise ValueError("Config not found or wrong size.")
        self._own = ctx is None
        self._c = ctx or _Ctx(device)
        self.config = None if config is None else bytes(config)

    def begin(self):
        cfg = None if self.config is None else _as_u8(self.config)
        self._c.check(self._c.lib.bce_hip_set_config(self._c.h, cfg.ctypes.data if cfg is not None else None), "bce_hip_set_config")
        self._c.check(self._c.lib.bce_hip_model_begin(self._c.h), "bce_hip_model_begin")

    def flush(self, key_words, esc_words):
        """-> (the raw 64-bit model records, in the records' order; the long runs the flush queued)"""
        kw = np.ascontiguousarray(key_words, dtype=np.uint32)
        ew = np.ascontiguousarray(esc_words, dtype=np.uint32)
        if kw.shape != ew.shape or kw.ndim != 1:
            raise ValueError("key and escape words: two one-dimensional arrays of one length")
        out = np.empty(len(kw), dtype=np.uint64)
        nq = C.c_uint32()
        self._c.check(self._c.lib.bce_hip_model_flush(self._c.h, kw.ctypes.data, ew.ctypes.data, len(kw), out.ctypes.data, C.byref(nq)),
                      "bce_hip_model_flush")
        return out, nq.value

    def close(self):
        if self._own:
            self._c.close()


def stats(rf: RankFile) -> dict:
    st = Stats()
    rf._c.check(rf._c.lib.bce_hip_get_stats(rf._c.h, C.byref(st)), "bce_hip_get_stats")
    return st.as_dict()


def stats_of(ctx) -> dict:
    """The statistics of the context's last compression (as stats(rf), without the RankFile)."""
    st = Stats()
    ctx.check(ctx.lib.bce_hip_get_stats(ctx.h, C.byref(st)), "bce_hip_get_stats")
    return st.as_dict()


def compress(data, config=None, device=0, ctx=None) -> bytes:
    """`bce -c` on an in-memory buffer (bce.cpp:1403-1427 minus file I/O) -> archive bytes."""
    a = _as_u8(data)
    if len(a) == 0:
        raise BceError(-1, "RankFile", "empty input")
    c = ctx or _Ctx(device)
    try:
        return BCE(config).compress_loaded(
            c, lambda h, ln: c.check(c.lib.bce_hip_compress(h, a.ctypes.data, len(a), None, 0, ln), "bce_hip_compress"))
    finally:
        if ctx is None:
            c.close()


def count(data, patterns, device=0, ctx=None):
    """How often `patterns` (one bytes-like -> int, a sequence -> numpy uint64 array) occur in `data`, overlapping matches
    counted: K1 and K2 index the data on the GPU, RankFile.count asks the index."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.count(patterns)
    finally:
        if ctx is None:
            rf.close()


def locate(data, patterns, cyclic=False, limit=None, max_hits=1 << 26, device=0, ctx=None):
    """Where `patterns` occur in `data` (one bytes-like -> a numpy uint32 array of ascending byte offsets, a sequence -> a list of
    them): K1 and K2 index the data on the GPU, RankFile.locate asks the index and K1's suffix array."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.locate(patterns, cyclic=cyclic, limit=limit, max_hits=max_hits)
    finally:
        if ctx is None:
            rf.close()


def count_near(data, patterns, k, cyclic=False, device=0, ctx=None):
    """The hits of `patterns` in `data` within k mismatches, per distance (RankFile.count_near): K1 and K2 index the data on the
    GPU, the branching backward search asks the index."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.count_near(patterns, k, cyclic=cyclic)
    finally:
        if ctx is None:
            rf.close()


def locate_near(data, patterns, k, cyclic=False, limit=None, max_hits=1 << 26, device=0, ctx=None):
    """Where `patterns` occur in `data` within k mismatches -> (positions, dists) as RankFile.locate_near."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.locate_near(patterns, k, cyclic=cyclic, limit=limit, max_hits=max_hits)
    finally:
        if ctx is None:
            rf.close()


def count_edit(data, patterns, k, cyclic=False, device=0, ctx=None):
    """The hits of `patterns` in `data` within k edits, per distance (RankFile.count_edit): K1 and K2 index the data on the GPU,
    the search and its reduce ask the index and K1's suffix array."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.count_edit(patterns, k, cyclic=cyclic)
    finally:
        if ctx is None:
            rf.close()


def locate_edit(data, patterns, k, cyclic=False, limit=None, max_hits=1 << 26, device=0, ctx=None):
    """Where `patterns` occur in `data` within k edits -> (positions, lens, dists) as RankFile.locate_edit."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.locate_edit(patterns, k, cyclic=cyclic, limit=limit, max_hits=max_hits)
    finally:
        if ctx is None:
            rf.close()


def count_classes(data, patterns, cyclic=False, max_nodes=None, ignore_case=False, device=0, ctx=None):
    """The hits of patterns of byte classes in `data` -> (counts, over) as RankFile.count_classes: K1 and K2 index the data on the
    GPU, the branching backward search asks the index."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.count_classes(patterns, cyclic=cyclic, max_nodes=max_nodes, ignore_case=ignore_case)
    finally:
        if ctx is None:
            rf.close()


def locate_classes(data, patterns, cyclic=False, limit=None, max_hits=1 << 26, max_nodes=None, ignore_case=False, device=0, ctx=None):
    """Where patterns of byte classes occur in `data` -> (positions, over) as RankFile.locate_classes."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.locate_classes(patterns, cyclic=cyclic, limit=limit, max_hits=max_hits, max_nodes=max_nodes, ignore_case=ignore_case)
    finally:
        if ctx is None:
            rf.close()


def match(data, query, max_len, cyclic=False, positions=True, device=0, ctx=None):
    """The matching statistics of `query` against `data` -> (lens, pos) as RankFile.match: K1 and K2 index the data on the GPU,
    every end position of the query is searched in the index."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.match(query, max_len, cyclic=cyclic, positions=positions)
    finally:
        if ctx is None:
            rf.close()


def coverage(data, query, min_len, cyclic=False, device=0, ctx=None) -> int:
    """How many bytes of `query` lie in strings of min_len bytes or more that occur in `data` (RankFile.coverage)."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.coverage(query, min_len, cyclic=cyclic)
    finally:
        if ctx is None:
            rf.close()


def parse(data, query, min_len, max_len=PARSE_MAX_LEN, device=0, ctx=None):
    """`query` as copies out of `data` plus literal bytes -> (ops, lits, info) as RankFile.parse: K1 and K2 index the data on the GPU."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.parse(query, min_len, max_len)
    finally:
        if ctx is None:
            rf.close()


def patch(data, ops, lits, device=0, ctx=None):
    """The bytes that `ops` and `lits` describe over `data` (RankFile.patch; the data is loaded, not indexed) -> a numpy uint8 array."""
    rf = RankFile(data, device=device, ctx=ctx, build=False, index=False)
    try:
        return rf.patch(ops, lits)
    finally:
        if ctx is None:
            rf.close()


def delta(base, new, min_len=16, max_len=PARSE_MAX_LEN, device=0, ctx=None) -> bytes:
    """`new` as a delta against `base`: a "BCED" file (container.pack_delta) of the parse of `new` in the index of `base`, with the
    CRC-32 of both sides -- the base's from the context that indexed it, on the GPU.  An empty base raises BceError."""
    from . import container
    rf = RankFile(base, device=device, ctx=ctx)
    try:
        ops, lits, _ = rf.parse(new, min_len, max_len)
        return container.pack_delta(rf.size(), input_crc32(rf._c), len(_as_u8(new)), crc32(new), min_len, max_len, ops, lits)
    finally:
        if ctx is None:
            rf.close()


def apply_delta(base, blob, device=0, ctx=None) -> bytes:
    """What delta(base, ...) was made from, rebuilt from `base` and the delta file `blob`.  The file is read and judged before
    anything goes to a device; a base of another size or CRC-32, or a result with another CRC-32: ChecksumError, nothing returned."""
    from . import container
    d = container.unpack_delta(blob)
    base = _as_u8(base)
    if len(base) != d["n"]:
        raise ChecksumError(0, d["base_crc"], crc32(base))
    rf = RankFile(base, device=device, ctx=ctx, build=False, index=False)
    try:
        have = input_crc32(rf._c)
        if have != d["base_crc"]:
            raise ChecksumError(0, d["base_crc"], have)
        out = rf.patch(d["ops"], d["lits"])
        if len(out) != d["q"] or crc32(out) != d["crc"]:
            raise ChecksumError(0, d["crc"], crc32(out))
        return out.tobytes()
    finally:
        if ctx is None:
            rf.close()


def lpf(data, max_len=PARSE_MAX_LEN, sources=True, device=0, ctx=None):
    """The longest previous factors of `data` -> (lpf, src) as RankFile.lpf: K1 and K2 index the data on the GPU."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.lpf(max_len, sources=sources)
    finally:
        if ctx is None:
            rf.close()


def self_parse(data, min_len, max_len=PARSE_MAX_LEN, device=0, ctx=None):
    """`data` as copies of its own earlier bytes plus literal bytes -> (ops, lits, info) as RankFile.self_parse."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.self_parse(min_len, max_len)
    finally:
        if ctx is None:
            rf.close()


SUFCHECK_REASONS = (None, "range", "missing", "order")   # BCE_HIP_SUFCHECK_*: what bce_hip_sufcheck found, by its reason word


def _sufcheck_verdict(reason, bad):
    return None if reason == 0 else (SUFCHECK_REASONS[reason], int(bad))


def suffix_array(data, inverse=False, device=0, ctx=None):
    """The suffix array of `data` (bytes-like, 0 < n < 2^31 - 1), sorted on the GPU (bce_hip_suffix_array: K1 on data + a unique
    sentinel) -> a numpy int32 array of n rows, or (sa, isa) with inverse=True, isa[sa[r]] == r.  The context's compression state
    is dropped, as by the libdivsufsort seam's divbwt."""
    a = _as_u8(data)
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        sa = np.empty(len(a), dtype=np.int32)
        isa = np.empty(len(a), dtype=np.int32) if inverse else None
        c.check(c.lib.bce_hip_suffix_array(c.h, a.ctypes.data if len(a) else None, len(a), sa.ctypes.data, isa.ctypes.data if inverse else None),
                "bce_hip_suffix_array")
        return (sa, isa) if inverse else sa
    finally:
        if own:
            c.close()


def sufcheck(data, sa, device=0, ctx=None):
    """Is `sa` (n 32-bit words, any values) the suffix array of `data` (n bytes)?  Checked on the GPU in linear time
    (bce_hip_sufcheck) -> None for a sound array, else (reason, index): ("range", the first row with an entry outside [0, n)),
    ("missing", the first text position no row names) or ("order", the first row that stands below a larger suffix).  Valid in any
    state of `ctx`; nothing of a compression under way is touched."""
    a = _as_u8(data)
    s = np.ascontiguousarray(sa)
    if s.dtype.itemsize != 4 or s.dtype.kind not in "iu" or s.ndim != 1 or len(s) != len(a):
        raise ValueError("sa must hold one 32-bit integer per byte of data")
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        bad, reason = C.c_uint64(0), C.c_uint32(0)
        c.check(c.lib.bce_hip_sufcheck(c.h, a.ctypes.data if len(a) else None, s.ctypes.data if len(a) else None, len(a), C.byref(bad), C.byref(reason)),
                "bce_hip_sufcheck")
        return _sufcheck_verdict(reason.value, bad.value)
    finally:
        if own:
            c.close()


def suffix_array_device(ptr, n, sa_ptr, isa_ptr=None, ctx=None):
    """bce_hip_suffix_array_device on raw device pointers: the `n` bytes at `ptr` -> n uint32 words at `sa_ptr` and, unless None, at
    `isa_ptr`.  -> the status (0, or a negative BCE_HIP_E_* that the caller asserts).  Stream rule: as decompress_to_device."""
    return ctx.lib.bce_hip_suffix_array_device(ctx.h, _ptr(ptr), int(n), _ptr(sa_ptr), _ptr(isa_ptr))


def sufcheck_device(ptr, sa_ptr, n, ctx):
    """bce_hip_sufcheck_device on raw device pointers: `n` bytes at `ptr`, n uint32 words at `sa_ptr` -> (status, verdict), the
    verdict as sufcheck gives it (None where the status is not 0)."""
    bad, reason = C.c_uint64(0), C.c_uint32(0)
    rc = ctx.lib.bce_hip_sufcheck_device(ctx.h, _ptr(ptr), _ptr(sa_ptr), int(n), C.byref(bad), C.byref(reason))
    return rc, (_sufcheck_verdict(reason.value, bad.value) if rc == 0 else None)


def nsv_device(ptr_vals, n, ptr_psv, ptr_nsv, ctx):
    """Test hook (bce_hip_nsv_device): all nearest smaller values of `n` uint32 words at a device pointer, strictly smaller, into
    two arrays of n words (0xFFFFFFFF: none) -> the status."""
    return ctx.lib.bce_hip_nsv_device(ctx.h, _ptr(ptr_vals), int(n), _ptr(ptr_psv), _ptr(ptr_nsv))


def self_parse_of_lpf_device(ptr_lpf, ptr_src, ptr_text, n, min_len, ctx, ptr_ops=None, ops_cap=0, ptr_lits=None, lits_cap=0):
    """Test hook (bce_hip_self_parse_of_lpf_device): the self-parse's chain alone on `n` uint32 lengths (lpf[i] <= n - i), sources
    (ptr_src may be None: src = 0) and text bytes at device pointers -> (status, info dict); both outputs None with caps 0 sizes."""
    info = ParseInfo()
    rc = ctx.lib.bce_hip_self_parse_of_lpf_device(ctx.h, _ptr(ptr_lpf), _ptr(ptr_src), _ptr(ptr_text), int(n), int(min_len), _ptr(ptr_ops), int(ops_cap),
                                                  _ptr(ptr_lits), int(lits_cap), C.byref(info))
    return rc, info.as_dict()


def parse_of_lengths_device(ptr_len, ptr_pos, ptr_query, q, min_len, ctx, ptr_ops=None, ops_cap=0, ptr_lits=None, lits_cap=0):
    """Test hook (bce_hip_parse_of_lengths_device): the parse alone on `q` uint32 lengths (lens[i] <= i + 1), positions (ptr_pos may
    be None: src = 0) and query bytes at device pointers -> (status, info dict); both outputs None with caps 0 sizes."""
    info = ParseInfo()
    rc = ctx.lib.bce_hip_parse_of_lengths_device(ctx.h, _ptr(ptr_len), _ptr(ptr_pos), _ptr(ptr_query), int(q), int(min_len), _ptr(ptr_ops), int(ops_cap),
                                                 _ptr(ptr_lits), int(lits_cap), C.byref(info))
    return rc, info.as_dict()


def kgrams(data, ks, device=0, ctx=None):
    """The cyclic k-grams of `data` (RankFile.kgrams): K1 and K2 index the data on the GPU, the LCP array of the sorted rotations is
    built and reduced there."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.kgrams(ks)
    finally:
        if ctx is None:
            rf.close()


def maximal_repeats(data, min_len=1, max_len=MATCH_MAX_LEN, order="len", limit=100, bytes_per=64, device=0, ctx=None):
    """The maximal repeats of `data` (RankFile.maximal_repeats): indexed, found, selected and sorted on the GPU."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.maximal_repeats(min_len=min_len, max_len=max_len, order=order, limit=limit, bytes_per=bytes_per)
    finally:
        if ctx is None:
            rf.close()


def top_kgrams(data, k, limit, with_bytes=True, device=0, ctx=None):
    """The `limit` most frequent cyclic k-grams of `data` (RankFile.top_kgrams): indexed, selected and sorted on the GPU."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.top_kgrams(k, limit, with_bytes=with_bytes)
    finally:
        if ctx is None:
            rf.close()


def entropy_profile(data, K, device=0, ctx=None):
    """[H_0 .. H_K] of the circular text `data`, in bits per byte (RankFile.entropy_profile)."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.entropy_profile(K)
    finally:
        if ctx is None:
            rf.close()


def longest_repeat(data, max_len=MATCH_MAX_LEN, device=0, ctx=None):
    """(len, pos_a, pos_b) of the longest repeat of the circular text `data` (RankFile.longest_repeat)."""
    rf = RankFile(data, device=device, ctx=ctx)
    try:
        return rf.longest_repeat(max_len)
    finally:
        if ctx is None:
            rf.close()


def compress_device(device_ptr, n, config=None, device=0, ctx=None, out=None, symbol_capacity=0):
    """Same with the input already resident in HBM.  Returns (archive bytes, stats dict); `out`: see BCE.encode;
    `symbol_capacity`: records between two model flushes (0: the library's choice)."""
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        arch = BCE(config, symbol_capacity).compress_loaded(
            c, lambda h, ln: c.check(c.lib.bce_hip_compress_device(h, int(device_ptr), int(n), None, 0, ln), "bce_hip_compress_device"), out=out)
        return arch, stats_of(c)
    finally:
        if own:
            c.close()


class Estimate:
    """What bce_hip_estimate reports: the size of the archive `compress` would make, and where its bits go.

    .bytes           the archive's size in bytes (framing + the eight streams)
    .plane_cost_q24  per plane, the bits its coder codes in unsigned Q24 fixed point (integer sums: exact, order-independent)
    .plane_bits      the same as floats (Q24 sum / 2**24)
    .plane_steps     per plane, the adaptive coder's calls (model records); their sum is stats(...)["symbols"]"""

    __slots__ = ("bytes", "plane_cost_q24", "plane_steps")

    def __init__(self, nbytes, plane_cost_q24, plane_steps):
        self.bytes, self.plane_cost_q24, self.plane_steps = int(nbytes), [int(v) for v in plane_cost_q24], [int(v) for v in plane_steps]

    @property
    def plane_bits(self):
        return [v / float(1 << 24) for v in self.plane_cost_q24]

    def __repr__(self):
        return "Estimate(bytes=%d, plane_bits=[%s])" % (self.bytes, ", ".join("%.1f" % b for b in self.plane_bits))


def _estimate(c, config, call, where):
    cfg = None if config is None else _as_u8(bytes(config))
    if cfg is not None and len(cfg) != CONFIG_BYTES:
        raise ValueError("Config not found or wrong size.")
    c.check(c.lib.bce_hip_set_config(c.h, cfg.ctypes.data if cfg is not None else None), "bce_hip_set_config")
    cost, steps, nbytes = (C.c_uint64 * 8)(), (C.c_uint64 * 8)(), C.c_size_t()
    c.check(call(cost, steps, C.byref(nbytes)), where)
    return Estimate(nbytes.value, list(cost), list(steps))


def estimate(data, config=None, device=0, ctx=None) -> Estimate:
    """The size `compress(data, config)` would give, without coding: K1..K4 run, the range coders do not
    (bce_hip_estimate_host).  -> Estimate."""
    a = _as_u8(data)
    if len(a) == 0:
        raise BceError(-1, "estimate", "empty input")
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        return _estimate(c, config, lambda *out: c.lib.bce_hip_estimate_host(c.h, a.ctypes.data, len(a), *out), "bce_hip_estimate_host")
    finally:
        if own:
            c.close()


def estimate_device(device_ptr, n, config=None, device=0, ctx=None) -> Estimate:
    """The same with the input already resident in HBM (bce_hip_estimate_device); stream rule as decompress_to_device."""
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        ptr = None if device_ptr is None else int(device_ptr)
        return _estimate(c, config, lambda *out: c.lib.bce_hip_estimate_device(c.h, ptr, int(n), *out), "bce_hip_estimate_device")
    finally:
        if own:
            c.close()


def cost_q24(freq, total) -> int:
    """The cost of one range-coder step with probability freq / total: log2(total) - log2(freq) in unsigned Q24 fixed
    point, the integer function the cost kernel runs (bce_hip_cost_q24; no GPU).  1 <= freq <= total < 2**32."""
    return load_library().bce_hip_cost_q24(int(freq), int(total))


def set_plane_mask(ctx, mask):
    """The planes whose range coders context `ctx` runs from now on (bit p = plane p; 0xFF = all: the default)."""
    ctx.check(ctx.lib.bce_hip_set_plane_mask(ctx.h, int(mask) & 0xFF), "bce_hip_set_plane_mask")


def plane_stream(ctx, plane) -> np.ndarray:
    """The finished coded stream of one plane of the context's last encode (u16 words)."""
    n = C.c_size_t()
    ctx.check(ctx.lib.bce_hip_plane_stream_size(ctx.h, plane, C.byref(n)), "bce_hip_plane_stream_size")
    out = np.empty(n.value, dtype=np.uint16)
    ctx.check(ctx.lib.bce_hip_plane_stream_copy(ctx.h, plane, out.ctypes.data, n.value), "bce_hip_plane_stream_copy")
    return out


def set_plane_stream(ctx, plane, words):
    """Put another context's finished stream of `plane` (same input, same config) in the place of this context's own."""
    w = np.ascontiguousarray(words, dtype=np.uint16)
    ctx.check(ctx.lib.bce_hip_plane_stream_set(ctx.h, plane, w.ctypes.data, w.size), "bce_hip_plane_stream_set")


def archive_of(ctx) -> bytearray:
    """The archive of the context's last encode as it stands (after set_plane_stream: with the streams put in)."""
    n = C.c_size_t()
    ctx.check(ctx.lib.bce_hip_archive_size(ctx.h, C.byref(n)), "bce_hip_archive_size")
    out = bytearray(n.value)
    view = (C.c_uint8 * n.value).from_buffer(out)
    ctx.check(ctx.lib.bce_hip_archive_copy(ctx.h, C.addressof(view), n.value), "bce_hip_archive_copy")
    del view
    return out


class ContextPool:
    """`contexts` gated contexts on one device (bce_hip_set_gated), driven by one host thread each: their GPU phases take
    turns while the eight coder threads of the context that has just left the GPU finish its last batches, so the step
    time of a stream of inputs is the GPU phase instead of GPU phase + coding tail.  Buffers are kept between calls."""

    def __init__(self, contexts=2, device=0):
        self.ctxs = [_Ctx(device) for _ in range(max(1, int(contexts)))]

    def close(self):
        for c in self.ctxs:
            c.close()
        self.ctxs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def compress_many(self, inputs, config=None, on_device=False, with_stats=False, symbol_capacity=0, with_crc=False):
        """Independent inputs (files, or the blocks of `bce -cN`) -> their archives, in order; each is the archive
        `compress` gives for the same input.  `inputs`: buffers, or (device_ptr, n) pairs with on_device=True.
        with_crc: every result is a tuple that ends with the CRC-32 of the input, taken on the device between the load and
        the encoding (bce_hip_input_crc32): (archive, crc) or (archive, stats, crc)."""
        import threading
        inputs = list(inputs)
        results = [None] * len(inputs)
        errors = []
        ctxs = self.ctxs[:max(1, min(len(self.ctxs), len(inputs)))]
        lock = threading.Lock()
        nxt = [0]

        def worker(c):
            try:
                c.check(c.lib.bce_hip_set_gated(c.h, 1), "bce_hip_set_gated")
                while True:
                    with lock:
                        if errors or nxt[0] >= len(inputs):
                            return
                        i = nxt[0]
                        nxt[0] += 1
                    if on_device:
                        ptr, n = inputs[i]
                        rf = RankFile(n=n, device_ptr=ptr, ctx=c)
                    else:
                        rf = RankFile(inputs[i], ctx=c)
                    crc = input_crc32(c) if with_crc else None
                    arch = BCE(config, symbol_capacity).encode(rf)
                    res = (arch, stats(rf)) if with_stats else (arch,)
                    if with_crc:
                        res += (crc,)
                    results[i] = res if len(res) > 1 else arch
            except Exception as e:  # the other workers stop at their next input
                with lock:
                    errors.append(e)
            finally:
                c.lib.bce_hip_set_gated(c.h, 1)      # (gives the gate back if this context still holds it)

        threads = [threading.Thread(target=worker, args=(c,)) for c in ctxs]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        return results


def compress_many(inputs, config=None, device=0, contexts=2, on_device=False, with_stats=False, symbol_capacity=0, with_crc=False):
    """ContextPool.compress_many with a pool of its own."""
    with ContextPool(contexts, device) as pool:
        return pool.compress_many(inputs, config=config, on_device=on_device, with_stats=with_stats, symbol_capacity=symbol_capacity,
                                  with_crc=with_crc)


def scan(data, device=0):
    """`bce -s` on an in-memory buffer (bce.cpp:1384-1402 minus file I/O) -> (288-byte config, nine result sizes)."""
    rf = RankFile(data, device=device)
    try:
        cfg = np.zeros(CONFIG_BYTES, dtype=np.uint8)
        res = (C.c_double * 9)()
        rf._c.check(rf._c.lib.bce_hip_scan(rf._c.h, cfg.ctypes.data, res), "bce_hip_scan")
        return cfg.tobytes(), list(res)
    finally:
        rf.close()


def decompress(archive) -> bytes:
    """`bce -d` on an in-memory archive (bce.cpp:1428-1472 minus file I/O).  Host C++ decoder; needs no GPU."""
    lib = load_library()
    a = _as_u8(archive)
    n = C.c_size_t()
    rc = lib.bce_hip_decompress(a.ctypes.data, len(a), None, 0, C.byref(n))
    if rc != 0:
        raise BceError(rc, "bce_hip_decompress")
    out = np.empty(n.value, dtype=np.uint8)
    rc = lib.bce_hip_decompress(a.ctypes.data, len(a), out.ctypes.data, n.value, C.byref(n))
    if rc != 0:
        raise BceError(rc, "bce_hip_decompress")
    return out.tobytes()


def decoded_size(archive) -> int:
    """The number of bytes `archive` decodes to, from its header alone (no GPU, nothing decoded)."""
    a = _as_u8(archive)
    n = C.c_size_t()
    rc = load_library().bce_hip_decompress(a.ctypes.data if len(a) else None, len(a), None, 0, C.byref(n))
    if rc != 0:
        raise BceError(rc, "bce_hip_decompress")
    return n.value


def decompress_device(archive, device=0, ctx=None, out=None):
    """`bce -d` with the GPU doing everything but the eight sequential range decoders (kd_decode.hip) -> bytes.

    With `out` (a writable C-contiguous uint8 array at least as large as the original) the bytes are written there, as a
    caller of the C ABI would have them, and the number of bytes is returned: no allocation and no copy on this side."""
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        a = _as_u8(archive)
        n = C.c_size_t()
        if out is not None:
            if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("out must be a writable C-contiguous uint8 array")
            c.check(c.lib.bce_hip_decompress_device(c.h, a.ctypes.data, len(a), out.ctypes.data, out.size, C.byref(n)),
                    "bce_hip_decompress_device")
            return n.value
        c.check(c.lib.bce_hip_decompress_device(c.h, a.ctypes.data, len(a), None, 0, C.byref(n)), "bce_hip_decompress_device")
        buf = np.empty(n.value, dtype=np.uint8)
        c.check(c.lib.bce_hip_decompress_device(c.h, a.ctypes.data, len(a), buf.ctypes.data, n.value, C.byref(n)),
                "bce_hip_decompress_device")
        return buf.tobytes()
    finally:
        if own:
            c.close()


def decompress_to_device(archive, device_ptr, cap, device=0, ctx=None) -> int:
    """The GPU-assisted decoder with the text left in device memory: archive (host bytes) -> the decoded bytes at
    `device_ptr` (an int: `cap` bytes of the caller's memory on `device`, any alignment), the number of bytes returned.
    Nothing of the text crosses to the host.  device_ptr=None only reports the size; cap too small raises (status -5)
    with nothing written.  The library runs on a stream of its own: the memory must be ready when this is called
    (synchronise the stream that produced it), and it is complete when the call returns."""
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        a = _as_u8(archive)
        n = C.c_size_t()
        ptr = None if device_ptr is None else int(device_ptr)
        c.check(c.lib.bce_hip_decompress_to_device(c.h, a.ctypes.data, len(a), ptr, int(cap), C.byref(n)), "bce_hip_decompress_to_device")
        return n.value
    finally:
        if own:
            c.close()


_NO_DIFF = (1 << 64) - 1


def verify_device(archive, device_ptr, n, device=0, ctx=None):
    """Does `archive` decode to the `n` bytes at `device_ptr` (device memory of `device`, any alignment)?  Decoded and
    compared on the GPU; nothing of the text crosses to the host.  -> None when it does, else the first index at which
    they differ (min(n, decoded size) when only the sizes differ).  Stream rule: as decompress_to_device."""
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        a = _as_u8(archive)
        fd = C.c_uint64(_NO_DIFF)
        ptr = None if device_ptr is None else int(device_ptr)
        c.check(c.lib.bce_hip_verify_device(c.h, a.ctypes.data, len(a), ptr, int(n), C.byref(fd)), "bce_hip_verify_device")
        return None if fd.value == _NO_DIFF else fd.value
    finally:
        if own:
            c.close()


def verify(archive, data, device=0, ctx=None):
    """verify_device for host bytes: `data` is uploaded once and compared on the GPU with what `archive` decodes to.
    -> None when equal, else the first differing index."""
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        a, d = _as_u8(archive), _as_u8(data)
        fd = C.c_uint64(_NO_DIFF)
        c.check(c.lib.bce_hip_verify_host(c.h, a.ctypes.data, len(a), d.ctypes.data if len(d) else None, len(d), C.byref(fd)),
                "bce_hip_verify_host")
        return None if fd.value == _NO_DIFF else fd.value
    finally:
        if own:
            c.close()


def compare_device(ptr_a, ptr_b, n, ctx):
    """Test hook (bce_hip_compare_device): the first index at which the `n` bytes at device pointers `ptr_a` and `ptr_b`
    differ, None when they are equal.  Stream rule: as decompress_to_device."""
    fd = C.c_uint64(0)
    ctx.check(ctx.lib.bce_hip_compare_device(ctx.h, None if ptr_a is None else int(ptr_a), None if ptr_b is None else int(ptr_b),
                                             int(n), C.byref(fd)), "bce_hip_compare_device")
    return None if fd.value == _NO_DIFF else fd.value


def _ptr(p):
    return None if p is None else int(p)


def planes_from_ranks_device(ptr_R, n, ptr_bwt, ctx, ptr_words=None, ptr_rankw=None):
    """Test hook (bce_hip_planes_from_ranks_device): the decoder's planes stage -- boundary ranks u32 [8][n + 1] at device pointer
    `ptr_R` (0xFFFFFFFF = unknown) -> the n BWT bytes at `ptr_bwt`, and the plane words / word ranks (u32 [8][(n + 31) // 32 + 3]
    each) where asked for.  -> the status (0, or a negative BCE_HIP_E_* that the caller asserts); ctx.error() has the message."""
    return ctx.lib.bce_hip_planes_from_ranks_device(ctx.h, _ptr(ptr_R), int(n), _ptr(ptr_bwt), _ptr(ptr_words), _ptr(ptr_rankw))


def unbwt_device(ptr_bwt, n, offset, ptr_out, ctx):
    """Test hook (bce_hip_unbwt_device): the decoder's inverse BWT of the n bytes at device pointer `ptr_bwt` into `ptr_out`, text
    position i at (i + offset) % n.  -> (status, LF cycle length, walkers)."""
    lc, m = C.c_uint64(0), C.c_uint32(0)
    rc = ctx.lib.bce_hip_unbwt_device(ctx.h, _ptr(ptr_bwt), int(n), int(offset), _ptr(ptr_out), C.byref(lc), C.byref(m))
    return rc, lc.value, m.value


def lcp_reduce_device(ptr_lcp, n, ptr_sa, ks, ctx, repeat=True):
    """Test hook (bce_hip_lcp_reduce_device): the reductions of kgrams() and longest_repeat() on `n` uint32 words at device pointer
    `ptr_lcp` read as an LCP array, with the `n` words at `ptr_sa` as the suffix array -> (a list of KGram records, one per k of
    `ks`, and (len, pos_a, pos_b), or None with repeat=False)."""
    karr = np.array(list(ks), dtype=np.uint32)
    out = (KGram * max(len(karr), 1))()
    rep = (C.c_uint32 * 3)()
    ctx.check(ctx.lib.bce_hip_lcp_reduce_device(ctx.h, _ptr(ptr_lcp), int(n), _ptr(ptr_sa), karr.ctypes.data if len(karr) else None, len(karr),
                                                C.addressof(out), C.addressof(rep) if repeat else None), "bce_hip_lcp_reduce_device")
    return [out[i] for i in range(len(karr))], (tuple(rep) if repeat else None)


def top_classes_of_lcp_device(ptr_lcp, n, ptr_sa, k, limit, ctx):
    """Test hook (bce_hip_top_classes_of_lcp_device): the selection of top_kgrams() on `n` uint32 words at device pointer `ptr_lcp`
    read as an LCP array, with the `n` words at `ptr_sa` as the suffix array -> (a numpy record array (count, row, pos) of the
    entries found, distinct, size_hist)."""
    out = np.zeros(max(1, int(limit)), dtype=TOP_DTYPE)
    found, distinct, hist = C.c_uint32(0), C.c_uint64(0), (C.c_uint64 * 32)()
    ctx.check(ctx.lib.bce_hip_top_classes_of_lcp_device(ctx.h, _ptr(ptr_lcp), int(n), _ptr(ptr_sa), int(k), int(limit), out.ctypes.data, C.byref(found),
                                                        C.byref(distinct), C.addressof(hist)), "bce_hip_top_classes_of_lcp_device")
    return out[:found.value], distinct.value, [int(v) for v in hist]


def maxrep_of_arrays_device(ptr_lcp, n, ptr_sa, ptr_bw, min_len, max_len, order, limit, ctx):
    """Test hook (bce_hip_maxrep_of_arrays_device): the launches of maximal_repeats() behind the LCP pass on `n` uint32 words at device
    pointer `ptr_lcp` read as the LCP array, the `n` words at `ptr_sa` as the suffix array and the `n` bytes at `ptr_bw` as the
    preceding bytes -> (a numpy record array (len, count, row, pos) of the entries found, the info dict)."""
    min_len, max_len, order, limit, _ = _maxrep_args(min_len, max_len, order, limit, 0)
    out = np.zeros(max(1, min(limit, TOP_MAX)), dtype=MAXREP_DTYPE)
    info = MaxRepInfo()
    ctx.check(ctx.lib.bce_hip_maxrep_of_arrays_device(ctx.h, _ptr(ptr_lcp), int(n), _ptr(ptr_sa), _ptr(ptr_bw), min_len, max_len, order, limit, out.ctypes.data,
                                                      C.byref(info)), "bce_hip_maxrep_of_arrays_device")
    return out[:info.found].copy(), info.as_dict()


def coverage_of_lengths_device(ptr_len, q, min_len, ctx) -> int:
    """Test hook (bce_hip_coverage_of_lengths_device): the reduction of coverage() on `q` uint32 match lengths at device pointer
    `ptr_len` (lens[i] <= i + 1) -> the covered positions."""
    out = C.c_uint64(0)
    ctx.check(ctx.lib.bce_hip_coverage_of_lengths_device(ctx.h, _ptr(ptr_len), int(q), int(min_len), C.byref(out)),
              "bce_hip_coverage_of_lengths_device")
    return out.value


def sort_pairs_device(ptr_key, ptr_val, n, first_bit, bits, max_digit_bits, ctx):
    """Test hook (bce_hip_sort_pairs_device): the stable radix sort of `n` (u32 key, u32 value) pairs in device memory, in
    place, on key bits [first_bit, first_bit + bits).  Stream rule: as decompress_to_device."""
    ctx.check(ctx.lib.bce_hip_sort_pairs_device(ctx.h, int(ptr_key), int(ptr_val), int(n), int(first_bit), int(bits), int(max_digit_bits)),
              "bce_hip_sort_pairs_device")


def sort_wide_device(ptr_lo, ptr_hi, ptr_val, n, bits, max_digit_bits, ctx):
    """Test hook (bce_hip_sort_wide_device): the same with 64-bit keys in two u32 arrays (hi:lo), on key bits [0, bits)."""
    ctx.check(ctx.lib.bce_hip_sort_wide_device(ctx.h, int(ptr_lo), int(ptr_hi), int(ptr_val), int(n), int(bits), int(max_digit_bits)),
              "bce_hip_sort_wide_device")


def crc32(data, crc=0) -> int:
    """CRC-32 of host bytes as zlib.crc32 computes it (bce_hip_crc32: the library's own routine, no GPU)."""
    a = _as_u8(data)
    return load_library().bce_hip_crc32(int(crc) & 0xFFFFFFFF, a.ctypes.data if len(a) else None, len(a))


def crc32_combine(crc_a, crc_b, len_b) -> int:
    """CRC-32 of A || B from the CRC-32s of A and B and the length of B (bce_hip_crc32_combine; no GPU)."""
    return load_library().bce_hip_crc32_combine(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b))


def crc32_device(ptr, n, device=0, ctx=None) -> int:
    """CRC-32 of the `n` bytes at device pointer `ptr` (memory of `device`, any alignment, any n), computed on the GPU
    (kd_crc32.hip).  Stream rule: as decompress_to_device."""
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        v = C.c_uint32()
        c.check(c.lib.bce_hip_crc32_device(c.h, None if ptr is None else int(ptr), int(n), C.byref(v)), "bce_hip_crc32_device")
        return v.value
    finally:
        if own:
            c.close()


def input_crc32(ctx) -> int:
    """CRC-32 of the input context `ctx` holds (after a load, for as long as it keeps the bytes: bce_hip_input_crc32)."""
    v = C.c_uint32()
    ctx.check(ctx.lib.bce_hip_input_crc32(ctx.h, C.byref(v)), "bce_hip_input_crc32")
    return v.value


def decode_crc32(archive, device=0, ctx=None):
    """Decode `archive` on the GPU into the context's own buffer and checksum it there -> (decoded bytes, CRC-32 of the
    text).  Nothing of the text crosses to the host."""
    own = ctx is None
    c = ctx or _Ctx(device)
    try:
        a = _as_u8(archive)
        n, v = C.c_size_t(), C.c_uint32()
        c.check(c.lib.bce_hip_decode_crc32(c.h, a.ctypes.data, len(a), C.byref(n), C.byref(v)), "bce_hip_decode_crc32")
        return n.value, v.value
    finally:
        if own:
            c.close()


def synth_text(seed, n) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    load_library().bce_hip_synth_text(seed, out.ctypes.data, n)
    return out


def synth_rand(seed, n) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    load_library().bce_hip_synth_rand(seed, out.ctypes.data, n)
    return out
