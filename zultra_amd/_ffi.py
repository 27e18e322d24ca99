"""ctypes bindings for the C ABI of libzultra_amd.so (include/libzultra.h + include/zultra_hip.h).

Python here is plumbing for tests and benchmarks; the product is the shared library. The names mirror the
reference's API (src/libzultra.h:104-157): ``memory_bound``, ``memory_compress``, a ``Stream`` object for
``zultra_stream_init / set_dictionary / compress / end``, plus ``HipContext`` for the batched device layer.
"""
import ctypes as C

import numpy as np

ZULTRA_OK = 0
ZULTRA_STREAM_END = 1
ZULTRA_ERROR_SRC = -1
ZULTRA_ERROR_DST = -2
ZULTRA_ERROR_DICTIONARY = -3
ZULTRA_ERROR_MEMORY = -4
ZULTRA_ERROR_COMPRESSION = -5

FLAG_DEFLATE = 0
FLAG_ZLIB = 1
FLAG_GZIP = 2

CONTINUE = 0
FINALIZE = 1

_u8p = C.POINTER(C.c_uint8)
_SIZE_MAX = C.c_size_t(-1).value


class ZultraError(RuntimeError):
    pass


class _Stream(C.Structure):
    # layout of zultra_stream_t, reference src/libzultra.h:78-93
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_size_t), ("total_in", C.c_ulonglong),
                ("next_out", C.c_void_p), ("avail_out", C.c_size_t), ("total_out", C.c_ulonglong),
                ("zalloc", C.c_void_p), ("zfree", C.c_void_p), ("opaque", C.c_void_p),
                ("state", C.c_void_p), ("adler", C.c_uint)]


class Block(C.Structure):
    _fields_ = [("win_off", C.c_uint64), ("prev", C.c_uint32), ("n", C.c_uint32)]


class SubBlock(C.Structure):
    _fields_ = [("block", C.c_uint32), ("start", C.c_uint32), ("size", C.c_uint32), ("is_dynamic", C.c_uint32),
                ("static_cost", C.c_int32), ("dynamic_cost", C.c_int32), ("failed", C.c_uint32), ("reserved", C.c_uint32),
                ("nbits", C.c_uint64), ("bits_off", C.c_uint64)]


class Timing(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("h2d_ms", "matchfinder_ms", "tokenize_split_ms", "encode_ms", "d2h_ms", "total_ms",
                                         "group_ms", "frontier_ms", "stitch_ms", "init_ms", "parse_ms", "build_ms", "post_ms", "emit_ms", "head_ms", "tail_ms")]


class Stats(C.Structure):
    _fields_ = [("positions", C.c_uint64), ("huge_positions", C.c_uint64), ("blocks", C.c_uint32), ("subblocks", C.c_uint32),
                ("tasks", C.c_uint32), ("huge_tasks", C.c_uint32), ("cut_tasks", C.c_uint32), ("cut_segments", C.c_uint32),
                ("cut_redone", C.c_uint32), ("runs", C.c_uint32), ("settled_passes", C.c_uint32), ("settled_kib", C.c_uint32), ("cut_demoted", C.c_uint32),
                ("runs_without_chain_kernels", C.c_uint32), ("batches_rerun", C.c_uint32), ("runs_fitted", C.c_uint32), ("stream_collisions", C.c_uint32)]


class BitState(C.Structure):
    _fields_ = [("acc", C.c_uint32), ("nacc", C.c_uint32)]


class Verify(C.Structure):
    # zultra_hip_verify_t
    _fields_ = [("bad_subblocks", C.c_uint32), ("first_bad", C.c_uint32), ("reason", C.c_uint32), ("block", C.c_uint32),
                ("input_off", C.c_uint64), ("stream_bit", C.c_uint64), ("verified_bytes", C.c_uint64)]


class InflateItem(C.Structure):
    # zultra_hip_inflate_item_t
    _fields_ = [("src_off", C.c_uint64), ("src_size", C.c_uint64), ("dst_off", C.c_uint64), ("dst_cap", C.c_uint64)]


class InflateResult(C.Structure):
    # zultra_hip_inflate_result_t
    _fields_ = [("reason", C.c_uint32), ("blocks", C.c_uint32), ("out_size", C.c_uint64), ("src_used", C.c_uint64)]


class MemberResult(C.Structure):
    # zultra_hip_member_result_t
    _fields_ = [("reason", C.c_uint32), ("blocks", C.c_uint32), ("out_size", C.c_uint64), ("src_used", C.c_uint64), ("head_size", C.c_uint32), ("check", C.c_uint32)]


class IndexResult(C.Structure):
    # zultra_hip_index_result_t
    _fields_ = [("members", C.c_uint32), ("stop", C.c_uint32), ("out_size", C.c_uint64), ("src_used", C.c_uint64), ("tiles", C.c_uint32), ("tiles_rewalked", C.c_uint32)]


class RangeResult(C.Structure):
    # zultra_hip_range_result_t
    _fields_ = [("members", C.c_uint32), ("stop", C.c_uint32), ("file_size", C.c_uint64), ("src_used", C.c_uint64), ("first_member", C.c_uint32), ("range_members", C.c_uint32),
                ("out_size", C.c_uint64), ("tiles", C.c_uint32), ("tiles_rewalked", C.c_uint32)]


class ZipIndexResult(C.Structure):
    # zultra_hip_zip_index_result_t
    _fields_ = [("entries", C.c_uint32), ("stop", C.c_uint32), ("out_size", C.c_uint64), ("dir_used", C.c_uint64), ("tiles", C.c_uint32), ("tiles_rewalked", C.c_uint32)]


class ZipEnd(C.Structure):
    # zultra_zip_end_t
    _fields_ = [("nEntries", C.c_ulonglong), ("nCentralOff", C.c_ulonglong), ("nCentralSize", C.c_ulonglong), ("nPrefix", C.c_ulonglong), ("nZip64", C.c_int)]


MEMBER_DTYPE = [("off", "<u8"), ("size", "<u8"), ("check", "<u4"), ("flags", "<u4")]   # zultra_hip_member_t
FRAME_BGZF = 4   # ZULTRA_HIP_FRAME_BGZF
ZIP_ENTRY_DTYPE = [("local_off", "<u8"), ("comp_size", "<u4"), ("size", "<u4"), ("crc32", "<u4"), ("name_len", "<u4")]   # zultra_hip_zip_entry_t
ZIP_EMPTY = 0xFFFFFFFF   # entry_block: an empty entry (a zero-length file or a directory)
ZIP_DIRENT_DTYPE = [("central_at", "<u8"), ("local_off", "<u8"), ("dst_off", "<u8"), ("comp_size", "<u4"), ("size", "<u4"), ("crc32", "<u4"), ("name_len", "<u4"),
                    ("method", "<u2"), ("flags", "<u2"), ("extra_len", "<u2"), ("comment_len", "<u2")]   # zultra_hip_zip_dirent_t
ZIP_INFO_DTYPE = np.dtype([("nNameAt", "<u8"), ("nNameLen", "<u4"), ("nMethod", "<u4"), ("nFlags", "<u4"), ("nCrc32", "<u4"), ("nCompSize", "<u4"), ("nSize", "<u4"),
                           ("nOutOff", "<u8"), ("nStatus", "<u4")], align=True)   # zultra_zip_info_t
STITCH_ITEM_DTYPE = [("dst_bit", "<u8"), ("stored", "<u4"), ("is_final", "<u4")]   # zh_stitch_item_t (zultra_hip_stitch_items)
# zultra_hip_entropy_rec_t (zultra_hip_entropy_probe)
ENTROPY_REC_DTYPE = np.dtype([("lit_len", "u1", 288), ("dist_len", "u1", 32), ("lit_code", "<u2", 288), ("dist_code", "<u2", 32), ("pre_lit_len", "u1", 288), ("pre_dist_len", "u1", 32),
                              ("is_dynamic", "<u4"), ("failed", "<u4"), ("hdr_bits", "<u4"), ("static_cost", "<i4"), ("dynamic_cost", "<i4"), ("settled", "<u4"), ("reserved", "<u4", 2)])
ENTROPY_NSYM = 320    # ZULTRA_HIP_ENTROPY_NSYM
ENTROPY_SLOT = 1024   # ZULTRA_HIP_ENTROPY_SLOT
MEMBER_RESULT_DTYPE = [("reason", "<u4"), ("blocks", "<u4"), ("out_size", "<u8"), ("src_used", "<u8"), ("head_size", "<u4"), ("check", "<u4")]


EXPORTS = [
    # include/libzultra.h
    "zultra_stream_init", "zultra_stream_set_dictionary", "zultra_stream_compress", "zultra_stream_end",
    "zultra_memory_bound", "zultra_memory_compress", "zultra_memory_compress_dict", "zultra_set_device", "zultra_set_devices",
    "zultra_frame_get_header_size", "zultra_frame_encode_header", "zultra_frame_init_checksum",
    "zultra_frame_update_checksum", "zultra_frame_get_footer_size", "zultra_frame_encode_footer",
    "zultra_dictionary_load", "zultra_dictionary_free",
    # include/zultra_hip.h
    "zultra_hip_device_count", "zultra_hip_selftest", "zultra_hip_entropy_probe", "zultra_hip_traffic_probe", "zultra_hip_create", "zultra_hip_destroy", "zultra_hip_last_error",
    "zultra_hip_data_capacity", "zultra_hip_compress_blocks", "zultra_hip_subblocks", "zultra_hip_payload",
    "zultra_hip_last_timing", "zultra_hip_get_matches", "zultra_hip_get_splits", "zultra_hip_get_parse",
    "zultra_hip_stitch", "zultra_hip_stitch_finish",
    "zultra_hip_stitch_device", "zultra_hip_stitch_phase_table", "zultra_hip_stream_device", "zultra_hip_stream_read", "zultra_hip_block_crc32", "zultra_crc32_append", "zultra_crc32_append_many",
    "zultra_hip_create_files", "zultra_hip_compress_files", "zultra_hip_stitch_files", "zultra_hip_staging",
    "zultra_hip_block_adler32", "zultra_adler32_append", "zultra_hip_copy_bandwidth", "zultra_hip_last_stats", "zultra_hip_runs_for", "zultra_hip_mf_chunk",
    "zultra_hip_ctx_info", "zultra_hip_context_bytes", "zultra_hip_context_bytes_on", "zultra_release_cached_contexts", "zultra_hip_chain_trace", "zultra_hip_cut_tasks", "zultra_hip_stitch_with_batch",
    # verification
    "zultra_set_verify", "zultra_verified_bytes", "zultra_hip_verify_device", "zultra_hip_last_verify_ms", "zultra_hip_stream_write",
    # decompression
    "zultra_memory_decompress", "zultra_hip_inflate_streams", "zultra_memory_decompress_dict", "zultra_hip_inflate_streams_dict",
    "zultra_memory_decompress_batch", "zultra_hip_inflate_members",
    "zultra_hip_index_members", "zultra_hip_inflate_file", "zultra_memory_decompress_members",
    "zultra_hip_inflate_range", "zultra_memory_index_gzi", "zultra_memory_decompress_range",
    # framed members
    "zultra_hip_frame_members", "zultra_hip_last_frame_ms", "zultra_memory_bound_bgzf", "zultra_memory_compress_bgzf", "zultra_memory_compress_batch",
    # ZIP archives
    "zultra_hip_zip_members", "zultra_hip_zip_device", "zultra_hip_zip_read", "zultra_hip_last_zip_ms",
    "zultra_zip_end_records", "zultra_memory_bound_zip", "zultra_memory_compress_zip",
    "zultra_hip_zip_index", "zultra_hip_unzip", "zultra_zip_find_end", "zultra_memory_decompress_zip",
    # streams of several max-blocks in one batch
    "zultra_hip_frame_streams", "zultra_hip_zip_streams", "zultra_hip_last_streams_ms", "zultra_hip_stitch_items", "zultra_hip_plan_streams",
    "zultra_memory_compress_streams", "zultra_memory_compress_zip_streams",
]


def _as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


class Lib:
    def __init__(self, path, allow_missing=()):
        """allow_missing: exports an OLDER build of the library may lack (A/B tools under tools/ that load a previous round's build; the product loader passes none)."""
        self.path = path
        L = self.L = C.CDLL(path)
        missing = [n for n in EXPORTS if not hasattr(L, n) and n not in allow_missing]
        if missing:
            raise ZultraError("%s does not export %s" % (path, missing))
        L.zultra_stream_init.argtypes = [C.POINTER(_Stream), C.c_uint, C.c_uint]
        L.zultra_stream_init.restype = C.c_int
        L.zultra_stream_set_dictionary.argtypes = [C.POINTER(_Stream), C.c_void_p, C.c_int]
        L.zultra_stream_set_dictionary.restype = C.c_int
        L.zultra_stream_compress.argtypes = [C.POINTER(_Stream), C.c_int]
        L.zultra_stream_compress.restype = C.c_int
        L.zultra_stream_end.argtypes = [C.POINTER(_Stream)]
        L.zultra_stream_end.restype = None
        L.zultra_memory_bound.argtypes = [C.c_size_t, C.c_uint, C.c_uint]
        L.zultra_memory_bound.restype = C.c_size_t
        L.zultra_memory_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint]
        L.zultra_memory_compress.restype = C.c_size_t
        L.zultra_memory_compress_dict.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_void_p, C.c_int]
        L.zultra_memory_compress_dict.restype = C.c_size_t
        L.zultra_set_device.argtypes = [C.c_int]
        L.zultra_frame_update_checksum.argtypes = [C.c_uint, C.c_void_p, C.c_size_t, C.c_uint]
        L.zultra_frame_update_checksum.restype = C.c_uint
        L.zultra_frame_init_checksum.argtypes = [C.c_uint]
        L.zultra_frame_init_checksum.restype = C.c_uint
        L.zultra_frame_encode_header.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_void_p, C.c_int]
        L.zultra_frame_encode_footer.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_longlong, C.c_uint]
        L.zultra_frame_get_header_size.argtypes = [C.c_uint, C.c_void_p, C.c_int]
        L.zultra_frame_get_footer_size.argtypes = [C.c_uint]
        L.zultra_hip_device_count.restype = C.c_int
        L.zultra_hip_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
        L.zultra_hip_create.restype = C.c_void_p
        L.zultra_hip_destroy.argtypes = [C.c_void_p]
        L.zultra_hip_last_error.argtypes = [C.c_void_p]
        L.zultra_hip_last_error.restype = C.c_char_p
        L.zultra_hip_data_capacity.argtypes = [C.c_void_p]
        L.zultra_hip_data_capacity.restype = C.c_size_t
        L.zultra_hip_compress_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Block), C.c_uint32]
        L.zultra_hip_compress_blocks.restype = C.c_int
        L.zultra_hip_subblocks.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.zultra_hip_subblocks.restype = C.POINTER(SubBlock)
        L.zultra_hip_payload.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        L.zultra_hip_payload.restype = _u8p
        L.zultra_hip_last_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
        L.zultra_hip_get_matches.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.zultra_hip_get_splits.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]
        L.zultra_hip_get_parse.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.zultra_hip_stitch.argtypes = [C.POINTER(BitState), C.POINTER(SubBlock), C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]
        L.zultra_hip_stitch.restype = C.c_size_t
        L.zultra_hip_stitch_finish.argtypes = [C.POINTER(BitState), C.c_void_p, C.c_size_t]
        L.zultra_hip_stitch_finish.restype = C.c_size_t

    # ---- libzultra.h -------------------------------------------------------------------------------------
    def device_count(self):
        return self.L.zultra_hip_device_count()

    def traffic_probe(self, nbytes):
        self.L.zultra_hip_traffic_probe.argtypes = [C.c_size_t]
        return self.L.zultra_hip_traffic_probe(nbytes)

    def entropy_probe(self, grid=None, hist_part=None, in_force=None, pass_=0, tok_info=None, tok_off=None):
        """zh_sb_build on hist_part[n, ntasks, 320] with the lengths in_force[n, 320] (pass_ 0..3), or zh_sb_init on the tokens tok_info[tok_off[i]:tok_off[i + 1]]
        of sub-block i; sub-blocks [0, grid) in the one-per-workgroup form, the rest in the striding form (grid None: all in the first).
        -> (records [n] of ENTROPY_REC_DTYPE, slots uint8 [n, ENTROPY_SLOT], (settled, settled_kib))"""
        f = self.L.zultra_hip_entropy_probe
        f.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32] + [C.c_void_p] * 7
        f.restype = C.c_int
        if hist_part is not None:
            hist_part = np.ascontiguousarray(hist_part, dtype=np.uint32)
            n, ntasks, nsym = hist_part.shape
            in_force = np.ascontiguousarray(in_force, dtype=np.uint8)
            assert nsym == ENTROPY_NSYM and in_force.shape == (n, ENTROPY_NSYM)
            args = (1, n, n if grid is None else grid, pass_, ntasks, hist_part.ctypes.data, in_force.ctypes.data, None, None)
        else:
            tok_info = np.ascontiguousarray(tok_info, dtype=np.uint16)
            tok_off = np.ascontiguousarray(tok_off, dtype=np.uint32)
            n = len(tok_off) - 1
            assert n >= 1 and int(tok_off[-1]) == len(tok_info)
            keep = np.zeros(1, dtype=np.uint16) if len(tok_info) == 0 else tok_info   # (a pointer that is not NULL)
            args = (0, n, n if grid is None else grid, 0, 0, None, None, keep.ctypes.data, tok_off.ctypes.data)
        recs = np.zeros(n, dtype=ENTROPY_REC_DTYPE)
        slots = np.zeros((n, ENTROPY_SLOT), dtype=np.uint8)
        settled = np.zeros(2, dtype=np.uint32)
        rc = f(*args, recs.ctypes.data, slots.ctypes.data, settled.ctypes.data)
        if rc != 0:
            raise ZultraError("zultra_hip_entropy_probe failed: %d" % rc)
        return recs, slots, (int(settled[0]), int(settled[1]))

    def runs_for(self, batch_bytes, nblocks, streams_setting=0):
        """Staggered runs a batch is cut into (zultra_hip_runs_for: pure, no device)."""
        self.L.zultra_hip_runs_for.argtypes = [C.c_uint64, C.c_uint32, C.c_int]
        self.L.zultra_hip_runs_for.restype = C.c_uint32
        return int(self.L.zultra_hip_runs_for(batch_bytes, nblocks, streams_setting))

    def copy_bandwidth(self, nbytes=1 << 30, iters=5):
        """Measured GB/s (read + written) of a 16 B/lane streaming copy: the roofline's second denominator."""
        self.L.zultra_hip_copy_bandwidth.argtypes = [C.c_size_t, C.c_int]
        self.L.zultra_hip_copy_bandwidth.restype = C.c_double
        return self.L.zultra_hip_copy_bandwidth(nbytes, iters)

    def memory_bound(self, n, flags, max_block=0):
        return self.L.zultra_memory_bound(n, flags, max_block)

    def memory_compress(self, data, flags, max_block=0, dictionary=None, cap=None):
        """-> compressed bytes, or None where the reference returns (size_t)-1."""
        data = _as_u8(data)
        if cap is None:
            cap = self.memory_bound(len(data), flags, max_block) + 16
        out = np.empty(max(cap, 1), dtype=np.uint8)
        if dictionary is not None and len(dictionary):
            d = _as_u8(dictionary)
            r = self.L.zultra_memory_compress_dict(data.ctypes.data, len(data), out.ctypes.data, cap, flags, max_block, d.ctypes.data, len(d))
        else:
            r = self.L.zultra_memory_compress(data.ctypes.data, len(data), out.ctypes.data, cap, flags, max_block)
        if r == _SIZE_MAX:
            return None
        return out[:r].tobytes()

    def memory_compress_into(self, data, flags, max_block, out):
        """zultra_memory_compress into a caller-owned uint8 array (no allocation, no copy of the result): the number of bytes, or None."""
        data = _as_u8(data)
        r = self.L.zultra_memory_compress(data.ctypes.data, len(data), out.ctypes.data, len(out), flags, max_block)
        return None if r == _SIZE_MAX else int(r)

    def memory_decompress(self, data, flags, max_out):
        """zultra_memory_decompress -> the decompressed bytes, or None where the call returns (size_t)-1."""
        data = _as_u8(data)
        out = np.empty(max(max_out, 1), dtype=np.uint8)
        f = self.L.zultra_memory_decompress
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint]
        f.restype = C.c_size_t
        r = f(data.ctypes.data, len(data), out.ctypes.data, max_out, flags)
        if r == _SIZE_MAX:
            return None
        return out[:r].tobytes()

    def inflate_streams(self, src, src_size, dst, dst_size, items, device=0):
        """zultra_hip_inflate_streams. src / dst: a uint8 array (host memory, staged by the call) or an integer device pointer (used in place);
        items: (src_off, src_size, dst_off, dst_cap) each. -> (rc, results, kernel_ms): rc = number of items that did not decode, -1 for bad
        arguments and HIP errors; results = (reason, blocks, out_size, src_used) per item."""
        arr = np.ascontiguousarray(items, dtype=np.uint64).reshape(-1, 4)
        res = np.zeros(len(arr), dtype=[("reason", "<u4"), ("blocks", "<u4"), ("out_size", "<u8"), ("src_used", "<u8")])
        src_dev, dst_dev = not isinstance(src, np.ndarray), not isinstance(dst, np.ndarray)
        ms = C.c_float(0)
        f = self.L.zultra_hip_inflate_streams
        f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_float)]
        f.restype = C.c_int
        rc = f(device, int(src) if src_dev else src.ctypes.data, src_size, 1 if src_dev else 0, int(dst) if dst_dev else dst.ctypes.data, dst_size, 1 if dst_dev else 0,
               arr.ctypes.data, len(arr), res.ctypes.data, C.byref(ms))
        return rc, res, float(ms.value)

    def memory_decompress_dict(self, data, flags, max_out, dictionary):
        """zultra_memory_decompress_dict -> the decompressed bytes, or None where the call returns (size_t)-1. dictionary: bytes / uint8 array, or
        None (no dictionary)."""
        data = _as_u8(data)
        out = np.empty(max(max_out, 1), dtype=np.uint8)
        d = None if dictionary is None else _as_u8(dictionary)
        f = self.L.zultra_memory_decompress_dict
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_int]
        f.restype = C.c_size_t
        r = f(data.ctypes.data, len(data), out.ctypes.data, max_out, flags, None if d is None or not len(d) else d.ctypes.data, 0 if d is None else len(d))
        if r == _SIZE_MAX:
            return None
        return out[:r].tobytes()

    def inflate_streams_dict(self, src, src_size, dst, dst_size, dictionary, dict_size, items, device=0):
        """zultra_hip_inflate_streams_dict: inflate_streams with one preset dictionary for all items. dictionary: a uint8 array (host memory, staged
        by the call), an integer device pointer (used in place) or None; dict_size bytes of it."""
        arr = np.ascontiguousarray(items, dtype=np.uint64).reshape(-1, 4)
        res = np.zeros(len(arr), dtype=[("reason", "<u4"), ("blocks", "<u4"), ("out_size", "<u8"), ("src_used", "<u8")])
        src_dev, dst_dev = not isinstance(src, np.ndarray), not isinstance(dst, np.ndarray)
        dict_dev = dictionary is not None and not isinstance(dictionary, np.ndarray)
        ms = C.c_float(0)
        f = self.L.zultra_hip_inflate_streams_dict
        f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_float)]
        f.restype = C.c_int
        rc = f(device, int(src) if src_dev else src.ctypes.data, src_size, 1 if src_dev else 0, int(dst) if dst_dev else dst.ctypes.data, dst_size, 1 if dst_dev else 0,
               None if dictionary is None else int(dictionary) if dict_dev else dictionary.ctypes.data, dict_size, 1 if dict_dev else 0, arr.ctypes.data, len(arr), res.ctypes.data, C.byref(ms))
        return rc, res, float(ms.value)

    def inflate_members(self, src, src_size, dst, dst_size, dictionary, dict_size, framing, items, device=0):
        """zultra_hip_inflate_members: inflate_streams_dict over gzip (framing FLAG_GZIP) or zlib (FLAG_ZLIB) members, or raw streams (0), with the
        headers, checksums and trailers checked on the device. -> (rc, results, kernel_ms): results = (reason, blocks, out_size, src_used,
        head_size, check) per item (MemberResult's layout); kernel_ms = the device time of the three launches (frame, inflate, check)."""
        arr = np.ascontiguousarray(items, dtype=np.uint64).reshape(-1, 4)
        res = np.zeros(len(arr), dtype=MEMBER_RESULT_DTYPE)
        assert res.itemsize == C.sizeof(MemberResult)
        src_dev, dst_dev = not isinstance(src, np.ndarray), not isinstance(dst, np.ndarray)
        dict_dev = dictionary is not None and not isinstance(dictionary, np.ndarray)
        ms = (C.c_float * 3)()
        f = self.L.zultra_hip_inflate_members
        f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_void_p, C.c_uint32, C.c_void_p,
                      C.POINTER(C.c_float)]
        f.restype = C.c_int
        rc = f(device, int(src) if src_dev else src.ctypes.data, src_size, 1 if src_dev else 0, int(dst) if dst_dev else dst.ctypes.data, dst_size, 1 if dst_dev else 0,
               None if dictionary is None else int(dictionary) if dict_dev else dictionary.ctypes.data, dict_size, 1 if dict_dev else 0, framing, arr.ctypes.data, len(arr),
               res.ctypes.data, ms)
        return rc, res, [float(v) for v in ms]

    def index_members(self, src, src_size, cap, device=0):
        """zultra_hip_index_members. src: a uint8 array (host memory, staged by the call) or an integer device pointer; cap: room for that many
        items, 0 to pass items = NULL. -> (rc, IndexResult, items as rows of (src_off, src_size, dst_off, dst_cap), kernel_ms)."""
        items = np.zeros((cap, 4), dtype=np.uint64)
        res = IndexResult()
        src_dev = not isinstance(src, np.ndarray)
        ms = C.c_float(0)
        f = self.L.zultra_hip_index_members
        f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(IndexResult), C.POINTER(C.c_float)]
        f.restype = C.c_int
        rc = f(device, None if src is None else int(src) if src_dev else src.ctypes.data, src_size, 1 if src_dev else 0, items.ctypes.data if cap else None, cap, C.byref(res), C.byref(ms))
        return rc, res, items[:res.members if rc == 0 else 0], float(ms.value)

    def inflate_file(self, src, src_size, dst, dst_size, results_cap=None, device=0):
        """zultra_hip_inflate_file. src / dst: a uint8 array (host memory, staged by the call) or an integer device pointer (used in place);
        results_cap: room for that many per-member results, None to pass results = NULL. -> (rc, IndexResult, results (MemberResult's layout,
        the indexed members'), kernel_ms = [index, frame, inflate, check])."""
        res = IndexResult()
        out = np.zeros(results_cap or 0, dtype=MEMBER_RESULT_DTYPE)
        src_dev, dst_dev = not isinstance(src, np.ndarray), not isinstance(dst, np.ndarray)
        ms = (C.c_float * 4)()
        f = self.L.zultra_hip_inflate_file
        f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(IndexResult), C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
        f.restype = C.c_int
        rc = f(device, None if src is None else int(src) if src_dev else src.ctypes.data, src_size, 1 if src_dev else 0,
               None if dst is None else int(dst) if dst_dev else dst.ctypes.data, dst_size, 1 if dst_dev else 0, C.byref(res),
               out.ctypes.data if results_cap is not None else None, results_cap or 0, ms)
        return rc, res, out[:res.members if rc >= 0 else 0], [float(v) for v in ms]

    def inflate_range(self, src, src_size, first, nbytes, dst, dst_size, results_cap=None, device=0):
        """zultra_hip_inflate_range: bytes [first, first + nbytes) of the file's output. src / dst: a uint8 array (host memory, staged by the call) or an
        integer device pointer (used in place); results_cap: room for that many per-member results, None to pass results = NULL.
        -> (rc, RangeResult, results (MemberResult's layout, the decoded members'), kernel_ms = [index, select + items, frame, inflate, check + edges])."""
        res = RangeResult()
        out = np.zeros(results_cap or 0, dtype=MEMBER_RESULT_DTYPE)
        src_dev, dst_dev = not isinstance(src, np.ndarray), not isinstance(dst, np.ndarray)
        ms = (C.c_float * 5)()
        f = self.L.zultra_hip_inflate_range
        f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(RangeResult), C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
        f.restype = C.c_int
        rc = f(device, None if src is None else int(src) if src_dev else src.ctypes.data, src_size, 1 if src_dev else 0, first, nbytes,
               None if dst is None else int(dst) if dst_dev else dst.ctypes.data, dst_size, 1 if dst_dev else 0, C.byref(res),
               out.ctypes.data if results_cap is not None else None, results_cap or 0, ms)
        return rc, res, out[:min(res.range_members, len(out)) if rc >= 0 else 0], [float(v) for v in ms]

    def memory_index_gzi(self, data, cap=None, query=False):
        """zultra_memory_index_gzi -> the .gzi index of a BGZF file as bytes (query: the size needed, pGzi = NULL), or None where the call returns
        (size_t)-1. cap: bytes of room, default what the query says."""
        data = _as_u8(data)
        f = self.L.zultra_memory_index_gzi
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        f.restype = C.c_size_t
        src = data.ctypes.data if len(data) else None
        if query or cap is None:
            r = f(src, len(data), None, 0)
            if r == _SIZE_MAX:
                return None
            if query:
                return int(r)
            cap = int(r)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        r = f(src, len(data), out.ctypes.data, cap)
        return None if r == _SIZE_MAX else out[:r].tobytes()

    def memory_decompress_range(self, data, first, nbytes, max_out=None, gzi=None):
        """zultra_memory_decompress_range -> bytes [first, first + nbytes) of the output (short at the end of the file), or None where the call returns
        (size_t)-1. data: bytes or a uint8 array (used as it is); gzi: the .gzi index, or None; max_out: bytes of room, default nbytes."""
        data = _as_u8(data)
        if max_out is None:
            max_out = nbytes
        out = np.empty(max(max_out, 1), dtype=np.uint8)
        g = None if gzi is None else _as_u8(gzi)
        f = self.L.zultra_memory_decompress_range
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_ulonglong, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        f.restype = C.c_size_t
        r = f(data.ctypes.data if len(data) else None, len(data), first, nbytes, out.ctypes.data, max_out, None if g is None else g.ctypes.data if len(g) else out.ctypes.data, 0 if g is None else len(g))
        return None if r == _SIZE_MAX else out[:r].tobytes()

    def memory_decompress_members(self, data, max_out):
        """zultra_memory_decompress_members -> (the concatenated output, members), or (None, 0) where the call returns (size_t)-1."""
        data = _as_u8(data)
        out = np.empty(max(max_out, 1), dtype=np.uint8)
        members = C.c_size_t(0)
        f = self.L.zultra_memory_decompress_members
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        f.restype = C.c_size_t
        r = f(data.ctypes.data if len(data) else None, len(data), out.ctypes.data, max_out, C.byref(members))
        if r == _SIZE_MAX:
            return None, 0
        return out[:r].tobytes(), int(members.value)

    def memory_decompress_batch(self, data, members, flags, out_caps, dictionary=None):
        """zultra_memory_decompress_batch over the members [(offset, size)] of `data`, member i with out_caps[i] bytes of room (the outputs lie back
        to back). -> (rc, [bytes, or None for a member that failed]); rc = members that failed, -1 where the call returns (size_t)-1."""
        data = _as_u8(data)
        n = len(members)
        in_off = np.array([m[0] for m in members], dtype=np.uintp)
        in_size = np.array([m[1] for m in members], dtype=np.uintp)
        caps = np.array(out_caps, dtype=np.uintp)
        out_off = (np.cumsum(caps) - caps).astype(np.uintp)
        out_size = np.zeros(max(n, 1), dtype=np.uintp)
        out = np.empty(max(int(caps.sum()), 1), dtype=np.uint8)
        d = None if dictionary is None else _as_u8(dictionary)
        f = self.L.zultra_memory_decompress_batch
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_int]
        f.restype = C.c_size_t
        r = f(data.ctypes.data, len(data), in_off.ctypes.data, in_size.ctypes.data, out.ctypes.data, int(caps.sum()), out_off.ctypes.data, caps.ctypes.data, out_size.ctypes.data, n, flags,
              None if d is None or not len(d) else d.ctypes.data, 0 if d is None else len(d))
        if r == _SIZE_MAX:
            return -1, []
        return int(r), [None if int(out_size[i]) == _SIZE_MAX else out[int(out_off[i]): int(out_off[i]) + int(out_size[i])].tobytes() for i in range(n)]

    def memory_bound_bgzf(self, n, block_size=0):
        f = self.L.zultra_memory_bound_bgzf
        f.argtypes = [C.c_size_t, C.c_uint]
        f.restype = C.c_size_t
        return int(f(n, block_size))

    def memory_compress_bgzf(self, data, block_size=0, cap=None):
        """zultra_memory_compress_bgzf -> the BGZF file (members of block_size input bytes each, 0 = 65280, and the end marker), or None where
        the call returns (size_t)-1. cap: bytes of room, default the bound."""
        data = _as_u8(data)
        if cap is None:
            cap = self.memory_bound_bgzf(len(data), block_size)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        f = self.L.zultra_memory_compress_bgzf
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint]
        f.restype = C.c_size_t
        r = f(data.ctypes.data if len(data) else None, len(data), out.ctypes.data, cap, block_size)
        return None if r == _SIZE_MAX else out[:r].tobytes()

    def memory_compress_batch(self, data, inputs, flags, cap=None):
        """zultra_memory_compress_batch over the inputs [(offset, size)] of `data`: one member of framing `flags` (0, FLAG_ZLIB, FLAG_GZIP) each,
        back to back. -> (the bytes, out_off as n + 1 integers), or (None, None) where the call returns (size_t)-1."""
        data = _as_u8(data)
        n = len(inputs)
        in_off = np.array([m[0] for m in inputs], dtype=np.uintp)
        in_size = np.array([m[1] for m in inputs], dtype=np.uintp)
        if cap is None:
            cap = sum(self.memory_bound(int(m[1]), flags, 0) + 16 for m in inputs)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uintp)
        f = self.L.zultra_memory_compress_batch
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint]
        f.restype = C.c_size_t
        r = f(data.ctypes.data, len(data), in_off.ctypes.data, in_size.ctypes.data, n, out.ctypes.data, cap, out_off.ctypes.data, flags)
        if r == _SIZE_MAX:
            return None, None
        return out[:r].tobytes(), [int(v) for v in out_off]

    def zip_end_records(self, entries, central_off, central_size, cap=98):
        """zultra_zip_end_records -> the end records of a ZIP archive (22 bytes, 98 with more than 65535 entries), or None where the call returns (size_t)-1."""
        out = np.empty(max(cap, 1), dtype=np.uint8)
        f = self.L.zultra_zip_end_records
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong]
        f.restype = C.c_size_t
        r = f(out.ctypes.data, cap, entries, central_off, central_size)
        return None if r == _SIZE_MAX else out[:r].tobytes()

    def memory_bound_zip(self, in_total, names_total, n):
        f = self.L.zultra_memory_bound_zip
        f.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t]
        f.restype = C.c_size_t
        return int(f(in_total, names_total, n))

    def memory_compress_zip(self, data, inputs, names, dos_datetime=0, cap=None):
        """zultra_memory_compress_zip over the inputs [(offset, size)] of `data`, entry i named names[i] (bytes, or str encoded as UTF-8; size 0: an empty
        entry). -> the archive's bytes, or None where the call returns (size_t)-1. cap: bytes of room, default the bound."""
        data = _as_u8(data)
        n = len(inputs)
        names = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in names]
        assert len(names) == n
        blob = _as_u8(b"".join(names) + b"\0")
        name_off = np.concatenate([[0], np.cumsum([len(s) for s in names])]).astype(np.uintp)
        in_off = np.array([m[0] for m in inputs], dtype=np.uintp)
        in_size = np.array([m[1] for m in inputs], dtype=np.uintp)
        if cap is None:
            cap = self.memory_bound_zip(int(in_size.sum()), int(name_off[-1]), n)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        f = self.L.zultra_memory_compress_zip
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint]
        f.restype = C.c_size_t
        r = f(data.ctypes.data if len(data) else None, len(data), in_off.ctypes.data, in_size.ctypes.data, blob.ctypes.data, name_off.ctypes.data, n, out.ctypes.data, cap, dos_datetime)
        return None if r == _SIZE_MAX else out[:r].tobytes()

    def memory_compress_streams(self, data, inputs, flags, max_block=0, cap=None):
        """zultra_memory_compress_streams over the inputs [(offset, size)] of `data`, of any size: one member of framing `flags` each, back to back.
        -> (the bytes, out_off as n + 1 integers), or (None, None) where the call returns (size_t)-1. cap: bytes of room, default the sum of the bounds."""
        data = _as_u8(data)
        n = len(inputs)
        in_off = np.array([m[0] for m in inputs], dtype=np.uintp)
        in_size = np.array([m[1] for m in inputs], dtype=np.uintp)
        if cap is None:
            cap = sum(self.memory_bound(int(m[1]), flags, max_block) for m in inputs)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uintp)
        f = self.L.zultra_memory_compress_streams
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_uint]
        f.restype = C.c_size_t
        r = f(data.ctypes.data, len(data), in_off.ctypes.data, in_size.ctypes.data, n, out.ctypes.data, cap, out_off.ctypes.data, flags, max_block)
        if r == _SIZE_MAX:
            return None, None
        return out[:r].tobytes(), [int(v) for v in out_off]

    def memory_compress_zip_streams(self, data, inputs, names, dos_datetime=0, max_block=0, cap=None):
        """zultra_memory_compress_zip_streams: memory_compress_zip for inputs of any size, as streams of max-blocks of max_block bytes. -> the archive's
        bytes, or None where the call returns (size_t)-1. cap: bytes of room, default the sum of the bounds, both copies of the names, 76 per entry and 98."""
        data = _as_u8(data)
        n = len(inputs)
        names = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in names]
        assert len(names) == n
        blob = _as_u8(b"".join(names) + b"\0")
        name_off = np.concatenate([[0], np.cumsum([len(s) for s in names])]).astype(np.uintp)
        in_off = np.array([m[0] for m in inputs], dtype=np.uintp)
        in_size = np.array([m[1] for m in inputs], dtype=np.uintp)
        if cap is None:
            cap = sum(self.memory_bound(int(m[1]), 0, max_block) for m in inputs) + 2 * int(name_off[-1]) + 76 * n + 98
        out = np.empty(max(cap, 1), dtype=np.uint8)
        f = self.L.zultra_memory_compress_zip_streams
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint]
        f.restype = C.c_size_t
        r = f(data.ctypes.data if len(data) else None, len(data), in_off.ctypes.data, in_size.ctypes.data, blob.ctypes.data, name_off.ctypes.data, n, out.ctypes.data, cap, dos_datetime,
              max_block)
        return None if r == _SIZE_MAX else out[:r].tobytes()

    def zip_index(self, src, src_size, central_at, central_size, cap, device=0):
        """zultra_hip_zip_index. src: a uint8 array (host memory, staged by the call) or an integer device pointer; cap: room for that many dirents, 0 to
        pass dirents = NULL. -> (rc, ZipIndexResult, dirents (ZIP_DIRENT_DTYPE), kernel_ms)."""
        dirents = np.zeros(cap, dtype=ZIP_DIRENT_DTYPE)
        assert dirents.itemsize == 48
        res = ZipIndexResult()
        src_dev = not isinstance(src, np.ndarray)
        ms = C.c_float(0)
        f = self.L.zultra_hip_zip_index
        f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(ZipIndexResult), C.POINTER(C.c_float)]
        f.restype = C.c_int
        rc = f(device, None if src is None else int(src) if src_dev else src.ctypes.data, src_size, 1 if src_dev else 0, central_at, central_size,
               dirents.ctypes.data if cap else None, cap, C.byref(res), C.byref(ms))
        return rc, res, dirents[:res.entries if rc == 0 else 0], float(ms.value)

    def unzip(self, src, src_size, central_at, central_size, local_delta, dst, dst_size, cap=None, device=0):
        """zultra_hip_unzip. src / dst: a uint8 array (host memory, staged by the call) or an integer device pointer (used in place); cap: room for that
        many dirents and results, None to pass both as NULL. -> (rc, ZipIndexResult, dirents, results (MEMBER_RESULT_DTYPE), kernel_ms = [index,
        locals, inflate, copy, check])."""
        res = ZipIndexResult()
        dirents = np.zeros(cap or 0, dtype=ZIP_DIRENT_DTYPE)
        out = np.zeros(cap or 0, dtype=MEMBER_RESULT_DTYPE)
        src_dev, dst_dev = not isinstance(src, np.ndarray), not isinstance(dst, np.ndarray)
        ms = (C.c_float * 5)()
        f = self.L.zultra_hip_unzip
        f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(ZipIndexResult), C.c_void_p, C.c_void_p,
                      C.c_uint32, C.POINTER(C.c_float)]
        f.restype = C.c_int
        rc = f(device, None if src is None else int(src) if src_dev else src.ctypes.data, src_size, 1 if src_dev else 0, central_at, central_size, local_delta,
               None if dst is None else int(dst) if dst_dev else dst.ctypes.data, dst_size, 1 if dst_dev else 0, C.byref(res),
               dirents.ctypes.data if cap else None, out.ctypes.data if cap else None, cap or 0, ms)
        n = res.entries if rc >= 0 else 0
        return rc, res, dirents[:n], out[:n], [float(v) for v in ms]

    def zip_find_end(self, tail, archive_size):
        """zultra_zip_find_end over the last len(tail) bytes of an archive -> ZipEnd, or None where the call returns -1."""
        tail = _as_u8(tail)
        end = ZipEnd()
        f = self.L.zultra_zip_find_end
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_ulonglong, C.POINTER(ZipEnd)]
        f.restype = C.c_int
        return end if f(tail.ctypes.data if len(tail) else None, len(tail), archive_size, C.byref(end)) == 0 else None

    def memory_decompress_zip(self, data, max_out, max_info, list_only=False):
        """zultra_memory_decompress_zip -> (the output's bytes — in list-only mode the size it needs —, or None where the call returns (size_t)-1;
        the infos (ZIP_INFO_DTYPE) as far as they are known; *pnEntries)."""
        data = _as_u8(data)
        out = np.empty(max(max_out, 1), dtype=np.uint8)
        info = np.zeros(max(max_info, 1), dtype=ZIP_INFO_DTYPE)
        assert info.itemsize == 48
        entries = C.c_size_t(0)
        f = self.L.zultra_memory_decompress_zip
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        f.restype = C.c_size_t
        r = f(data.ctypes.data if len(data) else None, len(data), None if list_only else out.ctypes.data, 0 if list_only else max_out, info.ctypes.data if max_info else None, max_info,
              C.byref(entries))
        n = min(int(entries.value), max_info)
        if r == _SIZE_MAX:
            return None, info[:n], int(entries.value)
        return (int(r) if list_only else out[:r].tobytes()), info[:n], int(entries.value)

    def checksum(self, data, flags, start=None):
        data = _as_u8(data)
        if start is None:
            start = self.L.zultra_frame_init_checksum(flags)
        return self.L.zultra_frame_update_checksum(start, data.ctypes.data, len(data), flags)

    def crc32_append(self, crc, block_linear_crc, block_len):
        self.L.zultra_crc32_append.argtypes = [C.c_uint32, C.c_uint32, C.c_size_t]
        self.L.zultra_crc32_append.restype = C.c_uint32
        return self.L.zultra_crc32_append(crc, int(block_linear_crc), block_len)

    def adler32_append(self, adler, a, bw, block_len):
        self.L.zultra_adler32_append.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t]
        self.L.zultra_adler32_append.restype = C.c_uint32
        return self.L.zultra_adler32_append(adler, int(a), int(bw), block_len)

    def crc32_append_many(self, crc, block_linear_crcs, block_lens):
        a = np.ascontiguousarray(block_linear_crcs, dtype=np.uint32)
        n = np.ascontiguousarray(block_lens, dtype=np.uint32)
        f = self.L.zultra_crc32_append_many
        f.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        f.restype = C.c_uint32
        return f(crc, a.ctypes.data, n.ctypes.data, len(a))

    def set_verify(self, enable):
        """zultra_set_verify: every batch the host API stitches is inflated on the device and compared with its input."""
        self.L.zultra_set_verify.argtypes = [C.c_int]
        self.L.zultra_set_verify.restype = None
        self.L.zultra_set_verify(1 if enable else 0)

    def verified_bytes(self):
        self.L.zultra_verified_bytes.restype = C.c_ulonglong
        return int(self.L.zultra_verified_bytes())

    def stream(self, flags, max_block=0, zalloc=None, zfree=None):
        return Stream(self, flags, max_block, zalloc, zfree)

    def _stream_default(self, flags, max_block=0):
        return Stream(self, flags, max_block)

    def context(self, max_block, max_blocks, device=0):
        return HipContext(self, device, max_block, max_blocks)

    def files_context(self, max_file_size, max_files, device=0):
        return HipContext(self, device, max_file_size, max_files, files=True)


ZALLOC_T = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_uint, C.c_uint)
ZFREE_T = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)


class Stream:
    """zultra_stream_t driven the way tool/zultra.c:151-186 drives it."""

    def __init__(self, lib, flags, max_block=0, zalloc=None, zfree=None):
        """zalloc / zfree: ctypes callbacks (ZALLOC_T / ZFREE_T) for the stream's own memory, as libzultra.h:88-90; default malloc / free."""
        self.lib = lib
        self.s = _Stream()
        self._alloc = (zalloc, zfree)
        if zalloc is not None:
            self.s.zalloc = C.cast(zalloc, C.c_void_p)
            self.s.zfree = C.cast(zfree, C.c_void_p)
        rc = lib.L.zultra_stream_init(C.byref(self.s), flags, max_block)
        if rc != ZULTRA_OK:
            raise ZultraError("zultra_stream_init failed: %d (no HIP device? the library has no CPU path)" % rc)
        self._keep = []
        self.ended = False

    def set_dictionary(self, d):
        d = _as_u8(d)
        self._keep.append(d)
        return self.lib.L.zultra_stream_set_dictionary(C.byref(self.s), d.ctypes.data, len(d))

    def compress(self, chunk, finalize, out_chunk=1 << 16):
        """Feed one chunk; returns (status, bytes produced)."""
        chunk = _as_u8(chunk)
        self._keep = self._keep[-2:] + [chunk]
        self.s.next_in = chunk.ctypes.data if len(chunk) else None
        self.s.avail_in = len(chunk)
        out = bytearray()
        buf = np.empty(out_chunk, dtype=np.uint8)
        while True:
            self.s.next_out = buf.ctypes.data
            self.s.avail_out = out_chunk
            st = self.lib.L.zultra_stream_compress(C.byref(self.s), FINALIZE if finalize else CONTINUE)
            out += buf[: out_chunk - self.s.avail_out].tobytes()
            if st != ZULTRA_OK:
                return st, bytes(out)
            if self.s.avail_in == 0 and self.s.avail_out != 0:
                return st, bytes(out)

    @property
    def total_in(self):
        return self.s.total_in

    @property
    def total_out(self):
        return self.s.total_out

    def end(self):
        if not self.ended:
            self.lib.L.zultra_stream_end(C.byref(self.s))
            self.ended = True

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass


class HipContext:
    """zultra_hip_ctx_t: batches of independent max-blocks (include/zultra_hip.h)."""

    def __init__(self, lib, device, max_block, max_blocks, files=False):
        self.lib = lib
        lib.L.zultra_hip_create_files.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
        lib.L.zultra_hip_create_files.restype = C.c_void_p
        self.h = (lib.L.zultra_hip_create_files if files else lib.L.zultra_hip_create)(device, max_block, max_blocks)
        if not self.h:
            raise ZultraError("zultra_hip_create failed: no usable HIP device (there is no CPU fallback)")
        self.max_block = max_block
        self._data = None
        self._block_n = None   # sizes of the last batch's blocks (list or uint32 array)
        self._blocks_src = self._blocks_arr = None

    def close(self):
        if self.h:
            self.lib.L.zultra_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compress_blocks(self, data, blocks, data_on_device=False, data_size=None):
        """data: uint8 array (host) or an integer device pointer; blocks: list of (win_off, prev, n)."""
        if blocks is self._blocks_src:   # same list object as last time: reuse the marshalled descriptors
            arr = self._blocks_arr
        else:
            arr = (Block * len(blocks))(*[Block(int(o), int(p), int(n)) for (o, p, n) in blocks])
            self._blocks_src, self._blocks_arr = blocks, arr
            self._block_n = [int(b[2]) for b in blocks]
        if data_on_device:
            ptr, size = int(data), int(data_size)
        else:
            self._data = _as_u8(data)
            ptr, size = self._data.ctypes.data, len(self._data)
        n = self.lib.L.zultra_hip_compress_blocks(self.h, ptr, size, 1 if data_on_device else 0, arr, len(blocks))
        if n <= 0:
            raise ZultraError("zultra_hip_compress_blocks: " + self.lib.L.zultra_hip_last_error(self.h).decode())
        return n

    def compress_files(self, data, offsets, sizes, data_on_device=False, data_size=None):
        """Each (offset, size) is an independent input; -> uint64 array file_off[n+1] into the device stream buffer."""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        szs = np.ascontiguousarray(sizes, dtype=np.uint32)
        self._block_n = szs
        out = np.zeros(len(offs) + 1, dtype=np.uint64)
        if data_on_device:
            ptr, size = int(data), int(data_size)
        else:
            self._data = _as_u8(data)
            ptr, size = self._data.ctypes.data, len(self._data)
        f = self.lib.L.zultra_hip_compress_files
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        n = f(self.h, ptr, size, 1 if data_on_device else 0, offs.ctypes.data, szs.ctypes.data, len(offs), out.ctypes.data)
        if n <= 0:
            raise ZultraError("zultra_hip_compress_files: " + self.lib.L.zultra_hip_last_error(self.h).decode())
        return out

    def subblocks(self):
        cnt = C.c_uint32()
        p = self.lib.L.zultra_hip_subblocks(self.h, C.byref(cnt))
        return [p[i] for i in range(cnt.value)], p, cnt.value

    def subblocks_raw(self):
        """-> (pointer to zultra_hip_subblock_t[count], count) without building Python objects."""
        cnt = C.c_uint32()
        p = self.lib.L.zultra_hip_subblocks(self.h, C.byref(cnt))
        return p, cnt.value

    def subblock_bits(self, sb):
        size = C.c_size_t()
        p = self.lib.L.zultra_hip_payload(self.h, C.byref(size))
        nbytes = (sb.nbits + 7) // 8
        return bytes(bytearray(p[sb.bits_off: sb.bits_off + nbytes]))

    def timing(self):
        t = Timing()
        self.lib.L.zultra_hip_last_timing(self.h, C.byref(t))
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    def stats(self):
        st = Stats()
        self.lib.L.zultra_hip_last_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        self.lib.L.zultra_hip_last_stats.restype = None
        self.lib.L.zultra_hip_last_stats(self.h, C.byref(st))
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def mf_chunk(self, window_size):
        """-> (the matchfinder's chunk size for a segment window of window_size bytes, the notes a segment's table holds): zultra_hip_mf_chunk."""
        notes = C.c_uint32(0)
        self.lib.L.zultra_hip_mf_chunk.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        self.lib.L.zultra_hip_mf_chunk.restype = C.c_uint32
        cap = self.lib.L.zultra_hip_mf_chunk(self.h, window_size, C.byref(notes))
        return int(cap), int(notes.value)

    def matches(self, block):
        n = int(self._block_n[block])
        m = np.zeros((n, 8, 2), dtype=np.uint16)
        if self.lib.L.zultra_hip_get_matches(self.h, block, m.ctypes.data) != 0:
            raise ZultraError("get_matches")
        return m

    def splits(self, block):
        out = (C.c_int * 64)()
        k = self.lib.L.zultra_hip_get_splits(self.h, block, out)
        if k < 0:
            raise ZultraError("get_splits")
        return list(out[:k])

    def parse(self, block):
        n = int(self._block_n[block])
        m = np.zeros((n, 2), dtype=np.uint16)
        if self.lib.L.zultra_hip_get_parse(self.h, block, m.ctypes.data) != 0:
            raise ZultraError("get_parse")
        return m

    def stitch_with_batch(self, final_block, phase=0, enable=True):
        """Arms the next compress_blocks to stitch at `phase` behind its last kernel (zultra_hip_stitch_with_batch); stitch_device with the same
        arguments then returns that result without a launch."""
        L = self.lib.L
        L.zultra_hip_stitch_with_batch.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int]
        if L.zultra_hip_stitch_with_batch(self.h, 1 if enable else 0, phase, final_block) != 0:
            raise ZultraError("zultra_hip_stitch_with_batch")

    def stitch_device(self, final_block, phase=0):
        """Device stitcher over the last batch -> (end_bit, new_phase); the stream stays in HBM (stream_ptr)."""
        L = self.lib.L
        L.zultra_hip_stitch_device.argtypes = [C.c_void_p, C.POINTER(BitState), C.c_int, C.POINTER(C.c_uint64)]
        st = BitState(0, phase)
        eb = C.c_uint64()
        rc = L.zultra_hip_stitch_device(self.h, C.byref(st), final_block, C.byref(eb))
        if rc != 0:
            raise ZultraError("zultra_hip_stitch_device: %d %s" % (rc, L.zultra_hip_last_error(self.h).decode()))
        return eb.value, st.nacc

    def stream_ptr(self):
        self.lib.L.zultra_hip_stream_device.argtypes = [C.c_void_p]
        self.lib.L.zultra_hip_stream_device.restype = C.c_void_p
        return self.lib.L.zultra_hip_stream_device(self.h)

    def stream_read(self, nbytes, offset=0, out=None):
        """-> uint8 array of the stream bytes [offset, offset + nbytes). out: a uint8 array to read into (its first nbytes are returned) — a
        caller that reads batch after batch hands in one pinned buffer instead of touching fresh pageable memory every time."""
        if out is None:
            out = np.empty(nbytes, dtype=np.uint8)
        else:
            assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= nbytes
            out = out[:nbytes]
        self.lib.L.zultra_hip_stream_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        if self.lib.L.zultra_hip_stream_read(self.h, out.ctypes.data, offset, nbytes) != 0:
            raise ZultraError("stream_read")
        return out

    def stream_write(self, data, offset=0):
        """Overwrites stream bytes [offset, offset + len(data)) (zultra_hip_stream_write)."""
        d = _as_u8(data)
        self.lib.L.zultra_hip_stream_write.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        if self.lib.L.zultra_hip_stream_write(self.h, d.ctypes.data, offset, len(d)) != 0:
            raise ZultraError("stream_write")

    def stitch_files(self):
        """zultra_hip_stitch_files over the last batch -> uint64 array file_off[blocks + 1] into the stream buffer."""
        out = np.zeros(len(self._block_n) + 1, dtype=np.uint64)
        f = self.lib.L.zultra_hip_stitch_files
        f.argtypes = [C.c_void_p, C.c_void_p]
        rc = f(self.h, out.ctypes.data)
        if rc != 0:
            raise ZultraError("zultra_hip_stitch_files: %d %s" % (rc, self.lib.L.zultra_hip_last_error(self.h).decode()))
        return out

    def frame_members(self, framing, bgzf_eof=False, blocks=None):
        """zultra_hip_frame_members over the last batch: every max-block a complete member of `framing` (0, FLAG_ZLIB, FLAG_GZIP, FRAME_BGZF) in the
        stream buffer. -> (rc, members as a MEMBER_DTYPE array, total_bytes); rc 0, or -1 / -2 / -3 as the call returns them. blocks: how many
        max-blocks the last batch had, where this object did not see it."""
        n = len(self._block_n) if blocks is None else blocks
        members = np.zeros(max(n, 1), dtype=MEMBER_DTYPE)
        total = C.c_uint64(0)
        f = self.lib.L.zultra_hip_frame_members
        f.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
        f.restype = C.c_int
        rc = f(self.h, framing, 1 if bgzf_eof else 0, members.ctypes.data, C.byref(total))
        return rc, members[:n], int(total.value)

    def frame_ms(self):
        """Device time of the last frame_members' launches, milliseconds: (scan, mover, frame kernel)."""
        ms = (C.c_float * 3)()
        f = self.lib.L.zultra_hip_last_frame_ms
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        f.restype = None
        f(self.h, ms)
        return [float(v) for v in ms]

    def zip_members(self, names, entry_block=None, base_off=0, dos_datetime=0):
        """zultra_hip_zip_members over the last batch: names[i] (bytes, or str encoded as UTF-8) names entry i, which is max-block entry_block[i] of the
        batch or, for ZIP_EMPTY, an empty entry; None: entry i is max-block i. -> (rc, entries as a ZIP_ENTRY_DTYPE array, local_bytes, central_bytes,
        central_at); rc 0, or -1 / -2 as the call returns them."""
        names = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in names]
        n = len(names)
        blob = _as_u8(b"".join(names) + b"\0")
        name_off = np.concatenate([[0], np.cumsum([len(s) for s in names])]).astype(np.uint32)
        eb = None if entry_block is None else np.ascontiguousarray(entry_block, dtype=np.uint32)
        entries = np.zeros(max(n, 1), dtype=ZIP_ENTRY_DTYPE)
        local, central = C.c_uint64(0), C.c_uint64(0)
        f = self.lib.L.zultra_hip_zip_members
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        f.restype = C.c_int
        rc = f(self.h, blob.ctypes.data, name_off.ctypes.data, None if eb is None else eb.ctypes.data, n, base_off, dos_datetime, entries.ctypes.data, C.byref(local), C.byref(central))
        return rc, entries[:n], int(local.value), int(central.value), self.zip_ptr()[1]

    def frame_streams(self, stream_first, framing):
        """zultra_hip_frame_streams over the last batch: stream s = max-blocks stream_first[s] .. stream_first[s + 1] - 1, a complete member of `framing`
        (0, FLAG_ZLIB, FLAG_GZIP) each. -> (rc, members as a MEMBER_DTYPE array, total_bytes); rc 0, or -1 / -2 as the call returns them."""
        first = np.ascontiguousarray(stream_first, dtype=np.uint32)
        members = np.zeros(max(len(first), 1), dtype=MEMBER_DTYPE)
        total = C.c_uint64(0)
        f = self.lib.L.zultra_hip_frame_streams
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint, C.c_void_p, C.POINTER(C.c_uint64)]
        f.restype = C.c_int
        rc = f(self.h, first.ctypes.data if len(first) else None, len(first), framing, members.ctypes.data, C.byref(total))
        return rc, members[:len(first)], int(total.value)

    def zip_streams(self, stream_first, names, entry_stream=None, base_off=0, dos_datetime=0):
        """zultra_hip_zip_streams over the last batch: zip_members with the streams of the grouping stream_first as entries. -> (rc, entries as a
        ZIP_ENTRY_DTYPE array, local_bytes, central_bytes, central_at)."""
        first = np.ascontiguousarray(stream_first, dtype=np.uint32)
        names = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in names]
        n = len(names)
        blob = _as_u8(b"".join(names) + b"\0")
        name_off = np.concatenate([[0], np.cumsum([len(s) for s in names])]).astype(np.uint32)
        es = None if entry_stream is None else np.ascontiguousarray(entry_stream, dtype=np.uint32)
        entries = np.zeros(max(n, 1), dtype=ZIP_ENTRY_DTYPE)
        local, central = C.c_uint64(0), C.c_uint64(0)
        f = self.lib.L.zultra_hip_zip_streams
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        f.restype = C.c_int
        rc = f(self.h, first.ctypes.data if len(first) else None, len(first), blob.ctypes.data, name_off.ctypes.data, None if es is None else es.ctypes.data, n, base_off, dos_datetime,
               entries.ctypes.data, C.byref(local), C.byref(central))
        return rc, entries[:n], int(local.value), int(central.value), self.zip_ptr()[1]

    def streams_ms(self):
        """Device time of the last grouped assembly's launches, milliseconds: (scan, fold, frame kernel)."""
        ms = (C.c_float * 3)()
        f = self.lib.L.zultra_hip_last_streams_ms
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        f.restype = None
        f(self.h, ms)
        return [float(v) for v in ms]

    def stitch_items(self):
        """zultra_hip_stitch_items -> the items of the last assembly's scan, a STITCH_ITEM_DTYPE array (one per sub-block)."""
        cnt = C.c_uint32()
        self.lib.L.zultra_hip_subblocks(self.h, C.byref(cnt))
        items = np.zeros(max(cnt.value, 1), dtype=STITCH_ITEM_DTYPE)
        f = self.lib.L.zultra_hip_stitch_items
        f.argtypes = [C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        if f(self.h, items.ctypes.data) != cnt.value:
            raise ZultraError("zultra_hip_stitch_items")
        return items[:cnt.value]

    def plan_streams(self, stream_first, framing):
        """zultra_hip_plan_streams: the host planner's statement of a grouped assembly of the last batch -> (rc, items, file_off, end_bit)."""
        first = np.ascontiguousarray(stream_first, dtype=np.uint32)
        cnt = C.c_uint32()
        self.lib.L.zultra_hip_subblocks(self.h, C.byref(cnt))
        items = np.zeros(max(cnt.value, 1), dtype=STITCH_ITEM_DTYPE)
        file_off = np.zeros(len(first) + 1, dtype=np.uint64)
        end = C.c_uint64(0)
        f = self.lib.L.zultra_hip_plan_streams
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        f.restype = C.c_int
        rc = f(self.h, first.ctypes.data if len(first) else None, len(first), framing, items.ctypes.data, file_off.ctypes.data, C.byref(end))
        return rc, items[:cnt.value], file_off, int(end.value)

    def zip_ptr(self):
        """zultra_hip_zip_device -> (the device pointer of the zip buffer, or None before the first zip_members; where the central part starts in it)."""
        at = C.c_uint64(0)
        f = self.lib.L.zultra_hip_zip_device
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        f.restype = C.c_void_p
        return f(self.h, C.byref(at)), int(at.value)

    def zip_read(self, nbytes, offset=0):
        """-> uint8 array of the zip buffer's bytes [offset, offset + nbytes) (zultra_hip_zip_read)."""
        out = np.empty(max(nbytes, 1), dtype=np.uint8)
        f = self.lib.L.zultra_hip_zip_read
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
        f.restype = C.c_int
        if f(self.h, out.ctypes.data, offset, nbytes) != 0:
            raise ZultraError("zip_read")
        return out[:nbytes]

    def last_zip_ms(self):
        """Device time of the last zip_members' launches, milliseconds: (scan, records, copy)."""
        ms = (C.c_float * 3)()
        f = self.lib.L.zultra_hip_last_zip_ms
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        f.restype = None
        f(self.h, ms)
        return [float(v) for v in ms]

    def verify(self):
        """zultra_hip_verify_device over the last stitched batch -> dict of the report plus "rc" (0 verified, 1 mismatch) and "verify_ms"."""
        L = self.lib.L
        L.zultra_hip_verify_device.argtypes = [C.c_void_p, C.POINTER(Verify)]
        L.zultra_hip_last_verify_ms.argtypes = [C.c_void_p]
        L.zultra_hip_last_verify_ms.restype = C.c_float
        r = Verify()
        rc = L.zultra_hip_verify_device(self.h, C.byref(r))
        if rc < 0:
            raise ZultraError("zultra_hip_verify_device: " + L.zultra_hip_last_error(self.h).decode())
        out = {k: int(getattr(r, k)) for k, _ in Verify._fields_}
        out["rc"] = rc
        out["verify_ms"] = float(L.zultra_hip_last_verify_ms(self.h))
        return out

    def block_adler32(self):
        """-> uint32 array [n, 2]: per max-block / input the two Adler-32 sums (A, Bw) the device took next to the compression (zultra_adler32_append folds them)."""
        n = len(self._block_n)
        out = np.zeros((n, 2), dtype=np.uint32)
        self.lib.L.zultra_hip_block_adler32.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.L.zultra_hip_block_adler32(self.h, out.ctypes.data)
        return out

    def block_crc32(self):
        n = len(self._block_n)
        out = np.zeros(n, dtype=np.uint32)
        self.lib.L.zultra_hip_block_crc32.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.L.zultra_hip_block_crc32(self.h, out.ctypes.data)
        return out

    def stitch(self, raw, raw_offs, max_block, final_block, state=None, finish=True):
        """Host stitcher over the last batch -> (bytes, BitState)."""
        subs, p, cnt = self.subblocks()
        size = C.c_size_t()
        payload = self.lib.L.zultra_hip_payload(self.h, C.byref(size))
        raw = _as_u8(raw)
        offs = (C.c_uint64 * len(raw_offs))(*raw_offs)
        st = state or BitState(0, 0)
        cap = len(raw) + 64 * 6 * len(raw_offs) + 1024
        out = np.empty(cap, dtype=np.uint8)
        w = self.lib.L.zultra_hip_stitch(C.byref(st), p, cnt, payload, raw.ctypes.data, offs, max_block, final_block, out.ctypes.data, cap)
        if w == _SIZE_MAX:
            return None, st
        if finish:
            f = self.lib.L.zultra_hip_stitch_finish(C.byref(st), out.ctypes.data + w, cap - w)
            w += f
        return out[:w].tobytes(), st
