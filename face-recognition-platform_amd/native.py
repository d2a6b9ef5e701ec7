"""ctypes binding of libfrp.so (C ABI: include/frp.h).  No CPU fallback: if the library
or a GPU is missing every constructor raises -- the product path never routes around HIP."""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  Two handles that keep two batches
# in flight on one GPU (lanes.py) need their compute streams on DIFFERENT queues; next to torch's and RCCL's streams four
# queues were not enough (measured: no gain from the second lane in 3 of 3 processes with 4 queues, the full gain in 5 of
# 5 with 8).  The runtime reads the variable when it initialises, so this only helps when this module is imported before
# the first HIP call of the process - export it in the service's environment otherwise.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

# FRP_LIB: another build of the same library (same-box A/B of kernel variants: tools/ab_lib.sh)
LIB_PATH = os.environ.get("FRP_LIB") or os.path.join(_HERE, "libfrp.so")

EMB_DIM = 512
CHIP = 112
MAX_FACES_CAP = 128
MAX_TOPK = 64
FLAG_FORCED_K, FLAG_RGB, FLAG_NO_MATCH, FLAG_WITHIN, FLAG_GROUPS, FLAG_TRACK = 1, 2, 4, 8, 16, 32
FLAG_JPEG_OPTIMIZE = 64                      # include/frp.h: FRP_FLAG_JPEG_OPTIMIZE - encode_jpeg / encode_jpeg_enhanced(optimize=True)
JPEG_HIST_ELEMS = 544                        # include/frp.h: FRP_JPEG_HIST_ELEMS - per image dc [2][16], then ac [2][256]
GROUPS_ALL = 0xFFFFFFFF                      # include/frp.h: FRP_GROUPS_ALL - the mask of a gallery row that arrived without one
F32, F16, F64 = 0, 1, 2
JPEG_SUBSAMPLING = {"4:2:0": 420, "4:4:4": 444}      # include/frp.h: FRP_JPEG_420, FRP_JPEG_444
YUV_LAYOUTS = {"NV12": 0, "NV21": 1, "I420": 2, "YV12": 3}      # include/frp.h: FRP_YUV_NV12 ... (plane order: frp_upload_yuv)
YUV_MATRICES = {"BT601": 0, "BT709": 1, "JFIF": 2}             # FRP_YUV_BT601, FRP_YUV_BT709, FRP_YUV_JFIF
YUV_DEVICE = 1                                                  # frp_yuv_desc.flags: FRP_YUV_DEVICE
ENHANCE_MAX_RADIUS, ENHANCE_MAX_PIXELS = 2.0, 1 << 24      # include/frp.h: FRP_ENHANCE_MAX_RADIUS, FRP_ENHANCE_MAX_PIXELS (per output image)
CLUSTER_EXACT, CLUSTER_MAX_TILE = 1, 64                 # include/frp.h: FRP_CLUSTER_EXACT, FRP_CLUSTER_MAX_TILE
QUALITY_TILE_H, QUALITY_TILE_W = 32, 64      # csrc/frp_internal.h: one workgroup of the face-quality kernel covers this much of a crop

ABI_SYMBOLS = [
    "frp_create", "frp_destroy", "frp_last_error", "frp_version", "frp_load_weights",
    "frp_gallery_set", "frp_gallery_set_device", "frp_gallery_reserve", "frp_gallery_commit", "frp_gallery_cancel", "frp_gallery_device_ptr", "frp_gallery_update_row", "frp_gallery_remove_row",
    "frp_jpeg_info_get", "frp_jpeg_coefficients", "frp_upload_jpeg_async", "frp_debug_jpeg_device_batches", "frp_debug_graph_replays",
    "frp_set_jpeg_selfsync", "frp_debug_jpeg_selfsync_batches", "frp_jpeg_selfsync_coefficients",
    "frp_dist_unique_id", "frp_dist_init", "frp_dist_destroy", "frp_gallery_allgather",
    "frp_gallery_size", "frp_gallery_get", "frp_gallery_set_groups", "frp_gallery_get_groups", "frp_gallery_exact", "frp_gallery_distances", "frp_gallery_get_exact", "frp_gallery_cluster",
    "frp_process_frames", "frp_upload_frames", "frp_process_resident", "frp_fetch_results", "frp_synchronize",
    "frp_host_alloc", "frp_host_free", "frp_upload_frames_async", "frp_swap_frames",
    "frp_upload_yuv", "frp_upload_yuv_async", "frp_get_frames",
    "frp_detect", "frp_detect_resident", "frp_get_det_source", "frp_finish_faces", "frp_process_pyramid", "frp_debug_pyramid_merge", "frp_debug_fc_l2norm", "frp_get_head_map", "frp_debug_det_prefix", "frp_debug_det_hashes", "frp_decode_heads", "frp_align", "frp_debug_align_resident", "frp_embed_aligned", "frp_embed_faces",
    "frp_match", "frp_match_scores", "frp_debug_match_f16", "frp_match_within", "frp_set_within", "frp_fetch_within", "frp_match_groups", "frp_match_within_groups", "frp_set_frame_groups",
    "frp_track_config", "frp_set_frame_streams", "frp_track_reset", "frp_fetch_tracks", "frp_track_stats", "frp_debug_track_step",
    "frp_face_quality", "frp_jpeg_encode_headers", "frp_encode_jpeg", "frp_encode_jpeg_coefficients", "frp_jpeg_optimal_table", "frp_encode_jpeg_histograms", "frp_enhance_pixels", "frp_encode_jpeg_enhanced", "frp_conv2d_nhwc", "frp_conv_block64", "frp_conv2d_f8", "frp_get_counters", "frp_reset_counters", "frp_set_profile",
]


class FrpConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("max_batch", C.c_int32), ("max_faces", C.c_int32),
                ("max_h", C.c_int32), ("max_w", C.c_int32), ("profile", C.c_int32), ("reserved", C.c_int32 * 10)]


class FrpEnhanceParams(C.Structure):     # include/frp.h: frp_enhance_params
    _fields_ = [("radius", C.c_float), ("percent", C.c_int32), ("threshold", C.c_int32), ("sharpen", C.c_int32)]


class FrpCounters(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("calls", C.c_int32), ("frames", C.c_int64), ("faces", C.c_int64),
                ("ms_h2d", C.c_double), ("ms_preprocess", C.c_double), ("ms_det_conv", C.c_double),
                ("ms_decode", C.c_double), ("ms_align", C.c_double), ("ms_emb_conv", C.c_double),
                ("ms_l2norm", C.c_double), ("ms_match", C.c_double), ("ms_d2h", C.c_double), ("ms_total", C.c_double),
                ("det_conv_flops", C.c_double), ("emb_conv_flops", C.c_double),
                ("det_conv_launches", C.c_int64), ("emb_conv_launches", C.c_int64),
                ("match_bytes", C.c_double), ("match_launches", C.c_int64), ("gallery_rows", C.c_int64),
                ("f8_conv_flops", C.c_double), ("f8_conv_launches", C.c_int64), ("reserved", C.c_double * 6)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n not in ("reserved", "struct_size")}


class JpegInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("h_samp", C.c_int32 * 3), ("v_samp", C.c_int32 * 3),
                ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("restart_interval", C.c_int32), ("progressive", C.c_int32)]

    def as_dict(self) -> dict:
        return {"width": self.width, "height": self.height, "components": self.components, "h_samp": list(self.h_samp),
                "v_samp": list(self.v_samp), "mcus_x": self.mcus_x, "mcus_y": self.mcus_y, "restart_interval": self.restart_interval}


class FrpYuvDesc(C.Structure):
    """include/frp.h: frp_yuv_desc"""
    _fields_ = [("struct_size", C.c_int32), ("layout", C.c_int32), ("matrix", C.c_int32), ("flags", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("y_pitch", C.c_int64), ("c_pitch", C.c_int64)]


def _byte_ptr(data):
    """(pointer, keep-alive) to the bytes of `data` without copying them where the object allows it (bytes and its subclasses:
    the object's own buffer; a bytearray: its buffer; anything else is copied once).  A 1080p JPEG is ~0.7 MB and a batch holds
    32 of them: per-call copies were tens of megabytes of memcpy on the thread that feeds the lane."""
    if isinstance(data, bytes):
        p = C.c_char_p(data)
        return C.cast(p, C.c_void_p), (p, data)
    if isinstance(data, bytearray):
        buf = (C.c_char * len(data)).from_buffer(data)
        return C.cast(buf, C.c_void_p), buf
    buf = (C.c_char * len(data)).from_buffer_copy(data)
    return C.cast(buf, C.c_void_p), buf


def jpeg_info(data: bytes):
    """header of a baseline JPEG as the library's decoder sees it, or None when it does not cover the file (progressive,
    arithmetic-coded, 12-bit, CMYK, multi-scan): include/frp.h frp_jpeg_info_get.  Needs no GPU."""
    info = JpegInfo()
    ptr, keep = _byte_ptr(data)
    rc = load_library().frp_jpeg_info_get(ptr, len(data), C.byref(info))
    del keep
    return info.as_dict() if rc == 0 else None


def jpeg_coefficients(data: bytes):
    """host entropy decode alone (parity tests): -> (info dict, int16 coefficients, uint16 [3, 64] tables)"""
    info = jpeg_info(data)
    if info is None:
        raise FrpError(-1, "not a baseline JPEG the decoder covers")
    n = sum(info["mcus_x"] * info["h_samp"][c] * info["mcus_y"] * info["v_samp"][c] * 64 for c in range(info["components"]))
    coef = np.zeros(n, np.int16)
    q = np.zeros((3, 64), np.uint16)
    ji = JpegInfo()
    ptr, keep = _byte_ptr(data)
    rc = load_library().frp_jpeg_coefficients(ptr, len(data), _ptr(coef), n, _ptr(q), C.byref(ji))
    del keep
    if rc != 0:
        raise FrpError(rc, "corrupt JPEG scan data")
    return info, coef, q


def _subsampling_code(subsampling) -> int:
    """"4:2:0" / "4:4:4" -> the library's constant; anything else goes through as -1 for the library to refuse"""
    return JPEG_SUBSAMPLING.get(subsampling, -1)


def jpeg_encode_headers(width: int, height: int, quality: int = 95, subsampling: str = "4:2:0", restart_mcus: int = 0) -> bytes:
    """the segments the encoder puts in front of a scan - SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI (restart_mcus > 0), SOS: include/frp.h
    frp_jpeg_encode_headers.  Needs no GPU."""
    buf = np.zeros(1024, np.uint8)
    n = load_library().frp_jpeg_encode_headers(int(width), int(height), int(quality), _subsampling_code(subsampling), int(restart_mcus),
                                               _ptr(buf), buf.size)
    if n < 0:
        raise FrpError(int(n), "jpeg_encode_headers: argument out of range")
    return buf[:n].tobytes()


def jpeg_optimal_table(freq):
    """libjpeg's jpeg_gen_optimal_table: the counts of the 256 symbols -> (bits [16]: codes of length 1..16, vals: the symbols by
    code length, then by value) of the length-limited Huffman code, as a DHT segment carries them: include/frp.h
    frp_jpeg_optimal_table.  Needs no GPU."""
    f = np.ascontiguousarray(freq, dtype=np.uint32).reshape(-1)
    if f.size != 256:
        raise ValueError(f"{f.size} counts, 256 expected")
    bits, vals = np.zeros(16, np.uint8), np.zeros(256, np.uint8)
    n = load_library().frp_jpeg_optimal_table(_ptr(f), _ptr(bits), _ptr(vals))
    if n < 0:
        raise FrpError(int(n), "jpeg_optimal_table: all counts are zero, or the code is deeper than 32 bits")
    return bits.tolist(), vals[:n].tolist()


class FrpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"frp error {code}: {msg}")
        self.code = code


_lib = None


def kernel_source_hash() -> str:
    """sha256 over the native sources (csrc/*.hip|h|cpp, include/*.h): ties a committed profile summary
    (profiles/*/pmc_traffic.json) to the kernels it was measured on"""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")) +
                   glob.glob(os.path.join(_HERE, "csrc", "*.cpp")) + glob.glob(os.path.join(os.path.dirname(_HERE), "include", "*.h")))
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load_library() -> C.CDLL:
    """dlopen libfrp.so; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not built: run `make -C {os.path.join(_HERE, 'csrc')}`")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint32
    lib.frp_create.argtypes = [C.c_int, C.POINTER(FrpConfig), C.POINTER(vp)]
    lib.frp_destroy.argtypes = [vp]
    lib.frp_destroy.restype = None
    lib.frp_last_error.argtypes = [vp]
    lib.frp_last_error.restype = C.c_char_p
    lib.frp_version.restype = C.c_char_p
    lib.frp_load_weights.argtypes = [vp, vp, C.c_size_t]
    lib.frp_gallery_set.argtypes = [vp, vp, i64, i32, i32]
    lib.frp_gallery_set_device.argtypes = [vp, vp, i64, i32]
    lib.frp_gallery_reserve.argtypes = [vp, i64, C.POINTER(C.c_void_p)]
    lib.frp_gallery_commit.argtypes = [vp, i64]
    lib.frp_gallery_cancel.argtypes = [vp]
    lib.frp_gallery_device_ptr.argtypes = [vp]
    lib.frp_gallery_device_ptr.restype = vp
    lib.frp_gallery_update_row.argtypes = [vp, i64, vp, i32, i32]
    lib.frp_gallery_remove_row.argtypes = [vp, i64]
    lib.frp_gallery_size.argtypes = [vp]
    lib.frp_gallery_size.restype = i64
    lib.frp_gallery_get.argtypes = [vp, vp, i64, i64]
    lib.frp_jpeg_info_get.argtypes = [vp, C.c_size_t, vp]
    lib.frp_jpeg_coefficients.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, vp]
    lib.frp_upload_jpeg_async.argtypes = [vp, vp, vp, i32]
    lib.frp_gallery_exact.argtypes = [vp, i32]
    lib.frp_gallery_distances.argtypes = [vp, vp, i32, vp, i64]
    lib.frp_gallery_get_exact.argtypes = [vp, vp, i64, i64]
    if hasattr(lib, "frp_gallery_cluster"):  # (an older build loaded through FRP_LIB as an A/B partner has none)
        lib.frp_gallery_cluster.argtypes = [vp, vp, i64, f32, C.c_double, i32, u32, vp, C.POINTER(i32)]
    lib.frp_process_frames.argtypes = [vp, vp, i32, i32, i32, i64, i32, f32, f32, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.frp_upload_frames.argtypes = [vp, vp, i32, i32, i32, i64]
    lib.frp_process_resident.argtypes = [vp, i32, f32, f32, u32]
    lib.frp_fetch_results.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.frp_synchronize.argtypes = [vp]
    lib.frp_host_alloc.argtypes = [vp, C.c_size_t]
    lib.frp_host_alloc.restype = vp
    lib.frp_host_free.argtypes = [vp, vp]
    lib.frp_host_free.restype = None
    lib.frp_upload_frames_async.argtypes = [vp, vp, i32, i32, i32, i64]
    lib.frp_swap_frames.argtypes = [vp]
    if hasattr(lib, "frp_upload_yuv"):       # (as frp_match_within below: an older A/B partner build has none)
        lib.frp_upload_yuv.argtypes = [vp, C.POINTER(FrpYuvDesc), vp, i32]
        lib.frp_upload_yuv_async.argtypes = [vp, C.POINTER(FrpYuvDesc), vp, i32]
        lib.frp_get_frames.argtypes = [vp, vp, i64, i32, i32]
    lib.frp_detect.argtypes = [vp, vp, i32, i32, i32, i64, i32, f32, f32, u32, vp, vp, vp, vp, vp]
    lib.frp_detect_resident.argtypes = [vp, i32, i32, i32, i32, f32, f32, u32, vp, vp, vp, vp, vp]
    lib.frp_get_det_source.argtypes = [vp, vp, i64, C.POINTER(i32), C.POINTER(i32)]
    lib.frp_finish_faces.argtypes = [vp, i32, vp, vp, vp, vp, i32, u32, vp, vp, vp]
    if hasattr(lib, "frp_process_pyramid"):  # (as frp_match_within below: an older A/B partner build has none)
        lib.frp_process_pyramid.argtypes = [vp, i32, vp, i32, i32, f32, f32, u32]
        lib.frp_debug_pyramid_merge.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp]
        lib.frp_debug_fc_l2norm.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.frp_get_head_map.argtypes = [vp, i32, vp, i64, C.POINTER(i32), C.POINTER(i32)]
    lib.frp_debug_jpeg_device_batches.argtypes = [vp]
    lib.frp_debug_jpeg_device_batches.restype = C.c_int64
    lib.frp_set_jpeg_selfsync.argtypes = [vp, i32]
    lib.frp_debug_jpeg_selfsync_batches.argtypes = [vp]
    lib.frp_debug_jpeg_selfsync_batches.restype = C.c_int64
    lib.frp_jpeg_selfsync_coefficients.argtypes = [vp, vp, vp, i32, i32, vp, i64, vp]
    lib.frp_debug_graph_replays.argtypes = [vp]
    lib.frp_debug_graph_replays.restype = C.c_int64
    lib.frp_dist_unique_id.argtypes = [vp]
    lib.frp_dist_init.argtypes = [vp, vp, i32, i32]
    lib.frp_dist_destroy.argtypes = [vp]
    lib.frp_gallery_allgather.argtypes = [vp, vp, i64, i32, i64]
    lib.frp_debug_det_prefix.argtypes = [vp, i32, vp, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.frp_debug_det_hashes.argtypes = [vp, i32, vp]
    lib.frp_decode_heads.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, u32, vp, vp, vp, vp, vp]
    lib.frp_align.argtypes = [vp, vp, i32, i32, i64, vp, i32, u32, vp]
    if hasattr(lib, "frp_debug_align_resident"):     # (as frp_match_within below: an older A/B partner build has none)
        lib.frp_debug_align_resident.argtypes = [vp, vp, vp, i32, u32, i32, vp, i64]
    lib.frp_embed_aligned.argtypes = [vp, vp, i32, vp]
    lib.frp_embed_faces.argtypes = [vp, vp, i32, i32, i64, vp, i32, u32, vp]
    lib.frp_match.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.frp_match_scores.argtypes = [vp, vp, i32, vp, i64]
    if hasattr(lib, "frp_debug_match_f16"):  # (as frp_match_within below: an older A/B partner build has none)
        lib.frp_debug_match_f16.argtypes = [vp, vp, i32, i32, vp, vp, vp, i64]
    if hasattr(lib, "frp_match_within"):     # (an older build loaded through FRP_LIB as the A/B partner of tools/ab_bench.sh has none)
        lib.frp_match_within.argtypes = [vp, vp, i32, f32, i32, vp, vp, vp]
        lib.frp_set_within.argtypes = [vp, f32, i32]
        lib.frp_fetch_within.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    if hasattr(lib, "frp_match_groups"):     # (as frp_match_within above)
        lib.frp_gallery_set_groups.argtypes = [vp, vp, i64, i64]
        lib.frp_gallery_get_groups.argtypes = [vp, vp, i64, i64]
        lib.frp_set_frame_groups.argtypes = [vp, vp, i32]
        lib.frp_match_groups.argtypes = [vp, vp, i32, vp, i32, vp, vp]
        lib.frp_match_within_groups.argtypes = [vp, vp, i32, vp, f32, i32, vp, vp, vp]
    if hasattr(lib, "frp_track_config"):     # (as above)
        lib.frp_track_config.argtypes = [vp, i32, f32, i32, i32]
        lib.frp_set_frame_streams.argtypes = [vp, vp, i32]
        lib.frp_track_reset.argtypes = [vp, i32]
        lib.frp_fetch_tracks.argtypes = [vp, i32, i32, vp, vp, vp]
        lib.frp_track_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
        lib.frp_debug_track_step.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32), vp, vp, vp]
    if hasattr(lib, "frp_face_quality"):     # (as above: an older A/B partner build has none)
        lib.frp_face_quality.argtypes = [vp, vp, i32, u32, vp]
    if hasattr(lib, "frp_encode_jpeg"):      # (as above)
        lib.frp_jpeg_encode_headers.argtypes = [i32, i32, i32, i32, i32, vp, i64]
        lib.frp_jpeg_encode_headers.restype = i64
        lib.frp_encode_jpeg.argtypes = [vp, vp, i32, i32, i32, i32, u32, vp, i64, vp]
        lib.frp_encode_jpeg_coefficients.argtypes = [vp, vp, i32, i32, i32, u32, vp, i64]
    if hasattr(lib, "frp_jpeg_optimal_table"):   # (as above)
        lib.frp_jpeg_optimal_table.argtypes = [vp, vp, vp]
        lib.frp_encode_jpeg_histograms.argtypes = [vp, vp, i32, i32, i32, i32, u32, vp, i64]
    if hasattr(lib, "frp_enhance_pixels"):   # (as above)
        lib.frp_enhance_pixels.argtypes = [vp, vp, vp, i32, C.POINTER(FrpEnhanceParams), u32, vp, i64, vp]
        lib.frp_encode_jpeg_enhanced.argtypes = [vp, vp, vp, i32, C.POINTER(FrpEnhanceParams), i32, i32, i32, u32, vp, i64, vp]
    lib.frp_conv2d_nhwc.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp]
    if hasattr(lib, "frp_conv_block64"):   # (an older build loaded through FRP_LIB as an A/B partner has none)
        lib.frp_conv_block64.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp]
    lib.frp_conv2d_f8.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, i32, i32, f32, f32, vp, vp]
    if hasattr(lib, "frp_kstep_lab"):            # the FRP_LAB build (libfrp_lab.so, include/frp_lab.h): tuning hooks
        lib.frp_conv_bench.argtypes = [vp] + [i32] * 11 + [C.POINTER(C.c_float), vp]
        lib.frp_mfma_peak.argtypes = [vp, i32, i32, C.POINTER(C.c_float)]
        lib.frp_kstep_lab.argtypes = [vp, i32, i32, C.POINTER(C.c_float)]
    lib.frp_get_counters.argtypes = [vp, C.POINTER(FrpCounters)]
    lib.frp_reset_counters.argtypes = [vp]
    lib.frp_set_profile.argtypes = [vp, i32]
    _lib = lib
    return lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Engine:
    """One handle = one GPU + one stream (include/frp.h).  Thread-safe (library mutex);
    ctypes releases the GIL for the duration of every call."""

    def __init__(self, device: int = 0, max_batch: int = 32, max_faces: int = 10, max_h: int = 1080,
                 max_w: int = 1920, profile: bool = False):
        self._lib = load_library()
        cfg = FrpConfig()
        cfg.struct_size = C.sizeof(FrpConfig)
        cfg.max_batch, cfg.max_faces, cfg.max_h, cfg.max_w, cfg.profile = max_batch, max_faces, max_h, max_w, int(profile)
        h = C.c_void_p()
        rc = self._lib.frp_create(device, C.byref(cfg), C.byref(h))
        if rc != 0 or not h.value:
            raise FrpError(rc, "frp_create failed (no usable HIP device?)")
        self._h = h
        self.device = device
        self.max_batch = max_batch
        self.max_faces = max_faces
        # Multi-call sequences (upload -> process -> fetch, the pyramid) leave state on the handle between calls:
        # threads sharing one Engine take this lock around a whole sequence (`with eng.sequence(): ...`).  The
        # C side additionally checks every caller-sized buffer against the handle's state under its own mutex.
        self._seq = threading.RLock()
        # The shapes the caller-sized buffers of later calls follow; the library checks every one of them against the handle's own state,
        # so a call on an engine that has had no batch or pass reaches it with zeros and comes back as its refusal (FrpError).
        self._resident = (0, 0, 0)       # (B, H, W) of the resident frames
        self._staged = (0, 0, 0)         # ... of the staging frame buffer: resident at swap_frames()
        self._pass = (0, 0)              # (B, K) of the last pass that embeds faces: what fetch_results / fetch_within are sized for
        self._det_batch = 0              # frames of the detector run head_maps() reads back
        self._within_cap = 0             # set_within
        self._track_pass = (0, 0)        # (B, K) of the last pass with FLAG_TRACK (or track_step): what fetch_tracks is sized for
        self._yuv_keep = ()              # host planes of the last two upload_yuv_async batches

    _h = None                            # (an object whose __init__ raised is still closed by __del__)

    def close(self):
        if self._h is not None and self._h.value:
            self._lib.frp_destroy(self._h)
            self._h = C.c_void_p()

    def sequence(self):
        """lock held around a multi-call sequence on a shared Engine"""
        return self._seq

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != 0:
            raise FrpError(rc, (self._lib.frp_last_error(self._h) or b"").decode("utf-8", "replace"))

    @property
    def resident_shape(self) -> Tuple[int, int, int]:
        """(B, H, W) of the resident frames; zeros before the first batch"""
        return self._resident

    def _began(self, B: int, K: Optional[int] = None, heads: bool = False, flags: int = 0):
        """a pass over B frames has been taken by the library.  K: it embeds up to K faces per frame - the (B, K) fetch_results and
        fetch_within size their buffers for; heads: a detector run whose head maps head_maps() reads back, B frames of them"""
        if K is not None:
            self._pass = (B, K)
            if flags & FLAG_TRACK:
                self._track_pass = (B, K)
        if heads:
            self._det_batch = B

    # -- weights / gallery
    def load_weights(self, blob: bytes):
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        self._chk(self._lib.frp_load_weights(self._h, C.cast(buf, C.c_void_p), len(blob)))

    def gallery_set(self, emb: np.ndarray):
        emb = np.ascontiguousarray(emb)
        if emb.size == 0:
            self._chk(self._lib.frp_gallery_set(self._h, None, 0, EMB_DIM, F32))
            return
        dt = {np.dtype(np.float32): F32, np.dtype(np.float16): F16, np.dtype(np.float64): F64}.get(emb.dtype)
        if dt is None:
            emb, dt = emb.astype(np.float32), F32
        if emb.ndim == 2 and emb.shape[1] < EMB_DIM:          # narrower rows (128-d): zero-padded
            emb = np.ascontiguousarray(np.concatenate([emb, np.zeros((emb.shape[0], EMB_DIM - emb.shape[1]), emb.dtype)], axis=1))
        self._chk(self._lib.frp_gallery_set(self._h, _ptr(emb), emb.shape[0], emb.shape[1], dt))

    def gallery_set_device(self, dev_ptr: int, n: int):
        self._chk(self._lib.frp_gallery_set_device(self._h, C.c_void_p(dev_ptr), n, EMB_DIM))

    # -- multi-GPU: the gallery all-gather on the library's own RCCL communicator (include/frp.h: frp_dist_*)
    @staticmethod
    def dist_unique_id() -> bytes:
        """rank 0: a fresh 128-byte communicator id (carry it to the other ranks by any control channel)"""
        buf = C.create_string_buffer(128)
        rc = load_library().frp_dist_unique_id(buf)
        if rc != 0:
            raise FrpError(rc, "frp_dist_unique_id failed (librccl not loadable?)")
        return buf.raw

    def dist_init(self, unique_id: bytes, rank: int, world: int):
        """collective: this handle's communicator"""
        if len(unique_id) != 128:
            raise ValueError("the communicator id has 128 bytes")
        self._chk(self._lib.frp_dist_init(self._h, C.c_char_p(unique_id), rank, world))
        self._dist = (rank, world)

    def dist_destroy(self):
        self._chk(self._lib.frp_dist_destroy(self._h))
        self._dist = None

    def gallery_allgather(self, shard: np.ndarray, n_total: int):
        """collective: this rank's rows (host [rows, 512], any float dtype) -> the full unit fp16 gallery on every rank"""
        shard = np.ascontiguousarray(shard)
        if shard.dtype not in (np.float32, np.float16, np.float64):
            shard = shard.astype(np.float32)
        code = {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.float64): 2}[shard.dtype]
        shard = shard.reshape(-1, 512)
        self._chk(self._lib.frp_gallery_allgather(self._h, _ptr(shard) if shard.shape[0] else None, shard.shape[0], code, n_total))

    def gallery_reserve(self, capacity_rows: int) -> int:
        """device address of a fresh, not yet visible snapshot of capacity_rows x 512 fp16 (fill it, then gallery_commit)"""
        ptr = C.c_void_p()
        self._chk(self._lib.frp_gallery_reserve(self._h, capacity_rows, C.byref(ptr)))
        return int(ptr.value)

    def gallery_commit(self, n_rows: int):
        self._chk(self._lib.frp_gallery_commit(self._h, n_rows))

    def gallery_cancel(self):
        """discard a pending reservation (other gallery updates are refused while one is pending)"""
        self._chk(self._lib.frp_gallery_cancel(self._h))

    def gallery_device_ptr(self) -> int:
        """device address of the current snapshot (0 when empty); valid until the next gallery update"""
        return int(self._lib.frp_gallery_device_ptr(self._h) or 0)

    @staticmethod
    def _row512(emb: np.ndarray) -> Tuple[np.ndarray, int]:
        """one embedding as the library takes it: 512 float32 or - a float64 input stays float64, so the exact compat rows
        (gallery_exact) hold it bit for bit - float64 values; narrower rows (the reference's 128-d dlib encodings) are
        zero-padded, which changes neither a cosine nor a Euclidean distance"""
        e = np.asarray(emb)
        dt, code = (np.float64, F64) if e.dtype == np.float64 else (np.float32, F32)
        e = np.ascontiguousarray(e, dtype=dt).reshape(-1)
        if e.shape[0] < EMB_DIM:
            e = np.concatenate([e, np.zeros(EMB_DIM - e.shape[0], dt)])
        return e, code

    def gallery_update_row(self, row: int, emb: np.ndarray):
        e, code = self._row512(emb)
        self._chk(self._lib.frp_gallery_update_row(self._h, row, _ptr(e), e.shape[0], code))

    def upload_jpeg_async(self, jpegs: Sequence[bytes]):
        """B baseline JPEG stills of one geometry -> the staging frame buffer, decoded on the way: the bit streams on host
        threads, dequantisation / inverse DCT / chroma upsampling / YCbCr -> BGR on the GPU's copy stream (frp.h:
        frp_upload_jpeg_async).  Follow with swap_frames() as after upload_frames_async()."""
        B = len(jpegs)
        held = [_byte_ptr(j) for j in jpegs]                      # no copies: the call reads the callers' buffers (and returns after it has)
        ptrs = (C.c_void_p * B)(*[h[0] for h in held])
        sizes = (C.c_size_t * B)(*[len(j) for j in jpegs])
        self._chk(self._lib.frp_upload_jpeg_async(self._h, ptrs, sizes, B))
        del held
        info = jpeg_info(jpegs[0])
        self._staged = (B, info["height"], info["width"])

    def jpeg_device_batches(self) -> int:
        """diagnostic: upload_jpeg_async batches whose entropy decode ran on the device (restart-interval streams)"""
        return int(self._lib.frp_debug_jpeg_device_batches(self._h))

    def set_jpeg_selfsync(self, on=True):
        """upload_jpeg_async batches whose frames carry no restart markers: entropy decode on the device too (the self-synchronising
        decoder, frp.h: frp_set_jpeg_selfsync) instead of on host threads.  Off by default (FRP_JPEG_SELFSYNC: on for new handles)."""
        self._chk(self._lib.frp_set_jpeg_selfsync(self._h, int(on)))          # (an int above 1: on, with subsequences of that many bytes)

    def jpeg_selfsync_batches(self) -> int:
        """diagnostic: upload_jpeg_async batches decoded by the self-synchronising decoder"""
        return int(self._lib.frp_debug_jpeg_selfsync_batches(self._h))

    def jpeg_selfsync_coefficients(self, jpegs: Sequence[bytes], subseq_bytes: int = 0):
        """parity: the self-synchronising decode alone -> (coef [B, n] int16: every image in the layout of jpeg_coefficients, stats [B, 4]
        int32: subsequences, synchronisation rounds, blocks counted, error flag).  A corrupt image raises FrpError naming it; the
        statistics of that call are then in the error's `stats`."""
        B = len(jpegs)
        info = jpeg_info(jpegs[0]) if B else None
        if info is None:
            raise FrpError(-1, "JPEG 0: not a baseline JPEG the decoder covers")
        n = sum(info["mcus_x"] * info["h_samp"][c] * info["mcus_y"] * info["v_samp"][c] * 64 for c in range(info["components"]))
        coef = np.zeros((B, n), np.int16)
        stats = np.zeros((B, 4), np.int32)
        held = [_byte_ptr(j) for j in jpegs]
        ptrs = (C.c_void_p * B)(*[h[0] for h in held])
        sizes = (C.c_size_t * B)(*[len(j) for j in jpegs])
        rc = self._lib.frp_jpeg_selfsync_coefficients(self._h, ptrs, sizes, B, int(subseq_bytes), _ptr(coef), coef.size, _ptr(stats))
        del held
        if rc != 0:
            e = FrpError(rc, (self._lib.frp_last_error(self._h) or b"").decode("utf-8", "replace"))
            e.stats = stats
            raise e
        return coef, stats

    def graph_replays(self) -> int:
        """diagnostic: detector / embedder passes replayed from a captured hipGraph so far (frp.h: frp_debug_graph_replays)"""
        return int(self._lib.frp_debug_graph_replays(self._h))

    def gallery_exact(self, on: bool = True):
        """keep every row also as float64, as enrolled (frp.h: frp_gallery_exact): the rows behind gallery_distances"""
        self._chk(self._lib.frp_gallery_exact(self._h, 1 if on else 0))

    def gallery_distances(self, q: np.ndarray) -> np.ndarray:
        """Euclidean distances [M, N] (float64) of M queries to the exact rows: face_recognition.face_distance on the device"""
        q = np.asarray(q, dtype=np.float64)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        if q.shape[1] < EMB_DIM:
            q = np.concatenate([q, np.zeros((q.shape[0], EMB_DIM - q.shape[1]))], axis=1)
        q = np.ascontiguousarray(q)
        if q.shape[1] != EMB_DIM:
            raise ValueError("queries must have at most 512 values")
        for _ in range(8):
            n = self.gallery_size()
            out = np.empty((q.shape[0], n), np.float64)
            rc = self._lib.frp_gallery_distances(self._h, _ptr(q), q.shape[0], _ptr(out), n)
            if rc == 0:
                return out
            if self.gallery_size() == n:
                break
        self._chk(rc)
        return out

    def gallery_get_exact(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.gallery_size() - first if n is None else n
        out = np.empty((n, EMB_DIM), dtype=np.float64)
        self._chk(self._lib.frp_gallery_get_exact(self._h, _ptr(out), first, n))
        return out

    def gallery_cluster(self, order, *, min_cos: Optional[float] = None, max_dist: Optional[float] = None, tile: int = 0):
        """The greedy sweep of cluster_faces on the device (frp.h: frp_gallery_cluster) over the gallery rows `order`, one per
        position -> (seed_pos [n] int32: the position of the seed that took each position, the number of clusters).  Exactly one
        bound: min_cos - member iff the seed's frp_match_scores entry >= min_cos in float32 (unit fp16 rows); max_dist - member
        iff its frp_gallery_distances entry <= max_dist in float64 (FRP_CLUSTER_EXACT: the exact rows)."""
        if (min_cos is None) == (max_dist is None):
            raise ValueError("gallery_cluster: exactly one of min_cos and max_dist")
        order = np.ascontiguousarray(np.asarray(order, dtype=np.int64).reshape(-1))
        if order.size and (order.min() < -(1 << 31) or order.max() >= (1 << 31)):
            raise FrpError(-1, "gallery_cluster: a row does not fit 32 bits")
        order = order.astype(np.int32)
        seed_pos = np.full(order.size, -1, np.int32)
        n_clusters = C.c_int32(0)
        self._chk(self._lib.frp_gallery_cluster(self._h, _ptr(order), order.size, 0.0 if min_cos is None else float(min_cos),
                                                0.0 if max_dist is None else float(max_dist), int(tile),
                                                CLUSTER_EXACT if min_cos is None else 0, _ptr(seed_pos), C.byref(n_clusters)))
        return seed_pos, int(n_clusters.value)

    def gallery_remove_row(self, row: int):
        self._chk(self._lib.frp_gallery_remove_row(self._h, row))

    def gallery_size(self) -> int:
        return int(self._lib.frp_gallery_size(self._h))

    def gallery_get(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.gallery_size() - first if n is None else n
        out = np.empty((n, EMB_DIM), dtype=np.float16)
        self._chk(self._lib.frp_gallery_get(self._h, _ptr(out), first, n))
        return out

    # -- gallery groups (frp.h: frp_gallery_set_groups): one uint32 mask per row, bit g = member of group g
    @staticmethod
    def _masks(groups, n: int) -> np.ndarray:
        """n uint32 masks from one int (the same for all) or a sequence of n"""
        g = np.asarray(groups, dtype=np.uint32)
        g = np.full(n, g, np.uint32) if g.ndim == 0 else np.ascontiguousarray(g).reshape(-1)
        if g.shape[0] != n:
            raise ValueError(f"{n} masks expected, got {g.shape[0]}")
        return g

    def gallery_set_groups(self, groups, first: int = 0):
        """masks of the rows [first, first + len(groups)); rows that arrive without one have GROUPS_ALL"""
        g = np.ascontiguousarray(np.asarray(groups, dtype=np.uint32)).reshape(-1)
        self._chk(self._lib.frp_gallery_set_groups(self._h, _ptr(g), int(first), g.shape[0]))

    def gallery_get_groups(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.gallery_size() - first if n is None else n
        out = np.empty((max(n, 0),), np.uint32)
        self._chk(self._lib.frp_gallery_get_groups(self._h, _ptr(out), int(first), int(n)))
        return out

    def set_frame_groups(self, masks):
        """one mask per frame for the passes that run with FLAG_GROUPS from now on: the faces of frame b are matched against the
        gallery rows masks[b] permits (row mask & frame mask != 0)"""
        m = np.ascontiguousarray(np.asarray(masks, dtype=np.uint32)).reshape(-1)
        self._chk(self._lib.frp_set_frame_groups(self._h, _ptr(m), m.shape[0]))

    # -- face tracks (include/frp.h: frp_track_config; the semantics: tracks.TrackModel)
    def track_config(self, max_streams: int, iou_min: float = 0.3, refresh: int = 8, max_missed: int = 2):
        """tracking for the passes that run with FLAG_TRACK from now on: allocates the per-stream tables, clears every track, marks the
        next pass stale; max_streams = 0 releases everything.  (0.3 / 8 / 2 are ordinary defaults, not measured optima.)"""
        self._chk(self._lib.frp_track_config(self._h, int(max_streams), float(iou_min), int(refresh), int(max_missed)))

    def set_frame_streams(self, streams):
        """the stream of every frame, in [-1, max_streams), for the passes that run with FLAG_TRACK from now on (-1: the frame is not
        tracked: every face embedded, track_id -1)"""
        s = np.ascontiguousarray(np.asarray(streams, dtype=np.int32)).reshape(-1)
        self._chk(self._lib.frp_set_frame_streams(self._h, _ptr(s), s.shape[0]))

    def track_reset(self, stream: int = -1):
        """forget the tracks of one stream (a camera reconnect), -1: of all"""
        self._chk(self._lib.frp_track_reset(self._h, int(stream)))

    def fetch_tracks(self) -> dict:
        """track_id, reused, age [B, K] of the last pass that ran with FLAG_TRACK (slots without a face: -1 / 0 / 0)"""
        B, K = self._track_pass
        o = dict(track_id=np.full((B, K), -1, np.int32), reused=np.zeros((B, K), np.int32), age=np.zeros((B, K), np.int32))
        self._chk(self._lib.frp_fetch_tracks(self._h, B, K, _ptr(o["track_id"]), _ptr(o["reused"]), _ptr(o["age"])))
        return o

    def track_stats(self) -> Tuple[int, int]:
        """(faces embedded, faces reused) by the tracked passes since track_config"""
        e, r = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.frp_track_stats(self._h, C.byref(e), C.byref(r)))
        return int(e.value), int(r.value)

    def track_step(self, streams, boxes, counts, K: int, emb, idx, cos) -> dict:
        """the tracker's launches alone on host detections (frp.h: frp_debug_track_step; tracks.TrackModel.step's arguments and
        return value): needs no weights, advances the handle's track state"""
        streams = np.ascontiguousarray(np.asarray(streams, np.int32)).reshape(-1)
        B, K = streams.shape[0], int(K)
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(B, K, 4)
        counts = np.ascontiguousarray(counts, np.int32).reshape(B)
        emb = np.ascontiguousarray(emb, np.float32).reshape(B, K, EMB_DIM)
        idx = np.ascontiguousarray(idx, np.int32).reshape(B, K)
        cos = np.ascontiguousarray(cos, np.float32).reshape(B, K)
        o = dict(track_id=np.zeros((B, K), np.int32), reused=np.zeros((B, K), np.int32), age=np.zeros((B, K), np.int32),
                 face_slot=np.zeros((B * K,), np.int32), emb=np.zeros((B, K, EMB_DIM), np.float32), idx=np.zeros((B, K), np.int32),
                 cos=np.zeros((B, K), np.float32))
        n = C.c_int32(0)
        self._chk(self._lib.frp_debug_track_step(self._h, _ptr(streams), _ptr(boxes), _ptr(counts), B, K, _ptr(emb), _ptr(idx), _ptr(cos),
                                                 _ptr(o["track_id"]), _ptr(o["reused"]), _ptr(o["age"]), _ptr(o["face_slot"]), C.byref(n),
                                                 _ptr(o["emb"]), _ptr(o["idx"]), _ptr(o["cos"])))
        o["n_embed"] = int(n.value)
        self._track_pass = (B, K)
        return o

    # -- hot path
    @staticmethod
    def _frames(frames: np.ndarray) -> Tuple[np.ndarray, int, int, int, int]:
        if frames.ndim == 3:
            frames = frames[None]
        if frames.ndim != 4 or frames.shape[3] != 3 or frames.dtype != np.uint8:
            raise ValueError("frames must be uint8 [B,H,W,3]")
        frames = np.ascontiguousarray(frames)
        B, H, W, _ = frames.shape
        return frames, B, H, W, W * 3

    @staticmethod
    def _alloc(B, K):
        """zeroed result arrays of a pass over B frames with up to K faces each"""
        return dict(boxes=np.zeros((B, K, 4), np.float32), kps=np.zeros((B, K, 5, 2), np.float32),
                    scores=np.zeros((B, K), np.float32), counts=np.zeros((B,), np.int32),
                    emb=np.zeros((B, K, EMB_DIM), np.float32), match_idx=np.full((B, K), -1, np.int32),
                    match_cos=np.full((B, K), -1.0, np.float32))

    @classmethod
    def _alloc_det(cls, B, K):
        """... of a detector-only call: the same arrays and the anchor index of every detection"""
        return dict(cls._alloc(B, K), anchor_idx=np.full((B, K), -1, np.int32))

    def process_frames(self, frames: np.ndarray, max_faces: int = 10, det_thresh: float = 0.5, nms_iou: float = 0.4,
                       flags: int = 0) -> dict:
        frames, B, H, W, rs = self._frames(frames)
        o = self._alloc(B, max_faces)
        self._chk(self._lib.frp_process_frames(self._h, _ptr(frames), B, H, W, rs, max_faces, det_thresh, nms_iou, flags,
                                               _ptr(o["boxes"]), _ptr(o["kps"]), _ptr(o["scores"]), _ptr(o["counts"]),
                                               _ptr(o["emb"]), _ptr(o["match_idx"]), _ptr(o["match_cos"])))
        self._began(B, max_faces, heads=True, flags=flags)
        return o

    def upload_frames(self, frames: np.ndarray):
        frames, B, H, W, rs = self._frames(frames)
        self._chk(self._lib.frp_upload_frames(self._h, _ptr(frames), B, H, W, rs))
        self._resident = (B, H, W)

    def host_frames(self, B: int, H: int, W: int) -> np.ndarray:
        """page-locked u8 [B,H,W,3] array owned by the engine (freed with it): frames written here can be
        copied to the device while the previous batch is being processed"""
        n = B * H * W * 3
        p = self._lib.frp_host_alloc(self._h, n)
        if not p:
            raise FrpError(-6, (self._lib.frp_last_error(self._h) or b"frp_host_alloc failed").decode("utf-8", "replace"))      # FRP_ERR_OOM
        buf = (C.c_uint8 * n).from_address(p)
        return np.frombuffer(buf, dtype=np.uint8).reshape(B, H, W, 3)

    def upload_frames_async(self, frames: np.ndarray):
        """stage the NEXT batch (copy stream); becomes resident at swap_frames()"""
        frames, B, H, W, rs = self._frames(frames)
        self._chk(self._lib.frp_upload_frames_async(self._h, _ptr(frames), B, H, W, rs))
        self._staged = (B, H, W)

    def swap_frames(self):
        self._chk(self._lib.frp_swap_frames(self._h))
        self._resident = self._staged

    def _yuv(self, fn, batch):
        """one frp_upload_yuv* call for a yuv.YuvBatch (anything with its layout / matrix / hw / plane_table())
        -> ((B, H, W), what keeps the host planes alive)"""
        device, y_pitch, c_pitch, table, keep = batch.plane_table()
        B = len(table)
        d = FrpYuvDesc(C.sizeof(FrpYuvDesc), YUV_LAYOUTS.get(batch.layout, -1), YUV_MATRICES.get(batch.matrix, -1), YUV_DEVICE if device else 0,
                       int(batch.hw[1]), int(batch.hw[0]), int(y_pitch), int(c_pitch))
        ptrs = (C.c_void_p * (3 * B))(*[a or None for frame in table for a in frame])
        self._chk(fn(self._h, C.byref(d), ptrs, B))
        return (B, int(batch.hw[0]), int(batch.hw[1])), keep

    def upload_yuv(self, batch):
        """a yuv.YuvBatch of decoder surfaces (NV12 / NV21 / I420 / YV12, host arrays or device addresses) -> resident BGR frames,
        converted on the device (frp.h: frp_upload_yuv); blocking, as upload_frames(): the surfaces have been read on return"""
        self._resident, _ = self._yuv(self._lib.frp_upload_yuv, batch)

    def upload_yuv_async(self, batch):
        """the same into the staging frame buffer, on the copy stream: follow with swap_frames() as after upload_frames_async().
        The call only QUEUES the copies and the kernel: the surfaces, host arrays and device memory alike, must stay untouched
        until swap_frames() AND a call that waits for the pass (fetch_results, synchronize) have returned (frp.h).  The engine
        holds a reference to the host arrays of the last two staged batches - the library has finished with a batch when the
        second call after it returns - so that dropping a batch does not free memory under a running copy; it cannot keep a
        caller from REWRITING them."""
        self._staged, keep = self._yuv(self._lib.frp_upload_yuv_async, batch)
        self._yuv_keep = (self._yuv_keep + (keep,))[-2:]

    def get_frames(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """the resident BGR frames as they lie -> u8 [n, H, W, 3] (frp.h: frp_get_frames; parity tests, snapshots)"""
        B, H, W = self._resident
        n = B - first if n is None else n
        out = np.empty((max(n, 0), H, W, 3), np.uint8)
        self._chk(self._lib.frp_get_frames(self._h, _ptr(out), out.nbytes, first, n))
        return out

    def process_resident(self, max_faces: int = 10, det_thresh: float = 0.5, nms_iou: float = 0.4, flags: int = 0):
        self._chk(self._lib.frp_process_resident(self._h, max_faces, det_thresh, nms_iou, flags))
        self._began(self._resident[0], max_faces, flags=flags)

    def synchronize(self):
        self._chk(self._lib.frp_synchronize(self._h))

    def fetch_results(self) -> dict:
        B, K = self._pass
        o = self._alloc(B, K)
        self._chk(self._lib.frp_fetch_results(self._h, B, K, _ptr(o["boxes"]), _ptr(o["kps"]), _ptr(o["scores"]), _ptr(o["counts"]),
                                              _ptr(o["emb"]), _ptr(o["match_idx"]), _ptr(o["match_cos"])))
        return o

    # -- stages
    def detect(self, frames: np.ndarray, max_faces: int = 10, det_thresh: float = 0.5, nms_iou: float = 0.4, flags: int = 0):
        frames, B, H, W, rs = self._frames(frames)
        o = self._alloc_det(B, max_faces)
        self._chk(self._lib.frp_detect(self._h, _ptr(frames), B, H, W, rs, max_faces, det_thresh, nms_iou, flags,
                                       _ptr(o["boxes"]), _ptr(o["kps"]), _ptr(o["scores"]), _ptr(o["counts"]), _ptr(o["anchor_idx"])))
        self._began(B, heads=True)
        return o

    def detect_resident(self, det_hw, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        """detect on the resident frames resized to det_hw (pyramid scale); coordinates of the resized image"""
        B = self._resident[0]
        o = self._alloc_det(B, max_faces)
        self._chk(self._lib.frp_detect_resident(self._h, B, det_hw[0], det_hw[1], max_faces, det_thresh, nms_iou, flags,
                                                _ptr(o["boxes"]), _ptr(o["kps"]), _ptr(o["scores"]), _ptr(o["counts"]), _ptr(o["anchor_idx"])))
        self._began(B, heads=True)
        return {k: o[k] for k in ("boxes", "kps", "scores", "counts", "anchor_idx")}

    def det_source(self) -> np.ndarray:
        """the u8 frames the detector last read (resident frames or their pyramid resize)"""
        hs, ws = C.c_int32(), C.c_int32()
        self._chk(self._lib.frp_get_det_source(self._h, None, 0, C.byref(hs), C.byref(ws)))
        out = np.empty((self._resident[0], hs.value, ws.value, 3), np.uint8)
        self._chk(self._lib.frp_get_det_source(self._h, _ptr(out), out.nbytes, C.byref(hs), C.byref(ws)))
        return out

    def finish_faces(self, boxes, kps, scores, counts, max_faces, flags=0):
        """align (from the full-resolution resident frames) + embed + match for caller-supplied landmarks"""
        B = self._resident[0]
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(B, max_faces, 4)
        kps = np.ascontiguousarray(kps, np.float32).reshape(B, max_faces, 5, 2)
        scores = np.ascontiguousarray(scores, np.float32).reshape(B, max_faces)
        counts = np.ascontiguousarray(counts, np.int32).reshape(B)
        o = self._alloc(B, max_faces)
        self._chk(self._lib.frp_finish_faces(self._h, B, _ptr(boxes), _ptr(kps), _ptr(scores), _ptr(counts), max_faces, flags,
                                             _ptr(o["emb"]), _ptr(o["match_idx"]), _ptr(o["match_cos"])))
        o.update(boxes=boxes, kps=kps, scores=scores, counts=counts)
        self._began(B, max_faces, flags=flags)
        return o

    def process_pyramid_resident(self, det_hws, per_scale: int = 64, max_faces: int = 10, det_thresh: float = 0.5, nms_iou: float = 0.4,
                                 flags: int = 0):
        """the pyramid as ONE device pass on the resident frames (frp.h: frp_process_pyramid): detect at every size of det_hws
        [(h, w), ...], merge + NMS across the scales on the device (bit for bit pyramid.merge_scales), align / embed / match from the
        full-resolution frames.  Asynchronous like process_resident: fetch_results() waits for it and returns frame-pixel results."""
        hw = np.ascontiguousarray(det_hws, dtype=np.int32).reshape(-1, 2)
        self._chk(self._lib.frp_process_pyramid(self._h, hw.shape[0], _ptr(hw), per_scale, max_faces, det_thresh, nms_iou, flags))
        self._began(self._resident[0], max_faces)

    def pyramid_merge(self, det_hws, frame_hw, boxes, kps, scores, counts, max_faces: int, nms_iou: float = 0.4):
        """the cross-scale merge launch alone (frp.h: frp_debug_pyramid_merge) on host detections, scale-major: boxes [S, B, P, 4],
        kps [S, B, P, 5, 2], scores [S, B, P], counts [S, B] in the coordinates of each scale's det_hws[s] = (h, w) image
        -> boxes [B, K, 4], kps [B, K, 5, 2], scores [B, K], counts [B] in frame pixels (pyramid.merge_scales' return value)"""
        hw = np.ascontiguousarray(det_hws, dtype=np.int32).reshape(-1, 2)
        scores = np.ascontiguousarray(scores, np.float32)
        if scores.ndim != 3 or scores.shape[0] != hw.shape[0]:
            raise ValueError("scores must be [n_scales, B, per_scale]")
        S, B, P = scores.shape
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(S, B, P, 4)
        kps = np.ascontiguousarray(kps, np.float32).reshape(S, B, P, 10)
        counts = np.ascontiguousarray(counts, np.int32).reshape(S, B)
        K = int(max_faces)
        ob, ok = np.zeros((B, max(K, 0), 4), np.float32), np.zeros((B, max(K, 0), 5, 2), np.float32)
        osc, oc = np.zeros((B, max(K, 0)), np.float32), np.zeros((B,), np.int32)
        self._chk(self._lib.frp_debug_pyramid_merge(self._h, S, _ptr(hw), B, P, int(frame_hw[0]), int(frame_hw[1]), _ptr(boxes), _ptr(kps),
                                                    _ptr(scores), _ptr(counts), K, nms_iou, _ptr(ob), _ptr(ok), _ptr(osc), _ptr(oc)))
        return ob, ok, osc, oc

    def debug_fc_l2norm(self, x16, w16, bias, n: int, mode="host", flags: int = 0):
        """the embedder's tail alone (frp.h: frp_debug_fc_l2norm): x16 [cap, K] fp16, w16 [D, K] fp16, bias [D] fp32, n <= cap rows exist.
        mode "host" / "device" / "none" / an int s >= 2 (a forced split factor); flags: the tile-class bits 17 / 18 of conv2d
        -> (emb [cap, D] float32, emb16 [cap, D] float16, n_cu, the factor the host's rule gives n rows); rows at or beyond n of both
        outputs hold the 0xFF fill"""
        x16 = np.ascontiguousarray(x16, np.float16)
        w16 = np.ascontiguousarray(w16, np.float16)
        bias = np.ascontiguousarray(bias, np.float32)
        if x16.ndim != 2 or w16.ndim != 2 or x16.shape[1] != w16.shape[1] or bias.shape != (w16.shape[0],):
            raise ValueError("x16 [cap, K], w16 [D, K], bias [D]")
        cap, K = x16.shape
        D = w16.shape[0]
        m = {"host": 0, "device": -1, "none": 1}.get(mode, mode)
        emb, emb16 = np.zeros((cap, D), np.float32), np.zeros((cap, D), np.float16)
        ncu, factor = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.frp_debug_fc_l2norm(self._h, _ptr(x16), _ptr(w16), _ptr(bias), cap, int(n), K, D, int(m), int(flags), _ptr(emb),
                                                _ptr(emb16), C.byref(ncu), C.byref(factor)))
        return emb, emb16, int(ncu.value), int(factor.value)

    def process_frames_pyramid(self, frames, scales=(1.0, 0.5, 0.25), max_faces=10, det_thresh=0.5, nms_iou=0.4,
                               per_scale=64, flags=0, on_device: bool = False):
        """BASELINE config 4: detect at several scales of every frame, merge + NMS across scales
        (pyramid.merge_scales), then align / embed / match from the full-resolution frames.
        on_device: the whole pass in one call (process_pyramid_resident: the merge on the device, the face count never visits the
        host mid-pass, FLAG_WITHIN honoured) instead of one blocking call per scale and the merge here; the same bits."""
        from . import pyramid
        frames, B, H, W, _ = self._frames(frames)
        with self._seq:
            self.upload_frames(frames)
            if on_device:
                self.process_pyramid_resident([pyramid.scaled_size(H, W, s) for s in scales], per_scale=per_scale, max_faces=max_faces,
                                              det_thresh=det_thresh, nms_iou=nms_iou, flags=flags)
                return self.fetch_results()
            per = []
            for s in scales:
                hw = pyramid.scaled_size(H, W, s)
                per.append((hw, self.detect_resident(hw, max_faces=per_scale, det_thresh=det_thresh, nms_iou=nms_iou,
                                                     flags=flags & ~FLAG_FORCED_K)))
            boxes, kps, scores, counts = pyramid.merge_scales(per, (H, W), max_faces, nms_iou)
            return self.finish_faces(boxes, kps, scores, counts, max_faces, flags & (FLAG_RGB | FLAG_NO_MATCH))

    def head_maps(self):
        """fp16 head maps [B,H_l,W_l,32] of the last detect/process call, strides 8/16/32."""
        outs = []
        for lv in range(3):
            hl, wl = C.c_int32(), C.c_int32()
            self._chk(self._lib.frp_get_head_map(self._h, lv, None, 0, C.byref(hl), C.byref(wl)))
            a = np.empty((self._det_batch, hl.value, wl.value, 32), dtype=np.float16)
            self._chk(self._lib.frp_get_head_map(self._h, lv, _ptr(a), a.nbytes, C.byref(hl), C.byref(wl)))
            outs.append(a)
        return outs

    def det_prefix(self, n_ops: int) -> np.ndarray:
        """diagnostic: the detector on the RESIDENT frames up to and including op n_ops - 1; that op's output [B,h,w,c] fp16.
        By default both stems run as one kernel and the stem1 map (op 0) never reaches memory: n_ops == 1 raises FrpError
        unless FRP_NO_FUSED_STEM12 is set (stem1 and stem2 as two launches); n_ops == 2 is the fused kernel's output."""
        th, tw, tc = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._lib.frp_debug_det_prefix(self._h, n_ops, None, 0, C.byref(th), C.byref(tw), C.byref(tc)))
        a = np.empty((self._resident[0], th.value, tw.value, tc.value), dtype=np.float16)
        self._chk(self._lib.frp_debug_det_prefix(self._h, n_ops, _ptr(a), a.nbytes, C.byref(th), C.byref(tw), C.byref(tc)))
        return a

    def det_hashes(self, enable: bool = True, fetch: bool = True):
        """diagnostic: per-op output hashes of the last detector pass (uint64[64]); enable keeps them on for later passes"""
        out = np.zeros(64, np.uint64) if fetch else None
        self._chk(self._lib.frp_debug_det_hashes(self._h, 1 if enable else 0, _ptr(out) if fetch else None))
        return out

    def decode_heads(self, heads, canvas_hw, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
        hs = [np.ascontiguousarray(x, dtype=np.float16) for x in heads]
        B = hs[0].shape[0]
        o = self._alloc_det(B, max_faces)
        self._chk(self._lib.frp_decode_heads(self._h, _ptr(hs[0]), _ptr(hs[1]), _ptr(hs[2]), B, canvas_hw[0], canvas_hw[1],
                                             max_faces, det_thresh, nms_iou, flags, _ptr(o["boxes"]), _ptr(o["kps"]),
                                             _ptr(o["scores"]), _ptr(o["counts"]), _ptr(o["anchor_idx"])))
        return o

    def align(self, frame: np.ndarray, kps: np.ndarray, flags: int = 0) -> np.ndarray:
        frames, _, H, W, rs = self._frames(frame)
        k = np.ascontiguousarray(kps, dtype=np.float32).reshape(-1, 10)
        out = np.empty((k.shape[0], CHIP, CHIP, 8), dtype=np.float16)
        self._chk(self._lib.frp_align(self._h, _ptr(frames), H, W, rs, _ptr(k), k.shape[0], flags, _ptr(out)))
        return out

    def align_resident(self, kps: np.ndarray, counts, flags: int = 0, device_count: bool = False) -> np.ndarray:
        """diagnostic: the pipeline's own align launch on the RESIDENT frames for landmarks kps [B,K,5,2] and counts [B]; device_count:
        launched for the capacity with the count in device memory.  -> all B*K chips [B*K,112,112,8] fp16: the first sum(counts),
        frame-major, are the faces; a chip the launch did not write holds 0xFFFF."""
        B = self._resident[0]
        k = np.ascontiguousarray(kps, dtype=np.float32)
        K = k.size // (B * 10)
        k = k.reshape(B, K, 10)
        c = np.ascontiguousarray(counts, np.int32).reshape(B)
        out = np.empty((B * K, CHIP, CHIP, 8), dtype=np.float16)
        self._chk(self._lib.frp_debug_align_resident(self._h, _ptr(k), _ptr(c), K, flags, 1 if device_count else 0, _ptr(out), out.nbytes))
        return out

    def embed_aligned(self, chips_bgr_u8: np.ndarray) -> np.ndarray:
        c = np.ascontiguousarray(chips_bgr_u8, dtype=np.uint8).reshape(-1, CHIP, CHIP, 3)
        out = np.empty((c.shape[0], EMB_DIM), dtype=np.float32)
        self._chk(self._lib.frp_embed_aligned(self._h, _ptr(c), c.shape[0], _ptr(out)))
        return out

    def embed_faces(self, frame: np.ndarray, kps: np.ndarray, flags: int = 0) -> np.ndarray:
        frames, _, H, W, rs = self._frames(frame)
        k = np.ascontiguousarray(kps, dtype=np.float32).reshape(-1, 10)
        out = np.empty((k.shape[0], EMB_DIM), dtype=np.float32)
        self._chk(self._lib.frp_embed_faces(self._h, _ptr(frames), H, W, rs, _ptr(k), k.shape[0], flags, _ptr(out)))
        return out

    def match(self, q: np.ndarray, topk: int = 1, groups=None):
        """-> (row idx, cosine): [M] for topk == 1, else [M, topk] ordered by (cosine desc, row asc);
        columns beyond the gallery size hold -1 / -2.0.  groups (one mask per query, or one int for all): over the rows each query's
        mask permits only (frp.h: frp_match_groups); entries beyond the permitted rows hold -1 / -2.0"""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, EMB_DIM)
        shape = (q.shape[0],) if topk == 1 else (q.shape[0], topk)
        idx = np.empty(shape, np.int32)
        cos = np.empty(shape, np.float32)
        if groups is None:
            self._chk(self._lib.frp_match(self._h, _ptr(q), q.shape[0], int(topk), _ptr(idx), _ptr(cos)))
        else:
            g = self._masks(groups, q.shape[0])
            self._chk(self._lib.frp_match_groups(self._h, _ptr(q), q.shape[0], _ptr(g), int(topk), _ptr(idx), _ptr(cos)))
        return idx, cos

    def match_within(self, q: np.ndarray, min_cos: float, cap: int = 64, groups=None):
        """radius match -> (idx [M, cap], cos [M, cap], n_hits [M]): every gallery row whose cosine is >= min_cos, ordered by
        (cosine desc, row asc); n_hits is the true count and may exceed cap (the list then holds the first cap of that order);
        entries beyond min(n_hits, cap) hold -1 / -2.0.  groups: as in match() - lists and counts over the permitted rows only"""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, EMB_DIM)
        M, cap = q.shape[0], int(cap)
        ok = 1 <= cap <= 64                     # (the library refuses the others: size the buffers for something harmless)
        idx = np.empty((M, cap if ok else 1), np.int32)
        cos = np.empty((M, cap if ok else 1), np.float32)
        n_hits = np.empty((M,), np.int32)
        if groups is None:
            self._chk(self._lib.frp_match_within(self._h, _ptr(q), M, float(min_cos), cap, _ptr(idx), _ptr(cos), _ptr(n_hits)))
        else:
            g = self._masks(groups, M)
            self._chk(self._lib.frp_match_within_groups(self._h, _ptr(q), M, _ptr(g), float(min_cos), cap, _ptr(idx), _ptr(cos), _ptr(n_hits)))
        return idx, cos, n_hits

    def match_f16(self, q16: np.ndarray, n_device: Optional[int] = None, scores: bool = False):
        """diagnostic: the matcher on queries given as fp16 bits [M, 512], copied as they are (no normalisation) -> (idx [M], cos [M])
        or, with scores, (idx, cos, S [M, N]: the per-tile kernel's score matrix).  n_device: launched for the capacity M with that
        count in device memory (frp.h: frp_debug_match_f16 - refused where the launch has no such form).  The device buffers hold
        0xFF bytes before the launch: an entry no kernel wrote comes back as idx -1 / cos bits 0xFFFFFFFF."""
        q = np.ascontiguousarray(q16)
        if q.dtype != np.float16:
            raise TypeError("match_f16 takes float16 rows: the bits are the operands")
        q = q.reshape(-1, EMB_DIM)
        M = q.shape[0]
        idx = np.empty((M,), np.int32)
        cos = np.empty((M,), np.float32)
        n = self.gallery_size()
        S = np.empty((M, n), np.float32) if scores else None
        self._chk(self._lib.frp_debug_match_f16(self._h, _ptr(q), M, -1 if n_device is None else int(n_device), _ptr(idx), _ptr(cos),
                                                _ptr(S) if scores else None, n))
        return (idx, cos, S) if scores else (idx, cos)

    def set_within(self, min_cos: float, cap: int = 64):
        """bound and list size of the passes that run with FLAG_WITHIN from now on"""
        self._chk(self._lib.frp_set_within(self._h, float(min_cos), int(cap)))
        self._within_cap = int(cap)

    def fetch_within(self):
        """hit lists of the last pass that ran with FLAG_WITHIN (process_frames / process_resident / process_pyramid_resident / finish_faces)
        -> (idx [B, K, cap], cos [B, K, cap], n_hits [B, K]); slots without a face have n_hits 0"""
        B, K = self._pass
        cap = self._within_cap
        idx = np.empty((B, K, cap), np.int32)
        cos = np.empty((B, K, cap), np.float32)
        n_hits = np.empty((B, K), np.int32)
        self._chk(self._lib.frp_fetch_within(self._h, B, K, cap, _ptr(idx), _ptr(cos), _ptr(n_hits)))
        return idx, cos, n_hits

    def face_quality(self, rects, rgb: bool = False) -> np.ndarray:
        """blur / lighting sums of rectangles (frame, top, right, bottom, left) of the RESIDENT frames, as uploaded (rgb: their
        channel order) -> int64 [n, 4]: S1 = sum g, S2 = sum g^2, L1 = sum lap, L2 = sum lap^2 over each crop (frp.h: frp_face_quality;
        face_service.FaceService.quality_from_sums turns them into the reference's scores).  The last pass's results stay fetchable."""
        r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 5)
        sums = np.zeros((r.shape[0], 4), np.int64)
        self._chk(self._lib.frp_face_quality(self._h, _ptr(r), r.shape[0], FLAG_RGB if rgb else 0, _ptr(sums)))
        return sums

    def encode_jpeg(self, rects, quality: int = 95, subsampling: str = "4:2:0", restart_mcus: int = 0, rgb: bool = False, optimize: bool = False):
        """baseline JPEG files of rectangles (frame, top, right, bottom, left) of the RESIDENT frames, as uploaded (rgb: their channel
        order) -> list[bytes], one complete file per rectangle, byte for byte what libjpeg (PIL, cv2.imencode) writes for those pixels
        (frp.h: frp_encode_jpeg).  optimize: Huffman tables of every image's own (FLAG_JPEG_OPTIMIZE) - PIL's save(optimize=True),
        smaller files, one more wait inside the call.  The first call guesses the size; a second one with the reported size follows
        when it was too small."""
        flags = (FLAG_RGB if rgb else 0) | (FLAG_JPEG_OPTIMIZE if optimize else 0)
        r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 5)
        n = r.shape[0]
        offsets = np.zeros(n + 1, np.int64)
        px = int(np.clip((r[:, 3] - r[:, 1]).astype(np.int64), 0, None) @ np.clip((r[:, 2] - r[:, 4]).astype(np.int64), 0, None)) if n else 0
        cap = 1024 * n + px + 4096
        for _ in range(2):
            out = np.empty(cap, np.uint8)
            rc = self._lib.frp_encode_jpeg(self._h, _ptr(r), n, int(quality), _subsampling_code(subsampling), int(restart_mcus),
                                           flags, _ptr(out), cap, _ptr(offsets))
            if rc == 0 or offsets[n] <= cap:
                break
            cap = int(offsets[n])
        self._chk(rc)
        return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(n)]

    @staticmethod
    def _enhance_args(rects, sizes, radius, percent, threshold, sharpen):
        r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 5)
        sz = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 2)
        if sz.shape[0] != r.shape[0]:
            raise ValueError(f"{r.shape[0]} rectangles, {sz.shape[0]} output sizes")
        return r, sz, FrpEnhanceParams(float(radius), int(percent), int(threshold), 1 if sharpen else 0)

    def enhance_pixels(self, rects, sizes, radius: float = 1.0, percent: int = 120, threshold: int = 3, sharpen: bool = True, rgb: bool = False):
        """rectangles (frame, top, right, bottom, left) of the RESIDENT frames, each resized to its (out_w, out_h) of `sizes` with
        Pillow's BICUBIC and sharpened with UnsharpMask(radius, percent, threshold), byte for byte (frp.h: frp_enhance_pixels) ->
        list of [out_h, out_w, 3] u8 arrays in the frames' channel order.  An axis that keeps its size is not resampled;
        sharpen=False skips the mask.  The last pass's results stay fetchable."""
        r, sz, prm = self._enhance_args(rects, sizes, radius, percent, threshold, sharpen)
        n = r.shape[0]
        cap = int(3 * (np.clip(sz[:, 0].astype(np.int64), 0, None) @ np.clip(sz[:, 1].astype(np.int64), 0, None))) if n else 0
        out = np.empty(max(cap, 1), np.uint8)
        offsets = np.zeros(n + 1, np.int64)
        self._chk(self._lib.frp_enhance_pixels(self._h, _ptr(r), _ptr(sz), n, C.byref(prm), FLAG_RGB if rgb else 0, _ptr(out), cap, _ptr(offsets)))
        return [out[offsets[i]:offsets[i + 1]].reshape(int(sz[i, 1]), int(sz[i, 0]), 3).copy() for i in range(n)]

    def encode_jpeg_enhanced(self, rects, sizes, radius: float = 1.0, percent: int = 120, threshold: int = 3, sharpen: bool = True,
                             quality: int = 85, subsampling: str = "4:2:0", restart_mcus: int = 0, rgb: bool = False, optimize: bool = False):
        """the images of enhance_pixels as baseline JPEG files -> list[bytes], byte for byte Pillow's save(quality=quality) of the
        enhanced image - with optimize its save(quality=quality, optimize=True), the file the reference writes (frp.h:
        frp_encode_jpeg_enhanced): enhancer and encoder run back to back on the device.  The first call guesses the size; a second
        one with the reported size follows when it was too small."""
        flags = (FLAG_RGB if rgb else 0) | (FLAG_JPEG_OPTIMIZE if optimize else 0)
        r, sz, prm = self._enhance_args(rects, sizes, radius, percent, threshold, sharpen)
        n = r.shape[0]
        offsets = np.zeros(n + 1, np.int64)
        px = int(np.clip(sz[:, 0].astype(np.int64), 0, None) @ np.clip(sz[:, 1].astype(np.int64), 0, None)) if n else 0
        cap = 1024 * n + px + 4096
        for _ in range(2):
            out = np.empty(cap, np.uint8)
            rc = self._lib.frp_encode_jpeg_enhanced(self._h, _ptr(r), _ptr(sz), n, C.byref(prm), int(quality), _subsampling_code(subsampling),
                                                    int(restart_mcus), flags, _ptr(out), cap, _ptr(offsets))
            if rc == 0 or offsets[n] <= cap:
                break
            cap = int(offsets[n])
        self._chk(rc)
        return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(n)]

    def encode_jpeg_coefficients(self, rects, quality: int = 95, subsampling: str = "4:2:0", rgb: bool = False) -> np.ndarray:
        """parity: the quantised coefficients of the same rectangles before entropy coding (frp.h: frp_encode_jpeg_coefficients) -
        int16, one image after the other, each in the layout of jpeg_coefficients"""
        r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 5)
        f = {"4:2:0": 16, "4:4:4": 8}.get(subsampling, 8)
        per = 6 if f == 16 else 3
        n = sum(-(-int(b - t) // f) * -(-int(rt - lf) // f) * per * 64 for _, t, rt, b, lf in r.tolist() if b > t and rt > lf)
        coef = np.zeros(n, np.int16)
        self._chk(self._lib.frp_encode_jpeg_coefficients(self._h, _ptr(r), r.shape[0], int(quality), _subsampling_code(subsampling),
                                                         FLAG_RGB if rgb else 0, _ptr(coef), n))
        return coef

    def encode_jpeg_histograms(self, rects, quality: int = 95, subsampling: str = "4:2:0", restart_mcus: int = 0, rgb: bool = False) -> np.ndarray:
        """parity: the symbol counts encode_jpeg(optimize=True) makes its tables from (frp.h: frp_encode_jpeg_histograms) - uint32
        [n, JPEG_HIST_ELEMS]: per image dc [2][16] by magnitude category, then ac [2][256] by run / size symbol; table 1 counts Cb
        and Cr together"""
        r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 5)
        hist = np.zeros((r.shape[0], JPEG_HIST_ELEMS), np.uint32)
        self._chk(self._lib.frp_encode_jpeg_histograms(self._h, _ptr(r), r.shape[0], int(quality), _subsampling_code(subsampling), int(restart_mcus),
                                                       FLAG_RGB if rgb else 0, _ptr(hist), hist.size))
        return hist

    def match_scores(self, q: np.ndarray) -> np.ndarray:
        """all cosines [M, N].  The output is sized from gallery_size(); the library re-checks that size under
        its mutex and refuses (nothing written) if a concurrent update changed it -- then size again and retry."""
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, EMB_DIM)
        for _ in range(8):
            n = self.gallery_size()
            out = np.empty((q.shape[0], n), np.float32)
            rc = self._lib.frp_match_scores(self._h, _ptr(q), q.shape[0], _ptr(out), n)
            if rc == 0:
                return out
            if self.gallery_size() == n:
                break
        self._chk(rc)
        return out

    def conv2d(self, x, w, bias, stride=1, act=0, slope=None, res=None, flags=0):
        x = np.ascontiguousarray(x, dtype=np.float16)
        w = np.ascontiguousarray(w, dtype=np.float16)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        N, H, W, Cin = x.shape
        Cout, k = w.shape[0], w.shape[1]
        pad = k // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        out = np.empty((N, Ho, Wo, Cout), dtype=np.float32 if (flags & 2) else np.float16)
        rh = rw = 0
        if res is not None:
            res = np.ascontiguousarray(res, dtype=np.float16)
            rh, rw = res.shape[1], res.shape[2]
        if slope is not None:
            slope = np.ascontiguousarray(slope, dtype=np.float32)
        self._chk(self._lib.frp_conv2d_nhwc(self._h, _ptr(x), N, H, W, Cin, _ptr(w), Cout, k, stride, _ptr(bias), _ptr(slope),
                                            _ptr(res), rh, rw, act, flags, _ptr(out)))
        return out

    def conv_block64(self, x, w1, bias1, w2, bias2, act1=1, act2=1, slope1=None, slope2=None, flags1=0):
        """out = act2(conv2(act1(conv1(x))) + x), both convs 3x3 stride 1 64 -> 64, in one fused launch (conv3x3_block64.hip)"""
        x = np.ascontiguousarray(x, dtype=np.float16)
        w1 = np.ascontiguousarray(w1, dtype=np.float16)
        w2 = np.ascontiguousarray(w2, dtype=np.float16)
        bias1 = np.ascontiguousarray(bias1, dtype=np.float32)
        bias2 = np.ascontiguousarray(bias2, dtype=np.float32)
        if x.ndim != 4 or x.shape[3] != 64 or w1.shape != (64, 3, 3, 64) or w2.shape != (64, 3, 3, 64):
            raise ValueError("conv_block64: x [N,H,W,64], w1 / w2 [64,3,3,64]")
        if bias1.size != (576 if flags1 & 1 else 64) or bias2.size != 64:
            raise ValueError("conv_block64: bias1 [64] ([9,64] with border classes), bias2 [64]")
        if slope1 is not None:
            slope1 = np.ascontiguousarray(slope1, dtype=np.float32)
        if slope2 is not None:
            slope2 = np.ascontiguousarray(slope2, dtype=np.float32)
        N, H, W, _ = x.shape
        out = np.empty_like(x)
        self._chk(self._lib.frp_conv_block64(self._h, _ptr(x), N, H, W, _ptr(w1), _ptr(bias1), _ptr(slope1), act1, flags1,
                                             _ptr(w2), _ptr(bias2), _ptr(slope2), act2, _ptr(out)))
        return out

    def conv2d_f8(self, x8, w8, wscale, bias, act=0, slope=None, res=None, flags=0, in_scale=1.0, out_scale=1.0,
                  out_fp8=False, copy_fp8=False):
        """3x3 stride-1 conv on E4M3 operands (uint8 codes).  -> fp16 output (or uint8 codes with out_fp8), plus the
        uint8 copy with copy_fp8"""
        x8 = np.ascontiguousarray(x8, dtype=np.uint8)
        w8 = np.ascontiguousarray(w8, dtype=np.uint8)
        N, H, W, Cin = x8.shape
        Cout = w8.shape[0]
        wscale = np.ascontiguousarray(wscale, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        if slope is not None:
            slope = np.ascontiguousarray(slope, dtype=np.float32)
        if res is not None:
            res = np.ascontiguousarray(res, dtype=np.float16)
        out = np.empty((N, H, W, Cout), np.uint8 if out_fp8 else np.float16)
        out2 = np.empty((N, H, W, Cout), np.uint8) if copy_fp8 else None
        self._chk(self._lib.frp_conv2d_f8(self._h, _ptr(x8), N, H, W, Cin, _ptr(w8), Cout, _ptr(wscale), _ptr(bias), _ptr(slope),
                                          _ptr(res), act, flags | (64 if out_fp8 else 0), in_scale, out_scale, _ptr(out), _ptr(out2)))
        return (out, out2) if copy_fp8 else out

    def _lab(self, name: str):
        if not hasattr(self._lib, name):
            raise RuntimeError(f"{name} lives in the lab build only: `make -C face-recognition-platform_amd/csrc lab` and run with "
                               "FRP_LIB=face-recognition-platform_amd/libfrp_lab.so (tools/ do that through tools/_lab.py)")
        return getattr(self._lib, name)

    def conv_bench(self, N, H, W, Cin, Cout, k=3, stride=1, act=0, flags=0, with_res=False, iters=20, stamps=False):
        self._lab("frp_conv_bench")
        ms = C.c_float()
        st = np.zeros((256, 8), np.uint64) if stamps else None
        self._chk(self._lib.frp_conv_bench(self._h, N, H, W, Cin, Cout, k, stride, act, flags, int(with_res), iters, C.byref(ms), _ptr(st)))
        return (float(ms.value), st) if stamps else float(ms.value)

    def mfma_peak(self, waves_per_simd=1, iters=20000) -> float:
        t = C.c_float()
        self._lab("frp_mfma_peak")
        self._chk(self._lib.frp_mfma_peak(self._h, waves_per_simd, iters, C.byref(t)))
        return float(t.value)

    def mfma_lds_peak(self, reads_per_4_mfma: int = 4, iters: int = 5000) -> float:
        """TFLOP/s of the conv k-step's instruction mix alone (8 waves per CU, 64x64 wave tiles, fragments from LDS
        by ds_read_b128, random data, no DMA / barriers / epilogue): the ceiling of that wave layout"""
        return self.mfma_peak(16 * int(reads_per_4_mfma) + 2, iters)

    def kstep_lab(self, variant: int, iters: int = 3000) -> float:
        """TFLOP/s of the conv k-step's inner loop in isolation under schedule `variant` (csrc/kstep_lab.hip)"""
        t = C.c_float()
        self._lab("frp_kstep_lab")
        self._chk(self._lib.frp_kstep_lab(self._h, int(variant), int(iters), C.byref(t)))
        return float(t.value)

    def counters(self) -> dict:
        c = FrpCounters()
        self._chk(self._lib.frp_get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def set_profile(self, on: bool):
        """per-stage HIP-event timing on / off (on: every process call ends in a stream synchronise)"""
        self._chk(self._lib.frp_set_profile(self._h, int(bool(on))))

    def reset_counters(self):
        self._chk(self._lib.frp_reset_counters(self._h))
