"""imageencoder_amd -- MI355X-native (gfx950) implementation of ImageEncoder's block hot path.

The product is the C-ABI library ``lib/libie_hip.so`` (include/ie_hip.h); this module is a thin
ctypes binding over it for tests, the bench and Python callers.  It mirrors the reference's
encoder surface: a quantisation matrix (``MatrixReader``), block size N, ``use_rle``, and frame
encodes that append block records to a bit stream after a settings header
(``ImageEncoder::process``, ImageEncoder.cpp:52-175).

There is no CPU fallback: importing succeeds without the library, but constructing a
:class:`Codec` raises if ``libie_hip.so`` is missing or no HIP device is present.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIBDIR, "libie_hip.so")
HOST_LIB_PATH = os.path.join(LIBDIR, "libie_host.so")

IE_OK, IE_EINVAL, IE_ECAP, IE_EHIP, IE_ENOQUANT, IE_EFORMAT, IE_EDEVICE = 0, -1, -2, -3, -4, -5, -6
MODE_FAST, MODE_EXACT = 0, 1

_lib = None
_host = None


class IEError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ie error {code}: {msg}")
        self.code = code


def load_library(path: str | None = None) -> C.CDLL:
    """Load libie_hip.so (raises if absent: the HIP path is the only path).  IE_LIB overrides
    the path (kernel variants built by tools/variants.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("IE_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise IEError(IE_EHIP, f"{path} not built -- run `make lib` (or __graft_entry__.build())")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (same SONAME as
    # /opt/rocm's).  Loading torch first makes our DT_NEEDED resolve to the copy torch already
    # mapped, so device pointers and streams from torch are valid in this library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, u8p, u16p, u32p, u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)
    L.ie_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.ie_destroy.argtypes = [vp]
    L.ie_last_error.argtypes = [vp]
    L.ie_last_error.restype = C.c_char_p
    L.ie_set_stream.argtypes = [vp, vp]
    L.ie_sync.argtypes = [vp]
    L.ie_set_quant.argtypes = [vp, u16p, C.c_int]
    L.ie_cos_table.argtypes = [vp, vp]
    L.ie_last_stage_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.ie_set_stage_timing.argtypes = [vp, C.c_int]
    L.ie_stream_bound.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64]
    L.ie_stream_bound.restype = C.c_size_t
    L.ie_encode_frames.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                   u8p, C.c_size_t, C.c_uint64, u64p, u64p]
    L.ie_decode_gop.argtypes = [vp, u8p, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int, u8p, C.c_size_t, C.c_size_t, u64p]
    L.ie_gop_stream_bound.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64]
    L.ie_gop_stream_bound.restype = C.c_size_t
    L.ie_encode_gop.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, u8p, C.c_size_t, C.c_uint64, u64p, u64p]
    if hasattr(L, "ie_encode_gop_groups"):  # (absent from an older IE_LIB build under comparison)
        L.ie_encode_gop_groups.restype = C.c_int
        L.ie_encode_gop_groups.argtypes = L.ie_encode_gop.argtypes
    L.ie_encode_images.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                   u8p, C.c_size_t, C.c_uint64, u64p]
    L.ie_encode_images_counted.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                           C.c_int, u8p, C.c_size_t, C.c_uint64]
    L.ie_huffman_hist_batch_ends_async.argtypes = [vp, u8p, C.c_size_t, u64p, C.c_int, C.c_int]
    L.ie_huffman_hist_batch_wait.argtypes = [vp, C.c_int, vp, vp]
    L.ie_last_end_bits.argtypes = [vp]
    L.ie_last_end_bits.restype = C.c_void_p
    L.ie_last_fallbacks.argtypes = [vp, u64p]
    L.ie_quantize_frames.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp]
    if hasattr(L, "ie_probe_sizes"):  # (absent from an older IE_LIB build under comparison)
        L.ie_probe_sizes.restype = C.c_int
        L.ie_probe_sizes.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, u16p, C.c_int,
                                     u64p]
    if hasattr(L, "ie_probe_rd"):  # (absent from an older IE_LIB build under comparison)
        L.ie_probe_rd.restype = C.c_int
        L.ie_probe_rd.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, u16p, C.c_int,
                                  u64p, u64p]
    if hasattr(L, "ie_probe_gop"):  # (absent from an older IE_LIB build under comparison)
        L.ie_probe_gop.restype = C.c_int
        L.ie_probe_gop.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                   u16p, C.c_int, u64p]
    if hasattr(L, "ie_probe_gop_rd"):  # (absent from an older IE_LIB build under comparison)
        L.ie_probe_gop_rd.restype = C.c_int
        L.ie_probe_gop_rd.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, u16p, C.c_int, u64p, u64p]
    for name in ("ie_huffman_hist", "ie_huffman_pack", "ie_bitcopy", "ie_decode_frames"):
        if hasattr(L, name):
            getattr(L, name).restype = C.c_int
    if hasattr(L, "ie_huffman_hist"):
        L.ie_huffman_hist.argtypes = [vp, u8p, C.c_size_t, u32p, u64p]
        L.ie_huffman_pack.argtypes = [vp, u8p, C.c_size_t, u32p, u8p, u8p, C.c_size_t, C.c_uint64, u64p]
        L.ie_bitcopy.argtypes = [vp, u8p, C.c_size_t, u8p, C.c_size_t, C.c_uint64]
    if hasattr(L, "ie_huffman_hist_batch"):
        L.ie_huffman_hist_batch.restype = C.c_int
        L.ie_huffman_hist_batch.argtypes = [vp, u8p, C.c_size_t, u64p, C.c_int, u32p, u64p]
        L.ie_huffman_pack_batch.restype = C.c_int
        L.ie_huffman_pack_batch.argtypes = [vp, u8p, C.c_size_t, u64p, C.c_int, u32p, u8p, u8p, C.c_size_t, u8p,
                                            C.c_size_t, u64p, u64p]
    if hasattr(L, "ie_decode_frames"):
        L.ie_decode_frames.argtypes = [vp, u8p, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                       u8p, C.c_size_t, C.c_size_t, u64p]
    if hasattr(L, "ie_decode_images"):  # (absent from an older IE_LIB build under comparison)
        L.ie_decode_images.restype = C.c_int
        L.ie_decode_images.argtypes = [vp, u8p, C.c_size_t, u64p, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int,
                                       u8p, C.c_size_t, C.c_size_t, u64p]
    if hasattr(L, "ie_decode_region"):  # (absent from an older IE_LIB build under comparison)
        L.ie_decode_region.restype = C.c_int
        L.ie_decode_region.argtypes = [vp, u8p, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_size_t, C.c_size_t, u64p]
        L.ie_decode_images_region.restype = C.c_int
        L.ie_decode_images_region.argtypes = [vp, u8p, C.c_size_t, u64p, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_int, u8p, C.c_size_t, C.c_size_t, u64p]
    if hasattr(L, "ie_decode_scaled"):  # (absent from an older IE_LIB build under comparison)
        L.ie_decode_scaled.restype = C.c_int
        L.ie_decode_scaled.argtypes = [vp, u8p, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u8p,
                                       C.c_size_t, C.c_size_t, u64p]
        L.ie_decode_images_scaled.restype = C.c_int
        L.ie_decode_images_scaled.argtypes = [vp, u8p, C.c_size_t, u64p, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int,
                                              C.c_int, u8p, C.c_size_t, C.c_size_t, u64p]
    if hasattr(L, "ie_huffman_decode_batch"):  # (absent from an older IE_LIB build under comparison)
        L.ie_huffman_decode_batch.restype = C.c_int
        L.ie_huffman_decode_batch.argtypes = [vp, u8p, C.c_size_t, u64p, C.c_int, u64p, u16p, u8p, C.c_size_t, u64p]
    L.ie_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(C.c_void_p)]
    L.ie_host_free.argtypes = [vp, vp]
    L.ie_vstream_open.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, u8p, C.c_uint64,
                                  C.c_int, C.POINTER(C.c_void_p)]
    if hasattr(L, "ie_vstream_open_gop"):  # (absent from an older IE_LIB build under comparison)
        L.ie_vstream_open_gop.restype = C.c_int
        L.ie_vstream_open_gop.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                          C.c_int, u8p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.ie_vstream_push.argtypes = [vp, u8p, C.c_int]
    L.ie_vstream_pull.argtypes = [vp, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ie_vstream_finish.argtypes = [vp, u8p, C.c_size_t, C.POINTER(C.c_size_t), u64p, u64p]
    L.ie_vstream_device.argtypes = [vp]
    L.ie_vstream_device.restype = C.c_void_p
    L.ie_vstream_close.argtypes = [vp]
    if hasattr(L, "ie_vdec_open"):  # (absent from an older IE_LIB build under comparison)
        ip = C.POINTER(C.c_int)
        L.ie_vdec_open.restype = C.c_int
        L.ie_vdec_open.argtypes = [vp, u8p, C.c_size_t, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.ie_vdec_next.restype = C.c_int
        L.ie_vdec_next.argtypes = [vp, u8p, C.c_size_t, C.c_size_t, C.c_int, ip]
        L.ie_vdec_info.restype = C.c_int
        L.ie_vdec_info.argtypes = [vp, ip, ip, ip, u64p]
        L.ie_vdec_close.restype = C.c_int
        L.ie_vdec_close.argtypes = [vp]
    L.ie_huffman_decode.argtypes = [vp, u8p, C.c_size_t, C.c_uint64, vp, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ie_last_decode_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ie_set_exact_parse.argtypes = [vp, C.c_int]
    L.ie_set_spec_warm.argtypes = [vp, C.c_int]
    L.ie_last_decode_spec.argtypes = [vp]
    L.ie_malloc.argtypes = [vp, C.c_size_t, C.POINTER(C.c_void_p)]
    L.ie_free.argtypes = [vp, vp]
    L.ie_memcpy.argtypes = [vp, vp, vp, C.c_size_t]
    L.ie_memset.argtypes = [vp, vp, C.c_int, C.c_size_t]
    L.ie_is_device_ptr.argtypes = [vp]
    _lib = L
    return L


def load_host_library(path: str | None = None) -> C.CDLL:
    """Load libie_host.so: the file-level encoders/decoders (include/ie_host.hpp).  With IE_LIB set
    (an A/B build of libie_hip.so) the libie_host.so beside it is used, so that both libraries
    are the same build."""
    global _host
    if _host is not None:
        return _host
    load_library()
    if path is None:
        alt = os.environ.get("IE_LIB")
        path = os.path.join(os.path.dirname(alt), "libie_host.so") if alt else HOST_LIB_PATH
    if not os.path.exists(path):
        raise IEError(IE_EHIP, f"{path} not built -- run `make host` (or __graft_entry__.build())")
    H = C.CDLL(path)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    H.ieh_encode_image.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                   C.c_size_t]
    if hasattr(H, "ieh_encode_image_budget"):  # (absent from an older IE_LIB build under comparison)
        H.ieh_scale_matrix.restype = C.c_int
        H.ieh_scale_matrix.argtypes = [vp, C.c_int, C.c_int, vp]
        H.ieh_budget_ladder.restype = C.c_int
        H.ieh_budget_ladder.argtypes = [ip]
        H.ieh_encode_image_budget.restype = C.c_int64
        H.ieh_encode_image_budget.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_size_t, vp, C.c_size_t, ip]
    if hasattr(H, "ieh_encode_image_quality"):  # (absent from an older IE_LIB build under comparison)
        H.ieh_encode_image_quality.restype = C.c_int64
        H.ieh_encode_image_quality.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_uint64, vp, C.c_size_t, ip, C.POINTER(C.c_uint64)]
    if hasattr(H, "ieh_encode_video_budget"):  # (absent from an older IE_LIB build under comparison)
        H.ieh_encode_video_budget.restype = C.c_int64
        H.ieh_encode_video_budget.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_size_t, vp, C.c_size_t, ip]
    if hasattr(H, "ieh_encode_video_quality"):  # (absent from an older IE_LIB build under comparison)
        H.ieh_encode_video_quality.restype = C.c_int64
        H.ieh_encode_video_quality.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, C.c_size_t, ip,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    H.ieh_encode_video.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, vp, C.c_size_t]
    H.ieh_encode_video_gop.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, vp, C.c_size_t]
    H.ieh_decode_image.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, ip, ip]
    H.ieh_decode_video.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, ip, ip, ip]
    if hasattr(H, "ieh_decode_images"):  # (absent from an older IE_LIB build under comparison)
        H.ieh_decode_images.restype = C.c_int64
        H.ieh_decode_images.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_uint64), C.c_int, C.c_int, vp, C.c_size_t,
                                        ip, ip]
    if hasattr(H, "ieh_decode_image_region"):  # (absent from an older IE_LIB build under comparison)
        H.ieh_decode_image_region.restype = C.c_int64
        H.ieh_decode_image_region.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                              C.c_size_t, ip, ip]
    if hasattr(H, "ieh_decode_image_scaled"):  # (absent from an older IE_LIB build under comparison)
        H.ieh_decode_image_scaled.restype = C.c_int64
        H.ieh_decode_image_scaled.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, ip, ip]
    if hasattr(H, "ieh_vdec_open"):  # (absent from an older IE_LIB build under comparison)
        H.ieh_vdec_open.restype = C.c_int
        H.ieh_vdec_open.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, ip, ip, ip, ip, ip,
                                    C.POINTER(C.c_void_p)]
        H.ieh_vdec_next.restype = C.c_int
        H.ieh_vdec_next.argtypes = [vp, vp, C.c_size_t, ip]
        H.ieh_vdec_close.restype = C.c_int
        H.ieh_vdec_close.argtypes = [vp]
    H.ieh_huffman_encode.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    H.ieh_huffman_decode.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, ip]
    H.ieh_huffman_table.argtypes = [vp, C.c_size_t, vp, C.POINTER(C.c_uint64)]
    H.ieh_huffman_table.restype = C.c_int
    H.ieh_huffman_encode_after_encode.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
    H.ieh_huffman_encode_after_encode.restype = C.c_int
    H.ieh_huffman_begin_after_encode.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int]
    H.ieh_huffman_begin_after_encode.restype = C.c_int
    H.ieh_huffman_finish_after_encode.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, vp]
    H.ieh_huffman_finish_after_encode.restype = C.c_int
    H.ieh_write_header.argtypes = [vp, C.c_size_t, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int]
    H.ieh_write_header.restype = C.c_int64
    H.ieh_huffman_encode_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    H.ieh_huffman_encode_device.restype = C.c_int64
    H.ieh_huffman_encode_device_batch.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, vp, C.c_size_t, vp]
    H.ieh_huffman_encode_device_batch.restype = C.c_int
    H.ieh_release.argtypes = [vp]
    H.ieh_release.restype = None
    for f in ("ieh_encode_image", "ieh_encode_video", "ieh_encode_video_gop", "ieh_decode_image", "ieh_decode_video", "ieh_huffman_encode",
              "ieh_huffman_decode"):
        getattr(H, f).restype = C.c_int64
    _host = H
    return H


def _ptr(a):
    """Address of a numpy array or a torch tensor (host or device)."""
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    raise TypeError(type(a))


def _nbytes(a) -> int:
    if isinstance(a, np.ndarray):
        return a.nbytes
    return a.numel() * a.element_size()


def _pitches(w: int, h: int, stride, frame_pitch):
    """(stride, frame_pitch) with the defaults of packed rows and packed frames."""
    stride = w if stride is None else stride
    return stride, stride * h if frame_pitch is None else frame_pitch


def write_header(n: int, q, rle: bool, w: int, h: int, huffman: bool = False, video: bool = False,
                 frames: int = 0, gop: int = 1, merange: int = 0):
    """Settings header bytes + bit length (host library; ImageEncoder.cpp:84-94, VideoEncoder.cpp:60-73)."""
    H = load_host_library()
    q = np.ascontiguousarray(np.asarray(q, dtype=np.uint16).ravel())
    out = np.zeros(256, dtype=np.uint8)
    bits = H.ieh_write_header(out.ctypes.data, out.size, n, q.ctypes.data, int(rle), w, h, int(huffman),
                              int(video), frames, gop, merange)
    if bits < 0:
        raise IEError(int(bits), "ieh_write_header")
    return out[: (bits + 7) // 8].copy(), int(bits)


def read_matrix(path: str, n: int) -> np.ndarray:
    """A quantisation matrix file: n*n whitespace-separated unsigned values, row-major
    (dc::MatrixReader<N>::read, MatrixReader.cpp:65-134).  Raises ValueError on a malformed file."""
    with open(path) as f:
        vals = [int(t) for t in f.read().split()]
    if len(vals) != n * n or any(v <= 0 or v > 0xFFFF for v in vals):
        raise ValueError(f"{path}: expected {n * n} values in 1..65535, got {len(vals)}")
    return np.array(vals, dtype=np.uint16)


def scale_matrix(base, percent: int) -> np.ndarray:
    """``base`` (4x4 or 8x8) scaled to ``percent`` % (ieh_scale_matrix): every entry
    ``clamp((v * percent + 50) // 100, 1, 65535)``, uint16, flat.  Raises on ``percent < 1``."""
    H = load_host_library()
    base = np.ascontiguousarray(np.asarray(base, dtype=np.uint16).ravel())
    n = int(round(base.size ** 0.5))
    out = np.zeros(base.size, dtype=np.uint16)
    r = H.ieh_scale_matrix(base.ctypes.data, n, int(percent), out.ctypes.data)
    if r != IE_OK:
        raise IEError(r, f"scale_matrix: {n}x{n} matrix, percent {percent}")
    return out


def budget_ladder() -> list[int]:
    """The 32 percents :meth:`Codec.encode_image_budget` probes first (ieh_budget_ladder)."""
    H = load_host_library()
    out = (C.c_int * 32)()
    return list(out[: H.ieh_budget_ladder(out)])


def sse_for_psnr(psnr: float, npixels: int) -> int:
    """The largest squared error of ``npixels`` 8-bit pixels whose PSNR is still at least ``psnr``
    dB: ``floor(npixels * 255**2 / 10**(psnr / 10))``."""
    return int(math.floor(npixels * 255.0 ** 2 / 10.0 ** (psnr / 10.0)))


def psnr_of_sse(sse: int, npixels: int) -> float:
    """The PSNR in dB of a squared error ``sse`` over ``npixels`` 8-bit pixels:
    ``10 log10(npixels * 255**2 / sse)``; ``inf`` for 0."""
    if sse == 0:
        return math.inf
    return 10.0 * math.log10(npixels * 255.0 ** 2 / sse)


def stream_bound(w: int, h: int, n: int, nframes: int = 1, start_bit: int = 0) -> int:
    return int(load_library().ie_stream_bound(w, h, n, nframes, start_bit))


class _PinnedOwner:
    """Frees an ie_host_alloc block when the numpy array viewing it is collected."""
    _live = {}

    @classmethod
    def attach(cls, arr, codec, addr):
        import weakref
        key = id(arr)
        cls._live[key] = weakref.finalize(arr, cls._free, codec, addr, key)

    @classmethod
    def _free(cls, codec, addr, key):
        cls._live.pop(key, None)
        if getattr(codec, "h", None):
            codec.L.ie_host_free(codec.h, C.c_void_p(addr))


class VideoStream:
    """ie_vstream_*: push host frames, pull finished stream bytes, finish (see include/ie_hip.h)."""

    def __init__(self, codec, w, h, head, start_bit, max_frames, stride, frame_pitch, rle, mode, gop=1, merange=0):
        self.c = codec
        self.w, self.h = w, h
        self.stride, self.frame_pitch = _pitches(w, h, stride, frame_pitch)
        head = np.zeros(1, dtype=np.uint8) if head is None else np.ascontiguousarray(head, dtype=np.uint8)
        self._head = head
        v = C.c_void_p()
        codec._chk(codec.L.ie_vstream_open_gop(codec.h, w, h, self.stride, self.frame_pitch, gop, merange, int(rle),
                                               mode, head.ctypes.data, start_bit, max_frames, C.byref(v)))
        self.v = v
        self.max_frames = max_frames
        self.pushed = 0
        self.cap = (codec.gop_stream_bound(w, h, max_frames, merange, start_bit) if gop > 1
                    else stream_bound(w, h, codec.n, max_frames, start_bit))

    def push(self, frames, nframes: int):
        self.c._chk(self.c.L.ie_vstream_push(self.v, _ptr(frames), nframes))
        self.pushed += nframes

    def pull(self, dst: np.ndarray, offset: int) -> int:
        """Finished bytes into dst[offset:]; returns how many."""
        n = C.c_size_t(0)
        self.c._chk(self.c.L.ie_vstream_pull(self.v, dst.ctypes.data + offset, dst.size - offset, C.byref(n)))
        return int(n.value)

    def finish(self, dst: np.ndarray | None = None, offset: int = 0):
        """Remaining bytes into dst[offset:] (if given); returns (nbytes, end_bit, frame_bits)."""
        n, end = C.c_size_t(0), C.c_uint64(0)
        fb = np.zeros(max(self.pushed, 1), dtype=np.uint64)
        dp = dst.ctypes.data + offset if dst is not None else None
        cap = dst.size - offset if dst is not None else 0
        self.c._chk(self.c.L.ie_vstream_finish(self.v, dp, cap, C.byref(n), C.byref(end),
                                               fb.ctypes.data_as(C.POINTER(C.c_uint64))))
        return int(n.value), int(end.value), fb[: self.pushed]

    def device_ptr(self) -> int:
        return int(self.c.L.ie_vstream_device(self.v) or 0)

    def close(self):
        if getattr(self, "v", None):
            self.c.L.ie_vstream_close(self.v)
            self.v = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VideoDecodeStream:
    """ie_vdec_*: a video payload decoded in chunks of frames, handed out while later chunks still
    decode (see include/ie_hip.h).  The frames in order equal :meth:`Codec.decode_gop`'s."""

    def __init__(self, codec, stream, w, h, nframes, gop, merange, start_bit, rle, motioncomp, chunk_frames,
                 length=None):
        self.c = codec
        self.w, self.h, self.nframes = w, h, nframes
        self._in = stream  # (an aligned device stream is read in place until close)
        v = C.c_void_p()
        codec._chk(codec.L.ie_vdec_open(codec.h, _ptr(stream), _nbytes(stream) if length is None else length, start_bit,
                                        w, h, nframes, gop, merange, int(rle), int(motioncomp), chunk_frames,
                                        C.byref(v)))
        self.v = v

    def next(self, out, max_frames: int, stride: int | None = None, frame_pitch: int | None = None) -> int:
        """Up to ``max_frames`` frames into ``out`` (host or device; frame i of the call at
        ``i * frame_pitch``); returns how many, 0 after the last.  A stream that ends early raises
        :class:`IEError` (IE_EFORMAT) whose ``got`` is the number of whole frames written first."""
        stride, frame_pitch = _pitches(self.w, self.h, stride, frame_pitch)
        got = C.c_int(0)
        r = self.c.L.ie_vdec_next(self.v, _ptr(out), stride, frame_pitch, max_frames, C.byref(got))
        if r != IE_OK:
            e = IEError(r, self.c.L.ie_last_error(self.c.h).decode())
            e.got = int(got.value)
            raise e
        return int(got.value)

    def info(self) -> dict:
        """chunk_frames, chunks_enqueued, chunks_delivered, end_bit (2**64 - 1 until the last frame is out)."""
        k, e, d, end = C.c_int(0), C.c_int(0), C.c_int(0), C.c_uint64(0)
        self.c._chk(self.c.L.ie_vdec_info(self.v, C.byref(k), C.byref(e), C.byref(d), C.byref(end)))
        return dict(chunk_frames=int(k.value), chunks_enqueued=int(e.value), chunks_delivered=int(d.value),
                    end_bit=int(end.value))

    def close(self):
        if getattr(self, "v", None):
            if getattr(self.c, "h", None):
                self.c.L.ie_vdec_close(self.v)
            self.v = None
            self._in = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Codec:
    """One device context (``ie_ctx``) with its quantisation tables."""

    def __init__(self, device: int = 0, quant=None, n: int | None = None):
        self.L = load_library()
        h = C.c_void_p()
        r = self.L.ie_create(device, C.byref(h))
        if r != IE_OK:
            raise IEError(r, "ie_create failed (no HIP device?)")
        self.h = h
        self.n = None
        if quant is not None:
            self.set_quant(quant, n)

    def close(self):
        if getattr(self, "h", None):
            if _host is not None:
                _host.ieh_release(self.h)
            self.L.ie_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r: int):
        if r != IE_OK:
            raise IEError(r, self.L.ie_last_error(self.h).decode())

    def set_stream(self, stream_handle: int | None):
        self._chk(self.L.ie_set_stream(self.h, stream_handle))

    def sync(self):
        self._chk(self.L.ie_sync(self.h))

    def set_quant(self, q, n: int | None = None):
        q = np.ascontiguousarray(np.asarray(q, dtype=np.uint16).ravel())
        if n is None:
            n = int(round(q.size ** 0.5))
        assert q.size == n * n
        self._chk(self.L.ie_set_quant(self.h, q.ctypes.data, n))
        self.n = n

    def set_stage_timing(self, on: bool) -> None:
        """Record HIP events around the batched Huffman stages (for :meth:`last_stage_ms`; off by
        default, the events delay the pipelined launches)."""
        self._chk(self.L.ie_set_stage_timing(self.h, int(bool(on))))

    def last_stage_ms(self, stage: int) -> float:
        """Device time (ms) of the last batched Huffman histogram (0) or pack (1) (ie_last_stage_ms)."""
        v = C.c_float()
        self._chk(self.L.ie_last_stage_ms(self.h, stage, C.byref(v)))
        return float(v.value)

    def cos_table(self) -> np.ndarray:
        """The cos table the kernels use (read back from the device; ie_cos_table), n x n doubles."""
        out = np.zeros(self.n * self.n, np.float64)
        self._chk(self.L.ie_cos_table(self.h, out.ctypes.data))
        return out.reshape(self.n, self.n)

    def encode_frames(self, y, w: int, h: int, out, start_bit: int = 0, stride: int | None = None,
                      frame_pitch: int | None = None, nframes: int = 1, rle: bool = True,
                      mode: int = MODE_FAST, want_sizes: bool = True):
        """Append the block records of ``nframes`` frames to ``out`` from ``start_bit``.
        ``y``/``out``: numpy arrays (host) or torch tensors (device).  Returns
        ``(frame_bits, end_bit)`` or ``None`` when ``want_sizes`` is False (async)."""
        stride, frame_pitch = _pitches(w, h, stride, frame_pitch)
        fb = np.zeros(nframes, dtype=np.uint64)
        end = C.c_uint64(0)
        fbp = fb.ctypes.data_as(C.POINTER(C.c_uint64)) if want_sizes else None
        endp = C.pointer(end) if want_sizes else None
        self._chk(self.L.ie_encode_frames(self.h, _ptr(y), w, h, stride, frame_pitch, nframes, int(rle), mode,
                                          _ptr(out), _nbytes(out), start_bit, fbp, endp))
        if not want_sizes:
            return None
        return fb, int(end.value)

    def gop_stream_bound(self, w: int, h: int, nframes: int, merange: int, start_bit: int = 0) -> int:
        return int(self.L.ie_gop_stream_bound(w, h, self.n, nframes, merange, start_bit))

    def encode_gop(self, y, w: int, h: int, out, gop: int, merange: int, start_bit: int = 0,
                   stride: int | None = None, frame_pitch: int | None = None, nframes: int = 1, rle: bool = True,
                   mode: int = MODE_FAST):
        """The payload of a video with I- and P-frames (frame f is an I-frame when f % gop == 0;
        VideoEncoder.cpp:83-91, Frame.cpp:129-247) appended to ``out`` from ``start_bit``; ``out``
        holds :meth:`gop_stream_bound` bytes.  Returns ``(frame_bits, end_bit)``."""
        return self._encode_gop(self.L.ie_encode_gop, y, w, h, out, gop, merange, start_bit, stride, frame_pitch,
                                nframes, rle, mode)

    def encode_gop_groups(self, y, w: int, h: int, out, gop: int, merange: int, start_bit: int = 0,
                          stride: int | None = None, frame_pitch: int | None = None, nframes: int = 1,
                          rle: bool = True, mode: int = MODE_FAST):
        """:meth:`encode_gop` with the groups of pictures encoded side by side and spliced into the
        same stream (ie_encode_gop_groups): same arguments, same bytes, same return value."""
        return self._encode_gop(self.L.ie_encode_gop_groups, y, w, h, out, gop, merange, start_bit, stride,
                                frame_pitch, nframes, rle, mode)

    def _encode_gop(self, call, y, w, h, out, gop, merange, start_bit, stride, frame_pitch, nframes, rle, mode):
        stride, frame_pitch = _pitches(w, h, stride, frame_pitch)
        fb = np.zeros(nframes, dtype=np.uint64)
        end = C.c_uint64(0)
        self._chk(call(self.h, _ptr(y), w, h, stride, frame_pitch, nframes, gop, merange, int(rle), mode, _ptr(out),
                       _nbytes(out), start_bit, fb.ctypes.data_as(C.POINTER(C.c_uint64)), C.pointer(end)))
        return fb, int(end.value)

    def decode_gop(self, stream, w: int, h: int, out, gop: int, merange: int, nframes: int, start_bit: int = 0,
                   length: int | None = None, stride: int | None = None, frame_pitch: int | None = None,
                   rle: bool = True, motioncomp: bool = True) -> int:
        """Decode an I/P-frame payload (VideoDecoder / Frame::loadFromStream) into ``out``; the end bit."""
        stride, frame_pitch = _pitches(w, h, stride, frame_pitch)
        end = C.c_uint64(0)
        self._chk(self.L.ie_decode_gop(self.h, _ptr(stream), _nbytes(stream) if length is None else length, start_bit,
                                       w, h, nframes, gop, merange, int(rle), int(motioncomp), _ptr(out), stride,
                                       frame_pitch, C.pointer(end)))
        return int(end.value)

    def encode_images(self, y, w: int, h: int, out, out_pitch: int, nframes: int, start_bit: int = 0,
                      stride: int | None = None, frame_pitch: int | None = None, rle: bool = True,
                      mode: int = MODE_FAST, want_sizes: bool = True, count_bytes: bool = False):
        """count_bytes (device ``out``): also count every image's stream bytes for the following
        Huffman pass (:meth:`huffman_begin_after_encode` then skips its histogram kernel);
        implies want_sizes=False."""
        stride, frame_pitch = _pitches(w, h, stride, frame_pitch)
        if count_bytes:
            self._chk(self.L.ie_encode_images_counted(self.h, _ptr(y), w, h, stride, frame_pitch, nframes, int(rle),
                                                      mode, _ptr(out), out_pitch, start_bit))
            return None
        eb = np.zeros(nframes, dtype=np.uint64)
        ebp = eb.ctypes.data_as(C.POINTER(C.c_uint64)) if want_sizes else None
        self._chk(self.L.ie_encode_images(self.h, _ptr(y), w, h, stride, frame_pitch, nframes, int(rle), mode,
                                          _ptr(out), out_pitch, start_bit, ebp))
        return eb if want_sizes else None

    def quantize_frames(self, y, w: int, h: int, nframes: int = 1, stride: int | None = None,
                        frame_pitch: int | None = None, mode: int = MODE_FAST) -> np.ndarray:
        """Quantised coefficients (natural order) of every block: shape (blocks, n*n) int16."""
        stride, frame_pitch = _pitches(w, h, stride, frame_pitch)
        n = self.n
        coef = np.zeros((nframes * (w // n) * (h // n), n * n), dtype=np.int16)
        self._chk(self.L.ie_quantize_frames(self.h, _ptr(y), w, h, stride, frame_pitch, nframes, mode,
                                            coef.ctypes.data))
        return coef

    def probe_sizes(self, y, w: int, h: int, qs, nframes: int = 1, rle: bool = True, stride: int | None = None,
                    frame_pitch: int | None = None, out=None) -> np.ndarray:
        """The payload bits of every frame under every candidate matrix of ``qs`` (``(nq, n*n)``
        or a list of matrices; at most 64) from one pass over the pixels (ie_probe_sizes): shape
        ``(nq, nframes)`` uint64, entry ``[m, f]`` = the ``frame_bits[f]`` of :meth:`encode_frames`
        after ``set_quant(qs[m])``.  The codec's own matrix is left as it was.  ``y``: numpy array
        or torch tensor.  ``out``: an optional device tensor of ``nq * nframes`` 64-bit entries,
        which receives the sums instead -- the call is then asynchronous and returns ``out``."""
        return self._probe("probe_sizes", False, y, w, h, qs, nframes, (int(rle),), stride, frame_pitch, out)

    def _probe(self, name, rd, y, w, h, qs, nframes, ints, stride, frame_pitch, out):
        """The body of the four probes.  ``name``: the method, whose entry point is ``ie_<name>``;
        ``ints``: that call's integer arguments between ``nframes`` and the candidates; ``rd``: the
        results are the pair ``(bits, sse)``, not ``bits`` alone."""
        stride, frame_pitch = _pitches(w, h, stride, frame_pitch)
        nn = (self.n or 0) ** 2
        qs = np.ascontiguousarray(np.asarray(qs, dtype=np.uint16).reshape(-1, nn) if nn else
                                  np.asarray(qs, dtype=np.uint16))
        nq = qs.shape[0] if nn else 1
        u64p = C.POINTER(C.c_uint64)
        if out is not None:
            res = (out,)
            if rd:
                dbits, dsse = out
                res = (dbits, dsse)
            if any(t is not None and _nbytes(t) < 8 * nq * nframes for t in res):
                raise IEError(IE_EINVAL, f"{name}: out holds fewer than nq * nframes 64-bit entries")
            ptrs = [None if t is None else C.cast(C.c_void_p(_ptr(t)), u64p) for t in res]
        else:
            res = tuple(np.zeros((max(nq, 1), nframes), dtype=np.uint64) for _ in range(2 if rd else 1))
            ptrs = [t.ctypes.data_as(u64p) for t in res]
        self._chk(getattr(self.L, "ie_" + name)(self.h, _ptr(y), w, h, stride, frame_pitch, nframes, *ints,
                                                qs.ctypes.data, nq, *ptrs))
        if out is not None:
            return out
        return res if rd else res[0]

    def probe_gop(self, y, w: int, h: int, qs, gop: int, merange: int, nframes: int = 1, rle: bool = True,
                  stride: int | None = None, frame_pitch: int | None = None, out=None) -> np.ndarray:
        """:meth:`probe_sizes` for a video with P-frames (ie_probe_gop): shape ``(nq, nframes)``
        uint64, entry ``[m, f]`` = the ``frame_bits[f]`` of :meth:`encode_gop` with the same ``gop``
        and ``merange`` after ``set_quant(qs[m])``.  The codec's own matrix is left as it was.
        ``out``: an optional device tensor of ``nq * nframes`` 64-bit entries, which receives the
        sums instead -- the call is then asynchronous and returns ``out``."""
        return self._probe("probe_gop", False, y, w, h, qs, nframes, (gop, merange, int(rle)), stride, frame_pitch, out)

    def probe_rd(self, y, w: int, h: int, qs, nframes: int = 1, rle: bool = True, stride: int | None = None,
                 frame_pitch: int | None = None, out=None):
        """:meth:`probe_sizes`, and the distortion with it (ie_probe_rd): ``(bits, sse)``, each of
        shape ``(nq, nframes)`` uint64.  ``sse[m, f]`` is the exact sum over frame f's pixels of
        (decoded - original)^2, the decoded pixel being what :meth:`decode_frames` writes for the
        stream :meth:`encode_frames` writes after ``set_quant(qs[m])`` with the same ``rle``.  The
        codec's own matrix is left as it was.  ``out``: an optional pair ``(bits, sse)`` of device
        tensors of ``nq * nframes`` 64-bit entries each (``bits`` may be None), which receive the
        sums instead -- the call is then asynchronous and returns ``out``."""
        return self._probe("probe_rd", True, y, w, h, qs, nframes, (int(rle),), stride, frame_pitch, out)

    def probe_gop_rd(self, y, w: int, h: int, qs, gop: int, merange: int, nframes: int = 1, rle: bool = True,
                     motioncomp: bool = True, stride: int | None = None, frame_pitch: int | None = None, out=None):
        """:meth:`probe_gop`, and the distortion with it (ie_probe_gop_rd): ``(bits, sse)``, each of
        shape ``(nq, nframes)`` uint64.  ``sse[m, f]`` is the exact sum over frame f's pixels of
        (decoded - original)^2, the decoded pixel being what :meth:`decode_gop` writes with this
        ``motioncomp`` for the stream :meth:`encode_gop` writes after ``set_quant(qs[m])``.  With
        P-frames, ``w`` and ``h`` are multiples of 16 and the blocks 4x4 (what does not decode has
        nothing to measure: ``IE_EINVAL``).  The codec's own matrix is left as it was.  ``out``: an
        optional pair ``(bits, sse)`` of device tensors of ``nq * nframes`` 64-bit entries each
        (``bits`` may be None), which receive the sums instead -- the call is then asynchronous and
        returns ``out``."""
        return self._probe("probe_gop_rd", True, y, w, h, qs, nframes, (gop, merange, int(rle), int(motioncomp)), stride,
                           frame_pitch, out)

    def host_array(self, nbytes: int) -> np.ndarray:
        """A uint8 numpy array in page-locked host memory (ie_host_alloc): host buffers the
        streamed path DMAs directly.  Freed when the array (and the codec) are gone."""
        p = C.c_void_p()
        self._chk(self.L.ie_host_alloc(self.h, nbytes, C.byref(p)))
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8)
        _PinnedOwner.attach(arr, self, p.value)
        return arr

    def open_video_stream(self, w: int, h: int, head=None, start_bit: int = 0, max_frames: int = 1,
                          stride: int | None = None, frame_pitch: int | None = None, rle: bool = True,
                          mode: int = MODE_FAST, gop: int = 1, merange: int = 0) -> "VideoStream":
        """ie_vstream_open_gop: a video payload grown on the device from host frames pushed over
        time (Frame.cpp:31-45 / VideoEncoder.cpp:83-91); with gop > 1 the video has P-frames and is
        encoded in chunks of whole groups of pictures (the stream equals encode_gop's)."""
        return VideoStream(self, w, h, head, start_bit, max_frames, stride, frame_pitch, rle, mode, gop, merange)

    def open_video_decode(self, stream, w: int, h: int, nframes: int, gop: int = 1, merange: int = 0,
                          start_bit: int = 0, rle: bool = True, motioncomp: bool = True, chunk_frames: int = 0,
                          length: int | None = None) -> "VideoDecodeStream":
        """ie_vdec_open: the payload ``stream`` (host or device) decoded in chunks of
        ``chunk_frames`` frames (0: IE_CHUNK_MB's pixel target) through two device slots; the
        frames that :meth:`VideoDecodeStream.next` hands out equal :meth:`decode_gop`'s."""
        return VideoDecodeStream(self, stream, w, h, nframes, gop, merange, start_bit, rle, motioncomp, chunk_frames,
                                 length)

    def end_bits_into(self, dst, count: int = 1):
        """Stream-ordered device copy of the last encode's end bit(s) (one per chain) into the
        device tensor ``dst`` (uint64/int64): no host read-back."""
        src = self.L.ie_last_end_bits(self.h)
        self._chk(self.L.ie_memcpy(self.h, C.c_void_p(_ptr(dst)), C.c_void_p(src), 8 * count))

    def last_decode_info(self) -> tuple[int, int]:
        """(chunks, composition levels) of the last record decode's exact parse (ie_last_decode_info)."""
        f, r = C.c_int(0), C.c_int(0)
        self._chk(self.L.ie_last_decode_info(self.h, C.byref(f), C.byref(r)))
        return int(f.value), int(r.value)

    def set_exact_parse(self, exact: bool, warm: int = 0) -> None:
        """Record decodes parse exactly (composed transfer tables) instead of speculatively first
        (ie_set_exact_parse); a speculative parse may start each chunk's walk ``warm`` (<= 8)
        chunks early."""
        self._chk(self.L.ie_set_spec_warm(self.h, int(warm)))
        self._chk(self.L.ie_set_exact_parse(self.h, 1 if exact else 0))

    def last_decode_spec(self) -> bool:
        """True when the last record decode was completed by the speculative parse."""
        return bool(self.L.ie_last_decode_spec(self.h))

    def last_fallbacks(self) -> int:
        v = C.c_uint64(0)
        self._chk(self.L.ie_last_fallbacks(self.h, C.byref(v)))
        return int(v.value)

    # ---- Huffman post-pass (Huffman.cpp:233-344) and the inverse path
    def huffman_hist(self, data):
        """(hist[256] uint32, first_pos[256] uint64) of the bytes in ``data`` (host or device)."""
        hist = np.zeros(256, dtype=np.uint32)
        first = np.zeros(256, dtype=np.uint64)
        self._chk(self.L.ie_huffman_hist(self.h, _ptr(data), _nbytes(data), hist.ctypes.data,
                                         first.ctypes.data_as(C.POINTER(C.c_uint64))))
        return hist, first

    def huffman_pack(self, data, code, length, out, start_bit: int = 0) -> int:
        code = np.ascontiguousarray(code, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.uint8)
        end = C.c_uint64(0)
        self._chk(self.L.ie_huffman_pack(self.h, _ptr(data), _nbytes(data), code.ctypes.data, length.ctypes.data,
                                         _ptr(out), _nbytes(out), start_bit, C.byref(end)))
        return int(end.value)

    def bitcopy(self, data, out, start_bit: int):
        self._chk(self.L.ie_bitcopy(self.h, _ptr(data), _nbytes(data), _ptr(out), _nbytes(out), start_bit))

    def decode_frames(self, stream, w: int, h: int, out, start_bit: int = 0, nframes: int = 1, rle: bool = True,
                      stride: int | None = None, frame_pitch: int | None = None, length: int | None = None) -> int:
        """Decode ``nframes`` frames of block records from bit ``start_bit``; returns the end bit."""
        stride, frame_pitch = _pitches(w, h, stride, frame_pitch)
        end = C.c_uint64(0)
        n = _nbytes(stream) if length is None else length
        self._chk(self.L.ie_decode_frames(self.h, _ptr(stream), n, start_bit, w, h, nframes, int(rle), _ptr(out),
                                          stride, frame_pitch, C.byref(end)))
        return int(end.value)

    def decode_images(self, streams, in_pitch: int, nbits, w: int, h: int, out, start_bit: int = 0, rle: bool = True,
                      stride: int | None = None, frame_pitch: int | None = None) -> np.ndarray:
        """Decode ``len(nbits)`` independent images in one set of launches (ie_decode_images):
        image k's stream is the bits ``[0, nbits[k])`` of ``streams + k*in_pitch`` with its first
        record at ``start_bit``; its pixels go to ``out + k*frame_pitch``.  ``streams``/``out``:
        numpy arrays (host) or torch tensors (device).  Returns the end bits (uint64, one per
        image); raises :class:`IEError` (``IE_EFORMAT``, the message names the image) when an
        image's stream ends before its last block -- the other images are decoded all the same."""
        stride, frame_pitch = _pitches(w, h, stride, frame_pitch)
        nb = np.ascontiguousarray(nbits, dtype=np.uint64)
        eb = np.zeros(max(nb.size, 1), dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._chk(self.L.ie_decode_images(self.h, _ptr(streams), in_pitch, nb.ctypes.data_as(u64p), int(nb.size),
                                          start_bit, w, h, int(rle), _ptr(out), stride, frame_pitch,
                                          eb.ctypes.data_as(u64p)))
        return eb[: nb.size]

    def decode_region(self, stream, w: int, h: int, rect, out=None, start_bit: int = 0, nframes: int = 1,
                      rle: bool = True, stride: int | None = None, frame_pitch: int | None = None):
        """Decode only the rectangle ``rect = (x0, y0, rw, rh)`` of ``nframes`` frames of block records
        (ie_decode_region): row ``r`` of frame ``f`` goes to ``out + f*frame_pitch + r*stride``, ``rw``
        bytes of it; these pixels equal that crop of what :meth:`decode_frames` writes.  ``out``: a
        numpy array (host) or torch tensor (device); ``None`` makes a ``(nframes, rh, rw)`` uint8
        array.  Returns ``(out, end_bit)``: the whole stream is parsed, the end bit is the full
        decode's."""
        x0, y0, rw, rh = (int(v) for v in rect)
        stride, frame_pitch = _pitches(rw, rh, stride, frame_pitch)
        if out is None:
            if stride != rw or frame_pitch != rw * rh:
                raise IEError(IE_EINVAL, "decode_region: a stride or frame_pitch needs an out buffer")
            out = np.zeros((nframes, max(rh, 0), max(rw, 0)), dtype=np.uint8)
        end = C.c_uint64(0)
        self._chk(self.L.ie_decode_region(self.h, _ptr(stream), _nbytes(stream), start_bit, w, h, nframes, int(rle),
                                          x0, y0, rw, rh, _ptr(out), stride, frame_pitch, C.byref(end)))
        return out, int(end.value)

    def decode_images_region(self, streams, in_pitch: int, nbits, w: int, h: int, rect, out=None, start_bit: int = 0,
                             rle: bool = True, stride: int | None = None, frame_pitch: int | None = None):
        """The rectangle ``rect = (x0, y0, rw, rh)`` of ``len(nbits)`` independent images in one set
        of launches (ie_decode_images_region; the arguments of :meth:`decode_images`): image k's
        region goes to ``out + k*frame_pitch``.  ``out=None`` makes a ``(count, rh, rw)`` uint8
        array.  Returns ``(out, end_bits)``; raises :class:`IEError` (``IE_EFORMAT``, the message
        names the image) when an image's stream ends before its last block, wherever that is."""
        x0, y0, rw, rh = (int(v) for v in rect)
        stride, frame_pitch = _pitches(rw, rh, stride, frame_pitch)
        nb = np.ascontiguousarray(nbits, dtype=np.uint64)
        if out is None:
            if stride != rw or frame_pitch != rw * rh:
                raise IEError(IE_EINVAL, "decode_images_region: a stride or frame_pitch needs an out buffer")
            out = np.zeros((max(int(nb.size), 1), max(rh, 0), max(rw, 0)), dtype=np.uint8)
        eb = np.zeros(max(nb.size, 1), dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._chk(self.L.ie_decode_images_region(self.h, _ptr(streams), in_pitch, nb.ctypes.data_as(u64p), int(nb.size),
                                                 start_bit, w, h, int(rle), x0, y0, rw, rh, _ptr(out), stride,
                                                 frame_pitch, eb.ctypes.data_as(u64p)))
        return out, eb[: nb.size]

    def _scaled_out(self, what: str, count: int, w: int, h: int, scale: int, out, stride, frame_pitch):
        """(out, stride, frame_pitch) of a scaled decode with the defaults filled in: packed rows of
        ``w // scale`` bytes (a scale the library will refuse sizes ``out`` as scale 1)."""
        s = scale if isinstance(scale, int) and scale > 0 else 1
        ow, oh = max(w // s, 0), max(h // s, 0)
        stride, frame_pitch = _pitches(ow, oh, stride, frame_pitch)
        if out is None:
            if stride != ow or frame_pitch != ow * oh:
                raise IEError(IE_EINVAL, what + ": a stride or frame_pitch needs an out buffer")
            out = np.zeros((max(count, 1), oh, ow), dtype=np.uint8)
        return out, stride, frame_pitch

    def decode_scaled(self, stream, w: int, h: int, scale: int, out=None, start_bit: int = 0, nframes: int = 1,
                      rle: bool = True, stride: int | None = None, frame_pitch: int | None = None):
        """Decode ``nframes`` frames of block records at ``1/scale`` of their width and height
        (ie_decode_scaled; ``scale`` 1, 2, 4 or 8, at most the block size): every output pixel is the
        mean, rounded half up, of the ``scale x scale`` pixels :meth:`decode_frames` writes there.
        Row ``r`` of frame ``f`` goes to ``out + f*frame_pitch + r*stride``, ``w // scale`` bytes of
        it.  ``out``: a numpy array (host) or torch tensor (device); ``None`` makes a
        ``(nframes, h // scale, w // scale)`` uint8 array.  Returns ``(out, end_bit)``: the whole
        stream is parsed, the end bit is the full decode's."""
        out, stride, frame_pitch = self._scaled_out("decode_scaled", nframes, w, h, scale, out, stride, frame_pitch)
        end = C.c_uint64(0)
        self._chk(self.L.ie_decode_scaled(self.h, _ptr(stream), _nbytes(stream), start_bit, w, h, nframes, int(rle),
                                          scale, _ptr(out), stride, frame_pitch, C.byref(end)))
        return out, int(end.value)

    def decode_images_scaled(self, streams, in_pitch: int, nbits, w: int, h: int, scale: int, out=None, start_bit: int = 0,
                             rle: bool = True, stride: int | None = None, frame_pitch: int | None = None):
        """``len(nbits)`` independent images at ``1/scale`` of their size in one set of launches
        (ie_decode_images_scaled; the arguments of :meth:`decode_images`): image k's picture goes to
        ``out + k*frame_pitch``.  ``out=None`` makes a ``(count, h // scale, w // scale)`` uint8
        array.  Returns ``(out, end_bits)``; raises :class:`IEError` (``IE_EFORMAT``, the message
        names the image) when an image's stream ends before its last block."""
        nb = np.ascontiguousarray(nbits, dtype=np.uint64)
        out, stride, frame_pitch = self._scaled_out("decode_images_scaled", int(nb.size), w, h, scale, out, stride,
                                                    frame_pitch)
        eb = np.zeros(max(nb.size, 1), dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._chk(self.L.ie_decode_images_scaled(self.h, _ptr(streams), in_pitch, nb.ctypes.data_as(u64p), int(nb.size),
                                                 start_bit, w, h, int(rle), scale, _ptr(out), stride, frame_pitch,
                                                 eb.ctypes.data_as(u64p)))
        return out, eb[: nb.size]

    # ---- whole files (libie_host.so, include/ie_host.hpp)
    def _host_chk(self, r: int) -> int:
        if r < 0:
            raise IEError(int(r), self.L.ie_last_error(self.h).decode())
        return int(r)

    def encode_image_file(self, y, w: int, h: int, q, n: int, rle: bool = True, huffman: bool = True,
                          mode: int = MODE_FAST) -> bytes:
        H = load_host_library()
        q = np.ascontiguousarray(np.asarray(q, dtype=np.uint16).ravel())
        cap = stream_bound(w, h, n, 1, 2048) + 64
        out = np.zeros(cap, dtype=np.uint8)
        r = self._host_chk(H.ieh_encode_image(self.h, _ptr(y), w, h, q.ctypes.data, n, int(rle), int(huffman), mode,
                                              out.ctypes.data, cap))
        return out[:r].tobytes()

    def encode_image_budget(self, y, w: int, h: int, q, n: int, budget: int, rle: bool = True, huffman: bool = True,
                            mode: int = MODE_FAST):
        """An image file with the finest probed scale of ``q`` whose size -- header + payload,
        before the Huffman pass -- fits ``budget`` bytes (ieh_encode_image_budget): ``(bytes,
        percent)``.  Raises ``IEError(IE_ECAP, ...)`` (``e.percent`` = 5382) when no scale fits.
        The codec's matrix afterwards is the chosen one."""
        H = load_host_library()
        q = np.ascontiguousarray(np.asarray(q, dtype=np.uint16).ravel())
        cap = stream_bound(w, h, n, 1, 2048) + 64
        out = np.zeros(cap, dtype=np.uint8)
        pc = C.c_int(0)
        r = H.ieh_encode_image_budget(self.h, _ptr(y), w, h, q.ctypes.data, n, int(rle), int(huffman), mode,
                                      int(budget), out.ctypes.data, cap, C.byref(pc))
        if r < 0:
            e = IEError(int(r), self.L.ie_last_error(self.h).decode())
            e.percent = int(pc.value)
            raise e
        self.n = n
        return out[: int(r)].tobytes(), int(pc.value)

    def encode_image_quality(self, y, w: int, h: int, q, n: int, max_sse: int | None = None,
                             psnr: float | None = None, rle: bool = True, huffman: bool = True,
                             mode: int = MODE_FAST):
        """An image file with the coarsest probed scale of ``q`` whose distortion -- the squared
        error of the decoded pixels, :meth:`probe_rd` -- is at most ``max_sse``
        (ieh_encode_image_quality): ``(bytes, percent, sse)``.  Exactly one of ``max_sse`` and
        ``psnr`` (dB, turned into a squared error by :func:`sse_for_psnr`) is given.  Raises
        ``IEError(IE_ECAP, ...)`` (``e.percent`` = 25) when no scale meets it.  The codec's matrix
        afterwards is the chosen one."""
        if (max_sse is None) == (psnr is None):
            raise IEError(IE_EINVAL, "encode_image_quality: give exactly one of max_sse and psnr")
        if max_sse is None:
            max_sse = sse_for_psnr(psnr, w * h)
        H = load_host_library()
        q = np.ascontiguousarray(np.asarray(q, dtype=np.uint16).ravel())
        cap = stream_bound(w, h, n, 1, 2048) + 64
        out = np.zeros(cap, dtype=np.uint8)
        pc, se = C.c_int(0), C.c_uint64(0)
        r = H.ieh_encode_image_quality(self.h, _ptr(y), w, h, q.ctypes.data, n, int(rle), int(huffman), mode,
                                       min(max(int(max_sse), 0), 2 ** 64 - 1), out.ctypes.data, cap, C.byref(pc),
                                       C.byref(se))
        if r < 0:
            e = IEError(int(r), self.L.ie_last_error(self.h).decode())
            e.percent = int(pc.value)
            raise e
        self.n = n
        return out[: int(r)].tobytes(), int(pc.value), int(se.value)

    def encode_video_budget(self, yuv, w: int, h: int, q, n: int, budget: int, gop: int = 1, merange: int = 0,
                            rle: bool = True, huffman: bool = True, mode: int = MODE_FAST):
        """A video file (as :meth:`encode_video_file` writes it) with the finest probed scale of
        ``q`` whose size -- header + the frames' payload, before the Huffman pass -- fits ``budget``
        bytes (ieh_encode_video_budget, sized by :meth:`probe_gop`): ``(bytes, percent)``.  Raises
        ``IEError(IE_ECAP, ...)`` (``e.percent`` = 5382) when no scale fits.  The codec's matrix
        afterwards is the chosen one."""
        H = load_host_library()
        q = np.ascontiguousarray(np.asarray(q, dtype=np.uint16).ravel())
        frames = _nbytes(yuv) // (w * h + w * h // 2)
        cap = stream_bound(w, h, n, max(frames, 1), 2048) + (w // 16) * (h // 16) * 4 * max(frames, 1) + 64
        out = np.zeros(cap, dtype=np.uint8)
        pc = C.c_int(0)
        r = H.ieh_encode_video_budget(self.h, _ptr(yuv), _nbytes(yuv), w, h, q.ctypes.data, n, int(rle), int(huffman),
                                      gop, merange, mode, int(budget), out.ctypes.data, cap, C.byref(pc))
        if r < 0:
            e = IEError(int(r), self.L.ie_last_error(self.h).decode())
            e.percent = int(pc.value)
            raise e
        self.n = n
        return out[: int(r)].tobytes(), int(pc.value)

    def encode_video_quality(self, yuv, w: int, h: int, q, n: int, max_sse: int | None = None,
                             psnr: float | None = None, gop: int = 1, merange: int = 0, motioncomp: bool = True,
                             rle: bool = True, huffman: bool = True, mode: int = MODE_FAST):
        """A video file (as :meth:`encode_video_file` writes it) with the coarsest probed scale of
        ``q`` whose distortion -- the squared error of the decoded Y planes of all frames for a decoder
        run with this ``motioncomp``, :meth:`probe_gop_rd` -- is at most ``max_sse``
        (ieh_encode_video_quality): ``(bytes, percent, sse, frame_sse)``, ``frame_sse`` a uint64
        array with every frame's share of ``sse``.  Exactly one of ``max_sse`` and ``psnr`` (dB,
        turned into a squared error over ``frames * w * h`` pixels by :func:`sse_for_psnr`) is given.
        Raises ``IEError(IE_ECAP, ...)`` (``e.percent`` = 25) when no scale meets it.  The codec's
        matrix afterwards is the chosen one."""
        if (max_sse is None) == (psnr is None):
            raise IEError(IE_EINVAL, "encode_video_quality: give exactly one of max_sse and psnr")
        frames = _nbytes(yuv) // (w * h + w * h // 2)
        if max_sse is None:
            max_sse = sse_for_psnr(psnr, frames * w * h)
        H = load_host_library()
        q = np.ascontiguousarray(np.asarray(q, dtype=np.uint16).ravel())
        cap = stream_bound(w, h, n, max(frames, 1), 2048) + (w // 16) * (h // 16) * 4 * max(frames, 1) + 64
        out = np.zeros(cap, dtype=np.uint8)
        pc, se = C.c_int(0), C.c_uint64(0)
        fse = np.zeros(max(frames, 1), dtype=np.uint64)
        r = H.ieh_encode_video_quality(self.h, _ptr(yuv), _nbytes(yuv), w, h, q.ctypes.data, n, int(rle), int(huffman),
                                       gop, merange, int(motioncomp), mode, min(max(int(max_sse), 0), 2 ** 64 - 1),
                                       out.ctypes.data, cap, C.byref(pc), C.byref(se),
                                       fse.ctypes.data_as(C.POINTER(C.c_uint64)))
        if r < 0:
            e = IEError(int(r), self.L.ie_last_error(self.h).decode())
            e.percent = int(pc.value)
            raise e
        self.n = n
        return out[: int(r)].tobytes(), int(pc.value), int(se.value), fse[:frames]

    def encode_video_file(self, yuv, w: int, h: int, q, n: int, rle: bool = True, huffman: bool = True,
                          merange: int = 0, mode: int = MODE_FAST, gop: int = 1) -> bytes:
        """A video file as VideoEncoder writes it; gop > 1 adds P-frames (motion search + coded
        prediction error, Frame.cpp:160-243)."""
        H = load_host_library()
        q = np.ascontiguousarray(np.asarray(q, dtype=np.uint16).ravel())
        frames = _nbytes(yuv) // (w * h + w * h // 2)
        cap = stream_bound(w, h, n, max(frames, 1), 2048) + (w // 16) * (h // 16) * 4 * max(frames, 1) + 64
        out = np.zeros(cap, dtype=np.uint8)
        r = self._host_chk(H.ieh_encode_video_gop(self.h, _ptr(yuv), _nbytes(yuv), w, h, q.ctypes.data, n, int(rle),
                                                  int(huffman), gop, merange, mode, out.ctypes.data, cap))
        return out[:r].tobytes()

    def decode_image_file(self, data: bytes, n: int):
        """Pixels (h, w) uint8 of an encoded image file (ImageDecoder)."""
        H = load_host_library()
        src = np.frombuffer(data, dtype=np.uint8).copy()
        w, h = C.c_int(0), C.c_int(0)
        cap = 32767 * 32767
        # size from the header first: decode into a small buffer to learn w, h
        r = H.ieh_decode_image(self.h, src.ctypes.data, src.size, n, src.ctypes.data, 0, C.byref(w), C.byref(h))
        if r != IE_ECAP:
            self._host_chk(r)
        cap = w.value * h.value
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        r = self._host_chk(H.ieh_decode_image(self.h, src.ctypes.data, src.size, n, out.ctypes.data, cap, C.byref(w),
                                              C.byref(h)))
        return out[:r].reshape(h.value, w.value)

    def decode_image_file_region(self, file_bytes: bytes, rect, n: int | None = None) -> np.ndarray:
        """Pixels ``(rh, rw)`` uint8 of the rectangle ``rect = (x0, y0, rw, rh)`` of an encoded image
        file (ieh_decode_image_region): that crop of what :meth:`decode_image_file` returns.  ``n``:
        the file's block size (the file does not record it); default: the codec's current one.
        Raises :class:`IEError` (``IE_EINVAL``) for a rectangle that does not fit the image."""
        H = load_host_library()
        n = self.n if n is None else n
        if n is None:
            raise IEError(IE_EINVAL, "decode_image_file_region: no block size (pass n or set a matrix)")
        x0, y0, rw, rh = (int(v) for v in rect)
        src = np.frombuffer(file_bytes, dtype=np.uint8).copy()
        w, h = C.c_int(0), C.c_int(0)
        out = np.zeros(max(rw, 1) * max(rh, 1), dtype=np.uint8)
        r = self._host_chk(H.ieh_decode_image_region(self.h, src.ctypes.data, src.size, n, x0, y0, rw, rh, out.ctypes.data,
                                                     out.size, C.byref(w), C.byref(h)))
        self.n = n  # (the file's matrix is now the context's)
        return out[:r].reshape(rh, rw)

    def decode_image_file_scaled(self, file_bytes: bytes, scale: int, n: int | None = None) -> np.ndarray:
        """Pixels ``(h // scale, w // scale)`` uint8 of an encoded image file at ``1/scale`` of its
        size (ieh_decode_image_scaled): the rounded box means of what :meth:`decode_image_file`
        returns.  ``n``: the file's block size (the file does not record it); default: the codec's
        current one.  Raises :class:`IEError` (``IE_EINVAL``) for a scale that is not 1, 2, 4 or 8 or
        exceeds ``n``."""
        H = load_host_library()
        n = self.n if n is None else n
        if n is None:
            raise IEError(IE_EINVAL, "decode_image_file_scaled: no block size (pass n or set a matrix)")
        src = np.frombuffer(file_bytes, dtype=np.uint8).copy()
        w, h = C.c_int(0), C.c_int(0)
        # (the header gives the size: cap = 0 sizes the buffer, as for ieh_decode_image)
        r = H.ieh_decode_image_scaled(self.h, src.ctypes.data, src.size, n, scale, src.ctypes.data, 0, C.byref(w), C.byref(h))
        if r != IE_ECAP:
            self._host_chk(r)
        ow, oh = w.value // scale, h.value // scale
        out = np.zeros(ow * oh, dtype=np.uint8)
        r = self._host_chk(H.ieh_decode_image_scaled(self.h, src.ctypes.data, src.size, n, scale, out.ctypes.data, out.size,
                                                     C.byref(w), C.byref(h)))
        self.n = n  # (the file's matrix is now the context's)
        return out[:r].reshape(oh, ow)

    def decode_image_files(self, files: list[bytes], n: int) -> np.ndarray:
        """Pixels ``(count, h, w)`` uint8 of a batch of encoded image files that share their
        settings (ieh_decode_images): one batched Huffman decode into device slots, one batched
        record decode that reads them in place.  Raises :class:`IEError` naming the file when one
        is malformed or differs in its settings."""
        H = load_host_library()
        if not files:
            raise IEError(IE_EINVAL, "decode_image_files: no files")
        lens = np.array([len(f) for f in files], dtype=np.uint64)
        pitch = max((int(lens.max()) + 15) // 16 * 16, 16)
        src = np.zeros((len(files), pitch), dtype=np.uint8)
        for k, f in enumerate(files):
            src[k, : len(f)] = np.frombuffer(f, dtype=np.uint8)
        u64p = C.POINTER(C.c_uint64)
        w, h = C.c_int(0), C.c_int(0)
        # size from file 0's header first: w and h come back with IE_ECAP, before any record decode
        r = H.ieh_decode_images(self.h, src.ctypes.data, pitch, lens.ctypes.data_as(u64p), 1, n, src.ctypes.data, 0,
                                C.byref(w), C.byref(h))
        if r != IE_ECAP:
            self._host_chk(r)
        cap = len(files) * w.value * h.value
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        r = self._host_chk(H.ieh_decode_images(self.h, src.ctypes.data, pitch, lens.ctypes.data_as(u64p), len(files), n,
                                               out.ctypes.data, cap, C.byref(w), C.byref(h)))
        return out[:r].reshape(len(files), h.value, w.value)

    def decode_video_file(self, data: bytes, n: int):
        """Decoded YUV420 frames (Y + 0x80 UV fill), flat uint8, plus (w, h, frames)."""
        H = load_host_library()
        src = np.frombuffer(data, dtype=np.uint8).copy()
        w, h, f = C.c_int(0), C.c_int(0), C.c_int(0)
        r = H.ieh_decode_video(self.h, src.ctypes.data, src.size, n, src.ctypes.data, 0, C.byref(w), C.byref(h),
                               C.byref(f))
        if r != IE_ECAP:
            self._host_chk(r)
        cap = (w.value * h.value + w.value * h.value // 2) * f.value
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        r = self._host_chk(H.ieh_decode_video(self.h, src.ctypes.data, src.size, n, out.ctypes.data, cap, C.byref(w),
                                              C.byref(h), C.byref(f)))
        return out[:r], (w.value, h.value, f.value)

    def iter_video_file(self, data: bytes, n: int, motioncomp: bool = True, chunk_frames: int = 0):
        """The frames of an encoded video file chunk by chunk (ieh_vdec_*): yields
        ``(frames_in_chunk, ndarray)``, the array holding those frames in the file's layout (Y, then
        w*h/2 bytes of 0x80 each); all of them in order are :meth:`decode_video_file`'s bytes."""
        H = load_host_library()
        src = np.frombuffer(data, dtype=np.uint8).copy()
        w, h, f, gop, mer = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        v = C.c_void_p()
        self._host_chk(H.ieh_vdec_open(self.h, src.ctypes.data, src.size, n, int(motioncomp), chunk_frames, C.byref(w),
                                       C.byref(h), C.byref(f), C.byref(gop), C.byref(mer), C.byref(v)))
        self.n = n
        try:
            pitch = w.value * h.value + w.value * h.value // 2
            if chunk_frames > 0:
                k = chunk_frames
            else:
                mb = os.environ.get("IE_CHUNK_MB")
                target = int(float(mb) * 1048576) if mb and float(mb) > 0 else 8 << 20
                k = max(1, target // max(1, w.value * h.value))
            k = max(1, min(k, f.value))
            done = 0
            while done < f.value and pitch:
                buf = np.zeros(k * pitch, dtype=np.uint8)
                got = C.c_int(0)
                self._host_chk(H.ieh_vdec_next(v, buf.ctypes.data, buf.size, C.byref(got)))
                if got.value == 0:
                    break
                done += got.value
                yield got.value, buf[: got.value * pitch]
        finally:
            H.ieh_vdec_close(v)

    def huffman_encode_device(self, data, nbytes: int, out) -> int:
        """Huffman pass from device ``data[:nbytes]`` into device ``out``; returns output bytes."""
        H = load_host_library()
        return self._host_chk(H.ieh_huffman_encode_device(self.h, _ptr(data), nbytes, _ptr(out), _nbytes(out)))

    def huffman_encode_batch(self, data, in_pitch: int, sizes, out, out_pitch: int) -> list[int]:
        """Huffman pass over a batch of device strings (string k: ``sizes[k]`` bytes at
        ``data + k*in_pitch``) into device ``out + k*out_pitch``: one histogram launch, host tree
        builds, one pack launch (asynchronous on the context's stream).  Returns output bytes."""
        H = load_host_library()
        k = len(sizes)
        n = np.asarray(sizes, dtype=np.uint64)
        nb = np.zeros(k, dtype=np.int64)
        self._host_chk(H.ieh_huffman_encode_device_batch(self.h, _ptr(data), in_pitch, n.ctypes.data, k, _ptr(out),
                                                         out_pitch, nb.ctypes.data))
        return [int(v) for v in nb]

    def huffman_encode_after_encode(self, out, out_pitch: int, count: int, hout, hpitch: int) -> list[int]:
        """The batched Huffman pass over the ``count`` images the last :meth:`encode_images` call
        wrote to device ``out`` (lengths from the encoder's end bits, on the device: no size
        read-back).  Returns the Huffman output bytes per image."""
        H = load_host_library()
        nb = np.zeros(count, dtype=np.int64)
        self._host_chk(H.ieh_huffman_encode_after_encode(self.h, _ptr(out), out_pitch, count, _ptr(hout), hpitch,
                                                         nb.ctypes.data))
        return [int(v) for v in nb]

    def huffman_begin_after_encode(self, out, out_pitch: int, count: int, slot: int) -> None:
        """First half of :meth:`huffman_encode_after_encode` for pipelining batches: launches the
        histogram of the last :meth:`encode_images` output and returns (read-back into ``slot``,
        0 or 1).  Finish it with :meth:`huffman_finish_after_encode` on the same arguments after
        issuing the next batch's encode and begin."""
        H = load_host_library()
        self._host_chk(H.ieh_huffman_begin_after_encode(self.h, _ptr(out), out_pitch, count, slot))

    def huffman_finish_after_encode(self, out, out_pitch: int, count: int, slot: int, hout, hpitch: int) -> list[int]:
        """Second half: trees for the batch begun in ``slot``, then the pack launch into ``hout``.
        Returns the Huffman output bytes per image (``out`` must still hold that batch)."""
        H = load_host_library()
        nb = np.zeros(count, dtype=np.int64)
        self._host_chk(H.ieh_huffman_finish_after_encode(self.h, _ptr(out), out_pitch, count, slot, _ptr(hout), hpitch,
                                                         nb.ctypes.data))
        return [int(v) for v in nb]

    def huffman_hist_after_encode(self, out, out_pitch: int, count: int):
        """(hist [count, 256] uint32, first [count, 256] uint64) of the images the last encode
        wrote (counts fused into the encoder when it ran with count_bytes=True)."""
        u64p = C.POINTER(C.c_uint64)
        ends = C.cast(C.c_void_p(self.L.ie_last_end_bits(self.h)), u64p)
        self._chk(self.L.ie_huffman_hist_batch_ends_async(self.h, _ptr(out), out_pitch, ends, count, 0))
        hist = np.zeros((count, 256), dtype=np.uint32)
        first = np.zeros((count, 256), dtype=np.uint64)
        self._chk(self.L.ie_huffman_hist_batch_wait(self.h, 0, hist.ctypes.data, first.ctypes.data))
        return hist, first

    def huffman_table(self, data: bytes):
        """(lut uint16[32768], start_bit) of a Huffman-coded stream's dictionary, or None when the
        stream has none (passthrough)."""
        H = load_host_library()
        src = np.frombuffer(data, dtype=np.uint8)
        lut = np.zeros(32768, dtype=np.uint16)
        sb = C.c_uint64(0)
        r = H.ieh_huffman_table(src.ctypes.data, src.size, lut.ctypes.data, C.byref(sb))
        if r < 0:
            raise IEError(r, "ieh_huffman_table")
        return None if r == 1 else (lut, int(sb.value))

    def huffman_decode_device(self, stream, nbytes: int, lut, start_bit: int, out) -> int:
        """ie_huffman_decode with device-resident stream / table / output (torch tensors): the
        symbol count (raises on IE_ECAP / malformed streams)."""
        n = C.c_size_t(0)
        self._chk(self.L.ie_huffman_decode(self.h, _ptr(stream), nbytes, start_bit, _ptr(lut), _ptr(out),
                                           _nbytes(out), C.byref(n)))
        return int(n.value)

    def huffman_decode_batch(self, streams, in_pitch: int, lens, start_bits, luts, out, out_pitch: int) -> np.ndarray:
        """ie_huffman_decode_batch: ``len(lens)`` code streams in one set of launches.  Stream k is
        ``lens[k]`` bytes at ``streams + k*in_pitch``, its code stream from bit ``start_bits[k]``,
        its prefix table at ``luts + 32768*k`` (uint16); its symbols go to ``out + k*out_pitch``.
        ``streams``/``luts``/``out``: numpy arrays (host) or torch tensors (device).  Returns the
        symbol counts (uint64, one per stream); raises :class:`IEError` (``IE_EFORMAT`` /
        ``IE_ECAP``, the message names the lowest failing image, ``e.counts`` holds the counts) --
        the other images are decoded all the same."""
        ln = np.ascontiguousarray(lens, dtype=np.uint64)
        sb = np.ascontiguousarray(start_bits, dtype=np.uint64)
        if sb.size != ln.size:
            raise IEError(IE_EINVAL, "huffman_decode_batch: lens and start_bits differ in length")
        nout = np.zeros(max(ln.size, 1), dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        r = self.L.ie_huffman_decode_batch(self.h, _ptr(streams), in_pitch, ln.ctypes.data_as(u64p), int(ln.size),
                                           sb.ctypes.data_as(u64p), _ptr(luts), _ptr(out), out_pitch,
                                           nout.ctypes.data_as(u64p))
        if r != IE_OK:
            e = IEError(int(r), self.L.ie_last_error(self.h).decode())
            e.counts = nout[: ln.size]
            raise e
        return nout[: ln.size]

    def huffman_decode(self, data: bytes):
        """The Huffman decode alone (device bit walk): (decoded bytes, passthrough)."""
        H = load_host_library()
        src = np.frombuffer(bytes(data), dtype=np.uint8).copy()
        cap = 8 * src.size + 16
        out = np.zeros(cap, dtype=np.uint8)
        pt = C.c_int(0)
        r = self._host_chk(H.ieh_huffman_decode(self.h, src.ctypes.data, src.size, out.ctypes.data, cap, C.byref(pt)))
        return out[:r].tobytes(), bool(pt.value)

    def huffman_encode(self, data) -> bytes:
        """The Huffman post-pass alone (host or device input)."""
        H = load_host_library()
        n = _nbytes(data)
        cap = 4 * n + 4096
        out = np.zeros(cap, dtype=np.uint8)
        r = self._host_chk(H.ieh_huffman_encode(self.h, _ptr(data), n, out.ctypes.data, cap))
        return out[:r].tobytes()
