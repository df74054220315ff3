"""CPU check of the streamed video decoder's boundaries: include/ie_hip.h declares ie_vdec_open /
next / info / close, the built libie_hip.so exports them and libie_host.so the ieh_vdec_* functions,
the ctypes bindings declare as many parameters as the headers, and Codec.open_video_decode has the
documented defaults (no compute call -- there may be no GPU here)."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VDEC = {
    "ie_vdec_open": ["ie_ctx* ctx", "const uint8_t* in", "size_t len", "uint64_t start_bit", "int w", "int h",
                     "int nframes", "int gop", "int merange", "int use_rle", "int motioncomp", "int chunk_frames",
                     "ie_vdec** out"],
    "ie_vdec_next": ["ie_vdec* v", "uint8_t* out", "size_t stride", "size_t frame_pitch", "int max_frames", "int* got"],
    "ie_vdec_info": ["const ie_vdec* v", "int* chunk_frames", "int* chunks_enqueued", "int* chunks_delivered",
                     "uint64_t* end_bit"],
    "ie_vdec_close": ["ie_vdec* v"],
}
HOST = ["ieh_vdec_open", "ieh_vdec_next", "ieh_vdec_close"]


def _params(header, name):
    src = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
    assert m, f"include/{header} does not declare {name}"
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(VDEC))
def test_header_declares(name):
    assert _params("ie_hip.h", name) == VDEC[name]


def test_header_opens_like_decode_gop():
    """ie_decode_gop's arguments up to motioncomp, then chunk_frames and the handle in place of the
    pixel destination."""
    gop = _params("ie_hip.h", "ie_decode_gop")
    at = gop.index("int motioncomp") + 1
    assert _params("ie_hip.h", "ie_vdec_open") == gop[:at] + ["int chunk_frames", "ie_vdec** out"]


def test_libraries_export_the_functions():
    from imageencoder_amd import HOST_LIB_PATH, LIB_PATH
    assert os.path.exists(LIB_PATH), "libie_hip.so not built"
    lib = C.CDLL(LIB_PATH)
    for name in VDEC:
        assert hasattr(lib, name), name
    assert os.path.exists(HOST_LIB_PATH), "libie_host.so not built"
    host = C.CDLL(HOST_LIB_PATH)
    for name in HOST:
        assert hasattr(host, name), name


def test_bindings_declare_the_header_signatures():
    from imageencoder_amd import load_host_library, load_library
    L = load_library()
    for name in VDEC:
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert len(fn.argtypes) == len(_params("ie_hip.h", name)), name
    # open: ie_decode_gop's leading arguments, then chunk_frames and the handle
    assert list(L.ie_vdec_open.argtypes[:11]) == list(L.ie_decode_gop.argtypes[:11])
    H = load_host_library()
    for name in HOST:
        fn = getattr(H, name)
        assert fn.restype is C.c_int
        assert len(fn.argtypes) == len(_params("ie_host.hpp", name)), name


def test_open_video_decode_defaults():
    from imageencoder_amd import Codec, VideoDecodeStream
    p = inspect.signature(Codec.open_video_decode).parameters
    assert list(p)[:5] == ["self", "stream", "w", "h", "nframes"]
    want = dict(gop=1, merange=0, start_bit=0, rle=True, motioncomp=True, chunk_frames=0)
    assert {k: p[k].default for k in want} == want
    for k in ("stream", "w", "h", "nframes"):
        assert p[k].default is inspect.Parameter.empty
    for m in ("next", "info", "close"):
        assert callable(getattr(VideoDecodeStream, m))
    n = inspect.signature(VideoDecodeStream.next).parameters
    assert list(n) == ["self", "out", "max_frames", "stride", "frame_pitch"]
    assert n["stride"].default is None and n["frame_pitch"].default is None
    it = inspect.signature(Codec.iter_video_file).parameters
    assert list(it) == ["self", "data", "n", "motioncomp", "chunk_frames"]
    assert it["motioncomp"].default is True and it["chunk_frames"].default == 0
