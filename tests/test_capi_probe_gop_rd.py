"""CPU checks of the video quality-target boundary: include/ie_hip.h declares ie_probe_gop_rd and
include/ie_host.hpp declares ieh_encode_video_quality with the documented parameter lists, the built
libraries export them, the ctypes bindings declare the same types, and Codec.probe_gop_rd /
Codec.encode_video_quality have the documented parameters and defaults (no compute call: there may
be no GPU here)."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C parameter type -> the ctypes type the binding must declare (pointers travel as void pointers,
# as for every other entry point of the bindings, except the 64-bit result arrays)
CTYPES = {"ie_ctx*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "size_t": C.c_size_t,
          "const uint16_t*": C.c_void_p, "uint64_t*": C.POINTER(C.c_uint64), "int": C.c_int, "int*": C.POINTER(C.c_int),
          "uint64_t": C.c_uint64}

PROBE_GOP_RD = [("ie_ctx*", "ctx"), ("const uint8_t*", "y"), ("int", "w"), ("int", "h"), ("size_t", "stride"),
                ("size_t", "frame_pitch"), ("int", "nframes"), ("int", "gop"), ("int", "merange"), ("int", "use_rle"),
                ("int", "motioncomp"), ("const uint16_t*", "q"), ("int", "nq"), ("uint64_t*", "bits"), ("uint64_t*", "sse")]
VIDEO_QUALITY = [("ie_ctx*", "ctx"), ("const uint8_t*", "yuv"), ("size_t", "len"), ("int", "w"), ("int", "h"),
                 ("const uint16_t*", "base"), ("int", "n"), ("int", "rle"), ("int", "huffman"), ("int", "gop"),
                 ("int", "merange"), ("int", "motioncomp"), ("int", "mode"), ("uint64_t", "max_sse"), ("uint8_t*", "out"),
                 ("size_t", "cap"), ("int*", "percent"), ("uint64_t*", "sse"), ("uint64_t*", "frame_sse")]


def _declaration(header, ret, name):
    src = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(rf"^{ret}\s+{name}\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, f"include/{header} does not declare {name}"
    params = []
    for p in m.group(1).split(","):
        t, pname = p.strip().rsplit(" ", 1)
        params.append((re.sub(r"\s+", " ", t.strip()), pname))
    return params


def test_headers_declare_the_entry_points():
    assert _declaration("ie_hip.h", "int", "ie_probe_gop_rd") == PROBE_GOP_RD
    assert _declaration("ie_host.hpp", "int64_t", "ieh_encode_video_quality") == VIDEO_QUALITY


def test_libraries_export_them_with_the_binding_signatures():
    from imageencoder_amd import HOST_LIB_PATH, LIB_PATH, load_host_library, load_library
    assert os.path.exists(LIB_PATH), "libie_hip.so not built"
    assert os.path.exists(HOST_LIB_PATH), "libie_host.so not built"
    assert hasattr(C.CDLL(LIB_PATH), "ie_probe_gop_rd")
    fn = load_library().ie_probe_gop_rd
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [CTYPES[t] for t, _ in PROBE_GOP_RD]
    assert hasattr(C.CDLL(HOST_LIB_PATH), "ieh_encode_video_quality")
    fn = load_host_library().ieh_encode_video_quality
    assert fn.restype is C.c_int64
    # (the binding passes the 64-bit result arrays as typed pointers, every other pointer as void*)
    assert list(fn.argtypes) == [CTYPES[t] for t, _ in VIDEO_QUALITY]


def test_codec_has_the_methods():
    import imageencoder_amd as ie
    sig = inspect.signature(ie.Codec.probe_gop_rd)
    assert list(sig.parameters) == ["self", "y", "w", "h", "qs", "gop", "merange", "nframes", "rle", "motioncomp",
                                    "stride", "frame_pitch", "out"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["gop"] is inspect.Parameter.empty and d["merange"] is inspect.Parameter.empty
    assert d["nframes"] == 1 and d["rle"] is True and d["motioncomp"] is True
    assert d["stride"] is None and d["frame_pitch"] is None and d["out"] is None
    sig = inspect.signature(ie.Codec.encode_video_quality)
    assert list(sig.parameters) == ["self", "yuv", "w", "h", "q", "n", "max_sse", "psnr", "gop", "merange", "motioncomp",
                                    "rle", "huffman", "mode"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["max_sse"] is None and d["psnr"] is None
    assert d["gop"] == 1 and d["merange"] == 0 and d["motioncomp"] is True
    assert d["rle"] is True and d["huffman"] is True and d["mode"] == ie.MODE_FAST
