"""CPU checks of the rate-distortion boundary: include/ie_hip.h declares ie_probe_rd and
include/ie_host.hpp declares ieh_encode_image_quality with the documented parameter lists, the
built libraries export them, the ctypes bindings declare the same signatures, Codec has the two
methods, and the two PSNR helpers equal their formulas (no compute call: there may be no GPU here)."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C parameter type -> the ctypes type the binding must declare (pointers travel as void pointers,
# as for every other entry point of the bindings, except the 64-bit result arrays)
CTYPES = {"ie_ctx*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "size_t": C.c_size_t,
          "const uint16_t*": C.c_void_p, "uint64_t*": C.POINTER(C.c_uint64), "uint64_t": C.c_uint64, "int": C.c_int,
          "int*": C.POINTER(C.c_int)}

PROBE_RD = [("ie_ctx*", "ctx"), ("const uint8_t*", "y"), ("int", "w"), ("int", "h"), ("size_t", "stride"),
            ("size_t", "frame_pitch"), ("int", "nframes"), ("int", "use_rle"), ("const uint16_t*", "q"), ("int", "nq"),
            ("uint64_t*", "bits"), ("uint64_t*", "sse")]
QUALITY = [("ie_ctx*", "ctx"), ("const uint8_t*", "y"), ("int", "w"), ("int", "h"), ("const uint16_t*", "base"),
           ("int", "n"), ("int", "rle"), ("int", "huffman"), ("int", "mode"), ("uint64_t", "max_sse"),
           ("uint8_t*", "out"), ("size_t", "cap"), ("int*", "percent"), ("uint64_t*", "sse")]


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
    assert _declaration("ie_hip.h", "int", "ie_probe_rd") == PROBE_RD
    assert _declaration("ie_host.hpp", "int64_t", "ieh_encode_image_quality") == QUALITY


def test_libraries_export_them_with_the_binding_signatures():
    from imageencoder_amd import HOST_LIB_PATH, LIB_PATH, load_host_library, load_library
    assert os.path.exists(LIB_PATH), "libie_hip.so not built"
    assert os.path.exists(HOST_LIB_PATH), "libie_host.so not built"
    assert hasattr(C.CDLL(LIB_PATH), "ie_probe_rd")
    fn = load_library().ie_probe_rd
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [CTYPES[t] for t, _ in PROBE_RD]
    H = load_host_library()
    assert hasattr(C.CDLL(HOST_LIB_PATH), "ieh_encode_image_quality")
    assert H.ieh_encode_image_quality.restype is C.c_int64
    assert list(H.ieh_encode_image_quality.argtypes) == [CTYPES[t] for t, _ in QUALITY]


def test_codec_has_the_methods():
    import imageencoder_amd as ie
    sig = inspect.signature(ie.Codec.probe_rd)
    assert list(sig.parameters) == ["self", "y", "w", "h", "qs", "nframes", "rle", "stride", "frame_pitch", "out"]
    assert sig.parameters["nframes"].default == 1 and sig.parameters["rle"].default is True
    assert sig.parameters["out"].default is None
    sig = inspect.signature(ie.Codec.encode_image_quality)
    assert list(sig.parameters) == ["self", "y", "w", "h", "q", "n", "max_sse", "psnr", "rle", "huffman", "mode"]
    assert sig.parameters["max_sse"].default is None and sig.parameters["psnr"].default is None
    assert sig.parameters["rle"].default is True and sig.parameters["huffman"].default is True
    assert sig.parameters["mode"].default == ie.MODE_FAST
    assert list(inspect.signature(ie.sse_for_psnr).parameters) == ["psnr", "npixels"]
    assert list(inspect.signature(ie.psnr_of_sse).parameters) == ["sse", "npixels"]


def test_psnr_helpers_equal_their_formulas():
    from imageencoder_amd import psnr_of_sse, sse_for_psnr
    for psnr, n in ((30.0, 64 * 48), (40.0, 200 * 56), (20.0, 3840 * 2160), (48.13, 16), (10.0, 1)):
        exp = math.floor(n * 255.0 ** 2 / 10.0 ** (psnr / 10.0))
        got = sse_for_psnr(psnr, n)
        assert isinstance(got, int) and got == exp, (psnr, n)
    # 10 dB over one pixel: 255^2 / 10 = 6502.5; 20 dB over 100 pixels: 65025
    assert sse_for_psnr(10.0, 1) == 6502
    assert sse_for_psnr(20.0, 100) == 65025
    assert psnr_of_sse(0, 1234) == math.inf
    assert psnr_of_sse(65025, 100) == pytest.approx(20.0, abs=1e-12)
    for s, n in ((1, 16), (7, 3072), (65025, 100), (123456789, 3840 * 2160), (11200 * 65025, 11200)):
        assert psnr_of_sse(s, n) == pytest.approx(10.0 * math.log10(n * 255.0 ** 2 / s), abs=1e-12)
        assert abs(sse_for_psnr(psnr_of_sse(s, n), n) - s) <= 1, (s, n)
    # a coarser target allows a larger error
    assert sse_for_psnr(30.0, 4096) > sse_for_psnr(35.0, 4096) > sse_for_psnr(40.0, 4096) > 0
