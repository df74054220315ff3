"""CPU check of the region decode's boundaries: include/ie_hip.h declares ie_decode_region and
ie_decode_images_region with the documented parameter lists, the built library exports them, the
ctypes binding declares the same signatures, Codec has the three methods, and libie_host.so exports
ieh_decode_image_region (no compute call -- there may be no GPU here)."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTYPES = {"ie_ctx*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "size_t": C.c_size_t,
          "const uint64_t*": C.POINTER(C.c_uint64), "uint64_t*": C.POINTER(C.c_uint64), "int": C.c_int,
          "uint64_t": C.c_uint64}
RECT = [("int", "x0"), ("int", "y0"), ("int", "rw"), ("int", "rh")]
PARAMS = {
    "ie_decode_region": [("ie_ctx*", "ctx"), ("const uint8_t*", "in"), ("size_t", "len"), ("uint64_t", "start_bit"),
                         ("int", "w"), ("int", "h"), ("int", "nframes"), ("int", "use_rle")] + RECT +
                        [("uint8_t*", "out"), ("size_t", "stride"), ("size_t", "frame_pitch"), ("uint64_t*", "end_bit")],
    "ie_decode_images_region": [("ie_ctx*", "ctx"), ("const uint8_t*", "in"), ("size_t", "in_pitch"),
                                ("const uint64_t*", "nbits"), ("int", "count"), ("uint64_t", "start_bit"), ("int", "w"),
                                ("int", "h"), ("int", "use_rle")] + RECT +
                               [("uint8_t*", "out"), ("size_t", "stride"), ("size_t", "frame_pitch"),
                                ("uint64_t*", "end_bits")],
}


def _declaration(name):
    src = open(os.path.join(ROOT, "include", "ie_hip.h")).read()
    m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
    assert m, f"include/ie_hip.h does not declare {name}"
    params = []
    for p in m.group(1).split(","):
        t, pname = p.strip().rsplit(" ", 1)
        params.append((re.sub(r"\s+", " ", t.strip()), pname))
    return params


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_header_declares(name):
    assert _declaration(name) == PARAMS[name]


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_library_exports_with_the_binding_signature(name):
    from imageencoder_amd import LIB_PATH, load_library
    assert os.path.exists(LIB_PATH), "libie_hip.so not built"
    assert hasattr(C.CDLL(LIB_PATH), name)
    fn = getattr(load_library(), name)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [CTYPES[t] for t, _ in _declaration(name)]


def test_codec_has_the_region_methods():
    from imageencoder_amd import Codec
    sig = inspect.signature(Codec.decode_region)
    assert list(sig.parameters) == ["self", "stream", "w", "h", "rect", "out", "start_bit", "nframes", "rle", "stride",
                                    "frame_pitch"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["out"], d["start_bit"], d["nframes"], d["rle"], d["stride"], d["frame_pitch"]) == (None, 0, 1, True, None, None)
    sig = inspect.signature(Codec.decode_images_region)
    assert list(sig.parameters) == ["self", "streams", "in_pitch", "nbits", "w", "h", "rect", "out", "start_bit", "rle",
                                    "stride", "frame_pitch"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["out"], d["start_bit"], d["rle"], d["stride"], d["frame_pitch"]) == (None, 0, True, None, None)
    sig = inspect.signature(Codec.decode_image_file_region)
    # (the file does not record its block size: the optional n defaults to the codec's current one)
    assert list(sig.parameters)[:3] == ["self", "file_bytes", "rect"]
    assert all(p.default is not inspect.Parameter.empty for p in list(sig.parameters.values())[3:])


def test_host_library_exports_decode_image_region():
    from imageencoder_amd import HOST_LIB_PATH as path
    assert os.path.exists(path), "libie_host.so not built"
    assert hasattr(C.CDLL(path), "ieh_decode_image_region")
    src = open(os.path.join(ROOT, "include", "ie_host.hpp")).read()
    assert re.search(r"^int64_t\s+ieh_decode_image_region\s*\(", src, flags=re.M)
