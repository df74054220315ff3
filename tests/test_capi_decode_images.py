"""CPU check of the batch decode's C-ABI boundary: include/ie_hip.h declares ie_decode_images with
the documented parameter list, the built library exports it, and the ctypes binding declares the
same signature (no compute call -- there may be no GPU here)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C parameter type -> the ctypes type the binding must declare (pointers to bytes and the context
# travel as void pointers, as for every other entry point of the binding)
CTYPES = {"ie_ctx*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "size_t": C.c_size_t,
          "const uint64_t*": C.POINTER(C.c_uint64), "uint64_t*": C.POINTER(C.c_uint64), "int": C.c_int,
          "uint64_t": C.c_uint64}
PARAMS = [("ie_ctx*", "ctx"), ("const uint8_t*", "in"), ("size_t", "in_pitch"), ("const uint64_t*", "nbits"),
          ("int", "count"), ("uint64_t", "start_bit"), ("int", "w"), ("int", "h"), ("int", "use_rle"),
          ("uint8_t*", "out"), ("size_t", "stride"), ("size_t", "frame_pitch"), ("uint64_t*", "end_bits")]


def _declaration():
    src = open(os.path.join(ROOT, "include", "ie_hip.h")).read()
    m = re.search(r"^int\s+ie_decode_images\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "include/ie_hip.h does not declare ie_decode_images"
    params = []
    for p in m.group(1).split(","):
        t, name = p.strip().rsplit(" ", 1)
        params.append((re.sub(r"\s+", " ", t.strip()), name))
    return params


def test_header_declares_decode_images():
    assert _declaration() == PARAMS


def test_library_exports_decode_images_with_the_binding_signature():
    from imageencoder_amd import LIB_PATH, load_library
    assert os.path.exists(LIB_PATH), "libie_hip.so not built"
    assert hasattr(C.CDLL(LIB_PATH), "ie_decode_images")
    fn = load_library().ie_decode_images
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [CTYPES[t] for t, _ in _declaration()]


def test_codec_has_decode_images():
    import inspect

    from imageencoder_amd import Codec
    sig = inspect.signature(Codec.decode_images)
    assert list(sig.parameters) == ["self", "streams", "in_pitch", "nbits", "w", "h", "out", "start_bit", "rle",
                                    "stride", "frame_pitch"]
    assert sig.parameters["start_bit"].default == 0 and sig.parameters["rle"].default is True
