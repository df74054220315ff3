"""CPU check of ie_vstream_open_gop's C-ABI boundary: the header declares it, the built library
exports it, the ctypes binding declares as many parameters as the header, and
Codec.open_video_stream takes gop and merange with defaults that keep the gop = 1 stream (no
compute call -- there may be no GPU here)."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(name):
    src = open(os.path.join(ROOT, "include", "ie_hip.h")).read()
    m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
    assert m, f"include/ie_hip.h does not declare {name}"
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_header_declares_vstream_open_gop():
    """ie_vstream_open's parameters with gop and merange in front of use_rle."""
    want = _params("ie_vstream_open")
    at = want.index("int use_rle")
    assert _params("ie_vstream_open_gop") == want[:at] + ["int gop", "int merange"] + want[at:]


def test_library_exports_vstream_open_gop():
    from imageencoder_amd import LIB_PATH
    assert os.path.exists(LIB_PATH), "libie_hip.so not built"
    assert hasattr(C.CDLL(LIB_PATH), "ie_vstream_open_gop")


def test_binding_declares_the_header_signature():
    from imageencoder_amd import load_library
    L = load_library()
    assert L.ie_vstream_open_gop.restype is C.c_int
    args = list(L.ie_vstream_open_gop.argtypes)
    assert len(args) == len(_params("ie_vstream_open_gop"))
    old = list(L.ie_vstream_open.argtypes)
    assert args == old[:5] + [C.c_int, C.c_int] + old[5:]


def test_open_video_stream_takes_gop_and_merange():
    from imageencoder_amd import Codec
    p = inspect.signature(Codec.open_video_stream).parameters
    assert p["gop"].default == 1 and p["merange"].default == 0
