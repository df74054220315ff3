"""CPU check of ie_encode_gop_groups' C-ABI boundary: the built library exports it, the ctypes
binding declares the signature the header gives (ie_encode_gop's), and Codec.encode_gop_groups has
the signature of Codec.encode_gop (no compute call -- there may be no GPU here)."""
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


def test_header_declares_encode_gop_groups_like_encode_gop():
    assert _params("ie_encode_gop_groups") == _params("ie_encode_gop")


def test_library_exports_encode_gop_groups_with_the_binding_signature():
    from imageencoder_amd import LIB_PATH, load_library
    assert os.path.exists(LIB_PATH), "libie_hip.so not built"
    assert hasattr(C.CDLL(LIB_PATH), "ie_encode_gop_groups")
    L = load_library()
    assert L.ie_encode_gop_groups.restype is C.c_int
    assert list(L.ie_encode_gop_groups.argtypes) == list(L.ie_encode_gop.argtypes)
    assert len(L.ie_encode_gop_groups.argtypes) == len(_params("ie_encode_gop_groups"))


def test_codec_has_encode_gop_groups():
    from imageencoder_amd import Codec
    a, b = inspect.signature(Codec.encode_gop_groups), inspect.signature(Codec.encode_gop)
    assert [(p.name, p.default) for p in a.parameters.values()] == [(p.name, p.default) for p in b.parameters.values()]
