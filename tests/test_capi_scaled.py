"""CPU check of the scaled decode's boundaries: include/ie_hip.h declares ie_decode_scaled and
ie_decode_images_scaled with the documented parameter lists, the built library exports them, the
ctypes binding declares the same signatures, Codec has the three methods, and libie_host.so exports
ieh_decode_image_scaled (no compute call -- there may be no GPU here).  And a check of the GPU
tests' own expected value: the box mean of tests/scaled_common.py on the oracle's decoded pixels of
the noise streams those tests decode must hold exact ties, so that a kernel which truncates or
rounds ties to even cannot pass them."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import scaled_common as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTYPES = {"ie_ctx*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "size_t": C.c_size_t,
          "const uint64_t*": C.POINTER(C.c_uint64), "uint64_t*": C.POINTER(C.c_uint64), "int": C.c_int,
          "uint64_t": C.c_uint64}
PARAMS = {
    "ie_decode_scaled": [("ie_ctx*", "ctx"), ("const uint8_t*", "in"), ("size_t", "len"), ("uint64_t", "start_bit"),
                         ("int", "w"), ("int", "h"), ("int", "nframes"), ("int", "use_rle"), ("int", "scale"),
                         ("uint8_t*", "out"), ("size_t", "stride"), ("size_t", "frame_pitch"), ("uint64_t*", "end_bit")],
    "ie_decode_images_scaled": [("ie_ctx*", "ctx"), ("const uint8_t*", "in"), ("size_t", "in_pitch"),
                                ("const uint64_t*", "nbits"), ("int", "count"), ("uint64_t", "start_bit"), ("int", "w"),
                                ("int", "h"), ("int", "use_rle"), ("int", "scale"), ("uint8_t*", "out"),
                                ("size_t", "stride"), ("size_t", "frame_pitch"), ("uint64_t*", "end_bits")],
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


def test_codec_has_the_scaled_methods():
    from imageencoder_amd import Codec
    sig = inspect.signature(Codec.decode_scaled)
    assert list(sig.parameters) == ["self", "stream", "w", "h", "scale", "out", "start_bit", "nframes", "rle", "stride",
                                    "frame_pitch"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["out"], d["start_bit"], d["nframes"], d["rle"], d["stride"], d["frame_pitch"]) == (None, 0, 1, True, None, None)
    sig = inspect.signature(Codec.decode_images_scaled)
    assert list(sig.parameters) == ["self", "streams", "in_pitch", "nbits", "w", "h", "scale", "out", "start_bit", "rle",
                                    "stride", "frame_pitch"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["out"], d["start_bit"], d["rle"], d["stride"], d["frame_pitch"]) == (None, 0, True, None, None)
    sig = inspect.signature(Codec.decode_image_file_scaled)
    assert list(sig.parameters) == ["self", "file_bytes", "scale", "n"]
    assert sig.parameters["n"].default is None


def test_host_library_exports_decode_image_scaled():
    from imageencoder_amd import HOST_LIB_PATH as path, load_host_library
    assert os.path.exists(path), "libie_host.so not built"
    assert hasattr(C.CDLL(path), "ieh_decode_image_scaled")
    src = open(os.path.join(ROOT, "include", "ie_host.hpp")).read()
    m = re.search(r"^int64_t\s+ieh_decode_image_scaled\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m
    assert [p.strip().rsplit(" ", 1)[1] for p in m.group(1).split(",")] == ["ctx", "enc", "len", "n", "scale", "out", "cap",
                                                                            "w", "h"]
    fn = load_host_library().ieh_decode_image_scaled
    assert fn.restype is C.c_int64 and len(fn.argtypes) == 9


def test_box_is_the_rounded_mean():
    """The helper itself, on values worked out by hand: ties go up, sums are exact at 0 and 255."""
    a = np.array([[0, 1], [0, 1]], dtype=np.uint8)  # sum 2 of 4: the tie, 0.5 -> 1
    assert SC.box(a, 2).tolist() == [[1]]
    a = np.array([[1, 0], [0, 0]], dtype=np.uint8)  # 0.25 -> 0
    assert SC.box(a, 2).tolist() == [[0]]
    a = np.array([[1, 1], [1, 0]], dtype=np.uint8)  # 0.75 -> 1
    assert SC.box(a, 2).tolist() == [[1]]
    a = np.array([[2, 1], [1, 2]], dtype=np.uint8)  # 1.5 -> 2 (round-to-even would also give 2) ...
    b = np.array([[3, 2], [2, 3]], dtype=np.uint8)  # ... 2.5 -> 3 (round-to-even gives 2)
    assert SC.box(a, 2).tolist() == [[2]] and SC.box(b, 2).tolist() == [[3]]
    for v in (0, 128, 255):
        for s in (1, 2, 4, 8):
            assert (SC.box(np.full((3, 16, 24), v, dtype=np.uint8), s) == v).all()
    x = np.arange(2 * 8 * 16, dtype=np.uint8).reshape(2, 8, 16)
    assert np.array_equal(SC.box(x, 1), x)
    assert SC.box(x, 4).shape == (2, 2, 4)


@pytest.mark.parametrize("nframes", [1, 3])
@pytest.mark.parametrize("shape", [(4, 320, 240), (8, 512, 256)], ids=["n4_320x240", "n8_512x256"])
def test_noise_streams_hold_ties_and_both_sides(shape, nframes):
    """At each legal scale the expected picture of the noise streams the GPU tests decode has a
    cell whose sum is an exact tie (sum % s^2 == s^2/2: half up differs from truncation, and an odd
    quotient there differs from round-to-even), one above and one below it."""
    from tests import oracle_lib as O
    n, w, h = shape
    o = O.load()
    q = O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n)
    y = SC.frames("U", w, h, nframes, SC.stream_seed(w, nframes))
    full = np.stack([np.asarray(o.decode_image(o.encode_image(f, n, q, rle=True), n)).reshape(h, w) for f in y])
    for s in SC.scales(n):
        if s == 1:
            assert np.array_equal(SC.box(full, 1), full)
            continue
        sums = SC.box_sums(full, s)
        rem, half = sums % (s * s), s * s // 2
        assert (rem == half).any() and (rem > half).any() and (rem < half).any(), s
        # a tie whose truncated mean is even: round-half-even would give one less than half up
        assert ((rem == half) & ((sums // (s * s)) % 2 == 0)).any(), s
        exp = SC.box(full, s)
        assert np.array_equal(exp[rem == half], (sums // (s * s) + 1)[rem == half])
        assert (exp != (sums // (s * s))).any()  # truncation differs
