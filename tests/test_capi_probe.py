"""CPU checks of the rate-control boundary: include/ie_hip.h declares ie_probe_sizes and
include/ie_host.hpp declares ieh_scale_matrix, ieh_budget_ladder and ieh_encode_image_budget with
the documented parameter lists, the built libraries export them, the ctypes bindings declare the
same signatures, and the two entry points that need no GPU -- the matrix scaling and the search's
ladder -- equal their integer formulas (no compute call: there may be no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import matrix_sweep as MS
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C parameter type -> the ctypes type the binding must declare (pointers travel as void pointers,
# as for every other entry point of the bindings, except the 64-bit result arrays)
CTYPES = {"ie_ctx*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "size_t": C.c_size_t,
          "const uint16_t*": C.c_void_p, "uint16_t*": C.c_void_p, "uint64_t*": C.POINTER(C.c_uint64), "int": C.c_int,
          "int*": C.POINTER(C.c_int)}

PROBE = [("ie_ctx*", "ctx"), ("const uint8_t*", "y"), ("int", "w"), ("int", "h"), ("size_t", "stride"),
         ("size_t", "frame_pitch"), ("int", "nframes"), ("int", "use_rle"), ("const uint16_t*", "q"), ("int", "nq"),
         ("uint64_t*", "bits")]
SCALE = [("const uint16_t*", "base"), ("int", "n"), ("int", "percent"), ("uint16_t*", "out")]
BUDGET = [("ie_ctx*", "ctx"), ("const uint8_t*", "y"), ("int", "w"), ("int", "h"), ("const uint16_t*", "base"),
          ("int", "n"), ("int", "rle"), ("int", "huffman"), ("int", "mode"), ("size_t", "budget_bytes"),
          ("uint8_t*", "out"), ("size_t", "cap"), ("int*", "percent")]

IE_EINVAL = -1


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
    assert _declaration("ie_hip.h", "int", "ie_probe_sizes") == PROBE
    assert _declaration("ie_host.hpp", "int", "ieh_scale_matrix") == SCALE
    assert _declaration("ie_host.hpp", "int64_t", "ieh_encode_image_budget") == BUDGET
    assert re.search(r"IE_PROBE_MAX\s*=\s*64\b", open(os.path.join(ROOT, "include", "ie_hip.h")).read())


def test_libraries_export_them_with_the_binding_signatures():
    from imageencoder_amd import HOST_LIB_PATH, LIB_PATH, load_host_library, load_library
    assert os.path.exists(LIB_PATH), "libie_hip.so not built"
    assert os.path.exists(HOST_LIB_PATH), "libie_host.so not built"
    assert hasattr(C.CDLL(LIB_PATH), "ie_probe_sizes")
    fn = load_library().ie_probe_sizes
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [CTYPES[t] for t, _ in PROBE]
    H = load_host_library()
    raw = C.CDLL(HOST_LIB_PATH)
    for name in ("ieh_scale_matrix", "ieh_encode_image_budget", "ieh_budget_ladder"):
        assert hasattr(raw, name), name
    assert H.ieh_scale_matrix.restype is C.c_int
    assert list(H.ieh_scale_matrix.argtypes) == [CTYPES[t] for t, _ in SCALE]
    assert H.ieh_encode_image_budget.restype is C.c_int64
    assert list(H.ieh_encode_image_budget.argtypes) == [CTYPES[t] for t, _ in BUDGET]


def test_codec_has_the_methods():
    import inspect

    import imageencoder_amd as ie
    sig = inspect.signature(ie.Codec.probe_sizes)
    assert list(sig.parameters) == ["self", "y", "w", "h", "qs", "nframes", "rle", "stride", "frame_pitch", "out"]
    assert sig.parameters["nframes"].default == 1 and sig.parameters["rle"].default is True
    sig = inspect.signature(ie.Codec.encode_image_budget)
    assert list(sig.parameters) == ["self", "y", "w", "h", "q", "n", "budget", "rle", "huffman", "mode"]
    assert sig.parameters["huffman"].default is True and sig.parameters["mode"].default == ie.MODE_FAST
    assert list(inspect.signature(ie.scale_matrix).parameters) == ["base", "percent"]


def _scaled(base, percent):
    """The integer formula, in Python's unbounded integers."""
    return [min(max((int(v) * percent + 50) // 100, 1), 65535) for v in base]


MATRICES = [("matrix.txt", 4, lambda: O.read_matrix("matrix.txt", 4)),
            ("annex_k", 8, lambda: np.array(MS.ANNEX_K, dtype=np.uint16)),
            ("all_65535_4", 4, lambda: np.full(16, 65535, dtype=np.uint16)),
            ("all_65535_8", 8, lambda: np.full(64, 65535, dtype=np.uint16))]


@pytest.mark.parametrize("name,n,make", MATRICES, ids=[m[0] for m in MATRICES])
@pytest.mark.parametrize("percent", [1, 25, 100, 141, 5382])
def test_scale_matrix_equals_the_integer_formula(name, n, make, percent):
    from imageencoder_amd import scale_matrix
    base = make()
    got = scale_matrix(base, percent)
    assert got.dtype == np.uint16 and got.shape == (n * n,)
    assert got.tolist() == _scaled(base, percent)


def test_scale_matrix_clamps_at_both_ends():
    from imageencoder_amd import scale_matrix
    base = np.array([1, 2, 49, 50, 51, 149, 150, 1217, 1218, 12, 13, 65535, 40000, 655, 656, 32768], dtype=np.uint16)
    low = scale_matrix(base, 1)           # (v + 50) // 100: 0 below 50 -> clamped to 1
    assert low.tolist() == _scaled(base, 1) and low[0] == 1 and low[2] == 1 and low[3] == 1 and low[5] == 1 and low[6] == 2
    high = scale_matrix(base, 5382)       # 1218 * 53.82 = 65552.8 -> clamped to 65535; 1217 -> 65499
    assert high.tolist() == _scaled(base, 5382) and high[8] == 65535 and high[7] == 65499 and high[11] == 65535
    assert scale_matrix(base, 100).tolist() == base.tolist()


def test_scale_matrix_rejects_a_percent_below_one():
    from imageencoder_amd import load_host_library
    H = load_host_library()
    base = np.ones(16, dtype=np.uint16)
    out = np.zeros(16, dtype=np.uint16)
    for bad in (0, -5):
        assert H.ieh_scale_matrix(base.ctypes.data, 4, bad, out.ctypes.data) == IE_EINVAL
    assert H.ieh_scale_matrix(base.ctypes.data, 5, 100, out.ctypes.data) == IE_EINVAL
    assert H.ieh_scale_matrix(base.ctypes.data, 4, 1, out.ctypes.data) == 0


def ladder_formula():
    """round(100 * 2^(j/4)), j = -8 .. 23; no value lies within 0.01 of a tie (the nearest is 4525.483), so the rounding
    rule does not matter."""
    vals = [100.0 * 2.0 ** (j / 4.0) for j in range(-8, 24)]
    assert all(abs(v - np.floor(v) - 0.5) > 0.01 for v in vals)
    return [int(np.floor(v + 0.5)) for v in vals]


def test_budget_ladder_is_the_formula():
    from imageencoder_amd import budget_ladder
    lad = budget_ladder()
    assert lad == ladder_formula()
    assert len(lad) == 32 and lad[0] == 25 and lad[8] == 100 and lad[-1] == 5382
    assert lad == sorted(set(lad))
