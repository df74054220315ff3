"""The Huffman ENCODE side on the inputs the byte sets of tests/test_gpu_files.py never reach
(tests/huffman_inputs.py; tests/test_huffman_inputs.py shows on the CPU that every input is what its
name says).  Every comparison is byte for byte: whole files against the oracle's Huffman encode,
pack output against the plain per-bit packer, histograms against np.bincount and the first index.

  a. unaligned device input: the byte-wise branches of hist_body, first_scan_core and pack_kernel
  b. a tile whose LDS image is full: 256 codes of one length, both pack kernels
  c. longest codes of 15, 16 and 17 bits through the real pipeline: the switch between the kernels
  d. zero-bit codes: single-value strings, tiles that carry no bits
  e. the grid-stride loops of hist_body and first_full_body, single string and batch
  f. first-occurrence edges: chunk, round and scan ends; the scan's early exit
  g. tiles ordered by the atomic ticket, and the host's redo after a reported look-back timeout
  h. alphabets of equal counts: every tie-break of the tree build

Device outputs start out as a garbage byte; the bits before the start bit must come back unchanged
and the last word zero-padded.  Nothing past the returned length is looked at.
"""
import ctypes as C

import numpy as np
import pytest

from tests import huffman_inputs as HI
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

# The kernels' constants (imageencoder_amd/csrc/ie_huffman.hip), written once:
HIST_TILE = 4096          # :27   kHistTile = kTPB * 16, bytes per workgroup pass (kTPB = 256: ie_device.h:12)
HIST_STEP = 16384         # :43   kStep = kHistLoads (:28, 4) * kHistTile, a workgroup's grid-stride unit in hist_body
FIRST_SCAN_CHUNKS = 64    # :81   kFirstScanChunks, the prefix first_scan_core covers, in kHistTile chunks
FIRST_Q = 4               # :83   IE_FIRST_Q = kFirstScanQ (:85), chunks per round of the scan
PACK_TILE_SHORT = 16384   # :486  pack_tile_bytes: kTPB * IE_PACK_BPT (:484, 64) for codes of <= 16 bits, pack_kernel<64, 16>
PACK_TILE_LONG = 4096     # :486  pack_tile_bytes: kTPB * 16 for longer codes, pack_kernel<16, 32>
HIST_GRID = 2048          # :267  launch_hist: at most 2048 workgroups for a single string
BATCH_GRID = 4096         # :276  launch_hist_batch: about 4096 workgroups over a batch

GARBAGE = 0xA5
OFFSETS = (1, 3, 8, 15)
_STATE = {}
_u8p, _u32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def _codec():
    if "codec" not in _STATE:
        from imageencoder_amd import Codec
        _STATE["codec"] = Codec(0)
    return _STATE["codec"]


def _np(data) -> np.ndarray:
    return data if isinstance(data, np.ndarray) else np.frombuffer(data, np.uint8)


def _dev(data, off=0):
    """``data`` on the device, ``off`` bytes past a 16-byte boundary."""
    import torch
    a = _np(data)
    buf = np.full(a.size + off, 0xEE, dtype=np.uint8)
    buf[off:] = a
    t = torch.from_numpy(buf).cuda()[off:]
    assert t.data_ptr() % 16 == off % 16 and t.numel() == a.size
    return t


def _dptr(t, typ=_u8p):
    return C.cast(C.c_void_p(t.data_ptr()), typ)


def _want(data: bytes) -> bytes:
    return O.load().huffman_encode(data) if len(data) else b"\x00"  # empty: the bare stop bit


def _same(got: bytes, want: bytes, what):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        n = min(a.size, b.size)
        bad = np.flatnonzero(a[:n] != b[:n])
        pytest.fail(f"{what}: {a.size} bytes against {b.size}, first difference at byte "
                    f"{int(bad[0]) if bad.size else n} ({bad.size} differ)")


def _check_hist(codec, x, data, what=""):
    hist, first = codec.huffman_hist(x)
    eh, ef = HI.histogram(_np(data))
    assert np.array_equal(hist, eh), ("counts", what, np.flatnonzero(hist != eh)[:8])
    assert np.array_equal(first, ef), ("first positions", what, np.flatnonzero(first != ef)[:8])


def _check_pack(codec, din, n, code, length, start, ref, out_kind="device", what=""):
    """ie_huffman_pack of din (n bytes, host or device) at bit ``start`` into an output of GARBAGE:
    the end bit, the bits before start unchanged, the code bits == ref, the last word zero-padded."""
    import torch
    maxlen = int(length.max())
    need = (start + maxlen * n + 31) // 32 * 4
    garbage = np.full(need + 64, GARBAGE, dtype=np.uint8)
    out = torch.from_numpy(garbage.copy()).cuda() if out_kind == "device" else garbage.copy()
    end = codec.huffman_pack(din, code, length, out, start)
    got = out.cpu().numpy() if out_kind == "device" else out
    assert end == start + ref.size, (what, end, start + ref.size)
    # device: whole words are written; host: the bytes up to the one holding the last bit
    pad_end = (end + 31) // 32 * 32 if out_kind == "device" else ((end + 7) // 8 * 8 if end > start else end)
    bits = np.unpackbits(got[: pad_end // 8 + 1])
    assert np.array_equal(bits[:start], np.unpackbits(garbage[: start // 8 + 1])[:start]), (what, "bits before start")
    if not np.array_equal(bits[start:end], ref):
        bad = np.flatnonzero(bits[start:end] != ref)
        pytest.fail(f"{what}: {bad.size} of {ref.size} code bits differ, the first at bit {int(bad[0])}")
    assert not bits[end:pad_end].any(), (what, "padding")


def _encode_batch(codec, strings, pitch, bound=4):
    """huffman_encode_batch over ``strings`` laid out ``pitch`` bytes apart (the last may run past
    it) into an output filled with 0xAB: every string's file."""
    import torch
    K = len(strings)
    lens = [len(s) for s in strings]
    src = np.zeros((K - 1) * pitch + max(pitch, lens[-1]), dtype=np.uint8)
    for k, s in enumerate(strings):
        src[k * pitch: k * pitch + lens[k]] = _np(s)
    return _encode_batch_dev(codec, torch.from_numpy(src).cuda(), lens, pitch, bound)


def _encode_batch_dev(codec, dsrc, lens, pitch, bound=4):
    import torch
    K = len(lens)
    opitch = (bound * max(lens) + 4096 + 255) // 256 * 256
    out = torch.full((opitch * K,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the codec runs on its own stream
    sizes = codec.huffman_encode_batch(dsrc, pitch, lens, out, opitch)
    codec.sync()
    torch.cuda.synchronize()
    return [out[k * opitch: k * opitch + sizes[k]].cpu().numpy().tobytes() for k in range(K)]


def _check_batch(codec, strings, pitch, what=""):
    got = _encode_batch(codec, strings, pitch)
    for k, s in enumerate(strings):
        _same(got[k], _want(s), (what, "string", k, len(s)))


# ------------------------------------------------------------------ a. unaligned device input
HIST_N = HIST_STEP + HIST_TILE + 77  # one full step, one full tile, a tail


@pytest.mark.parametrize("off", (0,) + OFFSETS)
def test_unaligned_hist(off):
    """hist_body's and first_scan_core's byte-wise branches (ie_huffman.hip:57-69, :106-111); the
    same bytes at offset 0 take the vector loads."""
    data = HI.placed(HIST_N, ((210, HIST_STEP - 1), (211, HIST_STEP), (212, HIST_STEP + HIST_TILE), (213, HIST_N - 1)), 70)
    _check_hist(_codec(), _dev(data, off), data, off)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("maxlen,n", [(9, PACK_TILE_SHORT + 77), (20, PACK_TILE_LONG + 5)], ids=["short_codes", "long_codes"])
def test_unaligned_pack(maxlen, n, off):
    """pack_kernel's byte-wise loads (ie_huffman.hip:346-353) in both kernels: a full tile and a tail."""
    data = _np(HI.uniform(n, 71 + maxlen))
    code, length = HI.ragged_table(maxlen, 72 + maxlen)
    ref, _ = HI.pack_bits(data, code, length)
    for start in (0, 45):
        _check_pack(_codec(), _dev(data, off), n, code, length, start, ref, what=(maxlen, off, start))


@pytest.mark.parametrize("off", OFFSETS)
def test_unaligned_encode(off):
    data = HI.skewed(20_011, 73)
    _same(_codec().huffman_encode(_dev(data, off)), _want(data), off)


def test_unaligned_batch_odd_pitch():
    """in_pitch = 20 011: strings 1 .. 5 start at five different offsets within a 16-byte line."""
    _check_batch(_codec(), [s for _, s in HI.six_strings()], HI.SIX_PITCH)


# ------------------------------------------------------------------ b. full LDS image
STARTS = (0, 5, 31, 32, 33, 77)
T, U = PACK_TILE_SHORT, PACK_TILE_LONG
N_SHORT = (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)
N_LONG = (1, 15, 16, 17, U - 1, U, U + 1, 2 * U + 1)


def _pack_sweep(code, length, seed, what):
    ns = N_SHORT if int(length.max()) <= 16 else N_LONG
    data = _np(HI.uniform(max(ns), seed))
    din = _dev(data)
    for n in ns:
        ref, _ = HI.pack_bits(data[:n], code, length)
        for start in STARTS:
            _check_pack(_codec(), din[:n], n, code, length, start, ref, what=(what, n, start))
    return data


@pytest.mark.parametrize("L", [1, 7, 8, 15, 16, 17, 31, 32])
def test_full_image(L):
    """All 256 codes L bits long: every tile's image holds tile bytes * L bits, all that
    pack_image_words sized it for (L <= 16: pack_kernel<64, 16>; above: pack_kernel<16, 32>)."""
    code, length = HI.full_table(L, 80 + L)
    _pack_sweep(code, length, 81 + L, L)


@pytest.mark.parametrize("maxlen", [15, 16])
def test_ragged_codes_short_kernel(maxlen):
    """Random lengths up to exactly 15 and exactly 16 bits, six symbols of zero bits among them."""
    code, length = HI.ragged_table(maxlen, 90 + maxlen, zeros=6)
    data = _pack_sweep(code, length, 91 + maxlen, ("ragged", maxlen))
    assert (length[data] == 0).any() and (length[data] == maxlen).any()


# ------------------------------------------------------------------ c. 15 / 16 / 17-bit codes, real pipeline
def _fib(nsym, order) -> bytes:
    key = ("fib", nsym, order)
    if key not in _STATE:
        _STATE[key] = HI.fib_string(nsym, order)
    return _STATE[key]


@pytest.mark.parametrize("order", HI.ORDERS)
@pytest.mark.parametrize("nsym", [16, 17, 18])
def test_fib_encode(nsym, order):
    data = _fib(nsym, order)
    want = _want(data)
    _same(_codec().huffman_encode(_np(data).copy()), want, "host input")
    _same(_codec().huffman_encode(_dev(data)), want, "device input")


def test_fib_batch_all_nine():
    """One batch of the nine strings: the longest code of all, 17 bits, puts every string on the
    long-code kernel."""
    _check_batch(_codec(), [_fib(nsym, order) for nsym in (16, 17, 18) for order in HI.ORDERS], 27 * 256)


def test_fib_batch_short_kernel():
    """The three 16-symbol orders alone: 15 bits, the short-code kernel."""
    _check_batch(_codec(), [_fib(16, order) for order in HI.ORDERS], 11 * 256)


# ------------------------------------------------------------------ d. zero-bit codes
@pytest.mark.parametrize("value", HI.SINGLE_VALUES)
@pytest.mark.parametrize("n", HI.SINGLE_N)
def test_single_value_encode(n, value):
    """n >= 3 copies of one value: the 21-bit dictionary and no data bits.  Every tile has A == 0;
    the dictionary's last word reaches the output through the last tile's store alone."""
    data = HI.single_value(value, n)
    want = _want(data)
    assert want == HI.single_value_file(value)
    c = _codec()
    _same(c.huffman_encode(_np(data).copy()), want, "host input")
    _same(c.huffman_encode(_dev(data)), want, "device input")
    pitch = (n + 255) // 256 * 256
    _check_batch(c, [data], pitch, "alone")
    _check_batch(c, [HI.skewed(5000, 100 + n), data, HI.skewed(min(pitch, 777), 101 + n, p=0.3)], max(pitch, 5120), "between")


@pytest.mark.parametrize("out_kind", ["device", "host"])
def test_pack_zero_length_table(monkeypatch, out_kind):
    """Every code zero bits long: end == start and the caller's bits intact.  On a codec of its own,
    so that the host output's staging buffer is first reserved by this call (for no bits at all)."""
    n = PACK_TILE_SHORT + 77
    data = _np(HI.uniform(n, 110))
    code, length = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    codec = _own_codec(monkeypatch)
    try:
        for start in (0, 21, 45):
            _check_pack(codec, _dev(data), n, code, length, start, np.zeros(0, np.uint8), out_kind, what=start)
    finally:
        codec.close()


def test_batch_all_single_valued():
    strings = [HI.single_value(v, n) for v, n in ((42, 3), (0, 4), (7, 1000), (255, 16384), (42, 2 * 16384 + 5), (0, 16385), (129, 5))]
    assert [_want(s) for s in strings] == [HI.single_value_file(s[0]) for s in strings]
    _check_batch(_codec(), strings, 2 * 16384 + 256)


# ------------------------------------------------------------------ e. grid-stride loops
def _batch256():
    if "b256" not in _STATE:
        import torch
        strings = HI.batch256()
        lens = [len(s) for s in strings]
        pitch = HI.BATCH256_PITCH
        src = np.zeros(255 * pitch + lens[-1], dtype=np.uint8)
        for k, s in enumerate(strings):
            src[k * pitch: k * pitch + lens[k]] = _np(s)
        _STATE["b256"] = (strings, lens, torch.from_numpy(src).cuda())
    return _STATE["b256"]


def test_batch256_hist():
    """256 strings: hist_batch_kernel's grid is 4096 / 256 = 16 workgroups per string, so the last
    string's 400 003 bytes take a second stride of 16 * 16 384 bytes; first_full_body strides by
    16 * 4096 bytes from byte 262 144.  ie_huffman_hist_batch by ctypes."""
    import torch
    strings, lens, dsrc = _batch256()
    assert BATCH_GRID // 256 * HIST_STEP < lens[-1] and FIRST_SCAN_CHUNKS * HIST_TILE + BATCH_GRID // 256 * HIST_TILE < lens[-1]
    c = _codec()
    n = np.array(lens, dtype=np.uint64)
    hist = np.zeros((256, 256), dtype=np.uint32)
    first = np.zeros((256, 256), dtype=np.uint64)
    torch.cuda.synchronize()
    r = c.L.ie_huffman_hist_batch(c.h, _dptr(dsrc), HI.BATCH256_PITCH, n.ctypes.data_as(_u64p), 256,
                                  hist.ctypes.data_as(_u32p), first.ctypes.data_as(_u64p))
    assert r == 0, c.L.ie_last_error(c.h)
    for k, s in enumerate(strings):
        eh, ef = HI.histogram(s)
        assert np.array_equal(hist[k], eh), ("counts", k)
        assert np.array_equal(first[k], ef), ("first positions", k, np.flatnonzero(first[k] != ef)[:8])


def test_batch256_encode():
    strings, lens, dsrc = _batch256()
    got = _encode_batch_dev(_codec(), dsrc, lens, HI.BATCH256_PITCH)
    for k, s in enumerate(strings):
        _same(got[k], _want(s), ("string", k, len(s)))


def test_hist_second_grid_stride():
    """2048 * 16 384 + 16 384 + 5 bytes: hist_kernel's 2048 workgroups loop a second time --
    workgroup 0 over a full step, workgroup 1 over a 5-byte tail -- and values 200 .. 203 first
    occur there.  The expected result is the oracle's one pass (the plain reference's on the
    second stride)."""
    assert HI.BIG_STRIDE == HIST_GRID * HIST_STEP
    data = HI.big_hist_input()
    hist, first = _codec().huffman_hist(_dev(data))
    eh, ef = O.load().histogram(data)
    assert np.array_equal(hist, eh)
    assert np.array_equal(first, ef)
    assert [int(first[v]) for v, _ in HI.BIG_PLACES] == [at for _, at in HI.BIG_PLACES]
    th, _ = HI.histogram(data[HI.BIG_STRIDE:])
    assert np.array_equal(np.bincount(data[: HI.BIG_STRIDE], minlength=256).astype(np.uint32) + th, hist)


# ------------------------------------------------------------------ f. first-occurrence edges
@pytest.mark.parametrize("n", HI.EDGE_N)
def test_first_occurrence_edges(n):
    """Fresh values at the chunk edge (4095 / 4096), the round edge (16 383 / 16 384 / 16 385) and
    the scan's end (262 143 / 262 144); n = 16 384 ends the scan's loop with (ch + Q) * kHistTile == n."""
    assert FIRST_Q * HIST_TILE in HI.EDGE_N and max(HI.EDGE_AT) == FIRST_SCAN_CHUNKS * HIST_TILE
    data = HI.edge_string(n)
    d = _dev(data)
    _check_hist(_codec(), d, data, n)
    _same(_codec().huffman_encode(d), _want(data), n)
    _same(_codec().huffman_encode(_np(data).copy()), _want(data), (n, "host input"))


def test_first_scan_early_exit():
    """Every value within the first 16 bytes of 300 000: have == need after the scan's first round."""
    data = HI.all_values_early()
    d = _dev(data)
    _check_hist(_codec(), d, data)
    _same(_codec().huffman_encode(d), _want(data), "early")


def test_late_value_is_the_last_byte():
    data = HI.late_last_byte()
    d = _dev(data)
    _check_hist(_codec(), d, data)
    _same(_codec().huffman_encode(d), _want(data), "late")


# ------------------------------------------------------------------ g. ticket order and the redo
def _own_codec(monkeypatch, ticket=False, fake_timeouts=None):
    """A codec of its own: ie_create reads the debug switches.  They only change what the host
    counts and how tiles are numbered; no kernel is made to misbehave."""
    from imageencoder_amd import Codec
    if ticket:
        monkeypatch.setenv("IE_FORCE_TICKET", "1")
    else:
        monkeypatch.delenv("IE_FORCE_TICKET", raising=False)
    if fake_timeouts is not None:
        monkeypatch.setenv("IE_FAKE_TIMEOUTS", str(fake_timeouts))
    else:
        monkeypatch.delenv("IE_FAKE_TIMEOUTS", raising=False)
    return Codec(0)


def test_ticket_mode_encode_and_batch(monkeypatch):
    """pack_kernel's a.ticket branch in both kernels and in a batch; the second pass runs with a
    non-zero ticket_base."""
    short = HI.skewed(4 * PACK_TILE_SHORT + 100, 120, p=0.3)  # 5 tiles of the short-code kernel
    long_ = HI.fib_string(18, "shuffled", scale=3)            # 5 tiles of the long-code kernel (17 bits)
    assert (len(long_) + PACK_TILE_LONG - 1) // PACK_TILE_LONG == 5
    six = [s for _, s in HI.six_strings()]
    codec = _own_codec(monkeypatch, ticket=True)
    try:
        for run in range(2):
            _same(codec.huffman_encode(_dev(short)), _want(short), ("short codes", run))
            _same(codec.huffman_encode(_dev(long_)), _want(long_), ("long codes", run))
            _check_batch(codec, six, HI.SIX_PITCH, ("six", run))
    finally:
        codec.close()


@pytest.mark.parametrize("out_kind", ["host", "device"])
def test_timeout_redo_pack(monkeypatch, out_kind):
    """One reported look-back timeout: pack() runs itself again in ticket mode
    (ie_capi_huffman.cpp:76) and still returns the plain packer's stream from bit 45 with the bits
    before it kept; the context stays in ticket mode, and a second call passes too."""
    n = 2 * PACK_TILE_SHORT + 5
    data = _np(HI.uniform(n, 121))
    code, length = HI.ragged_table(12, 122, zeros=3)
    ref, _ = HI.pack_bits(data, code, length)
    codec = _own_codec(monkeypatch, fake_timeouts=1)
    try:
        for call in range(2):
            _check_pack(codec, _dev(data), n, code, length, 45, ref, out_kind, what=call)
    finally:
        codec.close()


def test_timeout_redo_pack_batch(monkeypatch):
    """ie_huffman_pack_batch by ctypes with a non-null end_bit under one reported timeout: its redo
    (ie_capi_huffman.cpp:591) returns the plain packer's end bits and bytes, each string's prefix
    bits in front, an empty string's prefix alone."""
    import torch
    ns = [2 * PACK_TILE_SHORT + 5, 0, 100, PACK_TILE_SHORT]
    starts = [45, 21, 0, 64]
    K, in_pitch, ppitch = len(ns), 33_024, 8
    rng = np.random.default_rng(123)
    datas = [_np(HI.uniform(n, 124 + k)) for k, n in enumerate(ns)]
    tables = [HI.ragged_table(12, 130 + k, zeros=3) for k in range(K)]
    code = np.concatenate([t[0] for t in tables])
    length = np.concatenate([t[1] for t in tables])
    prefix = rng.integers(0, 256, K * ppitch, dtype=np.uint8)
    src = np.zeros(K * in_pitch, dtype=np.uint8)
    for k, d in enumerate(datas):
        src[k * in_pitch: k * in_pitch + ns[k]] = d
    out_pitch = (max(s + 12 * n for s, n in zip(starts, ns)) // 8 + 4 + 255) // 256 * 256
    dsrc = torch.from_numpy(src).cuda()
    out = torch.full((K * out_pitch,), GARBAGE, dtype=torch.uint8, device="cuda")
    n64, s64, e64 = np.array(ns, np.uint64), np.array(starts, np.uint64), np.zeros(K, np.uint64)
    codec = _own_codec(monkeypatch, fake_timeouts=1)
    try:
        for call in range(2):
            out.fill_(GARBAGE)
            e64[:] = 0
            torch.cuda.synchronize()
            r = codec.L.ie_huffman_pack_batch(codec.h, _dptr(dsrc), in_pitch, n64.ctypes.data_as(_u64p), K,
                                              code.ctypes.data_as(_u32p), length.ctypes.data_as(_u8p),
                                              prefix.ctypes.data_as(_u8p), ppitch, _dptr(out), out_pitch,
                                              s64.ctypes.data_as(_u64p), e64.ctypes.data_as(_u64p))
            assert r == 0, codec.L.ie_last_error(codec.h)
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            for k in range(K):
                ref, end = HI.pack_bits(datas[k], tables[k][0], tables[k][1], starts[k])
                assert int(e64[k]) == end, (call, k)
                wend = (end + 31) // 32 * 32
                bits = np.unpackbits(host[k * out_pitch: k * out_pitch + wend // 8 + 1])
                pre = np.unpackbits(prefix[k * ppitch: (k + 1) * ppitch])
                assert np.array_equal(bits[: starts[k]], pre[: starts[k]]), (call, k, "prefix")
                assert np.array_equal(bits[starts[k]: end], ref), (call, k, "code bits")
                if ns[k]:
                    assert not bits[end:wend].any(), (call, k, "padding")
    finally:
        codec.close()


# ------------------------------------------------------------------ h. equal-count alphabets
@pytest.mark.parametrize("k", HI.EQUAL_K)
def test_equal_counts(k):
    """k values, 40 of each: every merge of the tree build is a tie, decided by the first-occurrence
    order alone (k = 255, 256: the no-gain decision on an exact tie)."""
    strings = [HI.equal_count(k, order, layout) for order in HI.ORDERS for layout in HI.LAYOUTS]
    c = _codec()
    for i, s in enumerate(strings):
        _same(c.huffman_encode(_dev(s)), _want(s), (k, HI.ORDERS[i // 2], HI.LAYOUTS[i % 2]))
    _check_batch(c, strings, (k * HI.EQUAL_M + 255) // 256 * 256, k)
