"""The encoder / decoder command lines (imageencoder_amd/csrc/cli/main.cpp) against the reference
CLI's contract (main.cpp:20-178): settings-file checks and exit codes 1-5 (CPU, no device call
happens before those exits), and byte-identical files on the GPU.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as O

ROOT = O.ROOT
BIN = os.path.join(ROOT, "imageencoder_amd", "lib")


def _bin(name):
    p = os.path.join(BIN, name)
    if not os.path.exists(p):
        pytest.skip(f"{name} not built (make host)")
    return p


def _write_conf(d, **kv):
    p = os.path.join(d, "set.conf")
    with open(p, "w") as f:
        for k, v in kv.items():
            f.write(f"{k}={v}\n")
    return p


def _image_conf(d, **over):
    kv = dict(rawfile="in.raw", encfile="out.enc", decfile="out.dec", width=8, height=8, rle=1,
              quantfile="matrix.txt", logfile="log.txt")
    kv.update(over)
    return _write_conf(d, **kv)


def _run(exe, conf, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([exe, conf], cwd=cwd, capture_output=True, text=True, timeout=120, env=e)


def _put(src, dst):
    """Copy contents only (the repo files may be read-only; the copies must stay writable)."""
    with open(src, "rb") as f, open(dst, "wb") as g:
        g.write(f.read())


@pytest.fixture
def work(tmp_path):
    for m in ("matrix.txt", "matrix4_2.txt", "matrix8_1.txt", "matrix8_2.txt"):
        _put(os.path.join(O.GOLDEN, m), tmp_path / m)
    _put(os.path.join(O.GOLDEN, "ex0.raw"), tmp_path / "in.raw")
    return str(tmp_path)


# ------------------------------------------------------------------ exit codes (CPU only)
def test_exit_1_argument_count(work):
    r = subprocess.run([_bin("encoder")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "One argument" in r.stderr


def test_exit_2_unreadable_or_malformed(work):
    exe = _bin("encoder")
    assert _run(exe, os.path.join(work, "missing.conf"), work).returncode == 2
    p = os.path.join(work, "bad.conf")
    open(p, "w").write("rawfile=a\nno equals sign\n")
    r = _run(exe, p, work)
    assert r.returncode == 2 and "Can't find '='" in r.stderr
    open(p, "w").write("rawfile=a\nrawfile=b\n")
    r = _run(exe, p, work)
    assert r.returncode == 2 and "more than once" in r.stderr
    open(p, "w").write("=x\n")
    assert _run(exe, p, work).returncode == 2


def test_exit_3_inconsistent_settings(work):
    exe = _bin("encoder")
    p = _write_conf(work, rawfile="in.raw", encfile="out.enc")  # neither image nor video
    r = _run(exe, p, work)
    assert r.returncode == 3 and "Error in settings!" in r.stderr
    r = _run(exe, _image_conf(work, encfile="in.raw"), work)  # encfile == rawfile
    assert r.returncode == 3
    r = _run(_bin("decoder"), _image_conf(work, decfile="out.enc"), work)  # decfile == encfile
    assert r.returncode == 3


def test_exit_4_bad_matrix(work):
    exe = _bin("encoder")
    open(os.path.join(work, "m3.txt"), "w").write("1 2 3\n4 5 6\n7 8 9\n")
    assert _run(exe, _image_conf(work, quantfile="m3.txt"), work).returncode == 4
    open(os.path.join(work, "mx.txt"), "w").write("1 2 3 4\n4 5 x 6\n1 1 1 1\n1 1 1 1\n")
    assert _run(exe, _image_conf(work, quantfile="mx.txt"), work).returncode == 4
    assert _run(exe, _image_conf(work, quantfile="nope.txt"), work).returncode == 4
    # an 8x8 matrix needs the 8x8 build (IE_BLOCKSIZE=8), like the reference's BlockSize
    assert _run(exe, _image_conf(work, quantfile="matrix8_1.txt"), work).returncode == 4


def test_exit_5_bad_number(work):
    exe = _bin("encoder")
    assert _run(exe, _image_conf(work, width="abc"), work).returncode == 5


# ------------------------------------------------------------------ byte-identical files (GPU)
# every reference asset: ex0, ex6 and the published example images ex1-ex4 (README.md:175-183);
# large outputs are pinned by md5
CLI_CASES = [c for c in O.manifest() if c["input"]["kind"] == "asset"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", CLI_CASES, ids=[c["name"] for c in CLI_CASES])
def test_cli_encode_decode_golden(work, c):
    _put(os.path.join(O.GOLDEN, c["input"]["file"]), os.path.join(work, "in.raw"))
    _put(os.path.join(O.GOLDEN, c["matrix"]), os.path.join(work, c["matrix"]))
    conf = _image_conf(work, width=c["w"], height=c["h"], rle=c["rle"], quantfile=c["matrix"])
    env = {"IE_BLOCKSIZE": str(c["n"])}
    enc_exe = _bin("encoder" if c["huffman"] else "encoder_nohuff")
    r = _run(enc_exe, conf, work, env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = open(os.path.join(work, "out.enc"), "rb").read()
    want = O.case_expected(c)
    if want is None:
        assert len(got) == c["size"] and hashlib.md5(got).hexdigest() == c["md5"], c["name"]
    else:
        assert got == want, c["name"]
    if c.get("decode"):
        r = _run(_bin("decoder"), conf, work, env)
        assert r.returncode == 0, r.stdout + r.stderr
        dec = open(os.path.join(work, "out.dec"), "rb").read()
        assert hashlib.md5(dec).hexdigest() == c["dec_md5"]


# (name, read-chunk MiB): the encoder streams the .yuv file in chunks of frames (IE_CHUNK_MB),
# one ie_vstream push each, so a small chunk makes every frame its own read + push + launch
VIDEO_CLI = [("vidU64x48x5_4x4_huff", None), ("vidU64x48x5_4x4_huff", 0.005), ("vidM64x48x5_4x4", 0.005),
             ("vidM1080x3_4x4", 3), ("vidU1080x3_4x4", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,chunk_mb", VIDEO_CLI, ids=[f"{n}-{m or 'default'}" for n, m in VIDEO_CLI])
def test_cli_video_gop1(work, name, chunk_mb):
    c = next(c for c in O.manifest() if c["name"] == name)
    w, h = c["w"], c["h"]
    open(os.path.join(work, "in.yuv"), "wb").write(O.case_input(c))
    conf = _write_conf(work, rawfile="in.yuv", encfile="v.enc", decfile="v.dec", width=w, height=h, rle=1,
                       quantfile="matrix.txt", logfile="", gop=1, merange=16)
    env = {"IE_CHUNK_MB": str(chunk_mb)} if chunk_mb else {}
    r = _run(_bin("encoder" if c["huffman"] else "encoder_nohuff"), conf, work, env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = open(os.path.join(work, "v.enc"), "rb").read()
    want = O.case_expected(c)
    if want is None:  # large cases are pinned by md5
        assert hashlib.md5(got).hexdigest() == c["md5"] and len(got) == c["size"]
    else:
        assert got == want
    if c["huffman"] or w * h > 64 * 48:
        return
    conf = _write_conf(work, encfile="v.enc", decfile="v.dec", motioncompensation=0)
    r = _run(_bin("decoder"), conf, work)
    assert r.returncode == 0, r.stdout + r.stderr
    dec = np.frombuffer(open(os.path.join(work, "v.dec"), "rb").read(), np.uint8)
    assert dec.size == c["input"]["frames"] * w * h * 3 // 2


# P-frame videos through the reference-shaped command lines: the settings file's gop / merange
# select I/P-frames (VideoEncoder), motioncompensation the decoder's handling of the coded error
GOP_CLI = ["gopP64x48x5_g3_m8", "gopM64x48x5_g2_m0", "gopP64x40x4_g4_m8"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOP_CLI)
def test_cli_video_pframes(work, name):
    c = next(c for c in O.manifest_gop() if c["name"] == name)
    w, h = c["w"], c["h"]
    open(os.path.join(work, "in.yuv"), "wb").write(O.case_input(c))
    conf = _write_conf(work, rawfile="in.yuv", encfile="v.enc", decfile="v.dec", width=w, height=h, rle=c["rle"],
                       quantfile=c["matrix"], logfile="", gop=c["gop"], merange=c["merange"])
    r = _run(_bin("encoder_nohuff"), conf, work)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(os.path.join(work, "v.enc"), "rb").read() == O.case_expected(c)
    if "dec1_md5" not in c:
        return
    for mc in (1, 0):
        conf = _write_conf(work, encfile="v.enc", decfile="v.dec", motioncompensation=mc)
        r = _run(_bin("decoder"), conf, work)
        assert r.returncode == 0, r.stdout + r.stderr
        dec = open(os.path.join(work, "v.dec"), "rb").read()
        assert hashlib.md5(dec).hexdigest() == c[f"dec{mc}_md5"], mc
