"""ie_encode_gop_groups against ie_encode_gop on device-resident frames and stream, alternating in
ONE process: synth "P" (panning) videos, 4x4 blocks, matrix.txt.

usage: python tools/gop_groups_ab.py [--parent-lib PATH] [--reps 21] [--frames 64] [--merange 16]
                                     [--cases 64x48:8,352x288:8,1920x1080:8,352x288:2,352x288:32] [--limit 120]

(a) ie_encode_gop of --parent-lib (a libie_hip.so built from the parent commit, loaded beside this
build's; without the option (a) is skipped), (b) this build's ie_encode_gop, (c) this build's
ie_encode_gop_groups.  Every repetition zeroes the stream, synchronises, then times one call with a
host clock (each call ends in its one synchronisation), (a), (b), (c) in turn; prints the medians in
ms per video, min and max, the ratio (c)/(a) and (c)/(b), the kernel launches and memsets each path
enqueues (counted from the shapes) and the scratch per group.  The three streams are compared byte
for byte before timing.  Every step runs under --limit seconds: a step that overruns ends the script.
"""
import argparse
import ctypes as C
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from imageencoder_amd import MODE_FAST, Codec, read_matrix, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--merange", type=int, default=16)
ap.add_argument("--cases", default="64x48:8,352x288:8,1920x1080:8,352x288:2,352x288:32")
ap.add_argument("--limit", type=int, default=120)
args = ap.parse_args()
assert args.reps >= 11, "at least 11 repetitions"


def overrun(signum, frame):
    print("step over its time limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)


def step(fn, *a):
    signal.alarm(args.limit)
    try:
        return fn(*a)
    finally:
        signal.alarm(0)


golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
q = read_matrix(os.path.join(golden, "matrix.txt"), 4)
codec = Codec(0, q, 4)
u64p = C.POINTER(C.c_uint64)

parent = None
if args.parent_lib:
    P = C.CDLL(os.path.abspath(args.parent_lib))
    vp = C.c_void_p
    P.ie_create.argtypes = [C.c_int, C.POINTER(vp)]
    P.ie_destroy.argtypes = [vp]
    P.ie_set_quant.argtypes = [vp, vp, C.c_int]
    P.ie_encode_gop.argtypes = codec.L.ie_encode_gop.argtypes
    assert not hasattr(P, "ie_encode_gop_groups"), "--parent-lib already has the new call: not the parent's build"
    parent = vp()
    assert P.ie_create(0, C.byref(parent)) == 0
    assert P.ie_set_quant(parent, q.ctypes.data, 4) == 0


def align256(b):
    return (b + 255) // 256 * 256


def plan(w, h, f, gop, merange):
    """(launches of ie_encode_gop, launches + memsets of ie_encode_gop_groups, scratch bytes per group, waves)."""
    nb = (w // 4) * (h // 4)
    groups = -(-f // gop)
    records = (w // 16) * (h // 16) > 0
    # one frame at a time: an I-frame is one launch; a P-frame the macroblock launch, then the
    # look-back emission (4x4 with a macroblock) or the end-bit launch
    old = groups + (f - groups) * 2
    per_group = (align256(codec.gop_stream_bound(w, h, gop, merange)) + align256(2 * w * h) + align256(nb * 32)
                 + align256(nb * 4) + align256((-(-nb // 512) + 1) * 8) + (gop + 2) * 8)
    gw = min(groups, 65535, max(1, ((1 << 30) - 1024) // per_group))
    env = os.environ.get("IE_GOP_BATCH_MAX")
    if env and int(env) > 0:
        gw = min(gw, int(env))
    waves = -(-groups // gw)
    steps = min(gop, f) - 1
    # a wave: two memsets, the I-frame batch, per step macroblocks + tile sums + tile scan +
    # emission (or macroblocks + end bits), the splice's scan and copy
    new = waves * (2 + 1 + steps * (4 if records else 2) + 2)
    return old, new, per_group, waves


for case in args.cases.split(","):
    dims, gop = case.split(":")
    w, h = (int(v) for v in dims.split("x"))
    gop, f, merange = int(gop), args.frames, args.merange
    y = step(lambda: torch.from_numpy(synth.frames("P", w, h, f, seed=5)).cuda())
    cap = codec.gop_stream_bound(w, h, f, merange)
    outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(3)]
    fb = np.zeros(f, dtype=np.uint64)
    end = C.c_uint64(0)

    def call(fn, ctx, out):
        r = fn(ctx, y.data_ptr(), w, h, w, w * h, f, gop, merange, 1, MODE_FAST, out.data_ptr(), cap, 0,
               fb.ctypes.data_as(u64p), C.byref(end))
        assert r == 0, r
        return int(end.value)

    paths = []
    if parent is not None:
        paths.append(("(a) parent ie_encode_gop    ", P.ie_encode_gop, parent, outs[0]))
    paths.append(("(b) ie_encode_gop           ", codec.L.ie_encode_gop, codec.h, outs[1]))
    paths.append(("(c) ie_encode_gop_groups    ", codec.L.ie_encode_gop_groups, codec.h, outs[2]))

    def timed(p):
        p[3].zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e = call(p[1], p[2], p[3])
        return (time.perf_counter() - t0) * 1e3, e

    ends = [step(timed, p)[1] for p in paths]
    assert len(set(ends)) == 1, ends
    for p in paths[1:]:
        assert torch.equal(p[3], paths[0][3]), "streams differ"
    for _ in range(args.warmup):
        for p in paths:
            step(timed, p)
    ts = [[] for _ in paths]
    for _ in range(args.reps):
        for k, p in enumerate(paths):
            ts[k].append(step(timed, p)[0])
    old, new, per_group, waves = plan(w, h, f, gop, merange)
    print(f"{w}x{h} 4x4, {f} frames, gop {gop}, merange {merange}: {(ends[0] + 7) // 8} stream bytes, reps {args.reps}")
    print(f"    enqueued: ie_encode_gop {old} launches; ie_encode_gop_groups {new} launches and memsets in {waves} wave(s); "
          f"scratch {per_group} bytes per group, {-(-f // gop)} groups")
    med = [statistics.median(t) for t in ts]
    for p, t, m in zip(paths, ts, med):
        print(f"    {p[0]}: median {m:8.3f} ms/video  min {min(t):8.3f}  max {max(t):8.3f}")
    print("    ratio " + "  ".join(f"(c)/{p[0][:3]} {med[-1] / m:.3f}" for p, m in zip(paths[:-1], med[:-1])))
    for p, t in zip(paths, ts):
        print(f"    raw {p[0][:3]} ms: " + " ".join(f"{v:.3f}" for v in t))
    sys.stdout.flush()
    del y, outs

if parent is not None:
    P.ie_destroy(parent)
codec.close()
