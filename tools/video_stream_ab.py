"""Wall time of dc::VideoEncoder::process on a P-frame .raw/YUV420 video file, this build against
another build of the libraries (the parent commit's, which reads the whole file and runs one
ie_encode_gop), alternating.

usage: python tools/video_stream_ab.py --parent-libdir DIR [--size 1920x1088] [--frames 64] [--gop 8]
                                       [--merange 16] [--rounds 5] [--reps 4] [--limit 300] [--out FILE]

DIR holds the other build's libie_host.so and libie_hip.so.  The video (synth "P", Huffman off,
4x4 blocks, matrix.txt) is written to a local temporary file.  tools/video_process_time.cpp is
compiled once and run with each build's library directory in turn: every run is a process of its
own that does one untimed process() (context creation, code object load, page cache) and --reps
timed ones; --rounds such pairs, parent first.  Prints per build the median, min and max in ms and
the quartiles' spread, the ratio of the medians, and every sample; the two builds' files are
compared by size and hash.  Every child runs under --limit seconds: one that overruns, or fails,
ends the script.
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imageencoder_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-libdir", required=True)
ap.add_argument("--size", default="1920x1088")
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--gop", type=int, default=8)
ap.add_argument("--merange", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--out", default=None)
args = ap.parse_args()
w, h = (int(v) for v in args.size.split("x"))

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


with tempfile.TemporaryDirectory() as tmp:
    exe, video = os.path.join(tmp, "video_process_time"), os.path.join(tmp, "in.yuv")
    libdirs = {"parent": os.path.abspath(args.parent_libdir), "this": os.path.join(ROOT, "imageencoder_amd", "lib")}
    # (linked against this build; the library directory of each run decides what is loaded)
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "video_process_time.cpp"), "-L" + libdirs["this"], "-lie_host", "-lie_hip",
                    "-o", exe], check=True, timeout=args.limit)
    with open(video, "wb") as f:
        f.write(synth.yuv420(synth.frames("P", w, h, args.frames, seed=5)))
    ts, files = {"parent": [], "this": []}, {}
    for _ in range(args.rounds):
        for name in ("parent", "this"):
            env = dict(os.environ, LD_LIBRARY_PATH=libdirs[name] + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
            r = subprocess.run([exe, video, str(w), str(h), os.path.join(ROOT, "tests", "golden", "matrix.txt"),
                                str(args.gop), str(args.merange), "1", str(args.reps)], env=env, capture_output=True,
                               text=True, timeout=args.limit)
            if r.returncode != 0:
                sys.exit(f"{name}: exit {r.returncode}: {r.stderr[-2000:]}")
            for ln in r.stdout.splitlines():
                t = ln.split()
                if t and t[0] == "ms":
                    ts[name].append(float(t[1]))
                    files.setdefault(name, set()).add((t[3], t[5]))
    assert files["parent"] == files["this"] and len(files["this"]) == 1, files
    say(f"{w}x{h} 4x4, {args.frames} frames, gop {args.gop}, merange {args.merange}, Huffman off: "
        f"{next(iter(files['this']))[0]} file bytes, identical in both builds; {args.rounds} rounds x {args.reps} "
        f"timed process() per build, alternating processes")
    med = {}
    for name in ("parent", "this"):
        t = sorted(ts[name])
        q = statistics.quantiles(t, n=4)
        med[name] = statistics.median(t)
        say(f"    {name:6s}: median {med[name]:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}  quartiles {q[0]:.3f} .. {q[2]:.3f}"
            f"  ({len(t)} samples)")
    say(f"    ratio this/parent {med['this'] / med['parent']:.3f}")
    for name in ("parent", "this"):
        say(f"    raw {name} ms: " + " ".join(f"{v:.3f}" for v in ts[name]))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
