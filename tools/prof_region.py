"""Region decode against the full decode plus a crop, for one 4K frame of the bench's noise content
(device-resident stream; 4x4 and 8x8; rectangles: the centred quarter, a 256x256 tile, the full
frame).  Baseline: ie_decode_frames into a device frame, then a 2D copy of the rectangle -- to a
device buffer, or to host memory with --host, where ie_decode_region copies only the rectangle's
rows and the baseline decodes into host memory and crops there.  The two paths alternate run by
run and the medians are compared (buffer placement moves single timings by several per cent).
usage: python tools/prof_region.py [--host] [--runs K] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from imageencoder_amd import Codec, stream_bound, synth  # noqa: E402
from tests import oracle_lib as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--host", action="store_true")
ap.add_argument("--runs", type=int, default=41)
ap.add_argument("--json")
args = ap.parse_args()

w, h = 3840, 2160
rects = {"quarter": (w // 4, h // 4, w // 2, h // 2), "tile256": (w // 2 - 128, h // 2 - 128, 256, 256), "full": (0, 0, w, h)}
rows = []
for n in (4, 8):
    c = Codec(0, O.read_matrix("matrix.txt" if n == 4 else "matrix8_1.txt", n), n)
    y = synth.frame("U", w, h, synth.DEFAULT_SEED)  # the bench's image 0
    out = torch.zeros(stream_bound(w, h, n, 1, 0), dtype=torch.uint8, device="cuda")
    _, end = c.encode_frames(torch.from_numpy(y).cuda(), w, h, out)
    stream = out[: (end + 7) // 8]
    pix = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    hpix = c.host_array(w * h).reshape(h, w) if args.host else None
    for name, (x0, y0, rw, rh) in rects.items():
        rect = (x0, y0, rw, rh)
        dreg = torch.empty((rh, rw), dtype=torch.uint8, device="cuda")
        dcrop = torch.empty((rh, rw), dtype=torch.uint8, device="cuda")
        hreg = c.host_array(rw * rh).reshape(rh, rw) if args.host else None
        hcrop = np.empty((rh, rw), dtype=np.uint8)

        def base():
            if args.host:  # the parent path for a host result: the whole frame crosses, the crop is the host's
                c.decode_frames(stream, w, h, hpix)
                np.copyto(hcrop, hpix[y0:y0 + rh, x0:x0 + rw])
            else:
                c.decode_frames(stream, w, h, pix)
                dcrop.copy_(pix[y0:y0 + rh, x0:x0 + rw])
                torch.cuda.synchronize()

        def region():
            c.decode_region(stream, w, h, rect, out=hreg if args.host else dreg)

        def full_only():
            c.decode_frames(stream, w, h, pix)

        for f in (base, region, full_only):
            f()
        got = hreg if args.host else dreg.cpu().numpy()
        exp = hcrop if args.host else dcrop.cpu().numpy()
        assert np.array_equal(got, exp), (n, name)
        t = {"base": [], "region": [], "full": []}
        for _ in range(args.runs):  # alternating: every path sees the same drift
            for key, f in (("base", base), ("region", region), ("full", full_only)):
                t0 = time.perf_counter()
                f()
                t[key].append((time.perf_counter() - t0) * 1e6)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: (min(v), sorted(v)[len(v) * 9 // 10]) for k, v in t.items()}
        row = {"n": n, "rect": name, "dest": "host" if args.host else "device", "base_us": round(med["base"], 1),
               "region_us": round(med["region"], 1), "decode_frames_us": round(med["full"], 1),
               "speedup": round(med["base"] / med["region"], 2),
               "region_min_p90_us": [round(x, 1) for x in spread["region"]],
               "base_min_p90_us": [round(x, 1) for x in spread["base"]]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    c.close()
if args.json:
    json.dump(rows, open(args.json, "w"), indent=1)
