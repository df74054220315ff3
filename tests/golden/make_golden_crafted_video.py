#!/usr/bin/env python3
"""Pin the reference's decode of every constructed video (tests/crafted_videos.py).

The twin of make_golden_crafted.py: runs on the CPU where oracle/_ref exists.  Every file of the
table is decoded by the REFERENCE ITSELF -- its `decoder`, through make_golden_gop.ref_video_decode
-- with motion compensation on and off, and manifest_crafted_video.json records the entry's name,
family and settings, the file's md5 and the md5 of the reference's output for both settings.  No
stream and no pixels are stored: stream_craft.pack_video rebuilds the files from the table.

Usage:  python tests/golden/make_golden_crafted_video.py
        (rewrites tests/golden/manifest_crafted_video.json)
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import REF, md5  # noqa: E402
from make_golden_gop import ref_video_decode  # noqa: E402
from tests import crafted_videos  # noqa: E402


def main():
    if not os.path.exists(os.path.join(REF, "decoder")):
        sys.exit("oracle/_ref not built: run `make -C oracle ref` where the reference sources exist")
    manifest = []
    for e in crafted_videos.entries():
        m = dict(name=e.name, family=e.family, **e.settings(), md5=md5(e.data))
        for mc in (1, 0):
            dec = ref_video_decode(e.data, mc)
            assert len(dec) == e.frames * (e.w * e.h * 3 // 2), (e.name, mc, len(dec))
            m[f"dec{mc}_md5"] = md5(dec)
        manifest.append(m)
        print(f"{e.name:28s} {len(e.data):8d} B  {m['dec1_md5'][:12]}  {m['dec0_md5'][:12]}", flush=True)
    with open(os.path.join(HERE, "manifest_crafted_video.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
