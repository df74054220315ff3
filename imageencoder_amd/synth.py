"""Seeded, portable synthetic 8-bit frames.

Counter-based splitmix64, so any pixel can be generated independently and numpy, a C harness
or a GPU can reproduce the same bytes.  Two generators:

* ``uniform`` (U): ``u8 = splitmix64(seed, i) & 0xFF`` over the frame in raster order -- the
  worst case (no all-zero blocks, many RLE-truncation blocks).
* ``mixed``   (M): 64x64 tiles whose kind is ``splitmix64(seed ^ TILE_SALT, tile) % 3``:
  0 = flat 128 (all-zero blocks, the ``ffs(0)`` path), 1 = slow gradient + [-2, 2] noise,
  2 = uniform noise.

``frames`` also builds whole videos: panning (P) and the constructed P-frame contents of
``_pattern_frames`` (static, flat, stripes, checkerboard, known translation).
"""
from __future__ import annotations

import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
TILE_SALT = 0x5EED7115
DEFAULT_SEED = 0x1E0C0DE


def splitmix64(seed: int, start: int, count: int) -> np.ndarray:
    """Outputs ``start .. start+count-1`` of the splitmix64 sequence seeded with ``seed``."""
    with np.errstate(over="ignore"):
        i = np.arange(start + 1, start + count + 1, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + i * GAMMA
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        return z ^ (z >> np.uint64(31))


def uniform(w: int, h: int, seed: int = DEFAULT_SEED) -> np.ndarray:
    return (splitmix64(seed, 0, w * h) & np.uint64(0xFF)).astype(np.uint8).reshape(h, w)


def mixed(w: int, h: int, seed: int = DEFAULT_SEED, tile: int = 64) -> np.ndarray:
    tx, ty = -(-w // tile), -(-h // tile)
    kind = (splitmix64(seed ^ TILE_SALT, 0, tx * ty) % np.uint64(3)).astype(np.int64).reshape(ty, tx)
    kmap = np.repeat(np.repeat(kind, tile, axis=0), tile, axis=1)[:h, :w]
    r = splitmix64(seed, 0, w * h).reshape(h, w)
    noise = (r & np.uint64(0xFF)).astype(np.int64)
    small = ((r >> np.uint64(8)) % np.uint64(5)).astype(np.int64) - 2
    yy, xx = np.mgrid[0:h, 0:w]
    grad = ((xx + 2 * yy) * 255) // max(1, (w + 2 * h))
    out = np.where(kmap == 0, 128, np.where(kmap == 1, np.clip(grad + small, 0, 255), noise))
    return out.astype(np.uint8)


def frame(kind: str, w: int, h: int, seed: int = DEFAULT_SEED) -> np.ndarray:
    if kind in ("U", "uniform"):
        return uniform(w, h, seed)
    if kind in ("M", "mixed"):
        return mixed(w, h, seed)
    raise ValueError(f"unknown synthetic kind {kind!r}")


SHIFTS = {"shiftA": (5, -3), "shiftB": (-17, 9)}  # true motion (dx, dy) per frame of the "shift" kinds


def smooth(w: int, h: int, seed: int = DEFAULT_SEED, k: int = 16) -> np.ndarray:
    """A k x k box sum of uniform noise stretched back over the 8-bit range: a picture whose SAD
    against a displaced copy of itself grows with the displacement over about k px, so a pattern
    search can descend to the true motion (integer arithmetic only)."""
    u = uniform(w + k, h + k, seed).astype(np.int64)
    s = np.zeros((h + k + 1, w + k + 1), dtype=np.int64)
    s[1:, 1:] = u.cumsum(axis=0).cumsum(axis=1)
    box = s[k: k + h, k: k + w] - s[:h, k: k + w] - s[k: k + h, :w] + s[:h, :w]
    return np.clip(128 + (8 * box - 1020 * k * k) // (k * k), 0, 255).astype(np.uint8)


PATTERNS = ("static", "flat128", "flat0255", "stripesV", "stripesH", "checker") + tuple(SHIFTS)


def _pattern_frames(kind: str, w: int, h: int, count: int, seed: int) -> np.ndarray:
    """The constructed P-frame contents: SAD ties, saturation, five-bit records, known motion."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((count, h, w), dtype=np.uint8)
    if kind == "static":      # every frame the same uniform picture
        out[:] = uniform(w, h, seed)
    elif kind == "flat128":   # every candidate of every search ties
        out[:] = 128
    elif kind == "flat0255":  # frame f is constant 0 (f even) or 255 (f odd)
        out[:] = (np.arange(count) % 2 * 255).astype(np.uint8)[:, None, None]
    elif kind in ("stripesV", "stripesH"):  # 0/255 stripes of period 8 px, moving 4 px per frame
        c = xx if kind == "stripesV" else yy
        for f in range(count):
            out[f] = ((c + 4 * f) // 4 % 2 * 255).astype(np.uint8)
    elif kind == "checker":   # 1-px 0/255 checkerboard, inverted every frame
        for f in range(count):
            out[f] = ((xx + yy + f) % 2 * 255).astype(np.uint8)
    elif kind in SHIFTS:      # frame f (x, y) = frame f - 1 (x + dx, y + dy): windows of one canvas
        dx, dy = SHIFTS[kind]
        n = count - 1
        base = smooth(w + abs(dx) * n, h + abs(dy) * n, seed)
        ox, oy = (0 if dx > 0 else -dx * n), (0 if dy > 0 else -dy * n)
        for f in range(count):
            out[f] = base[oy + dy * f: oy + dy * f + h, ox + dx * f: ox + dx * f + w]
    else:
        raise ValueError(f"unknown pattern kind {kind!r}")
    return out


def frames(kind: str, w: int, h: int, count: int, seed: int = DEFAULT_SEED) -> np.ndarray:
    """``count`` distinct frames (seed + frame index), shape (count, h, w).  Kind "P" (panning):
    windows of one larger "mixed" picture moving by (3, 2) px per frame plus +-2 noise -- content
    a motion search can follow (the P-frame tests).  The kinds of ``_pattern_frames`` are whole
    videos built to reach one P-frame path each."""
    if kind in PATTERNS:
        return _pattern_frames(kind, w, h, count, seed)
    out = np.empty((count, h, w), dtype=np.uint8)
    if kind in ("P", "panning"):
        base = mixed(w + 3 * count + 8, h + 2 * count + 8, seed).astype(np.int64)
        for f in range(count):
            noise = (splitmix64(seed + 1 + f, 0, w * h) % np.uint64(5)).astype(np.int64).reshape(h, w) - 2
            out[f] = np.clip(base[2 * f: 2 * f + h, 3 * f: 3 * f + w] + noise, 0, 255).astype(np.uint8)
        return out
    for f in range(count):
        out[f] = frame(kind, w, h, seed + f)
    return out


def yuv420(y: np.ndarray, fill: int = 0x80) -> bytes:
    """Pack (count, h, w) Y planes as a YUV420 file: Y then w*h/2 chroma bytes per frame
    (VideoBase.cpp:8-9,39-40 read only the Y plane)."""
    count, h, w = y.shape
    buf = np.full((count, h * w + h * w // 2), fill, dtype=np.uint8)
    buf[:, : h * w] = y.reshape(count, h * w)
    return buf.tobytes()


def _u64(v: int) -> int:
    """A 64-bit constant as the signed int64 torch stores (two's complement)."""
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def uniform_device(w: int, h: int, count: int, seed: int, device, torch=None):
    """``frames("U", w, h, count, seed)`` generated on a torch device: the same splitmix64 bytes
    (int64 arithmetic wraps like uint64; right shifts are masked to be logical).  Bench and test
    data only -- the generator, not the product."""
    if torch is None:
        import torch
    out = torch.empty((count, h, w), dtype=torch.uint8, device=device)
    n = w * h
    i = torch.arange(1, n + 1, dtype=torch.int64, device=device)
    g, m1, m2 = _u64(0x9E3779B97F4A7C15), _u64(0xBF58476D1CE4E5B9), _u64(0x94D049BB133111EB)

    def srl(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    for f in range(count):
        z = i * g + _u64(seed + f)
        z = (z ^ srl(z, 30)) * m1
        z = (z ^ srl(z, 27)) * m2
        z = z ^ srl(z, 31)
        out[f].view(-1).copy_((z & 0xFF).to(torch.uint8))
    return out
