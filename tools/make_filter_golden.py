#!/usr/bin/env python3
"""Writes tests/golden/filters/pillow_filters.json: what Pillow's Image.resize((ow, oh), F) gives for F in BOX, BILINEAR, HAMMING,
BICUBIC and LANCZOS on seeded images, as sha256 hashes.  tests/test_filters.py holds tests/filter_ref.py — the numpy statement of
DESIGN.md §4.15 — to every case, without Pillow.  Needs Pillow (any version whose 8-bit resample has PRECISION_BITS = 22; the file
records the one used).

A resize case is (seed, kind, H, W, C, ow, oh).  kind "random": np.random.default_rng(seed).integers(0, 256, (H, W, C), uint8); kind
"blocks": 0 / 255 blocks of 1..4 pixels (default_rng(seed).integers(0, 2, ...) * 255 repeated by 1 + seed % 4 and cut to size) — the
images on which negative lobes leave 0..255.  A placement case adds (rw, rh, x, y, fill): Image.new(mode, (ow, oh), fill) with
src.resize((rw, rh), F) pasted at (x, y).  No case has H > 100 W with a smaller output height: there Pillow's Python wrapper runs the
vertical pass first, which this project never does."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "filters", "pillow_filters.json")
FILTERS = ["bilinear", "box", "hamming", "bicubic", "lanczos"]

# (H, W, C, ow, oh)
FIXED = [(1080, 1920, 3, 224, 224), (2160, 3840, 1, 224, 224), (375, 500, 3, 224, 224), (17, 23, 3, 224, 224), (224, 224, 3, 224, 224),
         (300, 224, 3, 224, 224), (224, 500, 4, 224, 224), (1, 1, 3, 8, 8), (1, 1, 1, 1, 1), (9, 7, 3, 64, 48), (61, 97, 4, 37, 53),
         (1200, 16, 3, 16, 12), (3, 1079, 3, 300, 5), (64, 64, 4, 1, 1), (5, 5, 1, 2048, 3), (400, 64, 3, 24, 40), (480, 640, 4, 640, 480),
         (2160, 64, 3, 64, 224)]
# (H, W, C, rw, rh, x, y, ow, oh, fill)
PLACED = [(375, 500, 3, 224, 168, 0, 28, 224, 224, (114, 114, 114, 0)), (375, 500, 3, 298, 224, -37, 0, 224, 224, (0, 0, 0, 0)),
          (61, 97, 1, 40, 90, 30, -20, 64, 48, (7, 0, 0, 0)), (90, 50, 4, 25, 45, -3, 10, 32, 40, (1, 2, 3, 4)),
          (9, 7, 3, 64, 48, -10, -5, 37, 53, (255, 0, 128, 0))]


def image(seed, kind, H, W, C):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    s = 1 + seed % 4
    a = rng.integers(0, 2, ((H + s - 1) // s, (W + s - 1) // s, C), dtype=np.uint8) * np.uint8(255)
    return np.ascontiguousarray(a.repeat(s, axis=0).repeat(s, axis=1)[:H, :W])


def cases():
    out = [(100 + k, "blocks" if k % 2 else "random", *c) for k, c in enumerate(FIXED)]
    rng = np.random.default_rng(2025)
    while len(out) < 32:
        H, W, C = int(rng.integers(1, 700)), int(rng.integers(1, 900)), int(rng.choice([1, 3, 4]))
        ow, oh = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        if H > 100 * W and oh < H:
            continue
        out.append((1000 + len(out), "blocks" if len(out) % 2 else "random", H, W, C, ow, oh))
    return out


def main():
    import PIL
    from PIL import Image
    modes = {1: "L", 3: "RGB", 4: "CMYK"}
    rows = []
    for name in FILTERS:
        F = getattr(Image, name.upper())
        for seed, kind, H, W, C, ow, oh in cases():
            assert not (H > 100 * W and oh < H)
            a = image(seed, kind, H, W, C)
            im = Image.fromarray(a[:, :, 0] if C == 1 else a, modes[C])
            got = np.asarray(im.resize((ow, oh), F)).reshape(oh, ow, C)
            rows.append({"filter": name, "seed": seed, "kind": kind, "H": H, "W": W, "C": C, "ow": ow, "oh": oh,
                         "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()})
        for k, (H, W, C, rw, rh, x, y, ow, oh, fill) in enumerate(PLACED):
            assert not (H > 100 * W and rh < H)
            seed, kind = 500 + k, "blocks" if k % 2 else "random"
            a = image(seed, kind, H, W, C)
            im = Image.fromarray(a[:, :, 0] if C == 1 else a, modes[C])
            canvas = Image.new(modes[C], (ow, oh), fill[0] if C == 1 else tuple(fill[:C]))
            canvas.paste(im.resize((rw, rh), F), (x, y))
            got = np.asarray(canvas).reshape(oh, ow, C)
            rows.append({"filter": name, "seed": seed, "kind": kind, "H": H, "W": W, "C": C, "ow": ow, "oh": oh, "place": [rw, rh, x, y], "fill": list(fill),
                         "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"pillow": PIL.__version__, "filters": FILTERS, "cases": rows}, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} cases -> {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
