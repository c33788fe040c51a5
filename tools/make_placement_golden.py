#!/usr/bin/env python3
"""Writes tests/golden/placement/pillow_placement.json: what Pillow gives for
    canvas = Image.new(mode, (ow, oh), fill); canvas.paste(src.resize((rw, rh), Image.BILINEAR), (x, y))
on seeded random images, as sha256 hashes.  tests/test_placement.py holds tests/placement_ref.py — the numpy statement of DESIGN.md
§4.14 — to every case, without Pillow.  Needs Pillow (the file records the version used).

A case is (seed, H, W, C, ow, oh, rw, rh, x, y, fill); its input is np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8).
No case has H > 100 W with rh < H (Pillow runs the vertical pass first there, which differs by +-1)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "placement", "pillow_placement.json")

# (H, W, C, ow, oh, rw, rh, x, y, fill): the evaluation transform and the letterbox of real sizes; crop, pad and mixed; 1 x 1 visible at every
# corner; up-scaling; the identity
FIXED = [(375, 500, 3, 224, 224, 341, 256, -58, -16, (0, 0, 0, 0)), (1080, 1920, 3, 224, 224, 455, 256, -116, -16, (0, 0, 0, 0)),
         (500, 375, 3, 224, 224, 256, 341, -16, -58, (1, 2, 3, 0)), (480, 640, 3, 640, 640, 640, 480, 0, 80, (114, 114, 114, 0)),
         (500, 333, 3, 640, 640, 426, 640, 107, 0, (114, 114, 114, 0)), (33, 29, 4, 13, 21, 40, 50, -5, -7, (9, 8, 7, 6)),
         (97, 131, 1, 3, 3, 61, 45, -60, -44, (200, 0, 0, 0)), (97, 131, 1, 3, 3, 61, 45, 2, -44, (200, 0, 0, 0)),
         (97, 131, 3, 3, 3, 61, 45, -60, 2, (200, 100, 50, 0)), (97, 131, 4, 3, 3, 61, 45, 2, 2, (200, 100, 50, 25)),
         (17, 9, 3, 37, 53, 27, 51, 5, 1, (114, 7, 200, 0)), (17, 9, 1, 37, 53, 27, 51, -3, 30, (114, 0, 0, 0)),
         (34, 50, 3, 224, 224, 150, 102, 37, 61, (255, 0, 255, 0)), (34, 50, 4, 7, 9, 150, 102, -71, -40, (0, 0, 0, 0)),
         (50, 34, 3, 2048, 3, 102, 150, 1000, -70, (1, 1, 1, 0)), (50, 34, 1, 2048, 3, 2048, 3, 0, 0, (77, 0, 0, 0)),
         (161, 97, 3, 16, 200, 5, 8, 6, 150, (114, 114, 114, 0)), (1100, 24, 3, 7, 7, 2, 1, 1, 3, (5, 6, 7, 0)),
         (8, 1200, 3, 7, 7, 9, 1, -1, 6, (5, 6, 7, 0)), (224, 224, 3, 224, 224, 224, 224, 0, 0, (9, 9, 9, 0)),
         (34, 50, 4, 64, 48, 40, 27, 13, 11, (10, 20, 30, 40))]


def cases():
    out = [(300 + k, *c) for k, c in enumerate(FIXED)]
    rng = np.random.default_rng(414)
    while len(out) < 33:
        H, W, C = int(rng.integers(1, 300)), int(rng.integers(1, 400)), int(rng.choice([1, 3, 4]))
        ow, oh = int(rng.integers(1, 260)), int(rng.integers(1, 260))
        rw, rh = int(rng.integers(1, 500)), int(rng.integers(1, 500))
        x, y = int(rng.integers(1 - rw, ow)), int(rng.integers(1 - rh, oh))
        if H > 100 * W and rh < H:
            continue
        fill = tuple(int(v) for v in rng.integers(0, 256, 4))
        out.append((3000 + len(out), H, W, C, ow, oh, rw, rh, x, y, fill))
    return out


def main():
    import PIL
    from PIL import Image
    rows = []
    for seed, H, W, C, ow, oh, rw, rh, x, y, fill in cases():
        assert not (H > 100 * W and rh < H)
        a = np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)
        mode = {1: "L", 3: "RGB", 4: "CMYK"}[C]
        im = Image.fromarray(a[:, :, 0] if C == 1 else a, mode)
        canvas = Image.new(mode, (ow, oh), fill[0] if C == 1 else tuple(fill[:C]))
        canvas.paste(im.resize((rw, rh), Image.BILINEAR), (x, y))
        got = np.asarray(canvas).reshape(oh, ow, C)
        rows.append({"seed": seed, "H": H, "W": W, "C": C, "ow": ow, "oh": oh, "rw": rw, "rh": rh, "x": x, "y": y, "fill": list(fill),
                     "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"pillow": PIL.__version__, "filter": "BILINEAR", "cases": rows}, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} cases -> {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
