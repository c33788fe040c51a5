#!/usr/bin/env python3
"""Writes tests/golden/warp/pillow_warp.json: what Pillow gives for
    src.transform((W, H), Image.AFFINE, m, resample, fillcolor=fill)
on seeded random images, as sha256 hashes.  tests/test_warp.py holds tests/warp_ref.py — the numpy statement of DESIGN.md §4.16 — to
every case, without Pillow.  Needs Pillow (the file records the version used).

A case is (seed, H, W, C, filter, m, fill); its input is np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8), modes
L, RGB and CMYK for C = 1, 3, 4.  Every matrix passes the refusal rule of §4.16 for its size."""
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "warp", "pillow_warp.json")


def rotation(angle, w, h):
    """Image.rotate's matrix about the centre."""
    r = -math.radians(angle % 360.0)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2] + cx, m[3] * -cx + m[4] * -cy + m[5] + cy
    return tuple(m)


# (H, W, matrix): the kinds of DESIGN.md §4.16 — identity, fractional translation, pure scales, a negative m[0], a quarter turn on a
# non-square size, rotations, shears, everything outside, a large zoom, matrices at the refusal bounds
def fixed():
    H, W = 37, 53
    return [(H, W, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)), (H, W, (1.0, 0.0, 3.3, 0.0, 1.0, -2.7)), (H, W, (0.5, 0.0, 0.0, 0.0, 0.5, 0.0)),
            (H, W, (1.7, 0.0, -5.2, 0.0, 0.9, 3.1)), (H, W, (-1.0, 0.0, float(W), 0.0, 1.0, 0.0)), (H, W, (-0.77, 0.0, 40.4, 0.0, -1.3, 41.9)),
            (H, W, rotation(90, W, H)), (H, W, rotation(15, W, H)), (H, W, rotation(33.3, W, H)), (H, W, rotation(180, W, H)), (H, W, rotation(270, W, H)),
            (40, 40, rotation(90, 40, 40)), (H, W, (1.0, 0.3, -4.0, 0.0, 1.0, 0.0)), (H, W, (1.0, 0.0, 0.0, 0.2, 1.0, -3.0)),
            (H, W, (1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0)), (H, W, (1.0, 0.25, -9000.0, 0.1, 1.0, 0.0)),
            (H, W, (0.01, 0.002, 10.0, -0.003, 0.01, 7.0)), (H, W, (0.004, 0.0, 20.1, 0.0, 0.004, 11.3)),
            (3, 4, (16000.0, 0.0, -32000.0, 0.0, 16000.0, -16000.0)), (4, 4, (0.0, 16000.0, -32000.0, -16000.0, 0.0, 32000.0)),
            (H, W, (1.0, 0.0, 32000.0 - W, 0.0, 1.0, -32000.0)), (1, 1, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)), (1, 1, (0.3, 0.2, 0.1, -0.2, 0.3, 0.4))]


def cases():
    out = []
    for k, (H, W, m) in enumerate(fixed()):
        for f in (0, 1):
            out.append((500 + len(out), H, W, (1, 3, 4)[(k + f) % 3], f, m, (7 * k % 256, 200, 33, 91)))
    rng = np.random.default_rng(416)
    for k in range(16):  # rotation, scale, shear and translation together
        H, W = int(rng.integers(2, 70)), int(rng.integers(2, 90))
        ang, sc, sh = rng.uniform(0, 2 * math.pi), rng.uniform(0.4, 2.5), rng.uniform(-0.5, 0.5)
        a, b, d, e = sc * math.cos(ang), sc * (math.sin(ang) + sh), -sc * math.sin(ang), sc * math.cos(ang)
        cx, cy = W / 2.0 + rng.uniform(-5, 5), H / 2.0 + rng.uniform(-5, 5)
        m = (a, b, cx - a * cx - b * cy, d, e, cy - d * cx - e * cy)
        for f in (0, 1):
            out.append((5000 + len(out), H, W, (1, 3, 4)[k % 3], f, m, tuple(int(v) for v in rng.integers(0, 256, 4))))
    for k in range(10):  # N-sep at widths where the sequential sum of doubles parts from the fixed-point road
        H, W = 3, int(rng.integers(1000, 2049))
        m = (rng.uniform(0.3, 1.9), 0.0, rng.uniform(-300, 50), 0.0, rng.uniform(0.5, 1.5), rng.uniform(-1, 1))
        out.append((9000 + len(out), H, W, (3, 1, 4)[k % 3], 0, m, tuple(int(v) for v in rng.integers(0, 256, 4))))
    return out


def main():
    import PIL
    from PIL import Image
    rows = []
    for seed, H, W, C, f, m, fill in cases():
        a = np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)
        mode = {1: "L", 3: "RGB", 4: "CMYK"}[C]
        im = Image.fromarray(a[:, :, 0] if C == 1 else a, mode)
        got = im.transform((W, H), Image.AFFINE, tuple(float(v) for v in m), Image.BILINEAR if f else Image.NEAREST, fillcolor=fill[0] if C == 1 else tuple(fill[:C]))
        got = np.asarray(got).reshape(H, W, C)
        rows.append({"seed": seed, "H": H, "W": W, "C": C, "filter": f, "m": [float(v) for v in m], "fill": list(fill),
                     "sha256": hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump({"pillow": PIL.__version__, "cases": rows}, fh, indent=1)
        fh.write("\n")
    print(f"{len(rows)} cases -> {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
