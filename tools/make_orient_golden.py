#!/usr/bin/env python3
"""Writes tests/golden/orient/pillow_orient.json with Pillow (run on a machine that has it; the tests read the committed file).

  images: for each EXIF orientation 1..8 and 1, 3 and 4 channels, a small array, the bytes and size ImageOps.exif_transpose gives for
          it with that orientation in its EXIF, and the orientation Pillow read.
  exif:   hand-made EXIF blobs (the payload behind "Exif\\0\\0") — both byte orders, the tag absent, values 0 and 9, type LONG, count 2,
          an IFD cut short — each with the orientation include/jpgpu.h's rule gives (`orientation`, stated here by hand per blob) and
          what Pillow's Exif reader makes of the tag (`pillow`, null where it raises; it is laxer about the tag's type and count).
"""
import json
import os
import struct
import sys

import numpy as np
import PIL
from PIL import Image, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "orient", "pillow_orient.json")
MODES = {1: "L", 3: "RGB", 4: "CMYK"}
H, W = 5, 7


def ifd(e, entries, next_ifd=0):
    """IFD bytes: entries are (tag, type, count, value bytes of 4)."""
    b = struct.pack(e + "H", len(entries))
    for tag, typ, count, value in entries:
        b += struct.pack(e + "HHI", tag, typ, count) + value
    return b + struct.pack(e + "I", next_ifd)


def tiff(e, body, offset=8, magic=42):
    return (b"II" if e == "<" else b"MM") + struct.pack(e + "HI", magic, offset) + body


def short(e, v):
    return struct.pack(e + "HH", v, 0)


def blobs():
    out = []
    for e, name in (("<", "II"), (">", "MM")):
        make = (0x010F, 2, 4, b"abc\0")
        out.append((f"{name} orientation 6", tiff(e, ifd(e, [(0x0112, 3, 1, short(e, 6))])), 6))
        out.append((f"{name} orientation 8 behind another tag", tiff(e, ifd(e, [make, (0x0112, 3, 1, short(e, 8))])), 8))
        out.append((f"{name} tag absent", tiff(e, ifd(e, [make])), 1))
        out.append((f"{name} value 0", tiff(e, ifd(e, [(0x0112, 3, 1, short(e, 0))])), 1))
        out.append((f"{name} value 9", tiff(e, ifd(e, [(0x0112, 3, 1, short(e, 9))])), 1))
        out.append((f"{name} type LONG", tiff(e, ifd(e, [(0x0112, 4, 1, struct.pack(e + "I", 6))])), 1))
        out.append((f"{name} count 2", tiff(e, ifd(e, [(0x0112, 3, 2, struct.pack(e + "HH", 6, 6))])), 1))
        whole = tiff(e, ifd(e, [make, (0x0112, 3, 1, short(e, 6))]))
        out.append((f"{name} IFD cut inside the orientation entry", whole[:8 + 2 + 12 + 7], 1))
        out.append((f"{name} IFD offset beyond the blob", tiff(e, b"", offset=4000), 1))
        out.append((f"{name} wrong magic", tiff(e, ifd(e, [(0x0112, 3, 1, short(e, 6))]), magic=43), 1))
        out.append((f"{name} IFD at an offset of 12", tiff(e, b"\0\0\0\0" + ifd(e, [(0x0112, 3, 1, short(e, 3))]), offset=12), 3))
    out.append(("empty", b"", 1))
    out.append(("header alone", b"II*\0", 1))
    out.append(("no TIFF", b"XX*\0\x08\0\0\0" + b"\0" * 14, 1))
    return out


def pillow_reads(blob):
    try:
        ex = Image.Exif()
        ex.load(b"Exif\0\0" + blob)
        v = ex.get(0x0112)
        return v if isinstance(v, int) else (list(v) if isinstance(v, tuple) else None)
    except Exception:
        return None


def main():
    rng = np.random.default_rng(20)
    images = []
    for nc, mode in MODES.items():
        a = rng.integers(0, 256, (H, W, nc), dtype=np.uint8)
        for o in range(1, 9):
            im = Image.fromarray(a[:, :, 0] if nc == 1 else a, mode)
            im.getexif()[0x0112] = o
            read = im.getexif().get(0x0112)
            t = ImageOps.exif_transpose(im)
            images.append({"nc": nc, "orientation": o, "pillow_reads": read, "H": H, "W": W, "source": a.reshape(-1).tolist(),
                           "size": list(t.size), "oriented": np.asarray(t).reshape(-1).tolist()})
    exif = [{"name": n, "blob": b.hex(), "orientation": want, "pillow": pillow_reads(b)} for n, b, want in blobs()]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"pillow": PIL.__version__, "images": images, "exif": exif}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(images)} images, {len(exif)} blobs (Pillow {PIL.__version__})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
