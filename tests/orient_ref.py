"""TEST-ONLY: the EXIF orientation in numpy (include/jpgpu.h, "EXIF orientation") — the oriented image O of a source S
(H, W, nc) is Pillow's Image.transpose(method) under ImageOps.exif_transpose's mapping — the window mapping, and the reading of the
orientation tag out of an EXIF blob (the payload behind "Exif\\0\\0")."""
import struct

import numpy as np

PILLOW_METHOD = {1: None, 2: "FLIP_LEFT_RIGHT", 3: "ROTATE_180", 4: "FLIP_TOP_BOTTOM", 5: "TRANSPOSE", 6: "ROTATE_270", 7: "TRANSVERSE", 8: "ROTATE_90"}


def orient(a, o):
    """O of S = a (H, W[, nc]) under orientation o (1..8)."""
    a = np.asarray(a)
    if o == 1:
        out = a
    elif o == 2:
        out = np.flip(a, 1)
    elif o == 3:
        out = np.flip(np.flip(a, 0), 1)
    elif o == 4:
        out = np.flip(a, 0)
    elif o == 5:
        out = np.swapaxes(a, 0, 1)
    elif o == 6:
        out = np.rot90(a, -1, (0, 1))
    elif o == 7:
        out = np.flip(np.flip(np.swapaxes(a, 0, 1), 0), 1)
    elif o == 8:
        out = np.rot90(a, 1, (0, 1))
    else:
        raise ValueError(f"orientation {o}")
    return np.ascontiguousarray(out)


def oriented_size(o, w, h):
    """(w, h) of O for a source of w x h."""
    return (h, w) if o >= 5 else (w, h)


def source_window(o, w, h, window):
    """The window (x, y, ww, wh) of O — None: all of it — as the window of S (w x h) whose orientation it is; None stays None.
    ValueError for a window outside O."""
    if window is None or window[2] == 0 or window[3] == 0:
        return None
    x, y, ww, wh = window
    ow, oh = oriented_size(o, w, h)
    if x + ww > ow or y + wh > oh:
        raise ValueError(f"window {window} outside the oriented {ow}x{oh} image")
    # the table of the header, read for the corners: O's column x is S's column (2, 3) / row (5..8), and so on
    cx, cw, ry, rh = (y, wh, x, ww) if o >= 5 else (x, ww, y, wh)
    sx = w - cx - cw if o in (2, 3, 7, 8) else cx
    sy = h - ry - rh if o in (3, 4, 6, 7) else ry
    return (sx, sy, cw, rh)


def exif_orientation(blob):
    """The orientation an EXIF blob states: tag 0x0112 of IFD0, type SHORT, count 1, value 1..8 — else 1.  Never raises."""
    b = bytes(blob or b"")
    if len(b) < 8 or b[:2] not in (b"II", b"MM"):
        return 1
    e = "<" if b[:2] == b"II" else ">"
    if struct.unpack(e + "H", b[2:4])[0] != 42:
        return 1
    ifd = struct.unpack(e + "I", b[4:8])[0]
    if ifd + 2 > len(b):
        return 1
    n = struct.unpack(e + "H", b[ifd:ifd + 2])[0]
    for k in range(n):
        at = ifd + 2 + 12 * k
        if at + 12 > len(b):
            return 1
        tag, typ, count = struct.unpack(e + "HHI", b[at:at + 8])
        if tag != 0x0112:
            continue
        if typ != 3 or count != 1:
            return 1
        v = struct.unpack(e + "H", b[at + 8:at + 10])[0]
        return v if 1 <= v <= 8 else 1
    return 1
