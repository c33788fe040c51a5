"""The placement of DESIGN.md §4.14 stated in numpy and plain Python: `resample_ref.resize(src, rw, rh)` pasted at (x, y) into a canvas
of `fill`, and the two fit rules.  The reference of every placement test (CPU and GPU); the golden hashes of
tests/golden/placement/pillow_placement.json pin it to Pillow's `Image.new(mode, (ow, oh), fill)` + `paste(src.resize(...), (x, y))`."""
import numpy as np

import resample_ref as R


def place(src, ow, oh, placement, fill=(0, 0, 0, 0)):
    """src (H, W, C) u8 -> (oh, ow, C) u8: the resample of src to rw x rh with its top-left pixel at (x, y) of the canvas, cropped at
    the canvas, `fill[c]` where it does not cover.  placement None = (ow, oh, 0, 0)."""
    src = np.asarray(src, np.uint8)
    nc = src.shape[2]
    rw, rh, x, y = (ow, oh, 0, 0) if placement is None else placement
    canvas = np.empty((oh, ow, nc), np.uint8)
    canvas[:] = np.asarray(list(fill)[:nc], np.uint8)
    x0, x1, y0, y1 = max(x, 0), min(x + rw, ow), max(y, 0), min(y + rh, oh)
    assert x0 < x1 and y0 < y1, "the placement shows no pixel"
    r = R.resize(src, rw, rh)
    canvas[y0:y1, x0:x1] = r[y0 - y:y1 - y, x0 - x:x1 - x]
    return canvas


def fit_shorter_side_crop(w, h, size, ow, oh):
    """torchvision's Resize(size) then CenterCrop((oh, ow)) -> (rw, rh, x, y)."""
    if w <= h:
        rw, rh = size, int(size * h / w)
    else:
        rh, rw = size, int(size * w / h)

    def offset(r, out):
        if r >= out:
            return -int(round((r - out) / 2.0))  # (Python's round: a half goes to the even neighbour)
        return (out - r) // 2
    return rw, rh, offset(rw, ow), offset(rh, oh)


def fit_letterbox(w, h, ow, oh):
    """The aspect-preserving fit into ow x oh -> (rw, rh, x, y); IEEE double, one operation per statement."""
    r = min(ow / w, oh / h)
    rw = min(max(1, int(np.rint(w * r))), ow)
    rh = min(max(1, int(np.rint(h * r))), oh)
    x = int(np.rint((ow - rw) / 2.0 - 0.1))
    y = int(np.rint((oh - rh) / 2.0 - 0.1))
    return rw, rh, x, y

