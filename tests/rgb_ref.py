"""The RGB output of DESIGN.md §4.12 stated in numpy: what ``Image.convert("RGB")`` gives for the pixel formats the decoder writes —
gray replicated, three channels as they are, CMYK (ink amounts, 0 = no ink) through Pillow's integer cmyk2rgb.  Applied to the source
pixels BEFORE tests/resample_ref.py's resize: the reference of every RGB-output test (CPU and GPU)."""
import numpy as np


def cmyk_ink(x, k):
    """One ink channel X under black K (arrays or scalars, 0..255) -> the RGB channel, in 32-bit integers."""
    x = np.asarray(x, np.int32)
    nk = np.int32(255) - np.asarray(k, np.int32)
    t = x * nk + 128
    md = ((t >> 8) + t) >> 8
    return (nk - md).astype(np.uint8)


def to_rgb(hwc_u8):
    """(H, W, nc) u8 with nc in (1, 3, 4) -> (H, W, 3) u8."""
    a = np.asarray(hwc_u8, np.uint8)
    assert a.ndim == 3 and a.shape[2] in (1, 3, 4), a.shape
    if a.shape[2] == 3:
        return np.ascontiguousarray(a)
    if a.shape[2] == 1:
        return np.ascontiguousarray(np.repeat(a, 3, axis=2))
    k = a[:, :, 3]
    return np.ascontiguousarray(np.stack([cmyk_ink(a[:, :, c], k) for c in range(3)], axis=2))
