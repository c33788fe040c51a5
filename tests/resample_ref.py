"""The resample of DESIGN.md §4.10 stated in numpy: the 8-bit integer bilinear resample with antialiasing that Pillow's
`Image.resize(size, BILINEAR)` performs, horizontal pass first.  The reference of every resample test (CPU and GPU); the golden
hashes of tests/golden/resample/pillow_bilinear.json pin it to Pillow itself."""
import numpy as np

PRECISION_BITS = 22


def ksize_of(in_size, out_size):
    scale = in_size / out_size
    fs = scale if scale >= 1.0 else 1.0
    return int(np.ceil(fs)) * 2 + 1


def coefficients(in_size, out_size):
    """(bounds int32 (out_size, 2) of (xmin, n), coefs int32 (out_size, ksize), zero beyond n) — every step in IEEE double, in the
    order of the statement."""
    scale = in_size / out_size
    fs = scale if scale >= 1.0 else 1.0
    support = fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    w = np.zeros((out_size, ksize), np.float64)
    ww = np.zeros(out_size, np.float64)
    for x in range(ksize):
        a = np.abs(((x + xmin) - center + 0.5) * ss)
        wx = np.where((a < 1.0) & (x < n), 1.0 - a, 0.0)
        w[:, x] = wx
        ww = ww + wx  # (index order; the terms beyond n are +0.0)
    ww = np.where(ww != 0.0, ww, 1.0)
    k = np.trunc(w / ww[:, None] * float(1 << PRECISION_BITS) + 0.5).astype(np.int32)
    return np.stack([xmin, n], axis=1).astype(np.int32), k


def _pass_axis1(img, out_size):
    """img (H, W, C) u8 -> (H, out_size, C) u8 along axis 1."""
    W = img.shape[1]
    b, k = coefficients(W, out_size)
    acc = np.full((img.shape[0], out_size, img.shape[2]), 1 << (PRECISION_BITS - 1), np.int32)  # (the sum stays below 2^31)
    for x in range(k.shape[1]):
        idx = np.minimum(b[:, 0] + x, W - 1)  # (beyond n the coefficient is 0)
        acc += img[:, idx, :].astype(np.int32) * k[:, x][None, :, None]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, ow, oh):
    """img (H, W, C) u8 -> (oh, ow, C) u8: the horizontal pass, rounded to u8, then the vertical pass on its result.  (An axis whose
    size does not change is the identity under the rules, so it may run or not.)"""
    img = np.asarray(img, np.uint8)
    assert img.ndim == 3 and ow >= 1 and oh >= 1
    t = _pass_axis1(img, ow)
    t = _pass_axis1(t.transpose(1, 0, 2), oh).transpose(1, 0, 2)
    return np.ascontiguousarray(t)
