"""The resample of DESIGN.md §4.15 stated in numpy: Pillow's 8-bit `Image.resize(size, F)` for F in BOX, BILINEAR, HAMMING, BICUBIC and
LANCZOS, horizontal pass first.  The reference of every filter test (CPU and GPU); the golden hashes of
tests/golden/filters/pillow_filters.json pin it to Pillow itself.  sin and cos are math's (libm's), every step is IEEE double, one
operation at a time.  Its BILINEAR is resample_ref's, table for table."""
import math

import numpy as np

PRECISION_BITS = 22
BILINEAR, BOX, HAMMING, BICUBIC, LANCZOS = 0, 1, 2, 3, 4
NAMES = {"bilinear": BILINEAR, "box": BOX, "hamming": HAMMING, "bicubic": BICUBIC, "lanczos": LANCZOS}
SUPPORT = {BILINEAR: 1.0, BOX: 0.5, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
_F32_054 = float(np.float32(0.54))  # (Pillow's hamming constants are float literals promoted to double)
_F32_046 = float(np.float32(0.46))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def weight(f, x):
    """f(x) on the signed argument."""
    if f == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if f == LANCZOS:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    if x < 0.0:
        x = -x
    if f == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    if f == HAMMING:
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (_F32_054 + _F32_046 * math.cos(x))
    if f == BICUBIC:
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    raise ValueError(f)


def ksize_of(in_size, out_size, f=BILINEAR):
    scale = in_size / out_size
    fs = scale if scale >= 1.0 else 1.0
    return int(math.ceil(SUPPORT[f] * fs)) * 2 + 1


def coefficients_range(in_size, out_size, first, count, f=BILINEAR):
    """Entries [first, first + count) of the axis: (bounds int32 (count, 2) of (xmin, n), coefs int32 (count, ksize), zero beyond n)."""
    scale = in_size / out_size
    fs = scale if scale >= 1.0 else 1.0
    support = SUPPORT[f] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((count, 2), np.int32)
    coefs = np.zeros((count, ksize), np.int32)
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [weight(f, (x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww = ww + v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            coefs[i, x] = int(-0.5 + v * float(1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * float(1 << PRECISION_BITS))
        bounds[i] = (xmin, n)
    return bounds, coefs


_CACHE = {}


def coefficients(in_size, out_size, f=BILINEAR):
    key = (in_size, out_size, f)
    if key not in _CACHE:
        if len(_CACHE) > 64:
            _CACHE.clear()
        _CACHE[key] = coefficients_range(in_size, out_size, 0, out_size, f)
    return _CACHE[key]


def pass_sums(img, b, k):
    """The unclamped sums (int64, rounding term included) of one pass along axis 1 of img (H, W, C) under the tables (b, k)."""
    W = img.shape[1]
    acc = np.full((img.shape[0], b.shape[0], img.shape[2]), 1 << (PRECISION_BITS - 1), np.int64)
    for x in range(k.shape[1]):
        idx = np.minimum(b[:, 0] + x, W - 1)  # (beyond n the coefficient is 0)
        acc += img[:, idx, :].astype(np.int64) * k[:, x].astype(np.int64)[None, :, None]
    return acc


def _pass_axis1(img, b, k, sums=None):
    acc = pass_sums(img, b, k)
    assert acc.min() >= -(1 << 31) and acc.max() < (1 << 31)  # (the device's int32 holds it)
    if sums is not None:
        sums.append((int(acc.min()), int(acc.max())))
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, ow, oh, f=BILINEAR, xrange=None, yrange=None, sums=None):
    """img (H, W, C) u8 -> (oh, ow, C) u8: the horizontal pass, clamped and rounded to u8, then the vertical pass on its result.
    xrange / yrange = (first, count): only those columns / rows of the result (what a placement shows).  `sums`, a list, receives the
    (min, max) of the unclamped sums of the horizontal and of the vertical pass."""
    img = np.asarray(img, np.uint8)
    assert img.ndim == 3 and ow >= 1 and oh >= 1
    H, W = img.shape[:2]
    hb, hk = coefficients(W, ow, f) if xrange is None else coefficients_range(W, ow, xrange[0], xrange[1], f)
    vb, vk = coefficients(H, oh, f) if yrange is None else coefficients_range(H, oh, yrange[0], yrange[1], f)
    t = _pass_axis1(img, hb, hk, sums)
    t = _pass_axis1(t.transpose(1, 0, 2), vb, vk, sums).transpose(1, 0, 2)
    return np.ascontiguousarray(t)


def placed(img, rw, rh, x, y, ow, oh, fill, f=BILINEAR):
    """canvas = Image.new(mode, (ow, oh), fill); canvas.paste(src.resize((rw, rh), F), (x, y))."""
    img = np.asarray(img, np.uint8)
    C = img.shape[2]
    out = np.empty((oh, ow, C), np.uint8)
    out[:] = np.asarray(fill[:C], np.uint8)
    x0, x1, y0, y1 = max(x, 0), min(x + rw, ow), max(y, 0), min(y + rh, oh)
    assert x0 < x1 and y0 < y1
    out[y0:y1, x0:x1] = resize(img, rw, rh, f, (x0 - x, x1 - x0), (y0 - y, y1 - y0))
    return out
