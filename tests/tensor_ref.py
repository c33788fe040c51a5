"""The tensor output of DESIGN.md §4.11 stated in numpy: a table of nc x 256 elements made in IEEE single precision, one operation per
statement, looked up with the resized u8 image (tests/resample_ref.py), planes first, columns mirrored by a flip.  The reference of
every tensor test (CPU and GPU)."""
import numpy as np

DTYPES = ("float32", "float16", "bfloat16")
NP_DTYPE = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}  # (numpy has no bfloat16: its bit patterns)

# (mean, std) a loader meets
IMAGENET = ((0.485, 0.456, 0.406, 0.0), (0.229, 0.224, 0.225, 1.0))
CLIP = ((0.48145466, 0.4578275, 0.40821073, 0.0), (0.26862954, 0.26130258, 0.27577711, 1.0))
HALF = ((0.5, 0.5, 0.5, 0.5), (0.5, 0.5, 0.5, 0.5))
IDENTITY = ((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0))


def bf16_bits(f32):
    """float32 array -> uint16 bit patterns of bfloat16, round to nearest even."""
    x = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    nan = (x & 0x7FFFFFFF) > 0x7F800000
    r = (x + 0x7FFF + ((x >> 16) & 1)) >> 16
    return np.where(nan, (x >> 16) | 0x40, r).astype(np.uint16)


def table(fmt, nc):
    """fmt = (dtype name, mean, std) -> (nc, 256) array of NP_DTYPE[dtype]."""
    dtype, mean, std = fmt
    v = np.arange(256, dtype=np.float32)
    rows = []
    with np.errstate(over="ignore"):
        for c in range(nc):
            a = v / np.float32(255.0)
            b = a - np.float32(mean[c])
            t = b / np.float32(std[c])
            assert t.dtype == np.float32
            rows.append(t)
        t = np.stack(rows)
        if dtype == "float32":
            return t
        if dtype == "float16":
            return t.astype(np.float16)
    assert dtype == "bfloat16", dtype
    return bf16_bits(t)


def to_tensor(u8_hwc, tab, flip):
    """(oh, ow, nc) u8, table (nc, 256), flip -> (nc, oh, ow) of the table's dtype."""
    u8 = np.asarray(u8_hwc, np.uint8)
    if flip:
        u8 = u8[:, ::-1, :]
    nc = u8.shape[2]
    return np.ascontiguousarray(np.stack([tab[c][u8[:, :, c]] for c in range(nc)]))


def bits(a):
    """An array's bit patterns (NaNs and signed zeros compare as what they are)."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])
