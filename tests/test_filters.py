"""The resample filters of DESIGN.md §4.15 without a GPU: the numpy statement (tests/filter_ref.py) against Pillow's own output (hashes
made by tools/make_filter_golden.py — no Pillow needed here), the `_filtered` table functions of the C ABI against the statement, filter 0
against the functions that were there before, the 32-bit bound of the sums over a sweep of sizes, the refusals and the Python arguments."""
import ctypes as C
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import pytest

import jpeg_decoder_amd as J
import filter_ref as F
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_filter_golden as G  # noqa: E402  (the seeded images of the cases; its main() alone needs Pillow)

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "filters", "pillow_filters.json")))
FILTERS = ["bilinear", "box", "hamming", "bicubic", "lanczos"]


def test_golden_covers_what_it_should():
    assert GOLDEN["filters"] == FILTERS and [F.NAMES[n] for n in FILTERS] == [0, 1, 2, 3, 4]
    for name in FILTERS:
        cases = [c for c in GOLDEN["cases"] if c["filter"] == name]
        plain = [c for c in cases if "place" not in c]
        assert len(cases) >= 30 and len(cases) - len(plain) >= 3
        assert {c["C"] for c in plain} == {1, 3, 4} and {c["kind"] for c in plain} == {"random", "blocks"}
        assert any(c["H"] == 1 and c["W"] == 1 for c in plain) and any(c["H"] == 2160 for c in plain)
        assert not any(c["H"] > 100 * c["W"] and c["oh"] < c["H"] for c in plain)  # (Pillow's vertical-first order: not ours)
        assert any(c["ow"] > c["W"] and c["oh"] > c["H"] for c in plain) and any(c["ow"] < c["W"] and c["oh"] < c["H"] for c in plain)
        assert any((c["ow"] > c["W"]) != (c["oh"] > c["H"]) for c in plain) and any(c["ow"] == c["W"] and c["oh"] == c["H"] for c in plain)


def _case_id(c):
    return f"{c['filter']}-{c['W']}x{c['H']}x{c['C']}-{c['ow']}x{c['oh']}" + ("-placed" if "place" in c else "")


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=_case_id)
def test_numpy_statement_equals_pillow(case):
    a = G.image(case["seed"], case["kind"], case["H"], case["W"], case["C"])
    f = F.NAMES[case["filter"]]
    if "place" in case:
        got = F.placed(a, *case["place"], case["ow"], case["oh"], case["fill"], f)
    else:
        got = F.resize(a, case["ow"], case["oh"], f)
    assert got.shape == (case["oh"], case["ow"], case["C"]) and got.dtype == np.uint8
    assert hashlib.sha256(got.tobytes()).hexdigest() == case["sha256"]


def test_the_statements_bilinear_is_resample_ref():
    for pair in [(1, 1), (1080, 224), (224, 1080), (7, 7), (375, 224), (3, 2), (2, 3), (2160, 224)]:
        b, k = F.coefficients(*pair, F.BILINEAR)
        wb, wk = R.coefficients(*pair)
        assert np.array_equal(b, wb) and np.array_equal(k, wk) and F.ksize_of(*pair) == R.ksize_of(*pair)
    a = np.random.default_rng(1).integers(0, 256, (61, 97, 3), dtype=np.uint8)
    assert np.array_equal(F.resize(a, 37, 53), R.resize(a, 37, 53))


def _native_tables(f, in_size, out_size):
    lib = J.lib()
    ks = C.c_uint32(0)
    assert lib.jpgpu_resample_coefficients_filtered(f, in_size, out_size, None, None, C.byref(ks)) == 0
    bounds = np.full((out_size, 2), -1, np.int32)
    coefs = np.full((out_size, ks.value), -1, np.int32)
    assert lib.jpgpu_resample_coefficients_filtered(f, in_size, out_size, bounds.ctypes.data, coefs.ctypes.data, C.byref(ks)) == 0
    return bounds, coefs


def _native_range(f, in_size, out_size, first, count):
    lib = J.lib()
    ks = C.c_uint32(0)
    assert lib.jpgpu_resample_coefficients_range_filtered(f, in_size, out_size, first, count, None, None, C.byref(ks)) == 0
    bounds = np.full((count, 2), -1, np.int32)
    coefs = np.full((count, ks.value), -1, np.int32)
    assert lib.jpgpu_resample_coefficients_range_filtered(f, in_size, out_size, first, count, bounds.ctypes.data, coefs.ctypes.data, C.byref(ks)) == 0
    return bounds, coefs


PRIMES = [2, 3, 5, 7, 13, 97, 251, 509, 1021, 2039, 4093, 65521]
SWEEP = [(1, 1), (1, 2048), (2048, 1), (65535, 1), (1, 65535), (65535, 2048), (1080, 224), (224, 1080), (224, 224), (1920, 224), (540, 224), (960, 224),
         (2160, 224), (3840, 224), (375, 224), (500, 224), (2, 1), (1, 2), (3, 2), (2, 3), (65535, 65535), (65535, 65534), (16, 16), (1200, 1), (400, 40), (64, 24)] + \
        [(a, b) for a in PRIMES for b in PRIMES if a != b and a * b < 3_000_000]
# (the statement runs in Python, entry by entry: against it the pairs whose tables stay small)
SMALL = [p for p in SWEEP if p[1] * F.ksize_of(p[0], p[1], F.LANCZOS) <= 400_000]


def test_the_small_pairs_still_span_the_sweep():
    assert len(SMALL) >= 60 and (65535, 1) in SMALL and (2160, 224) in SMALL and (1, 2048) in SMALL and (2048, 1) in SMALL


@pytest.mark.parametrize("name", FILTERS)
def test_native_tables_equal_the_statement(name):
    f = F.NAMES[name]
    for in_size, out_size in SMALL:
        bounds, coefs = _native_tables(f, in_size, out_size)
        wb, wk = F.coefficients_range(in_size, out_size, 0, out_size, f)
        assert coefs.shape[1] == F.ksize_of(in_size, out_size, f) == wk.shape[1], (in_size, out_size)
        assert np.array_equal(bounds, wb), (in_size, out_size)
        assert np.array_equal(coefs, wk), (in_size, out_size)


@pytest.mark.parametrize("name", FILTERS)
def test_native_tables_keep_the_rules_and_the_32_bit_bound(name):
    """255 * sum |k| + 2^21 < 2^31 for every entry of the sweep: both passes, whole or in chunks, are exact in int32 in any order."""
    f = F.NAMES[name]
    worst = 0
    for in_size, out_size in SWEEP:
        bounds, coefs = _native_tables(f, in_size, out_size)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= in_size).all(), (in_size, out_size)
        assert (bounds[:, 1] <= coefs.shape[1]).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all()  # (what the band planner relies on)
        assert all((coefs[i, bounds[i, 1]:] == 0).all() for i in range(0, out_size, max(1, out_size // 64)))
        k = coefs.astype(np.int64)
        assert (np.abs(k.sum(axis=1) - (1 << 22)) <= coefs.shape[1]).all(), (in_size, out_size)  # (the weights sum to one within rounding)
        if name in ("bilinear", "box", "hamming"):
            assert (coefs >= 0).all()
        worst = max(worst, int(255 * np.abs(k).sum(axis=1).max()))
        assert 255 * int(np.abs(k).sum(axis=1).max()) + (1 << 21) < (1 << 31), (in_size, out_size)
    if name in ("bicubic", "lanczos"):
        assert worst > 255 << 22  # (negative lobes: the absolute sum exceeds one — the bound is not idle)


@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
def test_negative_weights_round_away_from_zero(name):
    f = F.NAMES[name]
    bounds, coefs = _native_tables(f, 1080, 224)
    assert (coefs < 0).any()
    _, wk = F.coefficients(1080, 224, f)
    assert np.array_equal(coefs, wk)


def test_filter_0_is_the_functions_that_were_there():
    lib = J.lib()
    for in_size, out_size in SWEEP:
        bounds, coefs = _native_tables(0, in_size, out_size)
        ks = C.c_uint32(0)
        ob, ok = np.full_like(bounds, -1), np.full_like(coefs, -1)
        assert lib.jpgpu_resample_coefficients(in_size, out_size, ob.ctypes.data, ok.ctypes.data, C.byref(ks)) == 0
        assert ks.value == coefs.shape[1] and np.array_equal(ob, bounds) and np.array_equal(ok, coefs)
        first, count = out_size // 3, out_size - out_size // 3 - out_size // 4
        rb, rk = _native_range(0, in_size, out_size, first, count)
        ob, ok = np.full_like(rb, -1), np.full_like(rk, -1)
        assert lib.jpgpu_resample_coefficients_range(in_size, out_size, first, count, ob.ctypes.data, ok.ctypes.data, C.byref(ks)) == 0
        assert np.array_equal(ob, rb) and np.array_equal(ok, rk)
        assert np.array_equal(rb, bounds[first:first + count]) and np.array_equal(rk, coefs[first:first + count])


@pytest.mark.parametrize("name", FILTERS)
def test_a_range_is_a_slice_of_the_whole_axis(name):
    f = F.NAMES[name]
    for in_size, out_size, first, count in [(375, 298, 37, 224), (61, 90, 20, 48), (9, 64, 10, 37), (2160, 224, 223, 1), (7, 7, 0, 7), (5, 5, 5, 0)]:
        bounds, coefs = _native_tables(f, in_size, out_size)
        rb, rk = _native_range(f, in_size, out_size, first, count)
        assert np.array_equal(rb, bounds[first:first + count]) and np.array_equal(rk, coefs[first:first + count])
        if count:
            wb, wk = F.coefficients_range(in_size, out_size, first, count, f)
            assert np.array_equal(rb, wb) and np.array_equal(rk, wk)


@pytest.mark.parametrize("name", FILTERS)
def test_an_unchanged_axis_is_the_identity(name):
    f = F.NAMES[name]
    for n in (1, 2, 224, 2048):
        bounds, coefs = _native_tables(f, n, n)
        assert coefs.shape[1] == F.ksize_of(n, n, f)
        rows = np.arange(n)
        at = rows - bounds[:, 0]  # (wide filters start left of the pixel: its weight is the only one that is not zero)
        assert (coefs[rows, at] == 1 << 22).all() and int(np.abs(coefs).sum()) == n << 22
    a = np.random.default_rng(0).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert np.array_equal(F.resize(a, 53, 37, f), a)


def test_python_tables_are_the_native_ones():
    for name in FILTERS:
        b, k = J.resample_coefficients(375, 224, name)
        nb, nk = _native_tables(F.NAMES[name], 375, 224)
        assert np.array_equal(b, nb) and np.array_equal(k, nk)
    b, k = J.resample_coefficients(375, 224)
    assert np.array_equal(k, _native_tables(0, 375, 224)[1])
    assert np.array_equal(J.resample_coefficients(375, 224, "BICUBIC")[1], J.resample_coefficients(375, 224, 3)[1])
    with pytest.raises(ValueError):
        J.resample_coefficients(375, 224, "nearest")
    with pytest.raises(J.FormatError):
        J.resample_coefficients(375, 224, 9)
    with pytest.raises(J.FormatError):
        J.resample_coefficients(0, 224, "box")


def test_native_tables_refuse_bad_arguments():
    lib = J.lib()
    E = J._native.ERR_FORMAT
    ks = C.c_uint32(7)
    buf = np.zeros(64, np.int32)
    for f in (5, 9, 15, 16, 0xffffffff):
        assert lib.jpgpu_resample_coefficients_filtered(f, 4, 4, None, None, C.byref(ks)) == E
        assert lib.jpgpu_resample_coefficients_range_filtered(f, 4, 4, 0, 4, None, None, C.byref(ks)) == E
    for f in range(5):
        for in_size, out_size in [(0, 1), (1, 0), (65536, 1), (1, 65536)]:
            assert lib.jpgpu_resample_coefficients_filtered(f, in_size, out_size, None, None, C.byref(ks)) == E
        assert lib.jpgpu_resample_coefficients_filtered(f, 4, 4, None, None, None) == E
        assert lib.jpgpu_resample_coefficients_filtered(f, 4, 4, buf.ctypes.data, None, C.byref(ks)) == E  # (both tables or neither)
        assert lib.jpgpu_resample_coefficients_range_filtered(f, 4, 4, 3, 2, None, None, C.byref(ks)) == E
    assert ks.value == 7 and (buf == 0).all()


def _gray_desc():
    comps, _ = J.make_components(16, 16, [(1, 1)])
    return J.image_desc(list(comps), [[1] * 64], 16, 16, "Grayscale")


def test_a_batch_refuses_a_bad_filter_before_it_touches_a_device():
    """The flags are checked first: an id above 4 is a FormatError, a filter without an output size an UnsupportedError, with or
    without a GPU in the machine."""
    N = J._native
    assert N.BATCH_FILTER(3) == 0x300 and N.BATCH_FILTER(0) == 0
    with pytest.raises(J.FormatError, match="filter 9"):
        J.Batch([_gray_desc()], output_size=(8, 8), filter=9)
    with pytest.raises(J.FormatError, match="filter 5"):
        J.Batch([_gray_desc()], output_size=(8, 8), flags=N.BATCH_FILTER(5))
    with pytest.raises(J.UnsupportedError, match="bicubic.*output size"):
        J.Batch([_gray_desc()], filter="bicubic")
    with pytest.raises(J.UnsupportedError, match="lanczos.*output size"):
        J.Batch([_gray_desc()], windows=[(0, 0, 8, 8)], flags=N.BATCH_FILTER(N.FILTER_LANCZOS))
    with pytest.raises(ValueError):
        J.Batch([_gray_desc()], output_size=(8, 8), filter="nearest")


def test_new_symbols_and_python_arguments():
    text = open(os.path.join(ROOT, "include", "jpgpu.h")).read() + open(os.path.join(ROOT, "include", "jpgpu_decoder.h")).read()
    J.build()
    lib = C.CDLL(J._native.LIB_PATH)
    for name in ("jpgpu_resample_coefficients_filtered", "jpgpu_resample_coefficients_range_filtered", "jpgpu_pipeline_set_filter"):
        assert name + "(" in text and hasattr(lib, name) and name in J._native.exported_symbols(), name
    for name, value in [("BILINEAR", 0), ("BOX", 1), ("HAMMING", 2), ("BICUBIC", 3), ("LANCZOS", 4)]:
        assert f"JPGPU_FILTER_{name} = {value}" in text and getattr(J._native, "FILTER_" + name) == value
    assert "#define JPGPU_BATCH_FILTER(f) (((uint32_t)(f) & 15u) << 8)" in text
    assert inspect.signature(J.Batch.__init__).parameters["filter"].default is None
    assert inspect.signature(J.Pipeline.decode).parameters["filter"].default is None
    assert list(inspect.signature(J.resample_coefficients).parameters) == ["in_size", "out_size", "filter"]


def test_a_bad_filter_name_is_refused_before_any_native_call(monkeypatch):
    def no_native():
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(J._native, "lib", no_native)
    p = J.Pipeline.__new__(J.Pipeline)
    p._h = None
    for f in ("nearest", "", -1, 16):
        with pytest.raises(ValueError):
            p.decode([b"\xff\xd8"], output_size=(8, 8), filter=f)
