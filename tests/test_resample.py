"""The resample of DESIGN.md §4.10 without a GPU: the numpy statement (tests/resample_ref.py) against Pillow's own output (hashes made
by tools/make_resample_golden.py — no Pillow needed here), jpgpu_resample_coefficients against the numpy tables, the new symbols and
the Python arguments."""
import ctypes as C
import hashlib
import inspect
import json
import os

import numpy as np
import pytest

import jpeg_decoder_amd as J
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "resample", "pillow_bilinear.json")))


def test_golden_covers_what_it_should():
    cases = GOLDEN["cases"]
    assert len(cases) >= 40
    assert {c["C"] for c in cases} == {1, 3, 4}
    assert not any(c["H"] > 100 * c["W"] and c["oh"] < c["H"] for c in cases)  # (Pillow's vertical-first order: not ours)
    assert any(c["ow"] > c["W"] and c["oh"] > c["H"] for c in cases) and any(c["ow"] < c["W"] and c["oh"] < c["H"] for c in cases)
    assert any((c["ow"] > c["W"]) != (c["oh"] > c["H"]) for c in cases) and any(c["ow"] == c["W"] and c["oh"] == c["H"] for c in cases)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: f"{c['W']}x{c['H']}x{c['C']}-{c['ow']}x{c['oh']}")
def test_numpy_statement_equals_pillow(case):
    a = np.random.default_rng(case["seed"]).integers(0, 256, (case["H"], case["W"], case["C"]), dtype=np.uint8)
    got = R.resize(a, case["ow"], case["oh"])
    assert got.shape == (case["oh"], case["ow"], case["C"]) and got.dtype == np.uint8
    assert hashlib.sha256(got.tobytes()).hexdigest() == case["sha256"]


def _native_tables(in_size, out_size):
    lib = J.lib()
    ks = C.c_uint32(0)
    assert lib.jpgpu_resample_coefficients(in_size, out_size, None, None, C.byref(ks)) == 0
    bounds = np.full((out_size, 2), -1, np.int32)
    coefs = np.full((out_size, ks.value), -1, np.int32)
    assert lib.jpgpu_resample_coefficients(in_size, out_size, bounds.ctypes.data, coefs.ctypes.data, C.byref(ks)) == 0
    return bounds, coefs


PRIMES = [2, 3, 5, 7, 13, 97, 251, 509, 1021, 2039, 4093, 65521]
PAIRS = [(1, 1), (1, 2048), (2048, 1), (65535, 1), (1, 65535), (65535, 2048), (1080, 224), (224, 1080), (224, 224), (1920, 224), (540, 224), (960, 224),
         (2160, 224), (3840, 224), (2, 1), (1, 2), (3, 2), (2, 3), (65535, 65535), (65535, 65534)] + \
        [(a, b) for a in PRIMES for b in PRIMES if a != b and a * b < 3_000_000]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_native_coefficients_equal_the_numpy_tables(pair):
    in_size, out_size = pair
    bounds, coefs = _native_tables(in_size, out_size)
    wb, wk = R.coefficients(in_size, out_size)
    assert coefs.shape[1] == R.ksize_of(in_size, out_size) == wk.shape[1]
    assert np.array_equal(bounds, wb)
    assert np.array_equal(coefs, wk)
    # the rules' own consequences: inside the source, never negative, zero beyond n, sums within rounding of 2^22
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= in_size).all()
    assert (coefs >= 0).all()
    assert all((coefs[i, bounds[i, 1]:] == 0).all() for i in range(0, out_size, max(1, out_size // 64)))
    assert (np.abs(coefs.astype(np.int64).sum(axis=1) - (1 << 22)) <= coefs.shape[1]).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all()  # (what the band planner relies on)


def test_an_unchanged_axis_is_the_identity():
    for n in (1, 2, 224, 2048):
        bounds, coefs = _native_tables(n, n)
        assert coefs.shape[1] == 3
        assert np.array_equal(bounds[:, 0], np.arange(n))
        assert (coefs[:, 0] == 1 << 22).all() and (coefs[:, 1:] == 0).all()
    a = np.random.default_rng(0).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert np.array_equal(R.resize(a, 53, 37), a)


def test_native_coefficients_refuse_bad_arguments():
    lib = J.lib()
    ks = C.c_uint32(7)
    buf = np.zeros(64, np.int32)
    for in_size, out_size in [(0, 1), (1, 0), (65536, 1), (1, 65536)]:
        assert lib.jpgpu_resample_coefficients(in_size, out_size, None, None, C.byref(ks)) == J._native.ERR_FORMAT
    assert lib.jpgpu_resample_coefficients(4, 4, None, None, None) == J._native.ERR_FORMAT
    assert lib.jpgpu_resample_coefficients(4, 4, buf.ctypes.data, None, C.byref(ks)) == J._native.ERR_FORMAT  # (both tables or neither)
    assert (buf == 0).all()


def test_new_symbols_and_python_arguments():
    text = open(os.path.join(ROOT, "include", "jpgpu.h")).read() + open(os.path.join(ROOT, "include", "jpgpu_decoder.h")).read()
    J.build()
    lib = C.CDLL(J._native.LIB_PATH)
    for name in ("jpgpu_batch_create_resized", "jpgpu_resample_coefficients", "jpgpu_pipeline_set_output_size"):
        assert name + "(" in text and hasattr(lib, name) and name in J._native.exported_symbols(), name
    assert inspect.signature(J.Batch.__init__).parameters["output_size"].default is None
    assert inspect.signature(J.Pipeline.decode).parameters["output_size"].default is None
    T = J._native.PipelineTimings
    # (in the slot that was padding behind dev_times_valid: nothing moved, the struct's size and its last field are what they were)
    assert T.images_resized.offset == T.dev_times_valid.offset + 4 == T.dev_fill_ms.offset - 4 and T._fields_[-1][0] == "images_windowed"


def test_a_bad_output_size_is_refused_before_any_native_call(monkeypatch):
    def no_native():
        raise AssertionError("the native library was reached")

    monkeypatch.setattr(J._native, "lib", no_native)
    p = J.Pipeline.__new__(J.Pipeline)
    p._h = None
    for size in [(70000, 8), (-1, 8), (8,), (1, 2, 3)]:
        with pytest.raises(ValueError):
            p.decode([b"\xff\xd8"], output_size=size)
