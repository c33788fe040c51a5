"""Placements on the CPU (no GPU): the numpy statement of DESIGN.md §4.14 (tests/placement_ref.py) against Pillow's golden hashes, the
library's pure host functions — jpgpu_fit_placement, jpgpu_resample_coefficients_range — against the statement, and the planner, the
tables and the emulated kernel bodies as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_decoder_amd as J
import placement_ref as P
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "placement", "pillow_placement.json")
N = J._native


def test_the_numpy_statement_is_what_pillow_computes():
    g = json.load(open(GOLDEN))
    assert g["filter"] == "BILINEAR" and len(g["cases"]) >= 30
    kinds = set()
    for c in g["cases"]:
        assert not (c["H"] > 100 * c["W"] and c["rh"] < c["H"])
        a = np.random.default_rng(c["seed"]).integers(0, 256, (c["H"], c["W"], c["C"]), dtype=np.uint8)
        got = P.place(a, c["ow"], c["oh"], (c["rw"], c["rh"], c["x"], c["y"]), c["fill"])
        assert hashlib.sha256(got.tobytes()).hexdigest() == c["sha256"], c
        vw, vh = min(c["ow"], c["x"] + c["rw"]) - max(0, c["x"]), min(c["oh"], c["y"] + c["rh"]) - max(0, c["y"])
        kinds.add(("crop" if (c["x"] < 0 or c["x"] + c["rw"] > c["ow"]) else "pad", c["C"]))
        kinds.add("1x1" if (vw, vh) == (1, 1) else "upscale" if c["rw"] > c["W"] else "other")
    assert {("crop", 1), ("crop", 3), ("crop", 4), ("pad", 1), ("pad", 3), ("pad", 4), "1x1", "upscale"} <= kinds


ANCHORS = [(1, (500, 375), 256, (224, 224), (341, 256, -58, -16)), (1, (1920, 1080), 256, (224, 224), (455, 256, -116, -16)),
           (1, (259, 200), 256, (224, 224), (331, 256, -54, -16)), (1, (100, 1000), 256, (224, 224), (256, 2560, -16, -1168)),
           (1, (375, 500), 256, (224, 224), (256, 341, -16, -58)), (2, (333, 500), 0, (640, 640), (426, 640, 107, 0)),
           (2, (1920, 1080), 0, (640, 640), (640, 360, 0, 140)), (2, (100, 1000), 0, (640, 640), (64, 640, 288, 0))]
MODES = {0: "stretch", 1: "shorter_side_crop", 2: "letterbox"}


def test_fit_placement_anchors():
    for mode, src, size, out, want in ANCHORS:
        assert J.fit_placement(J.Fit(MODES[mode], size=size), src, out) == want, (mode, src)
        ref = P.fit_shorter_side_crop(*src, size, *out) if mode == 1 else P.fit_letterbox(*src, *out)
        assert ref == want, (mode, src, ref)
    assert J.fit_placement(J.Fit("stretch"), (500, 375), (224, 200)) == (224, 200, 0, 0)


def test_fit_placement_is_the_python_rule_for_random_sizes():
    rng = np.random.default_rng(2000)
    seen_pad = seen_half = 0
    for k in range(2000):
        w, h = (int(v) for v in rng.integers(1, 5000 if k % 3 else 300, 2))
        ow, oh = (int(v) for v in rng.integers(1, 2049, 2))
        size = int(rng.integers(1, 700))
        want = P.fit_shorter_side_crop(w, h, size, ow, oh)
        if max(want[0], want[1]) <= 65535:
            assert J.fit_placement(J.Fit("shorter_side_crop", size=size), (w, h), (ow, oh)) == want, (w, h, size, ow, oh)
            seen_pad += want[0] < ow or want[1] < oh
            seen_half += (want[0] - ow) % 2 == 1 and want[0] > ow
        else:
            with pytest.raises(J.FormatError):
                J.fit_placement(J.Fit("shorter_side_crop", size=size), (w, h), (ow, oh))
        got = J.fit_placement(J.Fit("letterbox"), (w, h), (ow, oh))
        assert got == P.fit_letterbox(w, h, ow, oh), (w, h, ow, oh)
        assert 1 <= got[0] <= ow and 1 <= got[1] <= oh and 0 <= got[2] <= ow - got[0] and 0 <= got[3] <= oh - got[1]
    assert seen_pad > 50 and seen_half > 50


def test_fit_refusals():
    pl = N.Placement()

    def call(mode, size, reserved, src=(100, 80), out=(64, 64)):
        s = N.FitStruct()
        s.mode, s.size, s.reserved = mode, size, reserved
        return N.lib().jpgpu_fit_placement(C.byref(s), src[0], src[1], out[0], out[1], C.byref(pl))

    assert call(1, 256, 0) == 0
    assert call(3, 256, 0) != 0            # unknown mode
    assert call(1, 256, 1) != 0            # reserved
    assert call(1, 0, 0) != 0              # no size
    assert call(1, 256, 0, (8, 4000)) != 0  # rh = 128000
    assert call(2, 0, 0, (0, 5)) != 0 and call(2, 0, 0, (5, 5), (0, 5)) != 0
    assert N.lib().jpgpu_fit_placement(None, 1, 1, 1, 1, C.byref(pl)) != 0
    with pytest.raises(ValueError):
        J.Fit("fill")
    with pytest.raises(ValueError):
        J.Fit("letterbox", fill=(1, 2, 3, 4, 5))


def _range(in_size, out_size, first, count):
    ks = C.c_uint32(0)
    assert N.lib().jpgpu_resample_coefficients_range(in_size, out_size, first, count, None, None, C.byref(ks)) == 0
    b, k = np.full((count, 2), -1, np.int32), np.full((count, ks.value), -1, np.int32)
    assert N.lib().jpgpu_resample_coefficients_range(in_size, out_size, first, count, b.ctypes.data, k.ctypes.data, C.byref(ks)) == 0
    return b, k


def test_range_tables_are_slices_of_the_whole_tables():
    rng = np.random.default_rng(7)
    for in_size, out_size in [(1, 65535), (65535, 1), (1080, 455), (1, 1), (375, 256), (13, 997), (2039, 251)]:
        wb, wk = R.coefficients(in_size, out_size)
        spans = [(0, min(out_size, 224)), (out_size - 1, 1), (out_size // 2, min(out_size - out_size // 2, 99))]
        spans += [(int(f), int(rng.integers(1, min(out_size - f, 300) + 1))) for f in rng.integers(0, out_size, 3)]
        for first, count in spans:
            b, k = _range(in_size, out_size, first, count)
            assert k.shape[1] == wk.shape[1]
            assert np.array_equal(b, wb[first:first + count]) and np.array_equal(k, wk[first:first + count]), (in_size, out_size, first, count)
    ks = C.c_uint32(0)
    assert N.lib().jpgpu_resample_coefficients_range(10, 20, 15, 6, None, None, C.byref(ks)) != 0  # beyond the axis
    assert N.lib().jpgpu_resample_coefficients_range(0, 20, 0, 1, None, None, C.byref(ks)) != 0


def test_reference_refuses_a_placement_that_shows_nothing():
    a = np.zeros((4, 4, 3), np.uint8)
    for pl in [(10, 10, 8, 0), (10, 10, -10, 0), (10, 10, 0, 8), (10, 10, 0, -10)]:
        with pytest.raises(AssertionError):
            P.place(a, 8, 8, pl)
    assert P.place(a, 8, 8, (10, 10, 7, -9)).shape == (8, 8, 3)


def test_planner_tables_and_kernel_bodies_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing is loaded into Python."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    emu = os.path.join(ROOT, "tests", "emu")
    exe = str(tmp_path / "placement_asan")
    cmd = [cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17", "-Wall",
           "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION", "-I", emu, "-include", os.path.join(emu, "hip_shim.hpp"), "-o", exe,
           os.path.join(emu, "placement_asan.cpp")]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "placement_asan: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
