"""Colour operations on the CPU (no GPU): the numpy statement of DESIGN.md §4.20 (tests/colour_ref.py) against Pillow's golden bytes,
the library's pure host functions — jpgpu_colour_check, jpgpu_colour_point_lut, jpgpu_colour_autocontrast_lut,
jpgpu_colour_equalize_lut — against the statement, the colour kernel's bodies emulated lane by lane (tests/emu/emu_colour.cpp,
-ffp-contract=off) against it, and the bodies plus the job builder as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import colour_ref as CR
import jpeg_decoder_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "colour", "pillow_colour.json")
_EMU = os.path.join(ROOT, "tests", "emu")
# the flags of tests/emu/Makefile, and no contraction of a + f * d (blend and AUTOCONTRAST round every operation)
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION", "-ffp-contract=off"]
N = J._native
FACTORS = (0.0, 1.0, 0.37, 1.9)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def _program(c):
    return [(n, v) for n, v in c["program"]]


def test_the_numpy_statement_is_what_pillow_computes(golden):
    cases = golden["cases"]
    assert len(cases) >= 60
    rounded_differs = unclipped_differs = 0
    for c in cases:
        P, want = CR.make_input(c), CR.expected(c)
        assert P.shape[0] <= 24 and P.shape[1] <= 24 or "rows" in c  # (the 30 x 30 two-level image is made of runs of rows)
        assert CR.check(_program(c)), c["program"]
        assert np.array_equal(CR.apply(P, _program(c)), want), {k: v for k, v in c.items() if k != "expect"}
        rounded_differs += not np.array_equal(CR.apply(P, _program(c), rounded=True), want)
        unclipped_differs += not np.array_equal(CR.apply(P, _program(c), clip=False), want)
    # the set discriminates: a blend that rounds and an EQUALIZE table without the clip give other bytes
    assert rounded_differs >= 1 and unclipped_differs >= 1


def test_golden_cases_cover_the_operations_and_the_degenerate_branches(golden):
    seen = set()
    for c in golden["cases"]:
        P, prog = CR.make_input(c), _program(c)
        ops = [CR.op_id(n) for n, _ in prog]
        seen.update(("op", o) for o in ops)
        for n, v in prog:
            o = CR.op_id(n)
            if o in (CR.BRIGHTNESS, CR.CONTRAST, CR.COLOR) and v in FACTORS:
                seen.add((o, v))
            if o in (CR.SOLARIZE, CR.POSTERIZE):
                seen.add((o, int(v)))
        if len(prog) == 1:
            hs = CR.histograms(P)
            if "const" in c and ops[0] in (CR.AUTOCONTRAST, CR.EQUALIZE):
                seen.add(("constant", ops[0]))
            if ops[0] == CR.EQUALIZE:
                nz = [int(v) for v in hs[0] if v]
                if len(nz) > 1 and (sum(nz) - nz[-1]) // 255 == 0:
                    seen.add("step 0")
                if len(nz) > 1 and (sum(nz) - nz[-1]) // 255 and np.any(CR.equalize_lut(hs[0], clip=False) != CR.equalize_lut(hs[0])):
                    seen.add("clip")
            if ops[0] == CR.CONTRAST:
                s, n = int(CR.luma(P).sum()), P.shape[0] * P.shape[1]
                if (2 * s) % (2 * n) == n:
                    seen.add("mean at .5")
        if 2 <= len(ops) <= 4:
            for k in range(1, len(ops)):
                if ops[k] in (CR.CONTRAST, CR.AUTOCONTRAST, CR.EQUALIZE):
                    seen.add("statistics behind COLOR" if CR.COLOR in ops[:k] else "statistics behind a point operation")
    want = {("op", o) for o in range(9)} | {(o, f) for o in (CR.BRIGHTNESS, CR.CONTRAST, CR.COLOR) for f in FACTORS}
    want |= {(CR.SOLARIZE, 0), (CR.SOLARIZE, 256), (CR.POSTERIZE, 1), (CR.POSTERIZE, 8), ("constant", CR.AUTOCONTRAST), ("constant", CR.EQUALIZE), "step 0", "clip",
             "mean at .5", "statistics behind COLOR", "statistics behind a point operation"}
    assert want <= seen, want - seen


# ---- host functions ----

def test_point_luts_are_the_reference_tables():
    rng = np.random.default_rng(420)
    factors = list(FACTORS) + [0.5, 2.0, 3.0, 255.99, 256.0, 1e-6, 0.999999, 1.000001] + [float(v) for v in rng.uniform(0, 3, 60)]
    for f in factors:
        assert np.array_equal(J.colour_point_lut("brightness", f), CR.point_lut(CR.BRIGHTNESS, f)), f
        for m in (0, 1, 11, 127, 128, 254, 255):
            assert np.array_equal(J.colour_point_lut("contrast", f, m), CR.point_lut(CR.CONTRAST, f, m)), (f, m)
    for t in range(257):
        assert np.array_equal(J.colour_point_lut("solarize", t), CR.point_lut(CR.SOLARIZE, t)), t
    for b in range(1, 9):
        assert np.array_equal(J.colour_point_lut("posterize", b), CR.point_lut(CR.POSTERIZE, b)), b
    assert np.array_equal(J.colour_point_lut("invert"), 255 - np.arange(256)) and np.array_equal(J.colour_point_lut("identity"), np.arange(256))
    assert np.array_equal(J.colour_point_lut("solarize", 0), 255 - np.arange(256)) and np.array_equal(J.colour_point_lut("posterize", 8), np.arange(256))
    for op, v in (("saturation", 1.0), ("autocontrast", 0), ("equalize", 0), ("brightness", -1.0), ("solarize", 1.5), ("posterize", 0), (9, 0)):
        with pytest.raises(J.FormatError):
            J.colour_point_lut(op, v)
    with pytest.raises(J.FormatError):
        J.colour_point_lut("contrast", 1.0, 256)


def test_autocontrast_lut_for_every_pair_of_bounds():
    pairs = 0
    for lo in range(256):
        for hi in range(lo + 1, 256):
            h = np.zeros(256, np.uint32)
            h[lo], h[hi] = 1 + lo, 7
            if (lo + hi) % 3 == 0:
                h[(lo + hi) // 2] = 5  # (a value between the bounds changes nothing)
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            want = np.clip(np.trunc(np.arange(256) * scale + offset), 0, 255).astype(np.uint8)  # (doubles, one rounding per operation)
            assert np.array_equal(J.colour_autocontrast_lut(h), want), (lo, hi)
            pairs += 1
    assert pairs == 32640
    for lo, hi in ((0, 255), (0, 1), (254, 255), (50, 180), (3, 250), (100, 101), (17, 211)):  # (the loop's own statement against the reference's)
        h = np.zeros(256, np.uint32)
        h[lo] = h[hi] = 3
        assert np.array_equal(J.colour_autocontrast_lut(h), CR.autocontrast_lut(h)), (lo, hi)
    for h in (np.zeros(256, np.uint32), np.eye(256, dtype=np.uint32)[77] * 9):  # (nothing present, one value: the identity)
        assert np.array_equal(J.colour_autocontrast_lut(h), np.arange(256))


def test_equalize_lut_is_the_reference_table():
    rng = np.random.default_rng(421)
    hists = [np.zeros(256, np.uint32), np.eye(256, dtype=np.uint32)[5] * 900, np.full(256, 1, np.uint32), np.full(256, 2, np.uint32), np.full(256, 16384, np.uint32)]
    two = np.zeros(256, np.uint32)
    two[0], two[3], two[200] = 780, 60, 60  # (the 30 x 30 two-level image: the clip at 255)
    hists.append(two)
    big = np.zeros(256, np.uint32)
    big[0], big[255] = 2048 * 2048 - 1, 1
    hists.append(big)
    for k in range(300):
        n = int(rng.integers(2, 257))
        h = np.zeros(256, np.uint32)
        idx = rng.choice(256, n, replace=False)
        h[idx] = rng.integers(1, [4, 300, 70000][k % 3], n)
        hists.append(h)
    clipped = 0
    for h in hists:
        want = CR.equalize_lut(h)
        assert np.array_equal(J.colour_equalize_lut(h), want), h
        clipped += bool(np.any(CR.equalize_lut(h, clip=False) != want))
    assert clipped >= 1


REFUSED = [[("brightness", math.nan)], [("contrast", math.inf)], [("saturation", -0.5)], [("brightness", 256.5)], [("solarize", 1.5)], [("solarize", 257)],
           [("solarize", -1)], [("posterize", 0)], [("posterize", 9)], [("posterize", 2.5)], [(9, 0.0)], [(255, 1.0)], [("invert", 0)] * 5,
           [("invert", 0), ("equalize", 0), ("brightness", -1e-9)]]
ACCEPTED = [[], [("brightness", 256.0)], [("saturation", 0.0)], [("solarize", 0)], [("solarize", 256)], [("posterize", 1)], [("posterize", 8)], [("invert", 0)] * 4,
            [("identity", math.nan)], [("autocontrast", -3.0), ("equalize", math.inf)]]


def test_colour_check_is_the_reference_rule():
    for p in REFUSED:
        assert not CR.check(p) and not J.colour_check(p), p
    for p in ACCEPTED:
        assert CR.check(p) and J.colour_check(p), p
    assert N.lib().jpgpu_colour_check(None) != 0
    rng = np.random.default_rng(422)
    for _ in range(500):
        p = [(int(rng.integers(0, 11)), float(rng.choice([0.0, 1.0, 0.5, 8.0, 9.0, 128.0, 256.0, 257.0, -1.0, 2.5]))) for _ in range(int(rng.integers(0, 6)))]
        assert J.colour_check(p) == CR.check(p), p


# ---- the kernel bodies, lane by lane ----

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    so = str(tmp_path_factory.mktemp("emu_colour") / "libemucolour.so")
    subprocess.check_call([cxx, *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so, os.path.join(_EMU, "emu_colour.cpp")])
    L = C.CDLL(so)
    L.emu_colour.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(N.ColourProgram), C.c_uint32]
    L.emu_colour.restype = C.c_int
    return L


def _emu_colour(L, P, program, lanes=1024):
    H, W, _ = P.shape
    guard = 64
    buf = np.full(H * W * 3 + guard, 0x5A, np.uint8)
    buf[: H * W * 3] = P.reshape(-1)
    s = J.colour.program_struct(program)
    assert L.emu_colour(buf.ctypes.data, W, H, C.byref(s), lanes) == 0
    assert np.all(buf[H * W * 3:] == 0x5A)
    return buf[: H * W * 3].reshape(H, W, 3)


def test_the_kernel_bodies_give_pillows_bytes_on_the_golden_cases(golden, emu):
    for k, c in enumerate(golden["cases"]):
        got = _emu_colour(emu, CR.make_input(c), _program(c), (1024, 64, 192)[k % 3])
        assert np.array_equal(got, CR.expected(c)), {k: v for k, v in c.items() if k != "expect"}


def test_the_kernel_bodies_on_sizes_with_every_remainder(emu):
    rng = np.random.default_rng(423)
    programs = [[("brightness", 1.9), ("autocontrast", 0)], [("saturation", 0.37), ("equalize", 0), ("contrast", 1.9)], [("contrast", 0.37)], [("saturation", 1.9)],
                [("equalize", 0)], [("autocontrast", 0), ("solarize", 100), ("posterize", 3), ("invert", 0)], []]
    sizes = [(1, 1), (1, 2), (1, 3), (3, 1), (5, 7), (16, 16), (17, 33), (40, 48), (67, 131), (3, 1025), (224, 224)]
    for k, (H, W) in enumerate(sizes):
        lo, hi = [(0, 256), (30, 200), (100, 103)][k % 3]
        P = rng.integers(lo, hi, (H, W, 3), dtype=np.uint8)
        for q, program in enumerate(programs if H * W < 40000 else programs[:2]):
            got = _emu_colour(emu, P, program, (1024, 64, 192)[(k + q) % 3])
            assert np.array_equal(got, CR.apply(P, program)), (H, W, program)
    s = J.colour.program_struct([("posterize", 9)])
    px = np.arange(12, dtype=np.uint8)
    assert emu.emu_colour(px.ctypes.data, 2, 2, C.byref(s), 1024) != 0 and np.array_equal(px, np.arange(12))  # (refused: nothing written)


def test_bodies_and_job_builder_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing is loaded into Python."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "colour_asan")
    cmd = [cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17", "-Wall",
           "-Wno-unknown-pragmas", "-Wno-unused-function", "-ffp-contract=off", "-DJPGPU_HOST_EMULATION", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"),
           "-o", exe, os.path.join(_EMU, "colour_asan.cpp")]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "colour_asan: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
