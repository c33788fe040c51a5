"""HUE and SHARPNESS on the CPU (no GPU): the numpy statement of DESIGN.md §4.21 (tests/colour_pixel_ref.py) against Pillow's golden
bytes — explicit cases, and sha256 sums over all 2^24 colours for six hue shifts; the library's refusal rule; the colour kernel's bodies
with the two operations emulated lane by lane (tests/emu/emu_colour_pixel.cpp, -ffp-contract=off) against the statement, at strips of 1,
2, 3 rows and of as many as LDS holds; and the bodies plus the job builder as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import hashlib
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import colour_pixel_ref as PR
import colour_ref as CR
import jpeg_decoder_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "colour_pixel")
_EMU = os.path.join(ROOT, "tests", "emu")
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION", "-ffp-contract=off"]
N = J._native
SHIFTS = (0, 1, 43, 128, 213, 255)
FACTORS = (0.0, 0.37, 1.0, 1.9, 256.0)
LANES = (1024, 64, 192)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "pillow_colour_pixel.json")))


@pytest.fixture(scope="module")
def round_trip():
    return PR.RoundTrip()


def _program(c):
    return [(n, v) for n, v in c["program"]]


def _brief(c):
    return {k: v for k, v in c.items() if k != "expect"}


def test_the_numpy_statement_is_what_pillow_computes(golden):
    cases = golden["cases"]
    seen = set()
    changed = clamped = 0
    for c in cases:
        P, want, prog = PR.make_input(c), PR.expected(c), _program(c)
        assert PR.check(prog), c["program"]
        assert np.array_equal(PR.apply(P, prog), want), _brief(c)
        if len(prog) == 1 and prog[0][0] == "sharpen":
            seen.add((prog[0][1], c["W"], c["H"]))
            seen.add(("const" in c, "checker" in c, prog[0][1]))
            if "checker" in c and prog[0][1] > 1:
                clamped += bool((want[1:-1, 1:-1] == 0).any() and (want[1:-1, 1:-1] == 255).any())
            if min(c["W"], c["H"]) < 3:
                assert np.array_equal(want, P), _brief(c)  # (no interior: unchanged)
        changed += not np.array_equal(want, P)
    for f in FACTORS:
        assert {(f, w, h) for w, h in ((1, 1), (2, 5), (5, 2), (3, 3), (7, 5), (33, 17))} <= seen, f
        assert (True, False, f) in seen and (False, True, f) in seen, f
    assert clamped >= 2 and changed >= 40
    mixed = [[n for n, _ in _program(c)] for c in cases if len(c["program"]) > 1]
    assert ["sharpen", "contrast"] in mixed and ["hue", "equalize"] in mixed
    jitter = [m for m in mixed if sorted(m) == ["brightness", "contrast", "hue", "saturation"]]
    assert len({tuple(m) for m in jitter}) >= 2  # (ColorJitter's four operations in two orders)


def test_hue_over_every_colour_is_what_pillow_computes(round_trip):
    sums = json.load(open(os.path.join(GOLDEN, "hue_sha256.json")))["sha256"]
    assert sorted(int(k) for k in sums) == sorted(SHIFTS)
    for shift in SHIFTS:
        assert hashlib.sha256(round_trip.hue(shift).tobytes()).hexdigest() == sums[str(shift)], shift
    # (the table is the statement: a sample through hue() itself; shift 0 is not the identity)
    rng = np.random.default_rng(2101)
    idx = rng.integers(0, 1 << 24, 4096)
    every = PR.all_colours().reshape(-1, 3)
    for shift in (0, 43):
        assert np.array_equal(PR.hue(every[idx][None], shift)[0], round_trip.hue(shift).reshape(-1, 3)[idx])
    assert not np.array_equal(round_trip.hue(0), PR.all_colours())


def test_the_helpers_give_the_operations():
    assert J.hue(0.0) == ("hue", 0.0) and J.hue(0.5) == ("hue", 127.0) and J.hue(-0.5) == ("hue", 129.0) and J.hue(-0.001) == ("hue", 0.0)
    assert J.hue(0.1) == ("hue", 25.0) and J.hue(-0.1) == ("hue", 231.0)  # (truncated toward zero, modulo 256)
    for f in (-0.5, -0.37, -0.1, -0.004, 0.0, 0.004, 0.1, 0.37, 0.5):
        assert J.hue(f)[1] == float(np.int32(f * 255).astype(np.uint8)) == PR.hue_value(f), f
    with pytest.raises(ValueError):
        J.hue(0.51)
    assert J.sharpness(1.9) == ("sharpen", 1.9) and "sharpness" in J.sharpness.__doc__
    assert J.colour.OPS["hue"] == 16 and J.colour.OPS["sharpen"] == 17 and "sharpness" not in J.colour.OPS
    with pytest.raises(ValueError):
        J.colour.program_struct([("sharpness", 1.0)])
    assert J.colour_check([J.hue(0.2), J.brightness(1.2), J.contrast(0.8), J.saturation(1.3)]) and J.colour_check([J.sharpness(2.0)])


REFUSED = [[(k, 0.0)] for k in (9, 10, 11, 12, 13, 14, 15, 18, 19, 255)] + [[(k, 1.0)] for k in (9, 15, 18)] + [
    [("hue", 255.5)], [("hue", 256)], [("hue", -1)], [("hue", math.nan)], [("hue", math.inf)], [("hue", 0.5)], [("sharpen", math.nan)], [("sharpen", 256.5)],
    [("sharpen", -0.001)], [("sharpen", math.inf)], [("hue", 3)] * 5, [("invert", 0), ("sharpen", 1.0), ("hue", 256)]]
ACCEPTED = [[("hue", 0)], [("hue", 255)], [("hue", 43)], [("sharpen", 0.0)], [("sharpen", 256.0)], [("sharpen", 0.37)], [(16, 7.0)], [(17, 7.5)],
            [("hue", 1), ("sharpen", 2.0), ("equalize", 0), ("hue", 255)]]


def test_colour_check_accepts_and_refuses_as_stated():
    for p in REFUSED:
        assert not PR.check(p) and not J.colour_check(p), p
    for p in ACCEPTED:
        assert PR.check(p) and J.colour_check(p), p
    rng = np.random.default_rng(2102)
    for _ in range(600):
        p = [(int(rng.integers(0, 20)), float(rng.choice([0.0, 1.0, 0.5, 8.0, 9.0, 128.0, 255.0, 255.5, 256.0, 257.0, -1.0, 2.5]))) for _ in range(int(rng.integers(0, 6)))]
        assert J.colour_check(p) == PR.check(p), p


def test_point_lut_refuses_the_operations_without_a_table():
    for op, v in ((16, 0.0), (17, 1.0), ("hue", 43), ("sharpen", 0.5), (18, 0.0)):
        with pytest.raises(J.FormatError):
            J.colour_point_lut(op, v)
    assert np.array_equal(J.colour_point_lut("invert"), 255 - np.arange(256))


# ---- the kernel bodies, lane by lane ----

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    so = str(tmp_path_factory.mktemp("emu_colour_pixel") / "libemucolourpixel.so")
    subprocess.check_call([cxx, *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so, os.path.join(_EMU, "emu_colour_pixel.cpp")])
    L = C.CDLL(so)
    L.emu_colour_pixel.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(N.ColourProgram), C.c_uint32, C.c_uint32]
    L.emu_colour_pixel.restype = C.c_int
    for f in (L.emu_colour_strip_rows, L.emu_colour_sharp_steps, L.emu_colour_hue_pixel):
        f.restype = C.c_uint32
    L.emu_colour_strip_rows.argtypes = [C.c_uint32] * 2
    L.emu_colour_sharp_steps.argtypes = [C.c_uint32] * 3
    L.emu_colour_hue_pixel.argtypes = [C.c_uint32] * 4
    return L


def _emu(L, P, program, lanes=1024, rows=0):
    H, W, _ = P.shape
    guard = 64
    buf = np.full(H * W * 3 + guard, 0x5A, np.uint8)
    buf[: H * W * 3] = P.reshape(-1)
    s = J.colour.program_struct(program)
    assert L.emu_colour_pixel(buf.ctypes.data, W, H, C.byref(s), lanes, rows) == 0
    assert np.all(buf[H * W * 3:] == 0x5A)
    return buf[: H * W * 3].reshape(H, W, 3)


def test_the_kernel_bodies_give_pillows_bytes_on_the_golden_cases(golden, emu):
    for k, c in enumerate(golden["cases"]):
        for rows in (0, 1, 2, 3):
            got = _emu(emu, PR.make_input(c), _program(c), LANES[(k + rows) % 3], rows)
            assert np.array_equal(got, PR.expected(c)), (_brief(c), rows)


def test_the_kernel_bodies_at_every_strip_seam(emu):
    """K = 1, 2, 3 and the default; heights K, K + 1, 2 K, 2 K + 1; widths 1, 2, 3, 5, 33: every byte against the statement."""
    rng = np.random.default_rng(2103)
    programs = [[("sharpen", 1.9)], [("sharpen", 0.37)], [("hue", 43)], [("sharpen", 256.0), ("contrast", 1.9)], [("hue", 213), ("sharpen", 0.0), ("equalize", 0)]]
    n = 0
    for rows in (1, 2, 3, 0):
        K = rows or 4  # (the default holds every one of these images in one strip)
        assert emu.emu_colour_strip_rows(33, rows) == (rows or 49152 // 100 - 2)
        for H in (K, K + 1, 2 * K, 2 * K + 1):
            for W in (1, 2, 3, 5, 33):
                kind = n % 3
                P = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if kind == 0 else PR.make_input({"checker": 1, "H": H, "W": W}) if kind == 1 else \
                    PR.make_input({"const": [9, 200, 77], "H": H, "W": W})
                for q, program in enumerate(programs):
                    n += 1
                    got = _emu(emu, P, program, LANES[n % 3], rows)
                    assert np.array_equal(got, PR.apply(P, program)), (rows, H, W, program)
                assert emu.emu_colour_sharp_steps(W, H, K) == (0 if W < 3 or H < 3 else 2 * -(-H // K))
    # rows longer than one turn of the lanes; the widest image: six rows a strip
    assert emu.emu_colour_strip_rows(2048, 0) == 6 and emu.emu_colour_strip_rows(2048, 9) == 6 and emu.emu_colour_strip_rows(224, 0) == 71
    for (H, W), rows, lanes in (((9, 400), 2, 64), ((16, 2048), 0, 1024), ((75, 224), 0, 1024), ((7, 225), 3, 192)):
        P = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for program in ([("sharpen", 1.9)], [("hue", 128), ("sharpen", 0.37)]):
            assert np.array_equal(_emu(emu, P, program, lanes, rows), PR.apply(P, program)), (H, W, rows, program)
    s = J.colour.program_struct([("hue", 256)])
    px = np.arange(12, dtype=np.uint8)
    assert emu.emu_colour_pixel(px.ctypes.data, 2, 2, C.byref(s), 1024, 0) != 0 and np.array_equal(px, np.arange(12))  # (refused: nothing written)


def test_the_device_arithmetic_of_hue_over_every_colour(emu, round_trip):
    """The C++ float and double statement, as the kernel's HUE pass runs it, over all 2^24 colours against the numbers Pillow's sums pin."""
    every = PR.all_colours()
    want = round_trip.hue(43)
    for i in range(4):
        assert np.array_equal(_emu(emu, every[i], [("hue", 43)], 1024), want[i]), i
    rng = np.random.default_rng(2104)
    for shift in (0, 1, 128, 213, 255):  # (the other golden shifts: a sample of colours, pixel by pixel)
        w = round_trip.hue(shift).reshape(-1, 3)
        for k in rng.integers(0, 1 << 24, 3000):
            k = int(k)
            c = emu.emu_colour_hue_pixel(k >> 16, (k >> 8) & 255, k & 255, shift)
            assert (c & 255, (c >> 8) & 255, c >> 16) == tuple(int(v) for v in w[k]), (k, shift)


def test_bodies_and_job_builder_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing is loaded into Python."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "colour_pixel_asan")
    cmd = [cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17", "-Wall",
           "-Wno-unknown-pragmas", "-Wno-unused-function", "-ffp-contract=off", "-DJPGPU_HOST_EMULATION", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"),
           "-o", exe, os.path.join(_EMU, "colour_pixel_asan.cpp")]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "colour_pixel_asan: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
