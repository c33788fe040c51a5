"""EXIF orientation on the CPU (no GPU): the numpy statement (tests/orient_ref.py) against what Pillow's ImageOps.exif_transpose gave
(tests/golden/orient/pillow_orient.json, written by tools/make_orient_golden.py — Pillow itself is not needed here), and the library's
pure host functions — jpgpu_exif_orientation, jpgpu_oriented_window — against the file and the statement; then the kernel's body
emulated lane by lane (tests/test_orient_emulation.py, tests/emu/emu_orient.cpp).

One collected test, `test_orientation_on_the_cpu`, runs every check below and every check of tests/test_orient_emulation.py, and
reports all that fail."""
import json
import os

import numpy as np
import pytest

import jpeg_decoder_amd as J
import orient_ref as OR
import test_orient_emulation as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "orient", "pillow_orient.json")


def golden_file():
    return json.load(open(GOLDEN))


def the_numpy_statement_is_what_pillow_computes(golden):
    seen = set()
    for c in golden["images"]:
        a = np.array(c["source"], np.uint8).reshape(c["H"], c["W"], c["nc"])
        o = c["orientation"]
        assert c["pillow_reads"] == o
        got = OR.orient(a, o)
        assert [got.shape[1], got.shape[0]] == c["size"] == list(OR.oriented_size(o, c["W"], c["H"])), c
        assert got.reshape(-1).tolist() == c["oriented"], (c["nc"], o)
        seen.add((c["nc"], o))
    assert seen == {(nc, o) for nc in (1, 3, 4) for o in range(1, 9)}
    # the eight results of one array differ from each other: the set tells the orientations apart
    for nc in (1, 3, 4):
        assert len({tuple(c["oriented"]) + tuple(c["size"]) for c in golden["images"] if c["nc"] == nc}) == 8


def exif_orientation_against_the_golden_blobs(golden):
    blobs = golden["exif"]
    assert len(blobs) >= 12
    names = " | ".join(b["name"] for b in blobs)
    for must in ("II orientation", "MM orientation", "tag absent", "value 0", "value 9", "type LONG", "count 2", "cut inside"):
        assert must in names
    for b in blobs:
        blob = bytes.fromhex(b["blob"])
        assert OR.exif_orientation(blob) == b["orientation"], b["name"]
        assert J.exif_orientation(blob) == b["orientation"], b["name"]
        if b["orientation"] != 1:  # (where the rule finds an orientation Pillow reads the same one)
            assert b["pillow"] == b["orientation"], b["name"]
    assert J.exif_orientation(None) == 1 and J.exif_orientation(b"") == 1


def exif_orientation_reads_nothing_outside_the_blob(golden):
    """Every prefix of every golden blob, and random bytes behind a TIFF header: the library and the statement agree, nothing raises."""
    rng = np.random.default_rng(5)
    for b in golden["exif"]:
        blob = bytes.fromhex(b["blob"])
        for n in range(len(blob) + 1):
            assert J.exif_orientation(blob[:n]) == OR.exif_orientation(blob[:n]), (b["name"], n)
    for k in range(2000):
        head = (b"II*\0" if k & 1 else b"MM\0*")
        body = bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8))
        off = int(rng.integers(0, 40))
        blob = head + (off.to_bytes(4, "little") if k & 1 else off.to_bytes(4, "big")) + body
        assert J.exif_orientation(blob) == OR.exif_orientation(blob), blob.hex()


def oriented_window_host_function():
    rng = np.random.default_rng(9)
    for _ in range(300):
        w, h, o = int(rng.integers(1, 400)), int(rng.integers(1, 400)), int(rng.integers(1, 9))
        ow, oh = OR.oriented_size(o, w, h)
        assert J.oriented_size(o, (w, h)) == (ow, oh)
        x, y = int(rng.integers(0, ow)), int(rng.integers(0, oh))
        win = (x, y, int(rng.integers(1, ow - x + 1)), int(rng.integers(1, oh - y + 1)))
        assert J.oriented_window(o, (w, h), win) == ((ow, oh), OR.source_window(o, w, h, win))
        with pytest.raises(J.FormatError):
            J.oriented_window(o, (w, h), (x, y, ow - x + 1, 1))
    assert J.oriented_window(6, (10, 20), None) == ((20, 10), None)
    assert J.oriented_window(6, (10, 20), (0, 0, 20, 10)) == ((20, 10), (0, 0, 10, 20))
    for bad in (0, 9, 255):
        with pytest.raises(J.FormatError):
            J.oriented_window(bad, (10, 20), None)


def test_orientation_on_the_cpu(tmp_path):
    golden = golden_file()
    emu = EM.build(tmp_path)
    parts = [("the numpy statement is what Pillow computes", lambda: the_numpy_statement_is_what_pillow_computes(golden)),
             ("jpgpu_exif_orientation against the golden blobs", lambda: exif_orientation_against_the_golden_blobs(golden)),
             ("jpgpu_exif_orientation reads nothing outside the blob", lambda: exif_orientation_reads_nothing_outside_the_blob(golden)),
             ("jpgpu_oriented_window", oriented_window_host_function)] + EM.checks(emu)
    assert len(parts) == 9
    failed = []
    for name, part in parts:
        try:
            part()
        except Exception as e:  # (an AssertionError among them: every part runs, every failure is reported)
            failed.append(f"{name}: {type(e).__name__}: {e}")
    assert not failed, "\n".join(failed)
