"""The crafted streams of tests/entropy_cases.py on the MI355X: the device entropy decoders (chunk decoder with its second-level tables
and maxcode walk, restart segments, staging pass, DC prefix sums, range by-product, the 4:2:0 entry-list walk, the wave-per-scan
progressive decoder) on inputs no encoder writes from an image.  Expected value everywhere: the oracle's decode of the same bytes —
equal pixels or the same kind of error; and the route counters must say that the device did the work: a case the emulated device
decodes with status 0 (`stays_on_device`, asserted on the CPU by tests/test_entropy_cases_emulation.py) must not come back to the host."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import entropy_cases as E
import oracle as O
import resample_ref as R

pytestmark = pytest.mark.gpu
J = None
_WANT = {}


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    assert J.device_count() >= 1


def _expect(case):
    """the oracle's pixels or its error, decoded once per case"""
    if case.name not in _WANT:
        try:
            _WANT[case.name] = O.decode(case.data)
        except O.OracleError as e:
            _WANT[case.name] = e
    return _WANT[case.name]


def _check(cases, out, label=""):
    for c, got in zip(cases, out):
        want = _expect(c)
        if isinstance(want, O.OracleError):
            assert isinstance(got, J.Error) and got.kind == want.kind, (label, c.name, got, want)
        else:
            assert not isinstance(got, Exception), (label, c.name, got)
            assert np.array_equal(got, want.pixels), (label, c.name)


def _counters(p, label):
    t = p.timings()
    print(f"routes [{label}]: device={t['images_device_entropy']} rejected={t['images_device_rejected']} entry_walk={t['images_entry_pixels']} "
          f"host_light={t['images_host_light']} device_progressive={t['images_device_progressive']}")
    return t


def _expected_sequential(cases, entry_walk):
    """(images_device_entropy, images_device_rejected, images_entry_pixels) of a call of `cases` — the planner lets all of them through"""
    handed_back = [c for c in cases if not c.stays_on_device]
    # the entry-list walk runs the `sane` arithmetic on trust and flags what leaves it: the host decodes those with the wrap-exact kernels
    # (test_entry_lists_coefficients_outside_the_sane_class_go_back_to_the_host)
    out_of_class = [c for c in cases if entry_walk and c.entry_walk and c.stays_on_device and not c.in_sane_class]
    return len(cases), len(handed_back) + len(out_of_class), sum(c.entry_walk for c in cases) if entry_walk else 0


def _run_routes():
    """Every sequential case in one call, twice on the same pipeline (buffers and table sets reused), then with the entry-list walk off —
    staged by the host and by the device (host light) — then one case per call, so that the route of each is known, then through the
    host decoder as the control."""
    os.environ["JPGPU_PIPE_FORCE_DEVICE"] = "1"  # (small files: the cost model would keep some on the host)
    cases = E.ALL_SEQUENTIAL + E.DECODER
    files = [c.data for c in cases]
    p = J.Pipeline(threads=4)
    for host_light in (False, True):
        for entry_walk in (True, True, False):
            os.environ["JPGPU_PIPE_ENTRY_PIXELS"] = "1" if entry_walk else "0"
            out = p.decode(files, device_entropy=True, host_light=host_light)
            t = _counters(p, f"all sequential, entry walk {'on' if entry_walk else 'off'}, host_light={host_light}")
            _check(cases, out, f"entry walk {entry_walk}")
            n_device, n_rejected, n_entry = _expected_sequential(cases, entry_walk)
            assert t["images_device_entropy"] == n_device, t
            assert t["images_device_rejected"] == n_rejected, t
            assert t["images_entry_pixels"] == n_entry, t
            assert (t["images_host_light"] > 0) == host_light, t
    os.environ["JPGPU_PIPE_ENTRY_PIXELS"] = "1"
    for c in cases:
        out = p.decode([c.data], device_entropy=True)
        t = _counters(p, c.name)
        _check([c], out, "alone")
        assert (t["images_device_entropy"], t["images_device_rejected"], t["images_entry_pixels"]) == _expected_sequential([c], True), (c.name, t)
    out = p.decode(files, device_entropy=False)
    _check(cases, out, "host control")
    assert p.timings()["images_device_entropy"] == 0
    p.close()


def _run_small_chunks():
    cases = E.ALL_SEQUENTIAL
    p = J.Pipeline(threads=4)
    for rep in range(2):
        _check(cases, p.decode([c.data for c in cases], device_entropy=True), f"small chunks, call {rep}")
        t = _counters(p, f"small chunks, call {rep}")
        assert t["images_device_entropy"] == len(cases), t
    p.close()
    _run_decoder(device_route=False)  # (pixels only here too)


def _run_decoder(device_route=True):
    """the 1280 x 720 stream through Decoder.decode(); device_route: and as a one-image Pipeline call on the same bytes, which has
    counters — the stream (`settles_in_a_small_call`, asserted on the CPU twin) is decoded by the device and does not come back"""
    case = E.DECODER[0]
    assert case.stays_on_device and case.settles_in_a_small_call
    want = O.decode(case.data).pixels
    assert np.array_equal(J.Decoder(case.data).decode(), want)
    if device_route:
        p = J.Pipeline(threads=4)
        out = p.decode([case.data], device_entropy=True)
        t = _counters(p, case.name + ", one-image call")
        assert np.array_equal(out[0], want)
        assert t["images_device_entropy"] == 1 and t["images_device_rejected"] == 0, t
        p.close()


def _run_decoder_on_the_host():
    _run_decoder(device_route=False)


def _child(what, env):
    """`what` (a function of this module) in a process of its own: the library reads the settings in `env` once"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import jpeg_decoder_amd, test_gpu_entropy_cases as T\nT.J = jpeg_decoder_amd\nT.%s()\nprint('ok')\n") % (os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle"), here, what)
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])


# The chunking tests/emu decodes with — chunks of 48 blocks' worth of bits and at least 1,024, up to 32 launches of one pass: what
# `stays_on_device` was established under.  (Left to itself the library cuts a small call into chunks of 12 blocks and gives it 32
# passes; streams that settle one chunk per pass then come back unsettled, status 0x41, and the host decodes them: DESIGN.md §4.5;
# test_sequential_cases_in_the_chunking_of_a_small_call holds the device to what the CPU twin says of that chunking.)
EMULATION_CHUNKING = {"JPGPU_SYNC_BLOCKS": "48", "JPGPU_SYNC_MIN_SHIFT": "10", "JPGPU_SYNC_LAUNCHES": "32", "JPGPU_SYNC_ITERS": "1"}


def test_sequential_cases_stay_on_the_device():
    """images_device_rejected == the streams the emulated device hands back (+ the 4:2:0 ones the entry-list walk flags as out of its
    arithmetic class), images_device_entropy == every stream the planner lets through, images_entry_pixels == the 4:2:0 ones with
    tables per component; pixels or error kind as the oracle's, every call."""
    _child("_run_routes", EMULATION_CHUNKING)


def test_sequential_cases_in_chunks_of_a_dozen_blocks():
    """Chunks of 12 blocks' worth of bits and at least 512: nearly every chunk of the giant-block streams lies inside one block, and
    most chunks are corrected in the late launches.  Pixel or error equality only (what settles in 40 launches is not the point)."""
    _child("_run_small_chunks", {"JPGPU_PIPE_FORCE_DEVICE": "1", "JPGPU_SYNC_BLOCKS": "12", "JPGPU_SYNC_MIN_SHIFT": "9", "JPGPU_SYNC_TAIL": "1", "JPGPU_SYNC_LAUNCHES": "40"})


def test_decoder_long_codes_and_wrapping_predictors(monkeypatch):
    """One 1280 x 720 gray stream (above the Decoder's threshold for the device route) with `long16` tables and DC differences that wrap,
    in restart segments short enough to settle in a one-image call: through Decoder.decode(), through a one-image Pipeline call whose
    counters show the device route taken and nothing handed back, and with the Decoder's device route switched off in a process of its own."""
    monkeypatch.setenv("JPGPU_PIPE_FORCE_DEVICE", "1")
    _run_decoder()
    _child("_run_decoder_on_the_host", {"JPGPU_DECODER_NO_DEVICE_ENTROPY": "1"})


def test_sequential_cases_in_the_chunking_of_a_small_call(monkeypatch):
    """The library's own settings (no JPGPU_SYNC_* pinned): a one-image call is cut into chunks of 12 blocks and given 32 passes.  One case
    per call: a case the CPU twin settles in that chunking (`settles_in_a_small_call`) must stay on the device here too; one it does not
    may come back unsettled (the device can only be quicker than the twin, see tests/test_entropy_cases_emulation.py) — and must then be
    the oracle's pixels through the host."""
    monkeypatch.setenv("JPGPU_PIPE_FORCE_DEVICE", "1")
    monkeypatch.delenv("JPGPU_PIPE_ENTRY_PIXELS", raising=False)
    p = J.Pipeline(threads=4)
    try:
        for c in E.ALL_SEQUENTIAL + E.DECODER:
            out = p.decode([c.data], device_entropy=True)
            t = _counters(p, c.name + ", small call")
            _check([c], out, "small call")
            n_device, n_rejected, n_entry = _expected_sequential([c], True)
            assert (t["images_device_entropy"], t["images_entry_pixels"]) == (n_device, n_entry), (c.name, t)
            allowed = {n_rejected} if c.settles_in_a_small_call or not c.stays_on_device else {n_rejected, 1}
            assert t["images_device_rejected"] in allowed, (c.name, t)
    finally:
        p.close()


def _pillow(w, h, sub, seed, gray=False):
    from PIL import Image
    import synth
    rgb = synth.synthetic_rgb(w, h, seed=seed)
    buf = io.BytesIO()
    Image.fromarray(rgb[..., 0] if gray else rgb).save(buf, format="JPEG", quality=60 + 3 * seed, subsampling=sub, optimize=True)
    return buf.getvalue()


def _table_set(data):
    """the DHT payloads of a file, as one key"""
    key, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xFF and data[i + 1] != 0xDA:
        ln = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xC4:
            key.append(data[i + 4:i + 2 + ln])
        i += 2 + ln
    return b"".join(key)


def test_crafted_and_encoder_written_files_of_one_geometry_share_a_call(monkeypatch):
    """The 256 x 192 cases interleaved with Pillow-written files of the same size (optimised tables: a set per file) — several table sets
    per sub-batch, more distinct ones in the call than the process-wide cache of device table sets holds (8) — and the call again."""
    monkeypatch.setenv("JPGPU_PIPE_FORCE_DEVICE", "1")
    names, files, crafted = [], [], []
    k = 0
    for c in E.SEQUENTIAL:
        if len(_expect(c).pixels) not in (256 * 192, 256 * 192 * 3) or c.sampling == E.S444:
            continue
        crafted.append(c)
        names.append(c.name), files.append(c.data)
        names.append(f"pillow-{k}"), files.append(_pillow(256, 192, "4:2:0" if c.is_420 else "4:4:4", k, gray=not c.is_420))
        k += 1
    assert len({_table_set(f) for f in files}) > 8
    want = [O.decode(f).pixels for f in files]
    must_come_back = sum(c.entry_walk and not c.in_sane_class for c in crafted)  # (the entry-list walk's range flag)
    may_come_back = sum(not c.settles_in_a_small_call and (not c.entry_walk or c.in_sane_class) for c in crafted)
    p = J.Pipeline(threads=4)
    try:
        for rep in range(2):
            out = p.decode(files, device_entropy=True)
            t = _counters(p, f"mixed call {rep}")
            for n, got, w in zip(names, out, want):
                assert not isinstance(got, Exception) and np.array_equal(got, w), (rep, n)
            # (the library's own chunking: beyond those, only streams the CPU twin does not settle in a small call's chunking may come back)
            assert t["images_device_entropy"] == len(files) and must_come_back <= t["images_device_rejected"] <= must_come_back + may_come_back, t
    finally:
        p.close()


@pytest.mark.parametrize("variant", ["wave-per-scan", "lane-per-track"])
def test_progressive_cases_stay_on_the_device(monkeypatch, variant):
    """Dense blocks of extreme values under four steps of successive approximation, the end-of-band run at its cap of 32,767 blocks, DC
    values over the whole 16-bit range: every frame decoded by the device's progressive walk, twice, then by the host as the control."""
    monkeypatch.setenv("JPGPU_PIPE_PROG_DEVICE_PERCENT", "100")
    monkeypatch.delenv("JPGPU_PROG_LANES_MAX", raising=False)
    if variant == "lane-per-track":
        monkeypatch.setenv("JPGPU_PROG_LANES_MAX", "0")
    cases = [c for c in E.PROGRESSIVE if c.stays_on_device]
    assert len(cases) == len(E.PROGRESSIVE)
    files = [c.data for c in cases]
    p = J.Pipeline(threads=4)
    try:
        for rep in range(2):
            out = p.decode(files, device_entropy=True)
            t = _counters(p, f"progressive, {variant}, call {rep}")
            _check(cases, out, variant)
            assert t["images_device_progressive"] == len(cases) and t["images_device_rejected"] == 0, t
        out = p.decode(files, device_entropy=True, progressive_on_host=True)
        _check(cases, out, "host control")
        assert p.timings()["images_device_progressive"] == 0
    finally:
        p.close()


def _run_windows():
    os.environ["JPGPU_PIPE_FORCE_DEVICE"] = "1"
    cases = [c for c in E.SEQUENTIAL if c.name in ("dc-wrap-420-q1", "dc-wrap-420-q255", "ac-size-15-420-q1", "ac-size-15-420-q255", "ac-size-15-gray-q255")]
    assert len(cases) == 5
    wins = [(13, 7, 201, 151), (101, 33, 155, 159), (1, 1, 255, 191), (77, 9, 35, 171), (13, 7, 201, 151)]
    size = (37, 53)
    p = J.Pipeline(threads=4)
    out = p.decode([c.data for c in cases], device_entropy=True, windows=wins, output_size=size)
    t = _counters(p, "windows + resize")
    for c, (x, y, w, h), got in zip(cases, wins, out):
        want = _expect(c)
        nc = 3 if c.is_420 else 1
        src = want.pixels.reshape(want.height, want.width, nc)[y:y + h, x:x + w]
        assert not isinstance(got, Exception), (c.name, got)
        assert np.array_equal(got, R.resize(src, size[0], size[1]).reshape(-1)), c.name
    # (windowed images take the expansion and the window kernel, not the entry-list walk: nothing is flagged, nothing comes back)
    assert t["images_device_entropy"] == len(cases) and t["images_device_rejected"] == 0 and t["images_windowed"] == len(cases), t
    p.close()


def test_windows_and_resize_on_wrap_exact_coefficients():
    """Windows at odd coordinates resampled to 37 x 53 from coefficients that need the wrap-exact arithmetic (class 0, drawn from the
    range by-product of the device's expansion): the window kernel's rings and the resample behind it, against resample_ref of the
    oracle's slice.  In the emulation's chunking, so that the streams stay on the device."""
    _child("_run_windows", EMULATION_CHUNKING)
