"""The crafted streams of tests/entropy_cases.py through the CPU twins of the device entropy decoders (tests/emu): what the emulated
device makes of each must be what the host front-end makes of it, the oracle's outcome must be the host front-end's, and the flag
`stays_on_device` every case carries — which tests/test_gpu_entropy_cases.py holds the GPU to — must be exactly this result: status 0
under every emission parameter (sequential), the host's planes on every walk (progressive).  The streams themselves are checked too:
that their predictors do wrap, their magnitudes do reach 15 bits, their codes do take the routes they were built for."""
import numpy as np
import pytest

import entropy_cases as E
import jpeg_decoder_amd as J
import oracle as O
import test_device_entropy_emulation as S
import test_progressive_emulation as G
from test_device_entropy_emulation import emission  # noqa: F401  (the fixture: five settings of the emission)

_HOST = {}


def _host_outcome(case):
    """(desc, planes) of the host front-end, or its error — decoded once per case"""
    if case.name not in _HOST:
        try:
            _HOST[case.name] = S._host(case.data)
        except J.Error as e:
            _HOST[case.name] = e
    return _HOST[case.name]


@pytest.mark.parametrize("case", E.ALL_SEQUENTIAL + E.DECODER + E.PROGRESSIVE, ids=lambda c: c.name)
def test_oracle_and_host_front_end_agree(case):
    """pixels from the host front-end's coefficients through the oracle's pixel stage == the oracle's decode of the bytes; or the same
    kind of error from both"""
    host = _host_outcome(case)
    try:
        want = O.decode(case.data)
    except O.OracleError as e:
        assert isinstance(host, J.Error) and host.kind == e.kind, (host, e)
        return
    assert not isinstance(host, Exception), host
    hdesc, hcoefs = host
    sampling = [(hdesc.components[c].horizontal_sampling_factor, hdesc.components[c].vertical_sampling_factor) for c in range(hdesc.ncomp)]
    ocomps, _ = O.make_components(want.width, want.height, sampling)
    qts = [np.array(list(hdesc.quantization_tables[c]), np.uint16) for c in range(hdesc.ncomp)]
    got = O.pixels_from_coefficients(ocomps, qts, [np.asarray(p, np.int16) for p in hcoefs], want.width, want.height, "YCBCR" if hdesc.ncomp == 3 else "GRAYSCALE")
    assert np.array_equal(got, want.pixels)


@pytest.mark.parametrize("case", E.ALL_SEQUENTIAL + E.DECODER, ids=lambda c: c.name)
def test_sequential_cases_on_the_emulated_device(case, emission):  # noqa: F811
    got = S._device(case.data)
    assert got is not None  # (the planner lets every one of them through: what becomes of it is the status word's business)
    st, desc, planes, _ns, n_seg = got
    assert (st == 0) == case.stays_on_device, (case.name, hex(st), emission)  # the flag is this result and nothing else
    if st != 0:
        return
    hdesc, hcoefs = _host_outcome(case)
    for c in range(desc.ncomp):
        assert np.array_equal(planes[c], hcoefs[c]), c
    S._check_range_by_product(desc, planes)


@pytest.fixture(params=[8, 3], ids=["first-pass-over-whole-chunks", "first-pass-over-three-eighths"])
def small_call_chunking(request):
    """the chunking csrc/batch_entropy.cpp gives a small call (entropy_cases.SMALL_CALL_CHUNKING) instead of the emulation's 48 / 10 / 32"""
    k = E.SMALL_CALL_CHUNKING
    L = S.emu.lib()
    L.emu_huff_set_chunking(k["blocks"], k["min_shift"], k["launches"])
    L.emu_huff_set_launch(k["iters"], 256, 0)
    L.emu_huff_set_tail(request.param)  # (k["tail"]: a call of one or two sub-batches; 3: a larger one, which settles no less)
    yield request.param
    L.emu_huff_set_chunking(0, 0, 0)
    L.emu_huff_set_launch(1, 256, 0)
    L.emu_huff_set_tail(8)


@pytest.mark.parametrize("case", E.ALL_SEQUENTIAL + E.DECODER, ids=lambda c: c.name)
def test_sequential_cases_in_the_chunking_of_a_small_call(case, small_call_chunking):
    """Which streams settle in 16 launches of two passes over chunks of 12 blocks: `settles_in_a_small_call` is this result.  The twin
    runs the workgroups of a launch one after the other, each on what the launch before left — the least the device guarantees; on the
    device a lane may find what its left neighbour published earlier in the same pass, so a stream that does not settle here may
    settle there, never the other way round.  Where the status is 0 the planes are the host's."""
    got = S._device(case.data)
    assert got is not None
    st, desc, planes, _ns, _n_seg = got
    if small_call_chunking == E.SMALL_CALL_CHUNKING["tail"]:
        assert (st == 0) == case.settles_in_a_small_call, (case.name, hex(st), S._device.last_passes)
    elif case.settles_in_a_small_call:
        assert st == 0, (case.name, hex(st))
    if case.stays_on_device and st != 0:
        assert st & 64, hex(st)  # (unsettled, nothing else)
    if st == 0:
        _hdesc, hcoefs = _host_outcome(case)
        for c in range(desc.ncomp):
            assert np.array_equal(planes[c], hcoefs[c]), c
        S._check_range_by_product(desc, planes)


@pytest.mark.parametrize("case", E.TO_THE_HOST, ids=lambda c: c.name)
def test_streams_for_the_host_are_refused_or_flagged(case):
    got = S._device(case.data)
    assert got is None or got[0] != 0
    assert not case.stays_on_device


@pytest.mark.parametrize("case", E.PROGRESSIVE, ids=lambda c: c.name)
@pytest.mark.parametrize("order", [0, 4, 5], ids=["tracks-in-order", "a-wave-per-scan", "a-wave-per-track"])
def test_progressive_cases_on_the_emulated_device(case, order):
    assert case.stays_on_device
    G._same_as_host(case.data, order)


def _planes(case):
    desc, coefs = _host_outcome(case)
    return desc, [np.asarray(p, np.int64).reshape(-1, 64) for p in coefs]


@pytest.mark.parametrize("case", [c for c in E.ALL_SEQUENTIAL + E.DECODER + E.PROGRESSIVE if c.stays_on_device], ids=lambda c: c.name)
def test_sane_class_flag_is_what_the_coefficients_say(case):
    """in_sane_class: no product coefficient x quantization value reaches 2^15 (what the entry-list walk of 4:2:0 frames trusts)"""
    desc, planes = _planes(case)
    top = max(int(np.abs(p * np.array(list(desc.quantization_tables[c]), np.int64)).max()) for c, p in enumerate(planes))
    assert case.in_sane_class == (top < 1 << 15), top


def _case(name):
    return next(c for c in E.ALL_SEQUENTIAL + E.PROGRESSIVE if c.name == name)


def _eob_runs_of_first_ac_scan(data):
    """the end-of-band run lengths of the first AC scan (Ah = 0) of a progressive stream, read symbol by symbol with the scan's own table"""
    i, table = 2, None
    while True:
        m, ln = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == 0xC4 and data[i + 4] >> 4 == 1:
            table = (list(data[i + 5:i + 21]), list(data[i + 21:i + 2 + ln]))
        if m == 0xDA and data[i + 2 + ln - 3] >= 1 and data[i + 2 + ln - 1] >> 4 == 0:
            break
        i += 2 + ln
        if m == 0xDA:  # another scan's data: on to the next marker
            while not (data[i] == 0xFF and data[i + 1] not in (0, 0xFF) and not 0xD0 <= data[i + 1] <= 0xD7):
                i += 1
    start = i + 2 + ln
    end = start
    while not (data[end] == 0xFF and data[end + 1] != 0):
        end += 1
    bits = "".join(f"{b:08b}" for b in data[start:end].replace(b"\xff\x00", b"\xff"))
    code, length = E._code_table(table)
    by_code = {(int(length[s]), int(code[s])): s for s in table[1]}
    pos, runs = 0, []
    while pos < len(bits):
        for n in range(1, 17):
            if pos + n > len(bits):
                return runs  # (the padding of the last byte)
            sym = by_code.get((n, int(bits[pos:pos + n], 2)))
            if sym is not None:
                break
        else:
            return runs
        pos += n
        r, sz = sym >> 4, sym & 15
        if sz == 0 and r < 15:
            runs.append((1 << r) + (int(bits[pos:pos + r], 2) if r else 0))
            pos += r
        else:
            pos += sz
    return runs


def test_streams_are_what_their_names_say():
    # dc-wrap: the sum of the differences leaves the 16-bit range again and again, in both directions, in every component
    for name in ("dc-wrap-gray-q1", "dc-wrap-420-q255", "uniform-420"):
        desc, planes = _planes(_case(name))
        for p in planes:
            dc = p[:, 0]
            assert dc.max() > 32767 - 2047 and dc.min() < -32768 + 2047
            jumps = np.abs(np.diff(dc))
            assert (jumps > 60000).sum() >= 3, name  # (a difference of 2,047 that shows as one of 63,489: a wrap)
    # ac-size-15: both extremes of every size, both signs
    for name in ("ac-size-15-gray-q1", "ac-size-15-420-q1"):
        _desc, planes = _planes(_case(name))
        ac = np.concatenate([p[:, 1:].reshape(-1) for p in planes])
        for s in range(1, 16):
            for v in ((1 << s) - 1, 1 << (s - 1)):
                assert (ac == v).any() and (ac == -v).any(), (name, s, v)
    # long codes: coefficients at index 63, empty blocks, runs of every length, ZRL chains of 1..3
    _desc, planes = _planes(_case("long16-gray"))
    p = planes[0][:, E.UNZIGZAG]  # zig-zag order
    assert (p[:, 63] != 0).sum() > 20 and (~p[:, 1:].any(axis=1)).sum() > 20
    runs = set()
    for blk in p:
        pos = np.flatnonzero(blk[1:]) + 1
        runs |= set(np.diff(np.concatenate(([0], pos))) - 1)
    assert set(range(16)) <= {r % 16 for r in runs} and {r // 16 for r in runs} >= {0, 1, 2, 3}
    # giant blocks: longer than the smallest chunk
    data = _case("giant-blocks-all").data
    assert E.scan_density(data)[1] * 8 / 48 > 1500
    # 0xFF density
    for name in ("ff-dense-gray", "ff-dense-420", "ff-dense-420-ri1"):
        ff, total = E.scan_density(_case(name).data)
        assert 3 * ff >= total, (name, ff, total)
    # restart numbering wraps at least twice
    for c in E.SEQUENTIAL:
        if "-ri" in c.name:
            assert sum(c.data.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) >= 16, c.name
    # the end-of-band run at its cap: the first AC scan, parsed here, holds EOB14 followed by fourteen 1-bits (the refinement scan is
    # written by the same run counter, tools/progressive_encoder.py _ac_refine, over the same empty blocks)
    desc, planes = _planes(_case("prog-eobrun-cap"))
    assert planes[0].shape[0] >= 32768 and np.count_nonzero(planes[0][:, 1:]) == 5
    runs = _eob_runs_of_first_ac_scan(_case("prog-eobrun-cap").data)
    assert 32767 in runs and sum(runs) > 32768, runs
    # DC values at both ends of the 16-bit range
    for name in ("prog-dc-extreme-gray", "prog-dc-extreme-420"):
        _desc, planes = _planes(_case(name))
        for p in planes:
            assert p[:, 0].max() == 32767 and p[:, 0].min() == -32768, name
    _desc, planes = _planes(_case("prog-dense-extreme-420-split"))
    assert all((p[:, 1:] != 0).all() and np.abs(p[:, 1:]).max() == 1023 for p in planes)


def test_table_builders_send_codes_where_they_say():
    routes, n = E.code_routes(E.long16_ac())
    assert n <= E.HUFF_SUB_TABLES and sum(r == "lut2" for r in routes.values()) >= 142
    routes, n = E.code_routes(E.wide_ac())
    assert n > E.HUFF_SUB_TABLES and {"lut", "lut2", "walk"} == set(routes.values())
    for spec in (E.long16_ac(), E.long16_dc(), E.wide_ac(), E.wide_dc(), E.ones_dc(), E.ones_ac(), E.long16_ac(E.AC_SYMBOLS_15), E.wide_ac(E.AC_SYMBOLS_15)):
        assert E.kraft(spec) <= 1.0
    # the streams use them: symbols of every route occur in the `wide` stream
    _desc, planes = _planes(_case("wide-gray"))
    p = planes[0][:, E.UNZIGZAG]
    used = set()
    for blk in p:
        pos = np.flatnonzero(blk[1:]) + 1
        run = np.diff(np.concatenate(([0], pos))) - 1
        used |= {int(((r & 15) << 4) | int(abs(v)).bit_length()) for r, v in zip(run, blk[pos])}
    routes, _n = E.code_routes(E.wide_ac())
    assert {routes[s] for s in used} == {"lut", "lut2", "walk"}
