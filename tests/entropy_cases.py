"""Crafted entropy-coded streams at the limits of the format, defined once for tests/test_entropy_cases_emulation.py (the CPU twin of
the device decoders) and tests/test_gpu_entropy_cases.py (the device itself): 16-bit Huffman codes that go through the second-level
tables (DevHuffTable::lut2) and through the maxcode walk (huff_walk), DC predictors that pass the 16-bit wrap, AC magnitudes of up to
15 bits, blocks longer than a chunk, scans that are mostly 0xFF bytes, restart intervals of one MCU, three components on one pair of
tables, streams the device has to hand back (SYM_BAD and its relatives) — and progressive frames with dense blocks of extreme values,
end-of-band runs at the 32,767 cap and DC values at the ends of the 16-bit range.  Nothing here comes from an image: coefficients are
drawn from seeded generators, tables are built by hand and checked (Kraft sum, which route every code takes on the device).

pure numpy; the bit packing and the canonical code assignment are tools/baseline_encoder.py's, the progressive coder is
tools/progressive_encoder.py's."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import baseline_encoder as B  # noqa: E402
import progressive_encoder as P  # noqa: E402
from baseline_encoder import UNZIGZAG, _code_table, _marker, _pack_bits  # noqa: E402

HUFF_LUT_BITS, HUFF_SUB_TABLES = 10, 12  # csrc/huff_job.hpp
DC, AC, RAW = 0, 1, 2                    # token classes; RAW: `extra bits` bits of `extra value`, no Huffman code

GRAY, S420, S444 = [(1, 1)], [(2, 2), (1, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)]


# ---- (b) tables ---------------------------------------------------------------------------------------------------------------------
def kraft(spec):
    return sum(n * 2.0 ** -(ln + 1) for ln, n in enumerate(spec[0]))


def code_routes(spec):
    """symbol -> "lut" (code of at most HUFF_LUT_BITS bits), "lut2" (its 10-bit prefix is one of the first HUFF_SUB_TABLES unresolved
    prefixes in ascending order: csrc/host/frontend.cpp gives those second-level tables) or "walk" (huff_walk)."""
    code, length = _code_table(spec)
    long_ = [s for s in spec[1] if length[s] > HUFF_LUT_BITS]
    prefixes = sorted({int(code[s]) >> (int(length[s]) - HUFF_LUT_BITS) for s in long_})
    with_table = set(prefixes[:HUFF_SUB_TABLES])
    routes = {s: "lut" for s in spec[1]}
    for s in long_:
        routes[s] = "lut2" if (int(code[s]) >> (int(length[s]) - HUFF_LUT_BITS)) in with_table else "walk"
    return routes, len(prefixes)


def _checked(spec):
    bits, vals = spec
    assert len(bits) == 16 and sum(bits) == len(vals) == len(set(vals)) and kraft(spec) <= 1.0, (bits, len(vals), kraft(spec))
    code, length = _code_table(spec)
    assert all(int(code[s]) != (1 << int(length[s])) - 1 for s in vals if length[s] == 16)  # (no code of sixteen 1-bits)
    return list(bits), list(vals)


AC_SYMBOLS_10 = [0x00, 0xF0] + [(r << 4) | s for s in range(1, 11) for r in range(16)]  # the 162 of a baseline table
AC_SYMBOLS_15 = [0x00, 0xF0] + [(r << 4) | s for s in range(1, 16) for r in range(16)]  # ... and with sizes 11..15: 242


def long16_ac(symbols=AC_SYMBOLS_10):
    """lengths 2..9 once, 10..15 twice, everything else (142 of 162 symbols) 16 bits: few enough unresolved prefixes for every one of
    them to get a second-level table — 16-bit codes read through lut2."""
    bits = [0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, len(symbols) - 20]
    spec = _checked((bits, list(symbols)))
    routes, n_prefixes = code_routes(spec)
    assert n_prefixes <= HUFF_SUB_TABLES and "walk" not in routes.values() and sum(r == "lut2" for r in routes.values()) >= len(symbols) - 22
    return spec


def long16_dc():
    """one code of every length 5..16"""
    spec = _checked(([0, 0, 0, 0] + [1] * 12, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]))
    routes, _n = code_routes(spec)
    assert sum(r == "lut2" for r in routes.values()) == 6
    return spec


def wide_ac(symbols=AC_SYMBOLS_10):
    """twenty codes each of 11..15 bits: 15 unresolved prefixes under the 11- and 12-bit codes alone, so the first twelve (11-bit codes
    and some 12-bit ones) get second-level tables and every code of 13..16 bits takes huff_walk."""
    bits = [0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 20, 20, 20, 20, 20, len(symbols) - 110]
    spec = _checked((bits, list(symbols)))
    routes, n_prefixes = code_routes(spec)
    _code, length = _code_table(spec)
    assert n_prefixes > HUFF_SUB_TABLES
    in_lut2 = {int(length[s]) for s, r in routes.items() if r == "lut2"}
    in_walk = {int(length[s]) for s, r in routes.items() if r == "walk"}
    assert {11, 12} <= in_lut2 and {13, 14, 15, 16} <= in_walk and not (in_lut2 & {13, 14, 15, 16}), (in_lut2, in_walk)
    return spec


def wide_dc():
    """twelve symbols: 1 x 2 bits, 1 x 3, 2 x 11, 2 x 12, 2 x 13, 2 x 14, 1 x 15, 1 x 16 (so few codes share a handful of prefixes:
    every long one has a second-level table)"""
    return _checked(([0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 1, 1], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]))


def unary(symbols):
    """the k-th symbol has the code 1^k 0: the shortest codes a table can have, and — at its far end — the ones richest in 1-bits"""
    bits = [0] * 16
    for k in range(len(symbols)):
        bits[k] = 1
    return _checked((bits, list(symbols)))


def ones_dc():
    """unary with the categories the `ff-dense` streams use at the far end: category 10 is 1^11 0, category 0 is 1^10 0"""
    return unary([1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 0, 10])


def ones_ac():
    """sixteen symbols, unary: run 0 / size 10 is 1^15 0 (followed by ten 1-bits for +1023), size 9 is 1^14 0, the end-of-block code 1^13 0"""
    return unary([0xF0, 0x11, 0x21, 0x31, 0x02, 0x12, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x01, 0x00, 0x09, 0x0A])


ANNEX_K = {"dc": [B._DC_L, B._DC_C], "ac": [B._AC_L, B._AC_C]}


# ---- (a) the token-level writer -----------------------------------------------------------------------------------------------------
def _size(v):
    a = np.abs(np.asarray(v, np.int64))
    s = np.zeros(a.shape, np.int64)
    nz = a > 0
    s[nz] = np.floor(np.log2(a[nz])).astype(np.int64) + 1
    return s


def _extra(v, s):
    v = np.asarray(v, np.int64)
    return np.where(v >= 0, v, v + (np.int64(1) << s) - 1)


def tokens_from_blocks(zz):
    """zz: (n, 64) blocks in STREAM order, zig-zag order inside, column 0 the DC DIFFERENCE (not the value: the writer keeps no
    predictor), AC values of up to 15 bits.  -> (m, 4) tokens (class, symbol, extra value, extra bits) as T.81 F.1.2 orders them."""
    zz = np.asarray(zz, np.int64)
    n = zz.shape[0]
    blk = np.arange(n, dtype=np.int64)
    KEY = 65 * 4
    s = _size(zz[:, 0])
    assert int(s.max(initial=0)) <= 11
    rows = [(blk * KEY + 3, np.full(n, DC), s, _extra(zz[:, 0], s), s)]
    bi, pi = np.nonzero(zz[:, 1:])
    pos = pi + 1
    first = np.concatenate(([True], bi[1:] != bi[:-1])) if bi.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate(([0], pos[:-1]))) if bi.size else pos
    run = pos - prev - 1
    v = zz[bi, pos]
    s = _size(v)
    assert int(s.max(initial=0)) <= 15
    rows.append((bi * KEY + pos * 4 + 3, np.full(bi.size, AC), ((run & 15) << 4) | s, _extra(v, s), s))
    for j in range(3):  # ZRL in front of a coefficient whose run reaches 16 / 32 / 48
        mz = run >= 16 * (j + 1)
        z = np.zeros(int(mz.sum()), np.int64)
        rows.append((bi[mz] * KEY + pos[mz] * 4 + j, z + AC, z + 0xF0, z, z))
    last = np.zeros(n, np.int64)
    np.maximum.at(last, bi, pos)
    m = last < 63
    z = np.zeros(int(m.sum()), np.int64)
    rows.append((blk[m] * KEY + 64 * 4, z + AC, z, z, z))
    key = np.concatenate([r[0] for r in rows])
    tok = np.stack([np.concatenate([r[k] for r in rows]) for k in range(1, 5)], axis=1)
    return tok[np.argsort(key, kind="stable")]


def geometry(width, height, sampling):
    """-> (MCUs per row, MCU rows, component of every block of an MCU)"""
    if len(sampling) == 1:
        return -(-width // 8), -(-height // 8), [0]
    hmax, vmax = max(h for h, _v in sampling), max(v for _h, v in sampling)
    return -(-width // (8 * hmax)), -(-height // (8 * vmax)), [c for c, (h, v) in enumerate(sampling) for _ in range(h * v)]


def write_sequential(width, height, sampling, tables, selectors, qts, segments, restart_interval=0):
    """A sequential frame from tokens.  sampling: (h, v) per component (1 or 3 of them); tables: {"dc": [(BITS, HUFFVAL), ...], "ac":
    [...]} with one or two entries each; selectors: (dc id, ac id) per component; qts: per component 64 values <= 255 in natural order;
    segments: one (m, 4) token array per restart segment (one segment without a restart interval).  A block begins at every DC token;
    its position inside the MCU selects the component and with it the tables.  Nothing is checked: tokens that make no valid scan
    (the `to-the-host` streams) are written as they are.  -> JFIF bytes"""
    ncomp = len(sampling)
    assert ncomp in (1, 3) and len(selectors) == ncomp and len(qts) == ncomp
    _cols, _rows, q_comp = geometry(width, height, sampling)
    q_comp = np.array(q_comp)
    sel = np.array(selectors, np.int64)  # [component, class]
    coded = {(cls, t): _code_table(spec) for cls, key in ((DC, "dc"), (AC, "ac")) for t, spec in enumerate(tables[key])}
    parts = []
    for k, tok in enumerate(segments):
        tok = np.asarray(tok, np.int64).reshape(-1, 4)
        cls = tok[:, 0]
        comp = q_comp[np.maximum(np.cumsum(cls == DC) - 1, 0) % len(q_comp)]
        code = np.zeros(len(tok), np.int64)
        length = np.zeros(len(tok), np.int64)
        for (c_, t), (cd, ln) in coded.items():
            m = (cls == c_) & (sel[comp, np.minimum(cls, 1)] == t)
            code[m], length[m] = cd[tok[m, 1]], ln[tok[m, 1]]
            assert (length[m] > 0).all(), ("a symbol without a code", c_, t, sorted({hex(int(x)) for x in tok[m, 1][ln[tok[m, 1]] == 0]}))
        parts.append(_pack_bits((code << tok[:, 3]) | tok[:, 2], length + tok[:, 3]))
        if restart_interval and k + 1 < len(segments):
            parts.append(bytes([0xFF, 0xD0 + (k & 7)]))
    qts = [np.asarray(q, np.int64).reshape(64) for q in qts]
    assert all(int(q.max()) <= 255 and int(q.min()) >= 1 for q in qts)
    tq = [0 if np.array_equal(q, qts[0]) else 1 for q in qts]
    out = [b"\xff\xd8", _marker(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")]
    for t in sorted(set(tq)):
        out.append(_marker(0xDB, bytes([t]) + bytes(int(x) for x in qts[tq.index(t)][UNZIGZAG])))
    out.append(_marker(0xC0, bytes([8]) + int(height).to_bytes(2, "big") + int(width).to_bytes(2, "big") + bytes([ncomp]) +
                       b"".join(bytes([c + 1, (sampling[c][0] << 4) | sampling[c][1], tq[c]]) for c in range(ncomp))))
    for cls, key in ((0, "dc"), (1, "ac")):
        for t, spec in enumerate(tables[key]):
            out.append(_marker(0xC4, bytes([(cls << 4) | t]) + bytes(spec[0]) + bytes(spec[1])))
    if restart_interval:
        out.append(_marker(0xDD, int(restart_interval).to_bytes(2, "big")))
    out.append(_marker(0xDA, bytes([ncomp]) + b"".join(bytes([c + 1, (int(sel[c, 0]) << 4) | int(sel[c, 1])]) for c in range(ncomp)) + b"\0\x3f\0"))
    out += parts
    out.append(b"\xff\xd9")
    return b"".join(out)


def _frame(width, height, sampling, tables, selectors, q, zz, restart_interval=0):
    """zz: every block of the scan in stream order (see tokens_from_blocks), cut into restart segments here"""
    cols, rows, q_comp = geometry(width, height, sampling)
    assert zz.shape == (cols * rows * len(q_comp), 64), (zz.shape, cols, rows)
    per = (restart_interval or cols * rows) * len(q_comp)
    segments = [tokens_from_blocks(zz[a:a + per]) for a in range(0, zz.shape[0], per)]
    return write_sequential(width, height, sampling, tables, selectors, [np.full(64, q)] * len(sampling), segments, restart_interval)


def scan_density(data):
    """(0xFF bytes, bytes) of the entropy-coded data of a one-scan stream"""
    sos = data.rfind(b"\xff\xda")
    scan = data[sos + 2 + ((data[sos + 2] << 8) | data[sos + 3]):-2]
    return scan.count(b"\xff"), len(scan)


TWO = [(0, 0), (1, 1), (1, 1)]  # luma on tables 0, chroma on tables 1
ONE = [(0, 0), (0, 0), (0, 0)]  # `uniform`: every component on tables 0


def _sel(sampling, uniform=False):
    return [(0, 0)] if len(sampling) == 1 else (ONE if uniform else TWO)


# ---- (c) the sequential cases -------------------------------------------------------------------------------------------------------
def _dc_wrap_blocks(rng, n, q_comp):
    """DC differences of +-2047: every component's predictor climbs through +32767 (a wrap every 16 blocks), falls through -32768
    twice as long, then wanders; +-1023 at zig-zag positions 1 and 63 of some blocks"""
    zz = np.zeros((n, 64), np.int64)
    comp = np.tile(q_comp, n // len(q_comp))
    for c in set(q_comp):
        idx = np.flatnonzero(comp == c)
        m = idx.size
        d = np.full(m, 2047)
        d[m // 4:3 * m // 4] = -2047
        d[3 * m // 4:] = rng.choice([-2047, 2047, -2046, 1024, -1, 0], m - 3 * m // 4)
        zz[idx, 0] = d
    some = rng.random(n) < 0.3
    zz[some, 1] = rng.choice([-1023, 1023], int(some.sum()))
    some = rng.random(n) < 0.3
    zz[some, 63] = rng.choice([-1023, 1023], int(some.sum()))
    return zz


def dc_wrap(sampling, q, restart_interval=0, seed=1):
    w, h = 256, 192
    cols, rows, q_comp = geometry(w, h, sampling)
    zz = _dc_wrap_blocks(np.random.default_rng(seed), cols * rows * len(q_comp), q_comp)
    return _frame(w, h, sampling, ANNEX_K if len(sampling) == 3 else {"dc": [B._DC_L], "ac": [B._AC_L]}, _sel(sampling), q, zz, restart_interval)


def _sparse_blocks(rng, n, max_size, dc=60):
    """a few coefficients per block at random zig-zag positions — runs 0..15 and beyond (ZRL x 1..3) — of sizes 1..max_size, both signs,
    the extremes +-(2^s - 1) and +-2^(s-1) of every size among them; every eighth block has a coefficient at index 63 (no end-of-block
    code), every ninth is empty"""
    zz = np.zeros((n, 64), np.int64)
    ext = [sg * v for s in range(1, max_size + 1) for v in ((1 << s) - 1, 1 << (s - 1)) for sg in (1, -1)]
    for b in range(n):
        if b % 9 == 4:
            continue
        pos = np.sort(rng.choice(np.arange(1, 64), int(rng.integers(1, 7)), replace=False))
        if b % 8 == 1:
            pos = np.unique(np.append(pos, 63))
        if b % 16 == 3:
            pos = np.array([int(rng.integers(49, 64))])  # one coefficient behind three ZRLs
        s = rng.integers(1, max_size + 1, pos.size)
        lo = np.int64(1) << (s - 1)
        zz[b, pos] = (lo + (rng.integers(0, 1 << 30, pos.size) % lo)) * rng.choice([-1, 1], pos.size)
    flat = np.flatnonzero(zz[:, 1:].reshape(-1))
    put = rng.choice(flat, len(ext), replace=False)  # (the extremes of every size, at places that hold a coefficient anyway)
    zz[put // 63, put % 63 + 1] = ext
    zz[:, 0] = rng.integers(-dc, dc + 1, n)
    return zz


def ac_size_15(sampling, q, seed=2):
    w, h = 256, 192
    cols, rows, q_comp = geometry(w, h, sampling)
    zz = _sparse_blocks(np.random.default_rng(seed), cols * rows * len(q_comp), 15)
    tabs = {"dc": [long16_dc(), B._DC_C][:2 if len(sampling) == 3 else 1], "ac": [long16_ac(AC_SYMBOLS_15), wide_ac(AC_SYMBOLS_15)][:2 if len(sampling) == 3 else 1]}
    return _frame(w, h, sampling, tabs, _sel(sampling), q, zz)


def long_codes(sampling, which, restart_interval=0, seed=3, dc_wrap_too=False, size=(256, 192)):
    """`long16` / `wide` tables (4:2:0: luma on one pair, chroma on the other) under sparse blocks of sizes 1..10"""
    w, h = size
    cols, rows, q_comp = geometry(w, h, sampling)
    rng = np.random.default_rng(seed)
    n = cols * rows * len(q_comp)
    zz = _sparse_blocks(rng, n, 10)
    if dc_wrap_too:
        zz[:, 0] = _dc_wrap_blocks(rng, n, q_comp)[:, 0]
    pair = {"long16": (long16_dc(), long16_ac()), "wide": (wide_dc(), wide_ac())}
    other = "wide" if which == "long16" else "long16"
    tabs = {"dc": [pair[which][0], pair[other][0]], "ac": [pair[which][1], pair[other][1]]}
    if len(sampling) == 1:
        tabs = {k: v[:1] for k, v in tabs.items()}
    return _frame(w, h, sampling, tabs, _sel(sampling), 1, zz, restart_interval)


def giant_blocks(share, size=(256, 192), seed=4, cut=False):
    """blocks of 63 coefficients of +-1023 (size 10 under 16-bit codes: about 1,900 bits, more than a chunk of the smallest size) among
    blocks of two symbols; gray.  cut: the stream ends in the middle of a giant block."""
    w, h = size
    cols, rows, q_comp = geometry(w, h, GRAY)
    n = cols * rows
    rng = np.random.default_rng(seed)
    zz = np.zeros((n, 64), np.int64)
    giant = rng.random(n) < share
    giant[n // 2] = True
    zz[giant, 1:] = rng.choice([-1023, 1023, -512, 512, 1000, -777], (int(giant.sum()), 63))
    zz[:, 0] = rng.integers(-30, 31, n)
    tabs = {"dc": [long16_dc()], "ac": [long16_ac()]}
    _code, length = _code_table(tabs["ac"][0])
    assert int(length[0x0A]) == 16  # (what makes the block giant)
    data = whole = _frame(w, h, GRAY, tabs, [(0, 0)], 1, zz)
    if cut:
        first = int(np.flatnonzero(giant)[len(np.flatnonzero(giant)) // 2])
        upto = write_sequential(w, h, GRAY, tabs, [(0, 0)], [np.ones(64)], [tokens_from_blocks(zz[:first + 1])[:-20]])  # 20 symbols short of its end
        keep = len(upto) - 2 - 1  # without the end-of-image marker and the padded last byte
        assert whole[:keep] == upto[:keep]
        data = whole[:keep] + b"\xff\xd9"
    return data


def ff_dense(sampling, restart_interval=0, seed=5):
    """the `ones` tables under blocks of a few +1023 / +511 at run 0 and DC differences of +-1023: runs of 25 one-bits, one after the other"""
    w, h = 128, 96
    cols, rows, q_comp = geometry(w, h, sampling)
    n = cols * rows * len(q_comp)
    rng = np.random.default_rng(seed)
    zz = np.zeros((n, 64), np.int64)
    for b in range(n):
        m = int(rng.integers(0, 12))
        zz[b, 1:1 + m] = rng.choice([1023, 1023, 1023, 511, -1023, 1], m)
    zz[:, 0] = np.where(np.arange(n) % (2 * len(q_comp)) < len(q_comp), 1023, -1023)  # (per component: up, down, up ...)
    zz[rng.random(n) < 0.1, 0] = 0
    tabs = {"dc": [ones_dc(), ones_dc()][:len(sampling) // 2 + 1], "ac": [ones_ac(), ones_ac()][:len(sampling) // 2 + 1]}
    data = _frame(w, h, sampling, tabs, _sel(sampling), 1, zz, restart_interval)
    ff, total = scan_density(data)
    assert 3 * ff >= total, (ff, total)  # at least a third of the scan's bytes
    return data


def uniform_420(restart_interval=0, seed=6):
    """three components, 4:2:0, all on table 0 of both classes: the chunk decoder's `uniform` scan (it cannot tell the blocks of an MCU
    apart; DC values are summed per plane afterwards) — with DC differences that wrap and long codes"""
    w, h = 256, 192
    cols, rows, q_comp = geometry(w, h, S420)
    rng = np.random.default_rng(seed)
    n = cols * rows * 6
    zz = _sparse_blocks(rng, n, 10)
    zz[:, 0] = _dc_wrap_blocks(rng, n, q_comp)[:, 0]
    return _frame(w, h, S420, {"dc": [long16_dc()], "ac": [long16_ac()]}, ONE, 1, zz, restart_interval)


def _one_bad_block(tokens):
    """a small gray frame of sparse blocks whose block 40 is `tokens`"""
    w, h = 128, 64
    zz = _sparse_blocks(np.random.default_rng(7), 128, 10)
    tok = np.concatenate([tokens_from_blocks(zz[:40]), np.array(tokens, np.int64).reshape(-1, 4), tokens_from_blocks(zz[41:])])
    dc = ([0, 0, 0, 0] + [1] * 12, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12])  # (a code for category 12 where category 11's was)
    return write_sequential(w, h, GRAY, {"dc": [dc], "ac": [long16_ac(AC_SYMBOLS_10[:1] + [0x30] + AC_SYMBOLS_10[1:])]}, [(0, 0)], [np.ones(64)], [tok])


def to_the_host(kind):
    if kind == "dc-category-12":
        return _one_bad_block([(DC, 12, 0xABC, 12), (AC, 0x00, 0, 0)])
    if kind == "eob-run-in-a-sequential-scan":
        return _one_bad_block([(DC, 3, 5, 3), (AC, 0x11, 1, 1), (AC, 0x30, 5, 3), (AC, 0x00, 0, 0)])  # EOB3 and its run length
    if kind == "run-past-index-63":
        return _one_bad_block([(DC, 3, 5, 3), (AC, 0xF0, 0, 0), (AC, 0xF0, 0, 0), (AC, 0xF0, 0, 0), (AC, 0xF2, 3, 2), (AC, 0x21, 1, 1), (AC, 0x00, 0, 0)])
    if kind == "sixteen-one-bits":
        return _one_bad_block([(DC, 3, 5, 3), (AC, 0x11, 1, 1), (RAW, 0, 0xFFFF, 16), (AC, 0x00, 0, 0)])
    if kind == "cut-inside-a-giant-block":
        return giant_blocks(0.03, cut=True)
    raise KeyError(kind)


# ---- (d) the progressive cases ------------------------------------------------------------------------------------------------------
def _components(w, h, sampling):
    import jpeg_decoder_amd as J
    comps, _mcu = J.make_components(w, h, sampling)
    return list(comps)


# four steps of successive approximation (Al 3 -> 0) on a band cut in two, every part refined on its own: a dense block carries one
# correction bit per coefficient and scan
SPLIT_AL3_GRAY = [((0,), 0, 0, 0, 3), ((0,), 1, 5, 0, 3), ((0,), 6, 63, 0, 3), ((0,), 0, 0, 3, 2), ((0,), 1, 5, 3, 2), ((0,), 6, 63, 3, 2), ((0,), 6, 63, 2, 1),
                  ((0,), 0, 0, 2, 1), ((0,), 1, 5, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 5, 1, 0), ((0,), 6, 63, 1, 0)]
SPLIT_AL3_YCC = [((0, 1, 2), 0, 0, 0, 3), ((0,), 1, 5, 0, 3), ((0,), 6, 63, 0, 3), ((1,), 1, 63, 0, 2), ((2,), 1, 20, 0, 3), ((0,), 1, 5, 3, 2), ((0, 1, 2), 0, 0, 3, 2),
                 ((0,), 6, 63, 3, 2), ((2,), 21, 63, 0, 1), ((0,), 6, 63, 2, 1), ((1,), 1, 63, 2, 1), ((0,), 1, 5, 2, 1), ((2,), 1, 20, 3, 2), ((0, 1, 2), 0, 0, 2, 1),
                 ((2,), 1, 20, 2, 1), ((0,), 1, 5, 1, 0), ((0,), 6, 63, 1, 0), ((1,), 1, 63, 1, 0), ((2,), 21, 63, 1, 0), ((2,), 1, 20, 1, 0), ((0, 1, 2), 0, 0, 1, 0)]


def prog_dense_extreme(sampling, script, seed=8, size=(96, 64)):
    """every block with 63 coefficients in +-1023 and a DC value in +-1024; script: a list of scans, or "random": one of random_script"""
    w, h = size
    rng = np.random.default_rng(seed)
    comps = _components(w, h, sampling)
    if script == "random":
        script = P.random_script(np.random.default_rng(seed + 100), len(sampling))
    coefs = []
    for c in comps:
        a = rng.integers(-1023, 1024, (int(c.block_width) * int(c.block_height), 64))
        a[a == 0] = 1023
        a[::3] = rng.choice([-1023, 1023, -1022, 1], a[::3].shape)
        a[:, 0] = rng.integers(-1024, 1025, a.shape[0])
        coefs.append(a.astype(np.int16).reshape(-1))
    return P.encode_from_coefficients(comps, [np.ones(64, np.int64)] * len(comps), coefs, w, h, script)


def prog_eobrun_cap():
    """2048 x 1040 gray: 33,280 blocks with five non-zero AC coefficients between them — the first and the refinement scan each hold an
    end-of-band run of 32,767 blocks (the cap: EOB14 with fourteen 1-bits) and the runs on either side of it"""
    w, h = 2048, 1040
    comps = _components(w, h, GRAY)
    n = int(comps[0].block_width) * int(comps[0].block_height)
    assert n >= 32768 + 512
    a = np.zeros((n, 64), np.int16)
    a[:, 0] = (np.arange(n) % 256) - 128
    for blk, nat, v in ((3, 1, 2), (3, 8, -1), (200, 63, 3), (200 + 32767 + 40, 9, -2), (n - 2, 2, 1)):
        a[blk, nat] = v
    script = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)]
    return P.encode_from_coefficients(comps, [np.ones(64, np.int64)], [a.reshape(-1)], w, h, script)


def _dc_walk(rng, m):
    """m values in -4096 .. 4095 that go from end to end and back in steps of at most 2047, both ends reached"""
    out, cur, direction = [], 0, 1
    for _ in range(m):
        cur += direction * int(rng.integers(1000, 2048))
        if cur >= 4095:
            cur, direction = 4095, -1
        elif cur <= -4096:
            cur, direction = -4096, 1
        out.append(cur)
    return np.array(out, np.int64)


def prog_dc_extreme(sampling, seed=9):
    """DC values over the whole 16-bit range, -32768 and +32767 among them: written with Al = 3 their differences stay within category 11
    (a triangle wave of steps below 2047 << 3), the refinement scans add the low bits"""
    w, h = 128, 96
    rng = np.random.default_rng(seed)
    comps = _components(w, h, sampling)
    coefs = []
    for c in comps:
        n = int(c.block_width) * int(c.block_height)
        a = np.zeros((n, 64), np.int64)
        a[:, 1:4] = rng.integers(-3, 4, (n, 3))
        a[:, 0] = rng.integers(-32768, 32768, n)
        coefs.append(a)
    # the first scan codes differences in the order it walks the blocks, one predictor per component: plane order for chroma and gray;
    # luma's order in the interleaved scan differs — its walk goes from MCU to MCU, the four blocks of an MCU differ in the low bits only
    for ci, c in enumerate(comps):
        bw, bh = int(c.block_width), int(c.block_height)
        if len(sampling) == 3 and ci == 0:
            t = np.repeat(np.repeat(_dc_walk(rng, (bh // 2) * (bw // 2)).reshape(bh // 2, bw // 2), 2, axis=0), 2, axis=1).reshape(-1)
        else:
            t = _dc_walk(rng, bw * bh)
        low = rng.integers(0, 8, t.size)
        low[t == 4095], low[t == -4096] = 7, 0
        coefs[ci][:, 0] = t * 8 + low
        assert coefs[ci][:, 0].max() == 32767 and coefs[ci][:, 0].min() == -32768
    script = [(tuple(range(len(comps))), 0, 0, 0, 3)] + [((c,), 1, 63, 0, 0) for c in range(len(comps))] + [(tuple(range(len(comps))), 0, 0, al + 1, al) for al in (2, 1, 0)]
    return P.encode_from_coefficients(comps, [np.ones(64, np.int64)] * len(comps), [a.astype(np.int16).reshape(-1) for a in coefs], w, h, script)


# ---- the list -------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


class Case(SimpleNamespace):
    """name; kind "sequential" | "progressive"; sampling; make() -> bytes (cached by `data`); uniform: every component on one pair of
    tables.  Three flags, each asserted by tests/test_entropy_cases_emulation.py against the emulated device and set by nothing else:
    stays_on_device — status 0 under every emission parameter in the emulation's own chunking (sequential) / the host's planes on every
    walk (progressive); settles_in_a_small_call — status 0 in the chunking the library gives a small call (SMALL_CALL_CHUNKING);
    in_sane_class — every product |coefficient| x quantization value stays below 2^15 (with a table of ones only -32768 leaves it): the
    entry-list walk's `sane` arithmetic; beyond it the walk flags the image, status bit 9, and the host decodes it with the wrap-exact
    kernels."""

    @property
    def data(self):
        if self.name not in _CACHE:
            _CACHE[self.name] = self.make()
        return _CACHE[self.name]

    @property
    def is_420(self):
        return self.sampling == S420

    @property
    def entry_walk(self):
        """4:2:0 with tables of their own for luma and chroma: the pixel walk reads the entry lists itself (csrc/fused_entries.hpp)"""
        return self.kind == "sequential" and self.is_420 and not self.uniform


# csrc/batch_entropy.cpp for a call of fewer than 16,384 lanes: chunks of 12 blocks' worth of bits and at least 512, 16 launches of two
# passes; the first pass over whole chunks when the call is one or two sub-batches (tests/emu: emu_huff_set_chunking / _launch / _tail)
SMALL_CALL_CHUNKING = {"blocks": 12, "min_shift": 9, "launches": 16, "iters": 2, "tail": 8}


def _case(name, make, sampling, stays=True, kind="sequential", uniform=False, in_sane_class=True, small=True):
    return Case(name=name, make=make, sampling=sampling, stays_on_device=stays, kind=kind, uniform=uniform, in_sane_class=in_sane_class,
                settles_in_a_small_call=stays and small)


SEQUENTIAL = [
    _case("dc-wrap-gray-q1", lambda: dc_wrap(GRAY, 1), GRAY),
    _case("dc-wrap-gray-q255", lambda: dc_wrap(GRAY, 255), GRAY, in_sane_class=False),
    _case("dc-wrap-420-q1", lambda: dc_wrap(S420, 1), S420, small=False),
    _case("dc-wrap-420-q255", lambda: dc_wrap(S420, 255), S420, in_sane_class=False, small=False),
    _case("ac-size-15-gray-q1", lambda: ac_size_15(GRAY, 1), GRAY, small=False),
    _case("ac-size-15-gray-q255", lambda: ac_size_15(GRAY, 255), GRAY, in_sane_class=False, small=False),
    _case("ac-size-15-420-q1", lambda: ac_size_15(S420, 1), S420, small=False),
    _case("ac-size-15-420-q255", lambda: ac_size_15(S420, 255, seed=22), S420, in_sane_class=False, small=False),
    _case("long16-gray", lambda: long_codes(GRAY, "long16"), GRAY, small=False),
    _case("wide-gray", lambda: long_codes(GRAY, "wide"), GRAY, small=False),
    _case("long16-wide-420", lambda: long_codes(S420, "long16"), S420, small=False),
    _case("wide-long16-444", lambda: long_codes(S444, "wide", size=(128, 96)), S444, small=False),
    _case("giant-blocks-3-percent", lambda: giant_blocks(0.03), GRAY, small=False),
    _case("giant-blocks-all", lambda: giant_blocks(1.0, size=(64, 48)), GRAY),
    _case("ff-dense-gray", lambda: ff_dense(GRAY), GRAY),
    _case("ff-dense-420", lambda: ff_dense(S420), S420),
    _case("uniform-420", lambda: uniform_420(), S420, uniform=True, small=False),
    _case("uniform-420-ri7", lambda: uniform_420(7), S420, uniform=True),
    _case("dc-wrap-gray-ri1", lambda: dc_wrap(GRAY, 255, 1), GRAY, in_sane_class=False),
    _case("dc-wrap-420-ri5", lambda: dc_wrap(S420, 1, 5), S420),
    _case("long16-gray-ri1", lambda: long_codes(GRAY, "long16", 1, size=(128, 96)), GRAY),
    _case("long16-wide-420-ri5", lambda: long_codes(S420, "long16", 5), S420),
    _case("ff-dense-gray-ri7", lambda: ff_dense(GRAY, 7), GRAY),
    _case("ff-dense-420-ri1", lambda: ff_dense(S420, 1), S420),
]
TO_THE_HOST = [_case("to-the-host-" + k, (lambda k=k: to_the_host(k)), GRAY, stays=False)
               for k in ("dc-category-12", "eob-run-in-a-sequential-scan", "run-past-index-63", "sixteen-one-bits", "cut-inside-a-giant-block")]
PROGRESSIVE = [
    _case("prog-dense-extreme-gray-split", lambda: prog_dense_extreme(GRAY, SPLIT_AL3_GRAY), GRAY, kind="progressive"),
    _case("prog-dense-extreme-gray-random", lambda: prog_dense_extreme(GRAY, "random", seed=12), GRAY, kind="progressive"),
    _case("prog-dense-extreme-420-split", lambda: prog_dense_extreme(S420, SPLIT_AL3_YCC), S420, kind="progressive"),
    _case("prog-dense-extreme-420-random", lambda: prog_dense_extreme(S420, "random", seed=13), S420, kind="progressive"),
    _case("prog-dc-extreme-gray", lambda: prog_dc_extreme(GRAY), GRAY, kind="progressive", in_sane_class=False),
    _case("prog-dc-extreme-420", lambda: prog_dc_extreme(S420), S420, kind="progressive", in_sane_class=False),
    _case("prog-eobrun-cap", prog_eobrun_cap, GRAY, kind="progressive"),
]
ALL_SEQUENTIAL = SEQUENTIAL + TO_THE_HOST


def decoder_stream():
    """1280 x 720 gray, above the Decoder's threshold for the device route: `long16` tables and DC differences that wrap in every
    restart segment.  Restart interval 80: a scan on these tables settles one chunk per pass, and a one-image call
    gets 32 passes — the 14,400 blocks as ONE segment are over a thousand chunks and come back unsettled; 80 blocks are about eight."""
    return long_codes(GRAY, "long16", 80, seed=21, dc_wrap_too=True, size=(1280, 720))


DECODER = [_case("decoder-long16-dc-wrap-720p-ri80", decoder_stream, GRAY)]
