"""State carried from one call to the next: a Pipeline keeps its sub-batches (arenas, class tables, entry-list flags) while the
geometry repeats, a Batch keeps per-component classes, pending compact uploads and device statistics until something replaces
them.  Every test here sends NEW pictures in every slot of every call and asserts that the expected pixels did change, so a call
whose kernels skipped an image (and left the previous call's pixels in the arena) cannot pass."""
import collections
import io

import numpy as np
import pytest

import oracle as O
import stream_harness  # (at collection time: it imports torch before any test loads libjpgpu.so)
import synth

pytestmark = pytest.mark.gpu
J = None
N = 64  # kSubBatchImages: one device sub-batch per call

KNOBS = ("JPGPU_PIPE_ENTRY_PIXELS", "JPGPU_PIPE_PROG_DEVICE_PERCENT", "JPGPU_PROG_LANES_MAX", "JPGPU_PIPE_HOST_LIGHT")


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    assert J.device_count() >= 1


# ---- files and their oracle decodes, cached per file -------------------------------------------------------------------------------
_FILES, _WANT = {}, {}


def _file(geom, enc, pic):
    """Picture `pic` of geometry (w, h, subsampling or "gray") as a PIL-written JPEG: enc "base", "restart" (a marker per MCU row)
    or "prog"; always quality 85, so every file of a geometry carries the same tables."""
    key = (geom, enc, pic)
    if key not in _FILES:
        from PIL import Image
        w, h, sub = geom
        rgb = synth.synthetic_rgb(w, h, seed=1000 + pic)
        kw = {"quality": 85}
        if sub == "gray":
            im = Image.fromarray(rgb[..., 0])
        else:
            im = Image.fromarray(rgb)
            kw["subsampling"] = sub
        if enc == "prog":
            kw["progressive"] = True
        elif enc == "restart":
            kw["restart_marker_rows"] = 1
        buf = io.BytesIO()
        im.save(buf, format="JPEG", **kw)
        _FILES[key] = buf.getvalue()
        _WANT[key] = O.decode(_FILES[key]).pixels
    return _FILES[key], _WANT[key]


def _euler_circuit(k):
    """Hierholzer's algorithm on the complete directed graph with self-loops on k nodes: a closed walk of k*k + 1 nodes in which
    every ordered pair (a, b) follows each other exactly once."""
    unused = {a: list(range(k)) for a in range(k)}
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    pairs = collections.Counter(zip(walk, walk[1:]))
    assert len(walk) == k * k + 1 and len(pairs) == k * k and set(pairs.values()) == {1}
    return walk


# ---- call kinds: (encoding, decode() arguments, knobs, route check(timings, n)) ----------------------------------------------------------
def _entry(t, n):
    return t["images_device_entropy"] == n and t["images_entry_pixels"] == n and t["images_device_progressive"] == 0


def _expand(t, n):
    return t["images_device_entropy"] == n and t["images_entry_pixels"] == 0 and t["images_device_progressive"] == 0


def _prog(t, n):
    return t["images_device_progressive"] == n and t["images_entry_pixels"] == 0


def _host(t, n):
    return t["images_device_entropy"] == 0 and t["images_device_progressive"] == 0 and t["images_entry_pixels"] == 0


KINDS = {
    "base-entry": ("base", {}, {}, _entry),
    "base-expand": ("base", {}, {"JPGPU_PIPE_ENTRY_PIXELS": "0"}, _expand),
    "base-restart": ("restart", {}, {}, _entry),
    "base-staged": ("base", {"host_light": False}, {}, lambda t, n: t["images_device_entropy"] == n and t["images_host_light"] == 0),
    "prog-device": ("prog", {}, {"JPGPU_PIPE_PROG_DEVICE_PERCENT": "100"}, _prog),
    "prog-device-track": ("prog", {}, {"JPGPU_PIPE_PROG_DEVICE_PERCENT": "100", "JPGPU_PROG_LANES_MAX": "0"}, _prog),
    "prog-host": ("prog", {"progressive_on_host": True}, {}, lambda t, n: t["images_device_progressive"] == 0),
    "host": ("base", {"device_entropy": False}, {}, _host),
    "resident": ("base", {"download": False}, {}, _entry),
    # (layouts without the entry-list walk)
    "base-device": ("base", {}, {}, _expand),
}



def _call(p, monkeypatch, kind, files):
    _enc, kwargs, env, _route = KINDS[kind]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = p.decode(files, **kwargs)
    if kwargs.get("download", True) is False:  # (byte counts: the pixels stay in HBM until asked for)
        assert all(isinstance(o, int) for o in out), out
        out = [p.download(i) for i in range(len(files))]
    return out, p.timings()


class _Sequence:
    """Calls on one pipeline.  Slot k of call c holds picture (k + n/2 * (c % 2)) mod n of the pool, so no slot sees the same picture
    in two consecutive calls, and that the expected pixels differ is asserted.  Pixel mismatches are collected per transition (the
    report names every transition that went wrong); a wrong route stops the test at once."""

    def __init__(self, p, monkeypatch, geom, n):
        self.p, self.mp, self.geom, self.n = p, monkeypatch, geom, n
        self.prev_want, self.prev_label, self.calls, self.bad = None, None, 0, []

    def run(self, kind, encs=None, route=None, label=None):
        label = label or kind
        encs = encs or [KINDS[kind][0]] * self.n
        assert len(encs) == self.n
        par = self.calls % 2
        self.calls += 1
        files, want = [], []
        for k, enc in enumerate(encs):
            f, w = _file(self.geom, enc, (k + self.n // 2 * par) % self.n)
            files.append(f)
            want.append(w)
        if self.prev_want is not None:  # the precondition that makes a stale result visible
            same = [k for k in range(self.n) if np.array_equal(want[k], self.prev_want[k])]
            assert not same, f"fixture: slots {same} expect the same pixels in two consecutive calls"
        out, t = _call(self.p, self.mp, kind, files)
        assert t["images_ok"] == self.n and t["images_device_rejected"] == 0, (label, t)
        assert (route or (lambda t_: KINDS[kind][3](t_, self.n)))(t), (f"call {self.calls - 1} ({label}) took another route",
                                                                       {k: v for k, v in t.items() if k.startswith("images_")})
        bad = [k for k in range(self.n) if isinstance(out[k], Exception) or not np.array_equal(out[k], want[k])]
        if bad:
            stale = sum(1 for k in bad if self.prev_want is not None and not isinstance(out[k], Exception) and np.array_equal(out[k], self.prev_want[k]))
            self.bad.append(f"call {self.calls - 1}, {self.prev_label} -> {label}: {len(bad)} of {self.n} images differ from the oracle "
                            f"(slots {bad[0]}..{bad[-1]}), {stale} of them hold the previous call's pixels")
        self.prev_want, self.prev_label = want, label
        return t

    def check(self):
        assert not self.bad, "\n" + "\n".join(self.bad)


# ---- A. every ordered pair of call kinds on one 4:2:0 geometry with partial edge MCUs ------------------------------------------------
MATRIX = ["base-entry", "base-expand", "base-restart", "base-staged", "prog-device", "prog-device-track", "prog-host", "host", "resident"]


def test_transition_matrix_420(monkeypatch):
    """a sub-batch whose last call took the entry-list walk kept its images flagged as entry images; a progressive
    call of the same geometry reused it, the dense kernels skipped every image and the call returned the previous pixels."""
    pytest.importorskip("PIL")
    order = [MATRIX[v] for v in _euler_circuit(len(MATRIX))]
    p = J.Pipeline(threads=4)
    try:
        seq = _Sequence(p, monkeypatch, (333, 200, "4:2:0"), N)
        for kind in order:
            seq.run(kind)
        seq.check()
    finally:
        p.close()


# ---- B. a sub-batch other than the first, other layouts, two child pipelines ---------------------------------------------------------
def test_second_sub_batch_changes_kind_every_call(monkeypatch):
    """[64 baseline + 64 progressive] and [128 baseline] in turn: sub-batch 1 holds entry-list images in one call and progressive
    frames in the next, with the same geometry (reused) every time."""
    pytest.importorskip("PIL")
    p = J.Pipeline(threads=4)
    try:
        seq = _Sequence(p, monkeypatch, (333, 200, "4:2:0"), 2 * N)
        for c in range(6):
            if c % 2 == 0:
                seq.run("prog-device", ["base"] * N + ["prog"] * N, label="64 baseline + 64 progressive",
                        route=lambda t: t["images_entry_pixels"] == N and t["images_device_progressive"] == N)
            else:
                seq.run("prog-device", ["base"] * 2 * N, label="128 baseline",
                        route=lambda t: t["images_entry_pixels"] == 2 * N and t["images_device_progressive"] == 0)
        seq.check()
    finally:
        p.close()


@pytest.mark.parametrize("geom", [(250, 130, "4:4:4"), (300, 200, "gray")], ids=["444", "gray"])
def test_transition_matrix_other_layouts(monkeypatch, geom):
    """No entry-list walk here, but the class tables and statistics of the reused sub-batch cross from call to call."""
    pytest.importorskip("PIL")
    kinds = ["base-device", "prog-device", "host"]
    p = J.Pipeline(threads=4)
    try:
        seq = _Sequence(p, monkeypatch, geom, N)
        for v in _euler_circuit(len(kinds)):
            seq.run(kinds[v])
        seq.check()
    finally:
        p.close()


def test_two_child_pipelines_on_one_device(monkeypatch):
    """Pipeline(devices=[0, 0]): each child gets every other image (64 each) and reuses its own sub-batch the same way."""
    pytest.importorskip("PIL")
    p = J.Pipeline(devices=[0, 0], threads=4)
    try:
        seq = _Sequence(p, monkeypatch, (333, 200, "4:2:0"), 2 * N)
        for kind in ["base-entry", "prog-device", "base-entry", "prog-device-track", "base-restart", "prog-device"]:
            seq.run(kind)
        seq.check()
    finally:
        p.close()


# ---- C. seeded random operation sequences on one Batch, checked against a host model --------------------------------------------------
def _to_j(comps):
    out = (J.Component * len(comps))()
    for i, c in enumerate(comps):
        out[i].identifier, out[i].horizontal_sampling_factor, out[i].vertical_sampling_factor = c.identifier, c.h, c.v
        out[i].quantization_table_index, out[i].dct_scale = c.tq, c.dct_scale
        out[i].size_width, out[i].size_height, out[i].block_width, out[i].block_height = c.size_w, c.size_h, c.block_w, c.block_h
    return out


def _content(rng, ocomps, kind):
    """(tables, coefficients) of one image, drawn as test_gpu_parity's _batch_case draws them."""
    if kind == "sparse":
        qts = [rng.integers(1, 200, 64).astype(np.uint16) for _ in ocomps]
        coefs = [synth.sparse_coefficients(rng, c.block_w * c.block_h) for c in ocomps]
    elif kind == "tight":  # column sums of |c*q| at the 5900 limit
        qts = [rng.integers(1, 32, 64).astype(np.uint16) for _ in ocomps]
        coefs = [synth.tight_blocks(rng, c.block_w * c.block_h, q) for c, q in zip(ocomps, qts)]
    elif kind == "sane":  # |c*q| < 2^15, column sums far above the tight limit
        qts = [rng.integers(1, 16, 64).astype(np.uint16) for _ in ocomps]
        coefs = [rng.integers(-2000, 2001, c.block_w * c.block_h * 64).astype(np.int16) for c in ocomps]
    else:  # "full": products that wrap
        qts = [rng.integers(1, 65536, 64).astype(np.uint16) for _ in ocomps]
        coefs = [rng.integers(-32768, 32768, c.block_w * c.block_h * 64).astype(np.int16) for c in ocomps]
    return qts, coefs


def _exact_class(qts, coefs):
    from jpeg_decoder_amd import _native as N_
    cls = 3
    for q, c in zip(qts, coefs):
        a = np.ascontiguousarray(c, np.int16).reshape(-1)
        qq = np.ascontiguousarray(q, np.uint16).reshape(64)
        cls = min(cls, N_.lib().jpgpu_range_class(a.ctypes.data, a.size, qq.ctypes.data))
    return cls


CONTENT = ("tight", "sparse", "sane", "full")
MODES = ("dense", "compact", "compact-unclassified")
L420 = [(2, 2), (1, 1), (1, 1)]
L444 = [(1, 1), (1, 1), (1, 1)]
LAYOUTS = {
    "420": [(64, 48, L420, "YCbCr"), (33, 17, L420, "YCbCr"), (136, 72, L420, "YCbCr"), (64, 48, L420, "YCbCr"), (250, 130, L420, "YCbCr"),
            (17, 40, L420, "YCbCr"), (64, 48, L420, "YCbCr")],
    "444": [(45, 29, L444, "YCbCr"), (64, 48, L444, "YCbCr"), (200, 120, L444, "YCbCr"), (9, 30, L444, "YCbCr"), (64, 48, L444, "YCbCr"),
            (33, 17, L444, "YCbCr")],
    "gray": [(37, 21, [(1, 1)], "Grayscale"), (64, 48, [(1, 1)], "Grayscale"), (100, 9, [(1, 1)], "Grayscale"), (8, 8, [(1, 1)], "Grayscale"),
             (64, 48, [(1, 1)], "Grayscale"), (30, 40, [(1, 1)], "Grayscale")],
    "311-generic": [(70, 40, [(3, 1), (1, 1), (1, 1)], "YCbCr")] * 3 + [(45, 17, [(3, 1), (1, 1), (1, 1)], "YCbCr")] * 3,
    "mixed": [(64, 48, L420, "YCbCr"), (33, 21, L444, "RGB"), (100, 9, [(1, 1)], "Grayscale"), (31, 70, [(2, 1), (1, 1), (1, 1)], "YCbCr"),
              (16, 16, [(1, 1)] * 4, "CMYK"), (70, 40, [(3, 1), (1, 1), (1, 1)], "YCbCr"), (50, 61, [(1, 2), (1, 1), (1, 1)], "YCbCr"),
              (64, 48, L420, "YCbCr")],
}


def _random_ops(layout, seed, n_ops=200):
    """A replayable operation list for _run_ops, drawn against a host model of the batch (range hints never promise more than the
    exact class of what the image holds at that point)."""
    rng = np.random.default_rng(seed)
    ocs = [O.make_components(w, h, samp)[0] for (w, h, samp, _ct) in layout]
    qts, coefs = [], []
    for oc in ocs:
        q, c = _content(rng, oc, str(rng.choice(CONTENT)))
        qts.append(q)
        coefs.append(c)
    ops = [("create", [list(q) for q in qts])]
    ops += [("up", i, c, coefs[i][c], "dense") for i in range(len(ocs)) for c in range(len(ocs[i]))]
    ops.append(("decode",))
    while len(ops) < n_ops:
        r = rng.random()
        i = int(rng.integers(len(ocs)))
        nc = len(ocs[i])
        if r < 0.25:  # the image becomes another picture: new tables AND new coefficients, component steps in a random order
            kind = str(rng.choice(CONTENT))
            q, cf = _content(rng, ocs[i], kind)
            steps = [("qt", i, c, q[c]) for c in range(nc)] + [("up", i, c, cf[c], MODES[int(rng.integers(3))]) for c in range(nc)]
            for s in rng.permutation(len(steps)):
                ops.append(steps[s] + (kind,))
            qts[i], coefs[i] = q, cf
        elif r < 0.37:  # the same component once more, another transport
            c = int(rng.integers(nc))
            ops.append(("up", i, c, coefs[i][c], MODES[int(rng.integers(3))], "again"))
        elif r < 0.45:  # another table under the same coefficients
            c = int(rng.integers(nc))
            q = rng.integers(1, 200, 64).astype(np.uint16) if rng.random() < 0.8 else rng.integers(1, 65536, 64).astype(np.uint16)
            ops.append(("qt", i, c, q, "retable"))
            qts[i] = [q if k == c else qts[i][k] for k in range(nc)]
        elif r < 0.58:
            exact = _exact_class(qts[i], coefs[i])
            ops.append(("hint", i, int(rng.choice([h for h in (0, 1, 3) if h <= exact]))))
        elif r < 0.66:
            ops.append(("scan",))
        elif r < 0.74:
            ops.append(("classify",))
        else:
            ops.append(("decode",))
    ops.append(("decode",))
    return ops


def _describe(op):
    if op[0] == "create":
        return "create"
    if op[0] == "up":
        return f"up {op[1]}.{op[2]} {op[4]}" + (f" ({op[5]})" if len(op) > 5 else "")
    if op[0] == "qt":
        return f"qt {op[1]}.{op[2]}" + (f" ({op[4]})" if len(op) > 4 else "")
    if op[0] == "hint":
        return f"hint {op[1]} = {op[2]}"
    return op[0]


def _run_ops(layout, ops, label, stream=None, deferred=False):
    """Applies `ops` to a Batch and to the host model; after every decode, every image must equal the oracle's decode of the model,
    and on the fused paths the class split must not promise more than the exact classes allow.

    stream: a tests/stream_harness.py StreamHarness whose stream every call that takes one runs on (None: the null stream).
    deferred: the host does not wait after a decode — ballast in front of it and a snapshot of the output arena behind it, both on the
    stream, replace synchronize() and download(); the snapshots are compared with the model's state at their decode after one host
    wait at the end, the class split once, after the last decode.  Every mutating operation that directly follows a decode (nothing
    that drains the stream in between: a scan, the wrapper's compact upload, a dense upload, a classification) must find that decode
    pending; the count of those that did is returned."""
    ocs = [O.make_components(w, h, samp)[0] for (w, h, samp, _ct) in layout]
    assert ops[0][0] == "create"
    assert stream is not None or not deferred
    sh = None if stream is None else stream.handle
    qts = [list(q) for q in ops[0][1]]
    coefs = [[np.zeros(c.block_w * c.block_h * 64, np.int16) for c in oc] for oc in ocs]
    b = J.Batch([J.image_desc(list(_to_j(oc)), qts[i], w, h, ct) for i, (oc, (w, h, _s, ct)) in enumerate(zip(ocs, layout))])
    log = ["create"]

    def split_check(at):
        if b.path != "generic":
            exact = [_exact_class(qts[i], coefs[i]) for i in range(len(ocs))]
            counts = b.class_counts()
            assert counts[2] <= sum(e == 3 for e in exact) and counts[1] + counts[2] <= sum(e >= 1 for e in exact), (
                f"{label}: class split {counts} promises more than the exact classes {exact} after operation {at}:\n  " + "\n  ".join(log))

    snaps = stream.buffers(sum(op[0] == "decode" for op in ops), b.out_arena_bytes()) if deferred else None
    taken = []     # deferred: per decode (operation number, the model's tables and coefficients then)
    behind = None  # deferred: the event behind the last decode while nothing has drained the stream since
    try:
        for op in ops[1:]:
            log.append(_describe(op))
            if deferred and behind is not None and op[0] != "decode":
                stream.expect_pending(behind, f"operation {len(log) - 1} ({log[-1]}) of {label}")
                if op[0] not in ("qt", "hint"):  # (those two change host state only)
                    behind = None
            if op[0] == "up":
                _, i, c, cf, mode = op[:5]
                if mode == "dense":
                    b.upload(i, c, cf)
                else:
                    b.upload_compact(i, c, cf, stream=sh, classify=(mode == "compact"))
                coefs[i][c] = cf
            elif op[0] == "qt":
                _, i, c, q = op[:4]
                b.set_quantization_table(i, c, q)
                qts[i][c] = q
            elif op[0] == "hint":
                b.set_range_hint(op[1], op[2])
            elif op[0] == "scan":
                b.scan_ranges(sh)
            elif op[0] == "classify":
                b.classify_on_device(sh)
            elif deferred:
                stream.ballast()
                b.decode(sh)
                behind = stream.mark()
                stream.snapshot(snaps[len(taken)], b.out_arena(), b.out_arena_bytes())
                taken.append((len(log) - 1, [list(q) for q in qts], [list(c) for c in coefs]))
            else:
                b.decode(sh)
                b.synchronize(sh)
                bad = []
                for i, (oc, (w, h, _s, ct)) in enumerate(zip(ocs, layout)):
                    if not np.array_equal(b.download(i), O.pixels_from_coefficients(oc, qts[i], coefs[i], w, h, ct.upper())):
                        bad.append(i)
                if bad:
                    pytest.fail(f"{label}: images {bad} differ from the model after operation {len(log) - 1}:\n  " + "\n  ".join(log))
                split_check(len(log) - 1)
        if deferred:
            stream.finish()
            got = snaps.cpu().numpy()
            wrong = []
            for k, (at, q_then, c_then) in enumerate(taken):
                bad = []
                for i, (oc, (w, h, _s, ct)) in enumerate(zip(ocs, layout)):
                    want = O.pixels_from_coefficients(oc, q_then[i], c_then[i], w, h, ct.upper())
                    off = b.out_offset(i)
                    if not np.array_equal(got[k][off: off + want.size], want):
                        bad.append(i)
                if bad:
                    wrong.append(f"images {bad} after operation {at}")
            if wrong:
                pytest.fail(f"{label}: snapshots differ from the model: " + "; ".join(wrong) + ":\n  " + "\n  ".join(log))
            split_check(len(log) - 1)
            return stream.checked
    finally:
        b.close()


@pytest.mark.parametrize("run", [0, 1])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_random_batch_operation_sequences(layout, run):
    """On failure the message holds the seed and the operation log: shrink it by hand into a named test like the two below."""
    seed = 7000 + 10 * run + sorted(LAYOUTS).index(layout)
    _run_ops(LAYOUTS[layout], _random_ops(LAYOUTS[layout], seed), f"layout {layout}, seed {seed}")


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_random_batch_operation_sequences_on_a_nonblocking_stream(layout):
    """The lists of run 0 above with every call on a hipStreamNonBlocking stream and the host never waiting after a decode: each
    decode is still queued behind its ballast when the operations after it change tables, classes and coefficients."""
    seed = 7000 + sorted(LAYOUTS).index(layout)
    ops = _random_ops(LAYOUTS[layout], seed)
    h = stream_harness.StreamHarness("nonblocking")
    try:
        held = _run_ops(LAYOUTS[layout], ops, f"layout {layout}, seed {seed}, non-blocking stream", stream=h, deferred=True)
    finally:
        h.close()
    follow = sum(1 for prev, op in zip(ops[1:], ops[2:]) if prev[0] == "decode" and op[0] != "decode")
    print(f"layout {layout}: {held} mutating operations found the decode in front of them pending ({follow} directly behind a decode)")
    assert held >= follow > 0, (held, follow)


def _small_and_wrapping(layout, seed):
    """Per image: coefficients that are tight under a table of ones, and full-range ones that wrap under the same table."""
    rng = np.random.default_rng(seed)
    ocs = [O.make_components(w, h, samp)[0] for (w, h, samp, _ct) in layout]
    small = [[rng.integers(-20, 21, c.block_w * c.block_h * 64).astype(np.int16) for c in oc] for oc in ocs]
    wide = [[rng.integers(-32768, 32768, c.block_w * c.block_h * 64).astype(np.int16) for c in oc] for oc in ocs]
    ones = [[np.ones(64, np.uint16) for _ in oc] for oc in ocs]
    return ocs, ones, small, wide


@pytest.mark.parametrize("then", ["scan", "classify"])
@pytest.mark.parametrize("mode", ["compact", "compact-unclassified"])
def test_classification_after_a_pending_compact_upload(mode, then):
    """A compact upload lands in the arena at the next decode.  scan_ranges / classify_on_device called in between must classify
    what the images will hold (the new, wrapping coefficients), not what the arena still holds (the old, tight ones)."""
    layout = [LAYOUTS["420"][0], LAYOUTS["444"][1]]
    ocs, ones, small, wide = _small_and_wrapping(layout, 11)
    ops = [("create", ones)]
    ops += [("up", i, c, small[i][c], "dense") for i in range(2) for c in range(3)] + [("decode",)]
    ops += [("up", i, c, wide[i][c], mode) for i in range(2) for c in range(3)] + [(then,), ("decode",)]
    _run_ops(layout, ops, f"{mode} upload, then {then}")


@pytest.mark.parametrize("mode", ["compact", "compact-unclassified"])
def test_dense_upload_after_a_pending_compact_upload_wins(mode):
    """The last upload of a component before a decode is what it decodes: a dense upload replaces a compact one still waiting for
    its expansion."""
    layout = [LAYOUTS["420"][0], LAYOUTS["444"][1]]
    ocs, ones, small, wide = _small_and_wrapping(layout, 12)
    ops = [("create", ones)]
    ops += [("up", i, c, small[i][c], "dense") for i in range(2) for c in range(3)] + [("decode",)]
    ops += [("up", 0, c, wide[0][c], mode) for c in range(3)] + [("up", 0, c, small[0][c][::-1].copy(), "dense") for c in range(3)]
    ops += [("decode",)]
    _run_ops(layout, ops, f"{mode} upload, then a dense one")
