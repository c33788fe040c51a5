"""One kept Pipeline through every output option in turn, on the MI355X: which calls keep their sub-batches, which set fresh windows in
place and which create them anew (the `kept` / `re-windowed in place` / `created` words of JPGPU_PIPE_TRACE), and that every call's
bytes are those of a fresh Batch created with the same options.  That is a comparison of device against device: bit-exactness against
the references is what the feature tests and the output fuzzer assert."""
import re

import numpy as np
import pytest

import oracle as O
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ

pytestmark = pytest.mark.gpu

J = None
FILES = [("420", (32, 32), "YCbCr"), ("gray", (32, 24), "Grayscale"), ("444", (24, 32), "YCbCr")]
WINS_A = [(8, 8, 16, 16), (16, 8, 16, 16), (8, 16, 16, 16)]
WINS_B = [(0, 0, 16, 16), (3, 5, 16, 16), (7, 9, 16, 16)]
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg
    RZ.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def _cases(files):
    """Every file as the (components, tables, coefficients, colour transform, output size) a Batch is fed with, from the oracle's parse."""
    cases = []
    for data, (_layout, _size, ct) in zip(files, FILES):
        d = O.decode(data, keep_intermediates=True)
        cases.append((list(d.components), d.qtables, d.coefs, ct, d.width, d.height))
    return cases


def _fresh_batch(cases, opt):
    """The bytes of every image from a Batch created for this call alone."""
    size = opt.get("output_size")
    pls = None if opt.get("fit") is None else [J.fit_placement(opt["fit"], (w[2], w[3]), size) for w in opt["windows"]]
    b = J.Batch([RZ._desc(c) for c in cases], windows=opt["windows"], output_size=size, tensor=opt.get("tensor"), rgb=opt.get("rgb", False), placements=pls,
                fill=None if opt.get("fit") is None else opt["fit"].fill, filter=opt.get("filter"), warp=opt.get("warp"))
    try:
        RZ._upload(b, cases)
        if opt.get("flips") is not None:
            b.set_flips(opt["flips"])
        if opt.get("warps") is not None:
            b.set_warps(opt["warps"])
        b.decode()
        b.synchronize()
        return [np.ascontiguousarray(b.download(i)).view(np.uint8).reshape(-1) for i in range(len(cases))], b.path
    finally:
        b.close()


def test_thirteen_calls_on_one_kept_pipeline(monkeypatch, capfd):
    files = [PW._file(layout, "base", size) for layout, size, _ct in FILES]
    cases = _cases(files)
    f32, f16 = J.TensorFormat("float32", (0.4, 0.5, 0.6, 0.0), (0.2, 0.3, 0.25, 1.0)), J.TensorFormat("float16", (0.4, 0.5, 0.6, 0.0), (0.2, 0.3, 0.25, 1.0))
    fit = J.Fit("letterbox", fill=(7, 99, 200, 31))
    warp = J.WarpOptions("bilinear", (9, 250, 77, 140))
    turned = (0.9, -0.3, 2.0, 0.3, 0.9, -1.5)
    base = dict(windows=WINS_A, output_size=(8, 8), tensor=f32)
    steps = [("first", {}, "created"), ("same", {}, "kept"), ("windows", dict(windows=WINS_B), "re-windowed in place"),
             ("size", dict(output_size=(12, 10)), "created"), ("rgb", dict(rgb=True), "created"), ("dtype", dict(tensor=f16), "created"),
             ("filter", dict(filter="bicubic"), "created"), ("fit", dict(fit=fit), "created"), ("warp", dict(warp=warp), "created"), ("same", {}, "kept"),
             ("flips", dict(flips=[True, False, True]), "kept"), ("matrices", dict(warps=[turned, None, IDENTITY]), "kept"),
             ("off", dict(output_size=None, tensor=None, rgb=False, filter=None, fit=None, warp=None, flips=None, warps=None), "created")]
    assert len(steps) == 13
    opt = dict(base)
    p = J.Pipeline(threads=4)
    try:
        PW._env(monkeypatch, {})
        monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
        for c, (name, change, word) in enumerate(steps):
            opt.update(change)
            capfd.readouterr()
            out = p.decode(files, **opt)
            trace = capfd.readouterr().err
            hows = re.findall(r"pipeline trace: sub-batch \d+ \(\d+ images, (\d+) with a window\): (.*) in [0-9.]+ ms", trace)
            assert hows and all(h == word for _n, h in hows) and sum(int(n) for n, _h in hows) == 3, (c, name, word, hows, trace[-600:])
            want, path = _fresh_batch(cases, opt)
            assert len(hows) > 1 or p.kernel_path == path, (c, name, p.kernel_path, path)  # (one sub-batch: the batch's own path)
            if opt.get("fit") is not None:
                assert [p.placement(i) for i in range(3)] == [J.fit_placement(fit, (16, 16), opt["output_size"])] * 3
            for i in range(3):
                assert not isinstance(out[i], Exception), (c, name, i, out[i])
                got = np.ascontiguousarray(out[i]).view(np.uint8).reshape(-1)
                assert got.size == want[i].size and np.array_equal(got, want[i]), (c, name, i)
        assert "+" not in p.kernel_path  # (all options off: the windows' own bytes)
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()
