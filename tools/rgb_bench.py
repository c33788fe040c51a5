"""What RGB output (Batch(rgb=True)) costs, on 256 resident 1920x1080 q85 images, centred quarter windows -> 224 x 224
float32 tensors (the pixel stage: coefficients in HBM -> the model's input in HBM).

Three layouts, each decoded WITHOUT the option (3 / 1 / 4 planes per image) and WITH it (3 planes), in the same run, interleaved call
by call; each figure is the median over --reps calls of --iters decodes (jpgpu_batch_time: two events around the decodes):

  (a) 4:2:0 YCbCr   off against on: the same work, the only difference is the kernel instance (resample_tensor_rgb_kernel)
  (b) gray          on: three planes from one channel (RBand::hpass_walk<1>)
  (c) CMYK 4:4:4    on: three planes through Pillow's integer cmyk2rgb (RBand::hpass_cmyk)

    python tools/rgb_bench.py --out profiles/rgb/rgb_bench.json --commit <sha>

--only LAYOUT --option on|off: that one configuration alone, for a run under a profiler
(rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/rgb_bench.py --only cmyk --option on --reps 1 --iters 5).

The document carries the hashes of the sources it ran and the box's GPU_MAX_HW_QUEUES."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_decoder_amd as J  # noqa: E402
import synth  # noqa: E402
import tensor_ref as T  # noqa: E402
import window_bench as WB  # noqa: E402

W, H, N = WB.W, WB.H, WB.N
SIZE = (224, 224)
MEAN, STD = T.IMAGENET
SOURCES = ("tensor_band.hpp", "resample_band.hpp", "resample.hip", "window_band.hpp", "window.hip", "batch.cpp", "batch_internal.hpp", "batch_layout.hpp")
LAYOUTS = {"420": ([(2, 2), (1, 1), (1, 1)], "ycbcr", "YCbCr"), "gray": ([(1, 1)], "gray", "Grayscale"), "cmyk": ([(1, 1)] * 4, "cmyk", "CMYK")}


def make(layout, n, options):
    """-> ({option: batch}, source channels) for a layout; every batch owns its arenas and holds the same coefficients."""
    samp, mode, ct = LAYOUTS[layout]
    comps, _ = J.make_components(W, H, samp)
    lum, chroma = synth.quality_tables(85)
    qts = [lum, chroma, chroma, lum][: len(comps)]
    coefs = synth.coefficients_from_rgb(synth.synthetic_rgb(W, H), comps, mode, qts)
    desc = J.image_desc(list(comps), qts, W, H, ct)
    wins = [WB.centred(0.25)] * n
    fmt = J.TensorFormat("float32", MEAN, STD)
    out = {}
    for opt in options:
        b = J.Batch([desc] * n, windows=wins, output_size=SIZE, tensor=fmt, rgb=(opt == "on"))
        for i in range(n):
            for c in range(len(comps)):
                b.upload(i, c, coefs[c])
        out[opt] = b
    return out, len(comps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--images", type=int, default=N)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("RGB_BENCH_COMMIT", "unknown"))
    ap.add_argument("--only", default="", choices=["", *LAYOUTS], help="one layout alone (for a profiler run)")
    ap.add_argument("--option", default="", choices=["", "on", "off"], help="with --only: that option alone")
    args = ap.parse_args()
    assert J.device_count() >= 1, "needs an MI355X"
    n = args.images
    layouts = [args.only] if args.only else list(LAYOUTS)
    options = [args.option] if args.option else ["off", "on"]
    rows = []
    for layout in layouts:
        batches, nc = make(layout, n, options)
        try:
            for b in batches.values():  # warm-up
                b.time(2)
            if len(batches) == 2:  # a spot check: with three channels the option changes no bit; gray planes are T[c] of the one plane
                a, b = batches["off"].download(0), batches["on"].download(0)
                if nc == 3:
                    assert np.array_equal(T.bits(a), T.bits(b))
                elif nc == 1:
                    tab = T.table(("float32", MEAN, STD), 3)
                    u8 = np.searchsorted(tab[0], a[0])  # (T[0] is increasing: the u8 value back from the element)
                    assert np.array_equal(T.bits(tab[0][u8]), T.bits(a[0]))
                    for c in range(3):
                        assert np.array_equal(T.bits(b[c]), T.bits(tab[c][u8])), c
                else:
                    assert b.shape == (3, SIZE[1], SIZE[0]) and a.shape == (4, SIZE[1], SIZE[0])
            times = {opt: [] for opt in batches}
            for _ in range(args.reps):
                for opt, b in batches.items():
                    times[opt].append(b.time(args.iters))
            row = {"layout": layout, "source_channels": nc, "images": n}
            for opt, b in batches.items():
                row[f"{opt}_ms"] = round(float(np.median(times[opt])), 4)
                row[f"{opt}_ms_all"] = [round(t, 4) for t in times[opt]]
                row[f"{opt}_path"] = b.path
                row[f"{opt}_tensor_bytes"] = sum(b.out_bytes(i) for i in range(n))
            if len(batches) == 2:
                row["on_vs_off"] = round(row["on_ms"] / row["off_ms"], 4)
                lo, hi = min(times["off"]), max(times["off"])
                row["on_inside_the_spread_of_off"] = bool(lo <= row["on_ms"] <= hi)
            rows.append(row)
        finally:
            for b in batches.values():
                b.close()
    doc = {"tool": "tools/rgb_bench.py", "commit": args.commit, "sources_sha256": WB.sources_sha256(SOURCES), "library": os.path.basename(J._native.LIB_PATH),
           "host": socket.gethostname(), "device": WB.device_identity(), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
           "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "output_size": list(SIZE), "dtype": "float32", "reps": args.reps, "iters_per_rep": args.iters,
           "workload": f"{W}x{H} q85 x {n} resident images, centred quarter windows -> 224 x 224 float32 (pixel stage: coefficients in HBM -> tensors in HBM)",
           "env": {k: os.environ[k] for k in sorted(os.environ) if k.startswith("JPGPU_")}, "pixel_stage": rows}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
