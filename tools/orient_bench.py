"""What EXIF orientation in front of the fixed output size costs, measured in one run.

Pixel stage (coefficients resident in HBM -> f32 tensors in HBM): 256 resident 1080p 4:2:0 q85 images, centred quarter windows to
224 x 224 f32, every configuration on the same coefficient arena, interleaved call by call; a figure is the median over --reps calls
of jpgpu_batch_time (--iters decodes between two events):
    off            no orientations (the batch without the argument)
    all_6          every image at orientation 6 (a transposing one)
    all_3          every image at orientation 3 (not transposing: the resample job is the one of `off`, so all_3 - off IS the orient launch)
    one_in_8       one image in eight at orientation 6
    no_output_size the windowed decode alone: off - no_output_size is the resample launch
From JPEG bytes: 256 files to HBM through a kept Pipeline (device entropy), the option off against on (files carrying orientation 6),
the median over --reps calls after two uncounted calls each.  The pipeline a process creates first runs its calls one to three ms
faster than a later one, whatever it decodes (tools/tensor_bench.py), so the comparison is run in both creation orders: --first.

    python tools/orient_bench.py --out profiles/orient/orient_bench.json --commit <sha>
    python tools/orient_bench.py --no-pixel-stage --first on --out profiles/orient/orient_e2e_on_first.json --commit <sha>

The document carries the hashes of the sources it ran and the box's GPU_MAX_HW_QUEUES."""
import argparse
import ctypes as C
import json
import os
import socket
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_decoder_amd as J  # noqa: E402
import filter_ref as F  # noqa: E402
import orient_ref as OR  # noqa: E402
import synth  # noqa: E402
import tensor_ref as T  # noqa: E402
import window_bench as WB  # noqa: E402

N, W, H = WB.N, WB.W, WB.H
SIZE = (224, 224)
MEAN, STD = T.IMAGENET
SOURCES = ("orient_band.hpp", "orient.hip", "batch_output.hpp", "batch_output.cpp", "batch.cpp", "batch_internal.hpp", "resample_band.hpp", "resample.hip",
           "tensor_band.hpp", "window_band.hpp", "pipeline.cpp")


def oriented_window(o, win):
    """The window of the ORIENTED image whose source window is `win` (so that every configuration decodes the same source pixels)."""
    x, y, w, h = win
    if o == 1:
        return win
    if o == 3:
        return (W - x - w, H - y - h, w, h)
    if o == 6:
        return (H - y - h, x, h, w)
    raise ValueError(o)


def with_exif(data, o):
    blob = b"II" + struct.pack("<HI", 42, 8) + struct.pack("<H", 1) + struct.pack("<HHIHH", 0x0112, 3, 1, o, 0) + struct.pack("<I", 0)
    payload = b"Exif\0\0" + blob
    return data[:2] + b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload + data[2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("ORIENT_BENCH_COMMIT", "unknown"))
    ap.add_argument("--no-files", action="store_true", help="the pixel stage alone")
    ap.add_argument("--no-pixel-stage", action="store_true", help="the legs from JPEG bytes alone")
    ap.add_argument("--first", default="off", choices=["off", "on"], help="from JPEG bytes: the configuration whose pipeline is created first")
    args = ap.parse_args()
    assert J.device_count() >= 1, "needs an MI355X"
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    doc = {"tool": "tools/orient_bench.py", "commit": args.commit, "sources_sha256": WB.sources_sha256(SOURCES), "library": os.path.basename(J._native.LIB_PATH),
           "host": socket.gethostname(), "device": WB.device_identity(), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
           "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "output_size": list(SIZE), "reps": args.reps, "iters_per_rep": args.iters,
           "workload": f"4:2:0 q85 1080p x {N}, centred quarter windows to 224 x 224 f32 tensors",
           "env": {k: os.environ[k] for k in sorted(os.environ) if k.startswith("JPGPU_")}}
    fmt = J.TensorFormat("float32", MEAN, STD)
    win = WB.centred(0.25)
    for o in (3, 6):
        assert OR.source_window(o, W, H, oriented_window(o, win)) == win

    if not args.no_pixel_stage:
        pixel_stage(args, doc, hip, fmt, win)
    if not args.no_files:
        from_bytes(args, doc, fmt, win)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def pixel_stage(args, doc, hip, fmt, win):
    lum, chroma = synth.quality_tables(85)
    qts = [lum, chroma, chroma]
    comps, _ = J.make_components(W, H, [(2, 2), (1, 1), (1, 1)])
    coefs = synth.coefficients_from_rgb(synth.synthetic_rgb(W, H), comps, "ycbcr", qts)
    desc = J.image_desc(list(comps), qts, W, H, "YCbCr")
    full = J.Batch([desc] * N)
    for i in range(N):
        for c in range(3):
            full.upload(i, c, coefs[c])
    full.decode()
    full.synchronize()
    ref = full.download(0).reshape(H, W, 3)
    layouts = {"off": None, "all_6": [6] * N, "all_3": [3] * N, "one_in_8": [6 if i % 8 == 0 else 1 for i in range(N)]}
    configs, arenas = {}, []
    for name in ("no_output_size",) + tuple(layouts):
        ors = layouts.get(name)
        wins = [oriented_window(1 if ors is None else ors[i], win) for i in range(N)]
        b = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=None if name == "no_output_size" else SIZE,
                    tensor=None if name == "no_output_size" else fmt, orientations=ors)
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), b.out_arena_bytes()) == 0
        arenas.append(ptr)
        b.bind(full.coef_arena(), ptr.value)
        configs[name] = (b, ors)
    x, y, sw, sh = win
    tab = T.table(("float32", MEAN, STD), 3)
    for name, (b, ors) in configs.items():  # correctness spot check against the statements
        b.decode()
        b.synchronize()
        if name == "no_output_size":
            continue
        for i in (0, 1, N - 1):
            o = 1 if ors is None else ors[i]
            want = T.to_tensor(F.resize(OR.orient(ref[y:y + sh, x:x + sw], o), *SIZE), tab, False)
            assert np.array_equal(T.bits(b.download(i)), T.bits(want)), (name, i)
    times = {n: [] for n in configs}
    for _ in range(args.reps):
        for name, (b, _o) in configs.items():
            times[name].append(b.time(args.iters))
    med = {n: float(np.median(t)) for n, t in times.items()}
    rows = []
    for name, (b, ors) in configs.items():
        row = {"config": name, "path": b.path, "oriented_images": 0 if ors is None else sum(o != 1 for o in ors), "ms_median": round(med[name], 4),
               "ms_all": [round(t, 4) for t in times[name]]}
        if name not in ("no_output_size", "off"):
            row["extra_ms_vs_off"] = round(med[name] - med["off"], 4)
            row["call_vs_off"] = round(med[name] / med["off"], 4)
        rows.append(row)
    doc["pixel_stage"] = {"source_window": list(win), "configs": rows,
                          "resample_launch_ms": round(med["off"] - med["no_output_size"], 4),
                          "orient_launch_ms": round(med["all_3"] - med["off"], 4),
                          "orient_launch_note": "all_3 - off: orientation 3 leaves the resample job as it is, so the difference is the orient launch of 256 images; "
                                                "resample_launch_ms is off - no_output_size",
                          "off_spread": round((max(times["off"]) - min(times["off"])) / med["off"], 4)}
    for b, _o in configs.values():
        b.close()
    for ptr in arenas:
        hip.hipFree(ptr)
    full.close()


def from_bytes(args, doc, fmt, win):
    base, how = WB.e2e_files(4)
    plain = [base[k % 4] for k in range(N)]
    tagged = [with_exif(d, 6) for d in plain]
    wins_off, wins_on = [win] * N, [oriented_window(6, win)] * N
    legs = {"off": (plain, wins_off, False), "on": (tagged, wins_on, True)}
    order = ("off", "on") if args.first == "off" else ("on", "off")
    pipes = {name: (J.Pipeline(),) + legs[name] for name in order}
    e2e = {n: [] for n in pipes}
    for _ in range(2):  # (uncounted: the first call creates the sub-batches)
        for name, (p, files, wins, on) in pipes.items():
            out = p.decode(files, download=False, windows=wins, output_size=SIZE, tensor=fmt, exif_orientation=on)
            assert not any(isinstance(v, Exception) for v in out), name
    for _ in range(args.reps):
        for name, (p, files, wins, on) in pipes.items():
            t0 = time.perf_counter()
            p.decode(files, download=False, windows=wins, output_size=SIZE, tensor=fmt, exif_orientation=on)
            e2e[name].append((time.perf_counter() - t0) * 1e3)
    emed = {n: float(np.median(t)) for n, t in e2e.items()}
    doc["from_jpeg_bytes"] = {"files": f"{N} files to HBM, {how}", "pipeline_created_first": args.first, "paths": {n: pipes[n][0].kernel_path for n in pipes},
                              "ms_median": {n: round(v, 3) for n, v in emed.items()}, "ms_all": {n: [round(v, 3) for v in t] for n, t in e2e.items()},
                              "on_vs_off": round(emed["on"] / emed["off"], 4)}
    for p, *_r in pipes.values():
        p.close()


if __name__ == "__main__":
    main()
