"""The resample filters of DESIGN.md §4.15 beside BILINEAR on the band kernels, pixel stage (coefficients resident in HBM -> pixels in
HBM, 256 resident 4:2:0 q85 images): every case without an output size, and to 224 x 224 under each filter, on the same coefficient
arena.  The configurations are interleaved call by call; a figure is the median over --reps calls of jpgpu_batch_time (--iters
decodes between two events).  Beside every figure stands the planner's view of the job, computed here from the library's own
tables: rb, the bands, and the redundancy — the source rows its bands pass through the horizontal pass over the source rows there are.

    python tools/filter_bench.py --out profiles/filters/filter_bench.json --commit <sha>

Cases: 1080p whole; the shorter side to 224 and a centre crop of 224 (CLIP's transform, a placement); centred quarter windows of 1080p;
500 x 375 whole; 2160p whole.  The document carries the hashes of the sources it ran and the box's GPU_MAX_HW_QUEUES."""
import argparse
import ctypes as C
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
import filter_ref as F  # noqa: E402
import synth  # noqa: E402
import window_bench as WB  # noqa: E402

N = WB.N
SIZE = (224, 224)
LDS = 32 * 1024  # RS_MAX_LDS
FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")
SOURCES = ("resample_band.hpp", "resample.hip", "tensor_band.hpp", "placed_band.hpp", "placed.hip", "batch.cpp", "batch_internal.hpp", "image_job.cpp")


def plan(name, in_h, out_h, first, count, row_bytes):
    """resample_plan restated on the library's tables for output rows [first, first + count) of the axis in_h -> out_h: rb, bands,
    cap_rows, chunks of the widest band, and the redundancy (sum of the bands' source rows / the source rows any of them reads)."""
    vb, _ = J.resample_coefficients(in_h, out_h, name)
    vb = vb[first:first + count]
    pitch = (row_bytes + 3) & ~3
    cap = min(LDS // pitch, in_h)

    def spans(rb):
        return [(int(vb[r0, 0]), int(vb[min(r0 + rb, count) - 1].sum())) for r0 in range(0, count, rb)]

    rb = min(64, count)
    while rb > 1 and any(s1 - s0 > cap for s0, s1 in spans(rb)):
        rb -= 1
    sp = spans(rb)
    read = int(vb[-1].sum()) - int(vb[0, 0])
    return {"rb": rb, "bands": len(sp), "cap_rows": cap, "chunks_max": max(-(-(s1 - s0) // cap) for s0, s1 in sp),
            "redundancy": round(sum(s1 - s0 for s0, s1 in sp) / read, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default=os.environ.get("FILTER_BENCH_COMMIT", "unknown"))
    ap.add_argument("--only", default="", help="comma-separated cases")
    args = ap.parse_args()
    assert J.device_count() >= 1, "needs an MI355X"
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    lum, chroma = synth.quality_tables(85)
    qts = [lum, chroma, chroma]
    clip = J.fit_placement(J.Fit("shorter_side_crop", size=224), (WB.W, WB.H), SIZE)
    # case -> (source size, window, placement)
    cases = {"1080p_whole": ((1920, 1080), None, None), "1080p_clip_shorter_side_224_crop_224": ((1920, 1080), None, clip),
             "1080p_quarter_window": ((1920, 1080), WB.centred(0.25), None), "500x375_whole": ((500, 375), None, None), "2160p_whole": ((3840, 2160), None, None)}
    if args.only:
        cases = {k: v for k, v in cases.items() if k in args.only.split(",")}
    doc = {"tool": "tools/filter_bench.py", "commit": args.commit, "sources_sha256": WB.sources_sha256(SOURCES), "library": os.path.basename(J._native.LIB_PATH),
           "host": socket.gethostname(), "device": WB.device_identity(), "date": time.strftime("%Y-%m-%d %H:%M:%S"),
           "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "output_size": list(SIZE), "reps": args.reps, "iters_per_rep": args.iters,
           "workload": f"4:2:0 q85 x {N} resident images (pixel stage: coefficients in HBM -> pixels in HBM), band kernels",
           "env": {k: os.environ[k] for k in sorted(os.environ) if k.startswith("JPGPU_")}, "cases": []}
    os.environ["JPGPU_RS_ROLL"] = "1"  # (the band route unless a configuration asks for runs: read when a batch makes its tables)
    fulls = {}
    for case, ((w, h), win, pl) in cases.items():
        if (w, h) not in fulls:  # (one coefficient arena per source size; every batch of the size reads it)
            comps, _ = J.make_components(w, h, [(2, 2), (1, 1), (1, 1)])
            coefs = synth.coefficients_from_rgb(synth.synthetic_rgb(w, h), comps, "ycbcr", qts)
            desc = J.image_desc(list(comps), qts, w, h, "YCbCr")
            full = J.Batch([desc] * N)
            for i in range(N):
                for c in range(3):
                    full.upload(i, c, coefs[c])
            full.decode()
            full.synchronize()
            fulls[(w, h)] = (desc, full, full.download(0).reshape(h, w, 3))
        desc, full, ref = fulls[(w, h)]
        wins = None if win is None else [win] * N
        pls = None if pl is None else [pl] * N
        x, y, sw, sh = win if win else (0, 0, w, h)
        configs, arenas = {}, []
        for name in (None,) + FILTERS:
            if name is None and win is None:
                configs["no_output_size"] = full
                continue
            b = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=None if name is None else SIZE,
                        placements=None if name is None else pls, filter=name)
            ptr = C.c_void_p()
            assert hip.hipMalloc(C.byref(ptr), b.out_arena_bytes()) == 0
            arenas.append(ptr)
            b.bind(full.coef_arena(), ptr.value)
            configs[name or "no_output_size"] = b
            if name in ("bicubic", "lanczos") and pl is None:  # the run route beside the band route: the same job, bpr bands per workgroup
                for bpr in (2, 4, 8):
                    os.environ["JPGPU_RS_ROLL"] = str(bpr)
                    r = J.Batch([desc] * N, flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=SIZE, filter=name)
                    os.environ["JPGPU_RS_ROLL"] = "1"
                    if "+roll" not in r.path:  # (no candidate: chunked bands, or a single band)
                        r.close()
                        continue
                    ptr = C.c_void_p()
                    assert hip.hipMalloc(C.byref(ptr), r.out_arena_bytes()) == 0
                    arenas.append(ptr)
                    r.bind(full.coef_arena(), ptr.value)
                    configs[f"{name}+roll{bpr}"] = r
        for name, b in configs.items():  # correctness spot check: two images against the full decode, sliced and resampled by the statement
            b.decode()
            b.synchronize()
            if name == "no_output_size":
                continue
            src = ref[y:y + sh, x:x + sw]
            fname = name.split("+")[0]
            want = F.resize(src, *SIZE, F.NAMES[fname]) if pl is None else F.placed(src, *pl, *SIZE, (0, 0, 0, 0), F.NAMES[fname])
            for i in (0, N - 1):
                assert np.array_equal(b.download(i), want.reshape(-1)), (case, name, i)
        times = {n: [] for n in configs}
        for _ in range(args.reps):
            for name, b in configs.items():
                times[name].append(b.time(args.iters))
        med = {n: float(np.median(t)) for n, t in times.items()}
        rows = []
        for name, b in configs.items():
            row = {"config": name, "path": b.path, "ms_median": round(med[name], 4), "ms_all": [round(t, 4) for t in times[name]]}
            if name != "no_output_size":
                rw, rh, px, py = pl if pl else (SIZE[0], SIZE[1], 0, 0)
                first, count = max(0, -py), min(rh + py, SIZE[1]) - max(py, 0)
                vis_w = min(rw + px, SIZE[0]) - max(px, 0)
                row["resample_ms"] = round(med[name] - med["no_output_size"], 4)
                row["resample_vs_bilinear"] = round((med[name] - med["no_output_size"]) / (med["bilinear"] - med["no_output_size"]), 3)
                row["call_vs_bilinear"] = round(med[name] / med["bilinear"], 4)
                fname = name.split("+")[0]
                row["plan"] = plan(fname, sh, rh, first, count, vis_w * 3)
                row["hks"], row["vks"] = F.ksize_of(sw, rw, F.NAMES[fname]), F.ksize_of(sh, rh, F.NAMES[fname])
                if "+roll" in name:  # against the band route of the same filter, and that route's own spread over the repeats
                    row["vs_band_route"] = round(med[name] / med[fname], 4)
                    row["band_route_spread"] = round((max(times[fname]) - min(times[fname])) / med[fname], 4)
            rows.append(row)
        doc["cases"].append({"case": case, "source": [sw, sh], "window": win, "placement": pl, "configs": rows})
        for name, b in configs.items():
            if b is not full:
                b.close()
        for ptr in arenas:
            hip.hipFree(ptr)
    for _desc, full, _ref in fulls.values():
        full.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
