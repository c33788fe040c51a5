#!/usr/bin/env python3
"""Latency of ONE image through the drop-in surfaces: Decoder(data).decode() (the reference's API over the Worker ABI) and a
one-image Pipeline call.  python tools/decoder_latency.py [--window] [file ...]
--window: also Decoder.set_window / Pipeline.decode(windows=) with the centred quarter of the image (x, y, w, h multiples of 16), beside
the unwindowed figures of the same run."""
import io
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np

import jpeg_decoder_amd as J
J.process_init()  # GPU_MAX_HW_QUEUES before the HIP runtime starts (opt-in since round 4)


def med(f, n=30):
    f()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    window = "--window" in sys.argv[1:]
    files = [a for a in sys.argv[1:] if a != "--window"]
    datas = [(os.path.basename(f), open(f, "rb").read()) for f in files]
    if not datas:
        import synth
        from PIL import Image
        sizes = [tuple(int(v) for v in t.split('x')) for t in os.environ['SIZES'].split(',')] if os.environ.get('SIZES') else [(512, 512), (1920, 1080), (3840, 2160)]
        for (w, h) in sizes:
            buf = io.BytesIO()
            Image.fromarray(synth.synthetic_rgb(w, h, seed=1)).save(buf, format="JPEG", quality=85, subsampling="4:2:0")
            datas.append((f"synthetic {w}x{h} 4:2:0 q85", buf.getvalue()))
    p = J.Pipeline(threads=1)
    for name, d in datas:
        a = med(lambda: J.Decoder(d).decode())
        b = med(lambda: p.decode([d], device_entropy=False))
        c = med(lambda: p.decode([d], device_entropy=True))
        print(f"{name}: Decoder.decode {a:.2f} ms | Pipeline (1 image, host entropy) {b:.2f} ms | Pipeline (1 image, device entropy) {c:.2f} ms")
        if window:
            probe = J.Decoder(d)
            probe.read_info()
            iw, ih = probe.info().width, probe.info().height
            probe.close()
            w, h = max(16, iw // 2 & ~15), max(16, ih // 2 & ~15)
            win = ((iw - w) // 2 & ~15, (ih - h) // 2 & ~15, w, h)

            def windowed():
                dec = J.Decoder(d)
                dec.set_window(*win)
                return dec.decode()

            assert windowed().size == w * h * (J.Decoder(d).decode().size // (iw * ih))
            aw = med(windowed)
            bw = med(lambda: p.decode([d], device_entropy=False, windows=[win]))
            cw = med(lambda: p.decode([d], device_entropy=True, windows=[win]))
            print(f"{name}, window {win}: Decoder.decode {aw:.2f} ms ({aw / a:.2f} x) | Pipeline (host entropy) {bw:.2f} ms ({bw / b:.2f} x) | "
                  f"Pipeline (device entropy) {cw:.2f} ms ({cw / c:.2f} x)")


if __name__ == "__main__":
    main()
