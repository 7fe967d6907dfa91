"""Times the GIF path per 378 x 504 frame (the LLFF evaluation size), one JSON line:

  python tools/gif_bench.py                        # 378 x 504, 8 frames, 50 launches per kernel
  python tools/gif_bench.py --height 96 --width 128 --frames 3

The frames are synthetic: smooth gradients plus noise inside an ellipse on a flat white surround (about 3e4 occupied
colour cells, and one cell that holds most of the pixels), a different one per frame.  Per stage, the median over
`--repeats` runs after `--warmup` runs:
  hist_ms / map_ms / depth_ms    one launch of hn_color_hist / hn_palette_map / hn_depth_range + hn_depth_colormap on
                                 one frame, from device events around the launch (L.KERNEL_TIMES)
  hist_white_ms                  hn_color_hist on an all-white frame: every pixel in one cell
  palette_ms                     inference.palette_from_histogram on the host (the table's device-to-host copy included)
  lzw_ms                         functional.gif_lzw of one index map (host code)
  write_gif_ms                   inference.write_gif of all frames into a file, host wall clock, per frame
`bytes` is what the two kernels must move per frame: hist 3 N read (+ the cells touched), map 3 N read + N written."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=378)
    ap.add_argument("--width", type=int, default=504)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gif_restated as R
    from hypernerf_torch_amd import _lib as L
    from hypernerf_torch_amd import functional as F
    from hypernerf_torch_amd import inference as I
    if not torch.cuda.is_available():
        raise SystemExit("gif_bench.py needs the MI355X: a CPU run gives no time")
    h, w = args.height, args.width
    frames = [torch.from_numpy(R.synthetic_frame(h, w, surround=True, seed=s)).to(DEV) for s in range(args.frames)]
    white = torch.full((h, w, 3), 255, dtype=torch.uint8, device=DEV)
    depth = torch.rand((h, w), device=DEV) * 5 + 0.5
    lut = I.jet_lut().to(DEV)
    table = F.color_histogram(frames[0])
    pal, n_colors = I.palette_from_histogram(table)
    pal_dev = torch.from_numpy(pal[:n_colors]).to(DEV)
    index = F.palette_map(frames[0], pal_dev).cpu()

    def launches(fn, names):
        """median ms of the named launches of fn(), summed per call, from device events."""
        for _ in range(args.warmup):
            fn()
        per_call = []
        for _ in range(args.repeats):
            L.KERNEL_TIMES = {}
            try:
                fn()
                times = L.collect_kernel_times()
            finally:
                L.KERNEL_TIMES = None
            per_call.append(sum(sum(times[n]) for n in names))
        return statistics.median(per_call)

    def host(fn, repeats):
        fn()
        out = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    scratch = torch.zeros((1 << 18, 4), dtype=torch.int64, device=DEV)
    res = {
        "height": h, "width": w, "frames": args.frames, "repeats": args.repeats,
        "cells_frame0": int((table[:, 0] != 0).sum()), "largest_cell_share": float(table[:, 0].max()) / (h * w),
        "n_colors": n_colors,
        "hist_ms": launches(lambda: F.color_histogram(frames[0], out=scratch), ["hn_color_hist"]),
        "hist_white_ms": launches(lambda: F.color_histogram(white, out=scratch), ["hn_color_hist"]),
        "map_ms": launches(lambda: F.palette_map(frames[0], pal_dev), ["hn_palette_map"]),
        "depth_ms": launches(lambda: F.depth_colormap(depth, lut), ["hn_depth_range", "hn_depth_colormap"]),
        "palette_ms": host(lambda: I.palette_from_histogram(table), 5),
        "lzw_ms": host(lambda: F.gif_lzw(index), 10),
        "bytes": {"hist": 3 * h * w, "map": 4 * h * w},
        "build": L.build_id(),
    }
    res["lzw_bytes"] = len(F.gif_lzw(index))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bench.gif")
        for mode in ("global", "frame"):
            res[f"write_gif_{mode}_ms_per_frame"] = host(lambda: I.write_gif(path, frames, palette=mode), 3) / args.frames
            res[f"gif_{mode}_bytes"] = os.path.getsize(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
