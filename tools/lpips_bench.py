"""Times LPIPS per image pair at 378 x 504 (the LLFF evaluation size) for 'alex' and 'vgg', one JSON line per net:

  python tools/lpips_bench.py                          # both nets, 20 timed calls after 3 warm-up calls
  python tools/lpips_bench.py --nets alex --height 96 --width 128
  python tools/lpips_bench.py --no-torch               # skip the baseline

The weights are seeded random ones (tests/lpips_restated.py): the time does not depend on their values.  Per net:
  layers       one row per launch of ops.lpips.lpips_layers, in order: the entry point, the layer (torchvision's features
               index, or the tap for a distance), median ms from device events around the launch (L.KERNEL_TIMES), and
               for a convolution its 2 * M * K * pixels FLOPs (both images), the TFLOP/s they make and their share of the
               157.3 TFLOP/s fp32 matrix peak
  kernel_ms    the sum of the rows: what the kernels take
  call_ms      the host clock around one lpips_layers call ending in a synchronise: launches, allocations and kernels
  conv_tflops  all convolutions' FLOPs over all convolutions' kernel time, and `conv_peak_share`
  torch        the same network (conv2d + relu + max_pool2d, both images as one batch, the taps kept) through torch's own GPU
               convolutions on the same box in the same run: per-layer median ms from device events and `net_ms` their sum —
               what a user does today without the distance head; {'error': ...} when torch's convolution does not run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
DEV = "cuda:0"
PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=378)
    ap.add_argument("--width", type=int, default=504)
    ap.add_argument("--nets", nargs="+", default=["alex", "vgg"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as TF
    import lpips_restated as R
    from hypernerf_torch_amd import _lib as L
    from hypernerf_torch_amd.ops import lpips as P
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench.py needs the MI355X: a CPU run gives no time")
    h, w = args.height, args.width
    pred, gt = (t.to(DEV) for t in R.image_pair(1, h, w, 1))

    for net in args.nets:
        raw = R.random_weights(net, R.WEIGHT_SEED[net])
        weights = P.lpips_weights_from_state_dicts(net, *R.split_state_dicts(net, raw)).to(DEV)
        # FLOPs per convolution from the shapes
        flops, side = {}, (h, w)
        for layer in P.lpips_net(net):
            k, s, p = (layer[4], layer[5], layer[6]) if layer[0] == "conv" else (layer[2], layer[3], 0)
            side = tuple(P._out_side(v, k, s, p) for v in side)
            if layer[0] == "conv":
                flops[f"hn_lpips_conv[{layer[1]}]"] = 2 * layer[3] * layer[2] * k * k * 2 * side[0] * side[1]
        for _ in range(args.warmup):
            P.lpips_layers(pred, gt, weights)
        runs, order = [], []
        for _ in range(args.repeats):
            L.KERNEL_TIMES = {}
            try:
                P.lpips_layers(pred, gt, weights)
                times = L.collect_kernel_times()
            finally:
                L.KERNEL_TIMES = None
            order = list(times)
            runs.append({name: sum(v) for name, v in times.items()})
        rows, conv_ms, conv_flops = [], 0.0, 0
        for name in order:
            ms = statistics.median(r[name] for r in runs)
            row = {"launch": name, "ms": round(ms, 5)}
            if name in flops:
                tf = flops[name] / (ms * 1e-3) / 1e12
                row.update(gflop=round(flops[name] / 1e9, 4), tflops=round(tf, 2), peak_share=round(tf / PEAK_TFLOPS, 4))
                conv_ms += ms
                conv_flops += flops[name]
            rows.append(row)
        wall = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.lpips_layers(pred, gt, weights)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        conv_tf = conv_flops / (conv_ms * 1e-3) / 1e12
        res = {"net": net, "height": h, "width": w, "repeats": args.repeats, "layers": rows,
               "kernel_ms": round(sum(r["ms"] for r in rows), 4), "call_ms": round(statistics.median(wall), 4),
               "conv_gflop": round(conv_flops / 1e9, 3), "conv_ms": round(conv_ms, 4), "conv_tflops": round(conv_tf, 2),
               "conv_peak_share": round(conv_tf / PEAK_TFLOPS, 4), "peak_tflops": PEAK_TFLOPS}

        if not args.no_torch:
            try:
                tw = [(wt.to(DEV), b.to(DEV)) for wt, b in raw["convs"]]
                x0 = P.lpips_prepare(pred, gt, net)

                def torch_net(record):
                    x, ci, taps = x0, 0, []
                    for layer in P.lpips_net(net):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        if layer[0] == "pool":
                            x = TF.max_pool2d(x, layer[2], layer[3])
                        else:
                            x = TF.relu(TF.conv2d(x, tw[ci][0], tw[ci][1], stride=layer[5], padding=layer[6]))
                            ci += 1
                            if layer[7]:
                                taps.append(x)
                        e1.record()
                        record.append((f"{layer[0]}[{layer[1]}]", e0, e1))
                    return taps

                with torch.no_grad():
                    for _ in range(args.warmup):
                        torch_net([])
                    torch.cuda.synchronize()
                    truns = []
                    for _ in range(args.repeats):
                        rec = []
                        torch_net(rec)
                        torch.cuda.synchronize()
                        truns.append({name: e0.elapsed_time(e1) for name, e0, e1 in rec})
                trows = [{"layer": name, "ms": round(statistics.median(r[name] for r in truns), 5)} for name in truns[0]]
                res["torch"] = {"layers": trows, "net_ms": round(sum(r["ms"] for r in trows), 4)}
                ours = sum(r["ms"] for r in rows if not r["launch"].startswith(("hn_lpips_distance", "hn_lpips_prepare")))
                res["net_ms"] = round(ours, 4)
            except Exception as e:      # torch's GPU convolution is not this project's: report, do not fail
                res["torch"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        res["build"] = L.build_id()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
