"""What the distortion loss (TrainStep(distortion_loss=losses.DistortionLoss()); hn_distortion_*) costs per step at config 2
(1024 rays x (64+64), bf16, one captured graph per step), one JSON line per process:

  python tools/distortion_bench.py                    # step time without the term, with it (HIP head) and with the same
                                                      # loss in torch ops (cumsum form), alternated in ONE process
  python tools/distortion_bench.py --levels coarse fine
  python tools/distortion_bench.py --eager hip --steps 60
                                                      # eager steps of one variant, for a run of its own under
                                                      # rocprofv3 --kernel-trace --output-format csv
  python tools/distortion_bench.py --summarise kernel_trace.csv     # medians of the term's kernels in such a trace

The three variants are three TrainSteps over three models with the same seeded parameters and the same fixed rays; after
`--warmup` steps each, `--rounds` rounds time `--steps` steps of every variant in turn (host wall clock around steps that
end in a device synchronise): drift of the box hits all three alike.  The medians over the rounds and their spread are
reported."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
VARIANTS = ("off", "hip", "torch")
KERNELS = ("hn_distortion_fwd_kernel", "hn_distortion_bwd_kernel", "hn_composite_kernel", "hn_composite_pdf_kernel")


def summarise(path):
    """Median duration per kernel of KERNELS in a rocprofv3 --kernel-trace CSV (template arguments kept apart)."""
    times = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if any(k in name for k in KERNELS):
                key = name.split("(")[0]
                times.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    return {"part": "kernel", "trace": os.path.basename(path),
            "kernels": {k: {"launches": len(v), "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
                        for k, v in sorted(times.items())}}


class TorchHead:
    """The same loss in torch ops, O(S) per ray through cumsum, with DistortionLoss's interface towards TrainStep."""

    def __init__(self, weight, levels):
        self.weight, self.levels = weight, levels

    def per_level(self, model, results, root=1.0):
        import torch
        out = []
        for level in self.levels:
            w, z = results[level]["weights"], model.last_sampling["z_" + level]
            s = (z - model.near) / (model.far - model.near)
            m = torch.cat([(s[:, :-1] + s[:, 1:]) / 2, s[:, -1:]], dim=1)
            d = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, -1:])], dim=1)
            wm = w * m
            cw, cm = torch.cumsum(w, 1), torch.cumsum(wm, 1)
            a, am = cw - w, cm - wm                                  # exclusive prefixes
            b, bm = cw[:, -1:] - cw, cm[:, -1:] - cm                 # exclusive suffixes
            inner = m * (a - b) + (bm - am)
            out.append((w * (inner + w * d / 3.0)).sum(1).mean())
        return out


def _make(variant, a, eager):
    import torch
    from gpu_common import EMB
    from hypernerf_torch_amd.hypernerf.models import NerfModel
    from hypernerf_torch_amd.losses import DistortionLoss
    from hypernerf_torch_amd.training import TrainStep
    torch.manual_seed(0)
    m = NerfModel(EMB, n_samples_coarse=64, n_samples_fine=64, noise_std=1.0, view_fourier_dim=6,
                  hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True).to(DEV)
    levels = tuple(a.levels)
    term = {"off": None, "hip": DistortionLoss(weight=a.weight, levels=levels), "torch": TorchHead(a.weight, levels)}[variant]
    return TrainStep(m, lr=5e-4, use_graph=not eager, distortion_loss=term)


def run(a):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import hashprng as H
    import hypernerf_torch_amd as HN
    from gpu_common import rays_for
    HN.set_precision("bf16")
    b = 1024
    o, d, idx = rays_for(3, b)
    rays = torch.cat([o, d, torch.zeros(b, 1), torch.ones(b, 1), idx.float()[:, None]], dim=1).to(DEV)
    rgbs = H.uniform(3, "rgbs", (b, 3), 0.1, 0.9).to(DEV)
    workload = "NerfModel use_warp bendy_sheet nerf_embed+alpha_cond, 1024 rays x (64+64), bf16"
    if a.eager:
        ts = _make(a.eager, a, True)
        for _ in range(a.warmup + a.steps):
            log = ts.step(rays, rgbs)
        torch.cuda.synchronize()
        return {"part": "eager", "variant": a.eager, "steps": a.warmup + a.steps, "loss": float(log["train/loss"]),
                "workload": workload}
    steps = {v: _make(v, a, False) for v in VARIANTS}
    logs = {}
    for v, ts in steps.items():
        for _ in range(a.warmup):
            logs[v] = ts.step(rays, rgbs)
    torch.cuda.synchronize()
    ms = {v: [] for v in VARIANTS}
    for r in range(a.rounds):
        order = VARIANTS if r % 2 == 0 else VARIANTS[::-1]
        for v in order:
            ts = steps[v]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                logs[v] = ts.step(rays, rgbs)
            torch.cuda.synchronize()
            ms[v].append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {"part": "steps", "levels": list(a.levels), "weight": a.weight, "rounds": a.rounds, "steps": a.steps,
           "warmup": a.warmup, "workload": workload}
    for v in VARIANTS:
        out[v] = {"median_ms": statistics.median(ms[v]), "min_ms": min(ms[v]), "max_ms": max(ms[v]),
                  "loss": float(logs[v]["train/loss"]),
                  "distortion": float(logs[v]["train/distortion_loss"]) if "train/distortion_loss" in logs[v] else None}
    out["hip_minus_off_us"] = (out["hip"]["median_ms"] - out["off"]["median_ms"]) * 1e3
    out["torch_minus_off_us"] = (out["torch"]["median_ms"] - out["off"]["median_ms"]) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", nargs="+", default=["fine"], choices=["coarse", "fine"])
    ap.add_argument("--weight", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--eager", choices=VARIANTS, default=None, help="eager steps of one variant (for a kernel trace)")
    ap.add_argument("--summarise", metavar="CSV", default=None)
    a = ap.parse_args()
    print(json.dumps(summarise(a.summarise) if a.summarise else run(a)))


if __name__ == "__main__":
    main()
