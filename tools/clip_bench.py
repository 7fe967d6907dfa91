"""What gradient clipping (TrainStep(clip_grad_norm=, clip_grad_value=); hn_grad_norm / hn_grad_scale) costs per step at
config 2 (1024 rays x (64+64), bf16, one captured graph per step), one JSON line per process:

  python tools/clip_bench.py --variant off            # no keywords: the default step
  python tools/clip_bench.py --variant norm_inf       # clip_grad_norm=inf: the norm launch only ('train/grad_norm')
  python tools/clip_bench.py --variant norm           # an always-active clip_grad_norm: both launches, full pass
  python tools/clip_bench.py --variant value_norm     # clip_grad_value + clip_grad_norm, both always active
  python tools/clip_bench.py --variant off --tree DIR # the default step of ANOTHER checkout (the parent commit's tree with
                                                      # its own built library): the package is imported from DIR
  python tools/clip_bench.py --variant value_norm --eager --steps 60
                                                      # eager steps, for a run of its own under
                                                      # rocprofv3 --kernel-trace --output-format csv
  python tools/clip_bench.py --summarise kernel_trace.csv     # medians of the two kernels in such a trace

Run the variants as processes of their own, alternating, on one box.  Times are host wall clock around
`--steps` steps that end in a device synchronise, after `--warmup` steps; the rays are fixed and seeded."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ACTIVE_NORM, ACTIVE_VALUE = 1e-3, 1e-4      # far below the gradients of an untrained model: the clips always bite
VARIANTS = {"off": {}, "norm_inf": dict(clip_grad_norm=float("inf")), "norm": dict(clip_grad_norm=ACTIVE_NORM),
            "value_norm": dict(clip_grad_norm=ACTIVE_NORM, clip_grad_value=ACTIVE_VALUE)}
KERNELS = ("hn_grad_norm_kernel", "hn_grad_scale_kernel")


def summarise(path):
    """Median duration per kernel of KERNELS in a rocprofv3 --kernel-trace CSV."""
    times = {k: [] for k in KERNELS}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if row["Kernel_Name"].startswith(k):
                    times[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    return {"part": "kernel", "trace": os.path.basename(path),
            "kernels": {k: {"launches": len(v), "median_us": statistics.median(v) if v else None,
                            "min_us": min(v) if v else None, "max_us": max(v) if v else None} for k, v in times.items()}}


def run(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(ROOT, "tests")]
    import torch
    import hashprng as H
    import hypernerf_torch_amd as HN
    from gpu_common import EMB, rays_for
    from hypernerf_torch_amd.hypernerf.models import NerfModel
    from hypernerf_torch_amd.training import TrainStep
    assert os.path.abspath(HN.__file__).startswith(tree), (HN.__file__, tree)
    HN.set_precision("bf16")
    torch.manual_seed(0)
    m = NerfModel(EMB, n_samples_coarse=64, n_samples_fine=64, noise_std=1.0, view_fourier_dim=6,
                  hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True, use_alpha_cond=True).to(DEV)
    ts = TrainStep(m, lr=5e-4, use_graph=not a.eager, **VARIANTS[a.variant])
    b = 1024
    o, d, idx = rays_for(3, b)
    rays = torch.cat([o, d, torch.zeros(b, 1), torch.ones(b, 1), idx.float()[:, None]], dim=1).to(DEV)
    rgbs = H.uniform(3, "rgbs", (b, 3), 0.1, 0.9).to(DEV)
    for _ in range(a.warmup):
        log = ts.step(rays, rgbs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        log = ts.step(rays, rgbs)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    clip = getattr(ts, "clip", None)
    out = {"part": "steps", "variant": a.variant, "tree": os.path.relpath(tree, ROOT), "graph": not a.eager,
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt * 1e3, "arena_floats": ts.arena.numel,
           "loss": float(log["train/loss"]),
           "grad_norm": float(log["train/grad_norm"]) if "train/grad_norm" in log else None,
           "coef": float(clip.coef) if clip is not None else None,
           "workload": "NerfModel use_warp bendy_sheet nerf_embed+alpha_cond, 1024 rays x (64+64), bf16"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="off")
    ap.add_argument("--tree", default=ROOT, help="checkout to import the package (and its built library) from")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--eager", action="store_true", help="launch every kernel eagerly (for a kernel trace)")
    ap.add_argument("--summarise", metavar="CSV", default=None)
    a = ap.parse_args()
    print(json.dumps(summarise(a.summarise) if a.summarise else run(a)))


if __name__ == "__main__":
    main()
