"""What a smooth hidden activation costs at BASELINE config 2 (NerfModel use_warp + bendy_sheet, 1024 rays x (64+64),
bf16): one eager training step (forward + loss + backward, Adam excluded) with the reference's ReLU networks against the
same model whose warp field and template MLPs run Softplus (or another activation).  Prints one JSON line.

    python tools/act_cost.py [--act softplus|elu|leaky_relu|relu] [--steps 20] [--warmup 5]

Under `rocprofv3 --kernel-trace --stats -- python tools/act_cost.py --act softplus --only` the per-kernel times of
the variant alone come out of the trace."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import hashprng as H  # noqa: E402
import hypernerf_torch_amd as HN  # noqa: E402
from gpu_common import EMB, load_hash, rays_for  # noqa: E402
from hypernerf_torch_amd.hypernerf import models, modules, warping  # noqa: E402

ACTS = {"relu": None, "softplus": torch.nn.Softplus, "elu": torch.nn.ELU, "leaky_relu": torch.nn.LeakyReLU}


def build(act: str, nc: int, nf: int):
    torch.manual_seed(0)
    m = models.NerfModel(EMB, near=0.0, far=1.0, n_samples_coarse=nc, n_samples_fine=nf, noise_std=None,
                         view_fourier_dim=6, hyper_slice_method="bendy_sheet", use_warp=True, use_nerf_embed=True,
                         use_alpha_cond=True)
    if ACTS[act] is not None:
        make = ACTS[act]
        m.warp_field = warping.TranslationField(in_ch=3, in_ch_embed=m.warp_field.embed_dim
                                                if hasattr(m.warp_field, "embed_dim") else 8, activation=make())
        for lvl in ("coarse", "fine"):
            old = getattr(m, f"nerf_mlps_{lvl}")
            setattr(m, f"nerf_mlps_{lvl}", modules.NerfMLP(
                in_ch=old.in_ch, trunk_depth=old.trunk_depth, trunk_width=old.trunk_width,
                rgb_branch_depth=old.rgb_branch_depth, rgb_branch_width=old.rgb_branch_width, hidden_activation=make(),
                skips=old.skips, alpha_channels=old.alpha_channels, rgb_channels=old.rgb_channels,
                rgb_activation=torch.nn.Sigmoid(), alpha_condition_dim=old.alpha_condition_dim,
                rgb_condition_dim=old.rgb_condition_dim))
    load_hash(m, 7)
    return m.to("cuda:0")


def time_steps(m, b, nc, nf, steps, warmup):
    o, d, idx = rays_for(3, b)
    rays = {"origins": o.cuda(), "directions": d.cuda(), "viewdirs": None,
            "metadata": {k: idx.cuda() for k in ("warp", "camera", "appearance", "time")}}
    rng = {"t_rand": H.uniform(3, "t", (b, nc), 0, 1).cuda(), "u": H.uniform(3, "u", (b, nf), 0, 1).cuda()}
    gt = H.uniform(3, "gt", (b, 3), 0, 1).cuda()
    ts = []
    for i in range(warmup + steps):
        for p in m.parameters():
            p.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m(rays, {}, rng=rng)
        loss = ((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()
        loss.backward()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--act", default="softplus", choices=sorted(ACTS))
    ap.add_argument("--only", action="store_true", help="time the variant alone (no ReLU run)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1024)
    a = ap.parse_args()
    HN.set_precision("bf16")
    nc = nf = 64
    res = {"workload": "config-2 eager train step (fwd+loss+bwd)", "rays": a.rays, "nc": nc, "nf": nf,
           "precision": "bf16", "statistic": f"median of {a.steps} steps after {a.warmup} warm-up"}
    for act in ([a.act] if a.only else ["relu", a.act]):
        ms, loss = time_steps(build(act, nc, nf), a.rays, nc, nf, a.steps, a.warmup)
        res[f"ms_{act}"] = round(ms, 4)
        res[f"loss_{act}"] = loss
    if not a.only:
        res["ratio"] = round(res[f"ms_{a.act}"] / res["ms_relu"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
