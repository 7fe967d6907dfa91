#!/usr/bin/env python3
"""Golden vectors of the hidden / wide-output activations beyond ReLU: LeakyReLU, ELU, Softplus.

Imports the REFERENCE exactly as make_golden.py does (it IS imported: same shims, same load_hash_weights, same seeded
draw stream) and writes tests/golden/g18_activations.npz.  Run in the build container only:

    python tests/golden/make_act_golden.py

Recorded, per activation (defaults and LeakyReLU(0.2), ELU(0.7), Softplus(beta=2, threshold=5)):
  * reference modules.MLP with that hidden activation (skip connection included) and, separately, as the output
    activation of a wide (40-column) MLP: output, input gradient and every weight gradient (grad_summary) under the
    fixed loss sum(y * wy), wy a hashed uniform tensor.  The input rows include large-magnitude points (pre-activations
    past the Softplus threshold, far negative for ELU) and all-zero points with a zero first-layer bias (pre-activation
    exactly 0 for LeakyReLU);
  * a TranslationField(activation=Softplus()), a NerfMLP(hidden_activation=ELU()) and one bendy-sheet NerfModel (8+8
    samples, as g11) whose warp field / template MLPs are those two modules, with outputs, loss and gradients.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402  (the reference import, shims and helpers)

H = G.H
nn = torch.nn

ACTS = {
    "leaky_def": lambda: nn.LeakyReLU(),
    "leaky": lambda: nn.LeakyReLU(0.2),
    "elu_def": lambda: nn.ELU(),
    "elu": lambda: nn.ELU(0.7),
    "sp_def": lambda: nn.Softplus(),
    "sp": lambda: nn.Softplus(beta=2, threshold=5),
}
# hidden: depth 4, width 64, skip after layer 2; wide output: 40 columns
MLP_HIDDEN = dict(in_ch=20, out_ch=3, depth=4, width=64, skips=[2])
MLP_WIDE = dict(in_ch=20, out_ch=40, depth=2, width=64, skips=[])
N_POINTS = 100          # not a multiple of 32


def mlp_inputs(tag):
    """(N_POINTS, 20): moderate rows, rows scaled x 25 (far past every threshold, both signs) and all-zero rows."""
    x = H.uniform(18, "act_x_" + tag, (N_POINTS, 20), -1.0, 1.0)
    x[60:80] *= 25.0
    x[80:88] = 0.0
    return x


def prepare_mlp(m, tag):
    """Hashed weights (seed 18); linears.0.bias zeroed so that the zero rows reach z == 0 exactly."""
    G.load_hash_weights(m, 18)
    with torch.no_grad():
        m.linears[0].bias.zero_()


def g_mlps(arrs):
    for act_name, make in ACTS.items():
        for kind, kw in (("hidden", MLP_HIDDEN), ("wide", MLP_WIDE)):
            tag = f"{kind}_{act_name}"
            kw = dict(kw)
            if kind == "hidden":
                kw["hidden_activation"] = make()
            else:
                kw["output_activation"] = make()
            m = G.R_mod.MLP(**kw)
            prepare_mlp(m, tag)
            x = mlp_inputs(tag).requires_grad_(True)
            y = m(x)
            wy = H.uniform(18, "act_wy_" + tag, tuple(y.shape), -1.0, 1.0)
            (y * wy).sum().backward()
            arrs[f"{tag}/x"] = x.detach()
            arrs[f"{tag}/y"] = y.detach()
            arrs[f"{tag}/wy"] = wy
            arrs[f"{tag}/dx"] = x.grad
            arrs.update({f"{tag}/grad/{k}": v for k, v in G.grad_summary(m.named_parameters(), 18).items()})


def g_fields(arrs):
    # TranslationField(activation=Softplus()): points (B, S, 3), metadata (B, S, 8)
    tf = G.R_warp.TranslationField(in_ch=3, in_ch_embed=8, activation=nn.Softplus())
    G.load_hash_weights(tf, 19)
    pts = H.uniform(19, "tf_pts", (4, 16, 3), -1.5, 1.5).requires_grad_(True)
    meta = H.uniform(19, "tf_meta", (4, 16, 8), -0.5, 0.5).requires_grad_(True)
    out = tf(pts, meta, {"warp_alpha": None})
    y = out["warped_points"] if isinstance(out, dict) else out
    wy = H.uniform(19, "tf_wy", tuple(y.shape), -1.0, 1.0)
    (y * wy).sum().backward()
    arrs.update({"tf/pts": pts.detach(), "tf/meta": meta.detach(), "tf/y": y.detach(), "tf/wy": wy,
                 "tf/dpts": pts.grad, "tf/dmeta": meta.grad})
    arrs.update({f"tf/grad/{k}": v for k, v in G.grad_summary(tf.named_parameters(), 19).items()})

    # NerfMLP(hidden_activation=ELU()) with alpha / rgb conditions, trunk_width 256 (the trunk's output ELU included)
    nm = G.R_mod.NerfMLP(in_ch=27, trunk_depth=3, trunk_width=256, rgb_branch_depth=1, rgb_branch_width=128,
                         hidden_activation=nn.ELU(), skips=[1], alpha_condition_dim=8, rgb_condition_dim=12,
                         rgb_activation=nn.Sigmoid())
    G.load_hash_weights(nm, 20)
    x = H.uniform(20, "nm_x", (4, 16, 27), -2.0, 2.0).requires_grad_(True)
    ac = H.uniform(20, "nm_ac", (4, 8), -1.0, 1.0)
    rc = H.uniform(20, "nm_rc", (4, 12), -1.0, 1.0)
    out = nm(x, ac, rc)
    wr = H.uniform(20, "nm_wr", tuple(out["rgb"].shape), -1.0, 1.0)
    wa = H.uniform(20, "nm_wa", tuple(out["alpha"].shape), -1.0, 1.0)
    ((out["rgb"] * wr).sum() + (out["alpha"] * wa).sum()).backward()
    arrs.update({"nm/x": x.detach(), "nm/ac": ac, "nm/rc": rc, "nm/rgb": out["rgb"].detach(),
                 "nm/alpha": out["alpha"].detach(), "nm/wr": wr, "nm/wa": wa, "nm/dx": x.grad})
    arrs.update({f"nm/grad/{k}": v for k, v in G.grad_summary(nm.named_parameters(), 20).items()})


def swap_model_modules(m, mod, warp, glo_dim):
    """warp_field -> TranslationField(Softplus), nerf_mlps_* -> NerfMLP(ELU) with the model's own shapes."""
    m.warp_field = warp.TranslationField(in_ch=3, in_ch_embed=glo_dim, activation=nn.Softplus())
    for lvl in ("coarse", "fine"):
        old = getattr(m, f"nerf_mlps_{lvl}")
        new = mod.NerfMLP(in_ch=old.in_ch, trunk_depth=old.trunk_depth, trunk_width=old.trunk_width,
                          rgb_branch_depth=old.rgb_branch_depth, rgb_branch_width=old.rgb_branch_width,
                          hidden_activation=nn.ELU(), skips=old.skips, alpha_channels=old.alpha_channels,
                          rgb_channels=old.rgb_channels, rgb_activation=nn.Sigmoid(),
                          alpha_condition_dim=old.alpha_condition_dim, rgb_condition_dim=old.rgb_condition_dim)
        setattr(m, f"nerf_mlps_{lvl}", new)


MODEL_KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=False, use_alpha_cond=False)


def g_model(arrs):
    b, nc, nf, seed = 16, 8, 8, 100
    m = G.R_models.NerfModel(G.EMB, near=0.0, far=1.0, n_samples_coarse=nc, n_samples_fine=nf, noise_std=None,
                             view_fourier_dim=6, **MODEL_KW)
    swap_model_modules(m, G.R_mod, G.R_warp, m.GLO_dim if hasattr(m, "GLO_dim") else 8)
    G.load_hash_weights(m, seed)
    o, d, idx = G.rays_for(seed, b)
    gt = H.uniform(seed, "gt", (b, 3), 0.0, 1.0)
    rays = {"origins": o, "directions": d, "viewdirs": None,
            "metadata": {k: idx.clone() for k in ("warp", "camera", "appearance", "time")}}
    extra = {"nerf_alpha": None, "warp_alpha": None, "hyper_alpha": None, "hyper_sheet_alpha": None}
    dseed = seed
    while True:
        for prm in m.parameters():
            prm.grad = None
        with G.DrawRecorder(dseed) as rec:
            out = m(rays, extra)
        wmid = out["coarse"]["weights"][..., 1:-1].detach() + 1e-5
        pdf = wmid / torch.sum(wmid, -1, keepdim=True)
        cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
        u = [t for (k, s, t) in rec.log if k == "rand"][1]
        if G.tie_margin(cdf, u) > 1e-5:
            break
        dseed += 1000
    loss = G.R_losses.MSELoss()(out, gt)
    loss.backward()
    arrs.update({"model/seed": seed, "model/draw_seed": dseed, "model/b": b, "model/nc": nc, "model/nf": nf,
                 "model/loss": loss.detach()})
    for i, (k, s, t) in enumerate(rec.log):
        arrs[f"model/draw{i}_{k}"] = t
    for lvl in ("coarse", "fine"):
        for k in ("rgb", "depth", "acc", "weights"):
            if k in out[lvl]:
                arrs[f"model/{lvl}/{k}"] = out[lvl][k]
    arrs["model/keys"] = np.array(sorted(m.state_dict().keys()))
    arrs.update({"model/grad/" + k: v for k, v in G.grad_summary(m.named_parameters(), seed).items()})


if __name__ == "__main__":
    arrs = {}
    g_mlps(arrs)
    g_fields(arrs)
    g_model(arrs)
    G.save("g18_activations", **arrs)
