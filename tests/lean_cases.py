"""The cases of test_gpu_lean_builds.py, run in a child process of their own:  python lean_cases.py OUT.npz

Every case runs the bf16 machine forward and backward on seeded inputs and records forward outputs, source gradients,
every weight and bias gradient and (the model cases) the GLO tables' gradients.  Parameters live in a ParamArena: its
weight gradients go through the fixed-order partial-slab reduction and are reproducible bit for bit (without an arena
the jobs of a weight-gradient launch add with float atomics, in whatever order they finish).  The parent test runs this file twice,
once as it is and once under HN_FORCE_GENERIC=1, and compares the two files byte for byte.  Each program also records
whether it announced itself as ReLU-only (HnMlpArgs.wide_ops bit 2), i.e. which kernels its launches took."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import hashprng as H
import hypernerf_torch_amd as HN
from hypernerf_torch_amd import functional as F
from gpu_common import DEV, EMB, load_hash, rays_for
from hypernerf_torch_amd.hypernerf import models, modules, warping

# (points, samples per ray): 33 = one full and one partly filled block of a workgroup whose other waves idle;
# 288 = two workgroup tiles (a second ws.start()) of rays of 32 samples
SIZES = ((33, 1), (288, 32))


def field_case(out, tag, make, seed):
    """A stand-alone field: points and embedding differentiated.  33 points with a per-point embedding, 288 points as
    9 rays x 32 samples with a per-ray embedding."""
    for n, s in SIZES:
        m = make()
        load_hash(m, seed)
        m = m.to(DEV)
        arena = HN.ParamArena(m.parameters())
        arena.zero_grad()
        pts = H.uniform(seed, "p", (n, 3), -1, 1)
        emb = H.uniform(seed, "e", (n // s, 8), -1, 1)
        if s > 1:
            pts = pts.reshape(n // s, s, 3)
        pts, emb = pts.to(DEV).requires_grad_(True), emb.to(DEV).requires_grad_(True)
        y = m.warp(pts, emb, {"warp_alpha": None}) if hasattr(m, "warp") else m(pts, emb)
        wy = H.uniform(seed, "wy", tuple(y.shape), -1, 1).to(DEV)
        F.backward((y * wy).sum())
        torch.cuda.synchronize()
        key = f"{tag}/n{n}"
        out[key + "/y"], out[key + "/dpts"], out[key + "/demb"] = y.detach().cpu().numpy(), pts.grad.cpu().numpy(), emb.grad.cpu().numpy()
        for k, prm in m.named_parameters():
            out[f"{key}/grad/{k}"] = prm.grad.cpu().numpy()
        prog = m._call(s > 1, True, True).program
        out[key + "/relu_only_bit"] = np.array(prog.relu_only_bit())
        # the shapes the case is about: four plain 128 -> 128 (or 64 -> 64) layers behind the encoder layer, one skip layer
        out[key + "/widths"] = np.array([ly.nt * 32 for ly in prog.layers])


def model_case(out, seed=5):
    """The fused config-2 level programs (warp field -> hyper sheet -> template, GLO rows gathered in the machine)."""
    kw = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True)
    for b, ns in ((11, 3), (9, 32)):
        m = models.NerfModel(EMB, n_samples_coarse=ns, n_samples_fine=ns, noise_std=None, view_fourier_dim=6, **kw)
        load_hash(m, seed)
        m = m.to(DEV)
        arena = HN.ParamArena(m.parameters())
        arena.zero_grad()
        o, d, idx = rays_for(seed, b)
        rng = {"t_rand": H.uniform(seed, "t", (b, ns), 0, 1).to(DEV), "u": H.uniform(seed, "u", (b, ns), 0, 1).to(DEV)}
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx.to(DEV) for k in ("warp", "camera", "appearance", "time")}}
        res = m(rays, {}, rng=rng)
        loss = (res["coarse"]["rgb"] ** 2).mean() + (res["fine"]["rgb"] ** 2).mean()
        F.backward(loss)
        torch.cuda.synchronize()
        key = f"model/n{b * ns}"
        for lvl in ("coarse", "fine"):
            out[f"{key}/{lvl}/rgb"] = res[lvl]["rgb"].detach().cpu().numpy()
        for k, prm in m.named_parameters():
            if prm.grad is not None:
                out[f"{key}/grad/{k}"] = prm.grad.cpu().numpy()
        out[key + "/relu_only_bit"] = np.array([m._level_call(lvl).program.relu_only_bit() for lvl in ("coarse", "fine")])


def main(path):
    HN.set_precision("bf16")
    out = {}
    field_case(out, "warp128", lambda: warping.TranslationField(in_ch=3, in_ch_embed=8), 31)
    field_case(out, "sheet64", lambda: modules.HyperSheetMLP(in_ch=3, in_ch_embed=8), 32)
    field_case(out, "leaky128", lambda: warping.TranslationField(in_ch=3, in_ch_embed=8, activation=torch.nn.LeakyReLU(0.2)), 33)
    model_case(out)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
