#!/usr/bin/env python3
"""Golden vectors of LONG rays: the per-ray kernels' sizes between 256 and their 512-sample limit.

Imports the REFERENCE exactly as make_golden.py does (it IS imported: same shims, same load_hash_weights, same seeded
draw stream) and writes tests/golden/g19_long_rays.npz.  Run in the build container only:

    python tests/golden/make_long_rays_golden.py

Recorded:
  * comp/S{S}/...: volumetric_rendering and compute_depth_index at S in {256, 257, 384, 512} samples, every
    combination of sample_at_infinity and white background.  Ray 0 is all-transparent, ray 1 opaque at its first
    sample, rays 2..5 carry density only from sample k on (k in the last segments of 64: the median crossing falls in
    segment 5 or later where the ray has one), rays 6..7 are dense everywhere;
  * pdf/nc{nc}/...: piecewise_constant_pdf and sample_pdf in the fused shape (bins = midpoints of z, weights =
    columns 1..nc-2) at nc in {256, 257} with nf = 512 - nc; every u lies more than 1e-5 from every cdf entry
    (tie_margin, as g10).  Ray 0 has all-zero weights, ray 1 one-hot;
  * model/...: one bendy_cond NerfModel (as g11) at 257 + 255 samples and 4 rays: outputs, loss and gradient
    summaries, the draws with the fine draws `u` kept clear of the coarse cdf by the same margin.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402  (the reference import, shims and helpers)

H = G.H
COMP_S = (256, 257, 384, 512)
PDF_NC = (256, 257)
MARGIN = 1e-5


def comp_inputs(s):
    seed = 1900 + s
    b = 8
    o, d, _ = G.rays_for(seed, b)
    rgb = H.uniform(seed, "lr_rgb", (b, s, 3), 0.0, 1.0)
    sigma = H.uniform(seed, "lr_sig", (b, s), 0.0, 6.0)
    z, _ = torch.sort(H.uniform(seed, "lr_z", (b, s), 0.0, 1.0), dim=-1)
    sigma[0] = 0.0                                        # all-transparent
    sigma[1] = 0.0
    sigma[1, 0] = 1e4                                     # opaque at the first sample
    for r, k in zip(range(2, 6), (s - 1, s - 20, max(s - 64, s // 2), s // 2 + 1)):
        sigma[r, :k] = 0.0                                # density only from sample k on
        sigma[r, k:] *= 40.0
    return b, o, d, rgb, sigma, z


def g_comp(arrs):
    for s in COMP_S:
        b, o, d, rgb, sigma, z = comp_inputs(s)
        pre = f"comp/S{s}/"
        arrs.update({pre + "rgb": rgb, pre + "sigma": sigma, pre + "z": z, pre + "d": d})
        for inf in (True, False):
            for wb in (True, False):
                r = G.R_mu.volumetric_rendering(rgb, sigma, z, d, use_white_background=wb, sample_at_infinity=inf)
                tag = f"{pre}inf{int(inf)}_wb{int(wb)}/"
                for k, v in r.items():
                    arrs[tag + k] = v
                arrs[tag + "dindex"] = G.R_mu.compute_depth_index(r["weights"])


def ref_cdf(w):
    """The reference's cdf of bin weights w (model_utils.py:177-180), to keep every u clear of it."""
    ww = w + 1e-5
    pdf = ww / torch.sum(ww, -1, keepdim=True)
    return torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)


def clear_draws(seed, tag, cdf, nf):
    """(B, nf) uniform draws, each more than MARGIN from every cdf entry of its ray (redrawn from the hash stream)."""
    u = H.uniform(seed, tag, (cdf.shape[0], nf), 0.0, 1.0)
    for it in range(100):
        bad = (u[:, :, None] - cdf[:, None, :]).abs().min(-1).values <= MARGIN
        if not bool(bad.any()):
            break
        u = torch.where(bad, H.uniform(seed, f"{tag}_redraw{it}", tuple(u.shape), 0.0, 1.0), u)
    assert G.tie_margin(cdf, u) > MARGIN
    return u


class FixedDraws(G.DrawRecorder):
    """A DrawRecorder whose uniform draw number `i` is the given tensor (a u kept clear of the cdf)."""

    def __init__(self, seed, fixed):
        super().__init__(seed)
        self.fixed = fixed

    def rand(self, *args, **kw):
        if self.n in self.fixed:
            shp = self._shape(args)
            t = self.fixed[self.n]
            assert tuple(t.shape) == shp, (t.shape, shp)
            self.log.append(("rand", shp, t)); self.n += 1
            return t
        return super().rand(*args, **kw)


def g_pdf(arrs):
    for nc in PDF_NC:
        nf = 512 - nc
        seed, b = 1950 + nc, 6
        o, d, _ = G.rays_for(seed, b)
        z, _ = torch.sort(H.uniform(seed, "lp_z", (b, nc), 0.0, 1.0), dim=-1)
        w = H.uniform(seed, "lp_w", (b, nc), 0.0, 1.0) ** 3
        w[0] = 0.0                                        # all-zero weights
        w[1] = 0.0
        w[1, nc // 2] = 1.0                               # one-hot
        mid = 0.5 * (z[:, 1:] + z[:, :-1])
        wb = w[:, 1:-1]
        cdf = ref_cdf(wb)
        u = clear_draws(seed, "lp_u", cdf, nf)
        with FixedDraws(seed, {0: u}):
            zs = G.R_mu.piecewise_constant_pdf(mid, wb, nf, True)
        with FixedDraws(seed, {0: u}):
            z_all, pts = G.R_mu.sample_pdf(mid, wb, o, d, z, nf, True)
        pre = f"pdf/nc{nc}/"
        arrs.update({pre + "z": z, pre + "w": w, pre + "o": o, pre + "d": d, pre + "u": u,
                     pre + "inds": torch.searchsorted(cdf, u.contiguous(), right=True), pre + "z_samples": zs,
                     pre + "z_all": z_all, pre + "pts": pts})


def g_model(arrs):
    case, nc, nf, b, seed = "bendy_cond", 257, 255, 4, 1990
    m = G.R_models.NerfModel(G.EMB, near=0.0, far=1.0, n_samples_coarse=nc, n_samples_fine=nf, noise_std=None,
                             view_fourier_dim=6, **G.MODEL_CASES[case])
    G.load_hash_weights(m, seed)
    o, d, idx = G.rays_for(seed, b)
    gt = H.uniform(seed, "gt", (b, 3), 0.0, 1.0)
    rays = {"origins": o, "directions": d, "viewdirs": None,
            "metadata": {k: idx.clone() for k in ("warp", "camera", "appearance", "time")}}
    extra = {"nerf_alpha": None, "warp_alpha": None, "hyper_alpha": None, "hyper_sheet_alpha": None}
    # first pass: the coarse weights (they do not depend on u); second pass with u clear of their cdf
    with torch.no_grad(), G.DrawRecorder(seed):
        first = m(rays, extra)
    cdf = ref_cdf(first["coarse"]["weights"][..., 1:-1])
    u = clear_draws(seed, "lm_u", cdf, nf)
    with FixedDraws(seed, {1: u}) as rec:
        out = m(rays, extra)
    assert torch.equal(out["coarse"]["weights"].detach(), first["coarse"]["weights"])
    loss = G.R_losses.MSELoss()(out, gt)
    loss.backward()
    arrs.update({"model/seed": seed, "model/b": b, "model/nc": nc, "model/nf": nf, "model/noise_std": 0.0,
                 "model/loss": loss.detach(),
                 "model/draw_kinds": np.array([k for (k, s, t) in rec.log])})
    for i, (k, s, t) in enumerate(rec.log):
        arrs[f"model/draw{i}"] = t
    for lvl in ("coarse", "fine"):
        for k, v in out[lvl].items():
            arrs[f"model/{lvl}/{k}"] = v
    arrs["model/fine/inds"] = torch.searchsorted(cdf, u.contiguous(), right=True)
    arrs["model/keys"] = np.array(sorted(m.state_dict().keys()))
    arrs["model/shapes"] = np.array([str(tuple(m.state_dict()[k].shape)) for k in sorted(m.state_dict().keys())])
    arrs.update({"model/grad/" + k: v for k, v in G.grad_summary(m.named_parameters(), seed).items()})


if __name__ == "__main__":
    arrs = {}
    g_comp(arrs)
    g_pdf(arrs)
    g_model(arrs)
    G.save("g19_long_rays", **arrs)
