"""GPU test (MI355X) of what one NerfModel training pass launches on each of its paths: the entry points and tags of one
forward + backward under a ParamArena, in order, against the lists the model launched before its host side was
rearranged (tests/test_nerfmodel_host.py pins the same plans on the CPU, through stubs)."""
import pytest
import torch

import hashprng as H
import hypernerf_torch_amd as HN
from gpu_common import DEV, rays_for
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.hypernerf import models
from test_gpu_geometry import QUERY_CASES, small_model

pytestmark = pytest.mark.gpu

# path -> (case of QUERY_CASES, rays, Nc = Nf, NerfModel.REUSE_COARSE, metadata_encoded)
PLANS = {
    "fused_reuse": ("bendy_fused", 12, 8, True, False),
    "fused_noreuse": ("bendy_fused", 12, 8, False, False),
    "se3_outside": ("se3_axis", 12, 8, True, False),
    "networks": ("bendy_fused", 12, 8, True, True),
    # the in-machine GLO gradient reduction needs a multiple of 32 samples per ray; 9 rays leave a partly filled block
    "fused_reuse_9x32": ("bendy_fused", 9, 32, True, False),
}

# taken from a run of the commit before the rearrangement (the same lists in fp32 and bf16 mode)
EXPECTED = {
    "fused_reuse": [
        "hn_pack_units_multi[level_coarse+level_fine+template_fine_reuse]", "hn_sample_along_rays",
        "hn_mlp_forward[level_coarse]", "hn_composite_sample_pdf", "hn_mlp_forward[template_fine_reuse]",
        "hn_mlp_forward[level_fine]", "hn_composite_forward", "hn_composite_backward",
        "hn_mlp_backward[level_fine]", "hn_embed_backward", "hn_embed_backward", "hn_embed_backward",
        "hn_mlp_backward[template_fine_reuse]", "hn_embed_backward", "hn_embed_backward",
        "hn_composite_backward", "hn_mlp_backward[level_coarse]", "hn_embed_backward", "hn_embed_backward",
        "hn_embed_backward", "hn_mlp_wgrad_batched_t[batched]", "hn_mlp_wgrad_reduce"
    ],
    "fused_noreuse": [
        "hn_pack_units_multi[level_coarse+level_fine]", "hn_sample_along_rays", "hn_mlp_forward[level_coarse]",
        "hn_composite_sample_pdf", "hn_mlp_forward[level_fine]", "hn_composite_forward",
        "hn_composite_backward", "hn_mlp_backward[level_fine]", "hn_embed_backward", "hn_embed_backward",
        "hn_embed_backward", "hn_composite_backward", "hn_mlp_backward[level_coarse]", "hn_embed_backward",
        "hn_embed_backward", "hn_embed_backward", "hn_mlp_wgrad_batched_t[batched]", "hn_mlp_wgrad_reduce"
    ],
    "se3_outside": [
        "hn_sample_along_rays", "hn_pack_units[SE3Field]", "hn_mlp_forward[SE3Field]", "hn_se3_warp_forward",
        "hn_pack_units[template_coarse]", "hn_mlp_forward[template_coarse]", "hn_composite_sample_pdf",
        "hn_pack_units[template_fine]", "hn_mlp_forward[template_fine]", "hn_mlp_forward[SE3Field]",
        "hn_se3_warp_forward", "hn_mlp_forward[template_fine]", "hn_composite_forward", "hn_composite_backward",
        "hn_mlp_backward[template_fine]", "hn_embed_backward", "hn_embed_backward", "hn_se3_warp_backward",
        "hn_mlp_backward[SE3Field]", "hn_mlp_backward[template_fine]", "hn_embed_backward", "hn_embed_backward",
        "hn_composite_backward", "hn_mlp_backward[template_coarse]", "hn_embed_backward", "hn_embed_backward",
        "hn_se3_warp_backward", "hn_mlp_backward[SE3Field]", "hn_mlp_wgrad_batched_t[batched]",
        "hn_mlp_wgrad_reduce"
    ],
    "networks": [
        "hn_embed_gather", "hn_sample_along_rays", "hn_pack_units[TranslationField]",
        "hn_mlp_forward[TranslationField]", "hn_pack_units[HyperSheetMLP]", "hn_mlp_forward[HyperSheetMLP]",
        "hn_pack_units[template_coarse]", "hn_mlp_forward[template_coarse]", "hn_composite_sample_pdf",
        "hn_mlp_forward[TranslationField]", "hn_mlp_forward[HyperSheetMLP]", "hn_pack_units[template_fine]",
        "hn_mlp_forward[template_fine]", "hn_composite_forward", "hn_composite_backward",
        "hn_mlp_backward[template_fine]", "hn_embed_backward", "hn_mlp_backward[HyperSheetMLP]",
        "hn_embed_backward", "hn_mlp_backward[TranslationField]", "hn_embed_backward", "hn_composite_backward",
        "hn_mlp_backward[template_coarse]", "hn_embed_backward", "hn_mlp_backward[HyperSheetMLP]",
        "hn_embed_backward", "hn_mlp_backward[TranslationField]", "hn_embed_backward", "hn_embed_backward",
        "hn_mlp_wgrad_batched_t[batched]", "hn_mlp_wgrad_reduce"
    ],
    "fused_reuse_9x32": [
        "hn_pack_units_multi[level_coarse+level_fine+template_fine_reuse]", "hn_sample_along_rays",
        "hn_mlp_forward[level_coarse]", "hn_composite_sample_pdf", "hn_mlp_forward[template_fine_reuse]",
        "hn_mlp_forward[level_fine]", "hn_composite_forward", "hn_composite_backward",
        "hn_mlp_backward[level_fine]", "hn_mlp_backward[template_fine_reuse]", "hn_composite_backward",
        "hn_mlp_backward[level_coarse]", "hn_mlp_wgrad_batched_t[batched]", "hn_mlp_wgrad_reduce"
    ],
}


@pytest.mark.parametrize("path", sorted(PLANS))
def test_launches_of_one_training_pass(monkeypatch, path):
    case, b, n, reuse, encoded = PLANS[path]
    kw, warp_kind, call = QUERY_CASES[case]
    monkeypatch.setattr(models.NerfModel, "REUSE_COARSE", reuse)
    HN.set_precision("fp32")
    try:
        seed = 151
        m, _ = small_model(kw, warp_kind, seed, n, n)
        arena = HN.ParamArena(m.parameters())
        arena.zero_grad()
        o, d, _ = rays_for(seed, b)
        idx = ((torch.arange(b, dtype=torch.int64) * 7 + 3) % 100).to(DEV)        # one ray per frame id
        rays = {"origins": o.to(DEV), "directions": d.to(DEV), "viewdirs": None,
                "metadata": {k: idx for k in ("warp", "camera", "appearance", "time")}}
        rng = {"t_rand": H.uniform(seed, "t", (b, n), 0, 1).to(DEV), "u": H.uniform(seed, "u", (b, n), 0, 1).to(DEV),
               "noise_coarse": (H.normal(seed, "n1", (b, n, 1)) * 0.7).to(DEV),
               "noise_fine": (H.normal(seed, "n2", (b, 2 * n, 1)) * 0.7).to(DEV)}
        names = []
        launch = L.launch

        def spy(name, *a, tag="", **k):
            names.append(name + (f"[{tag}]" if tag else ""))
            return launch(name, *a, tag=tag, **k)

        monkeypatch.setattr(L, "launch", spy)
        fkw = dict(call)
        if encoded:
            row = m.warp_embed(idx)
            rays = dict(rays, metadata={"encoded_warp": row, "encoded_hyper": row, "encoded_nerf": row})
            fkw["metadata_encoded"] = True
        out = m(rays, {}, rng=rng, **fkw)
        loss = ((out["coarse"]["rgb"] ** 2).mean() + (out["fine"]["rgb"] ** 2).mean() + out["fine"]["depth"].mean()
                + (out["fine"]["warped_points"] ** 2).mean())
        loss.backward()
        torch.cuda.synchronize()
        monkeypatch.setattr(L, "launch", launch)
        print(path, names)
        assert names == EXPECTED[path]
        assert m._reused_coarse == {"fused_reuse": "fused", "fused_reuse_9x32": "fused", "se3_outside": "outside"}.get(path)
        assert all(isinstance(c, F.ProgramCall) for c in m._template_calls.values())
        assert torch.isfinite(arena.grad).all() and float(arena.grad.abs().max()) > 0
    finally:
        HN.set_precision("bf16")
