"""CPU restatement of NerfModel.query_points: the body of the oracle's `_render_level` up to the density, composed from
the oracle's public blocks (glo_embed, translation_field / se3_field, hyper_sheet, posenc_orig, nerf_mlp, softplus,
filter_sigma).  No sampling, no noise, no compositing."""
import torch
import torch.nn.functional as TF

from oracle import hypernerf_oracle as O


def query_points(p, cfg, level, pts, viewdirs, idx, use_warp=True, render_opts=None):
    """p: state dict, cfg: O.ModelCfg, pts (B,S,3), viewdirs (B,3), idx (B,) int64 ->
    {'warped_points': (B,S,3+H), 'rgb': (B,S,3), 'sigma': (B,S), 'alpha': (B,S) the raw density}."""
    use_warp = cfg.use_warp and use_warp
    b, s = pts.shape[:2]
    warp_embed = O.glo_embed(p["warp_embed.embed.weight"], idx) if use_warp else None
    hyper_embed = None
    if cfg.slice != "none":
        hyper_embed = warp_embed if cfg.use_warp else O.glo_embed(p["hyper_embed.embed.weight"], idx)
    we = None if warp_embed is None else warp_embed[:, None, :].expand(b, s, -1)
    he = None if hyper_embed is None else hyper_embed[:, None, :].expand(b, s, -1)
    if not use_warp:
        warped = pts
    else:
        if cfg.warp_kind == "se3":
            spatial = O.se3_field(p, "warp_field", pts)
        else:
            spatial = O.translation_field(p, "warp_field", pts, we)
        if cfg.slice == "axis_aligned_plane":
            hyper = he
        elif cfg.slice == "bendy_sheet":
            hyper = O.hyper_sheet(p, "hyper_sheet_mlp", pts, he)
        else:
            hyper = None
        warped = spatial if hyper is None else torch.cat([spatial, hyper], dim=-1)
    rgb_conds = [O.posenc_orig(viewdirs, cfg.view_f)]
    alpha_conds = []
    if cfg.use_nerf_embed:
        ne = O.glo_embed(p["warp_embed.embed.weight" if cfg.use_warp else "nerf_embed.embed.weight"], idx)
        if cfg.use_alpha_cond:
            alpha_conds.append(ne)
        if cfg.use_rgb_cond:
            rgb_conds.append(ne)
    alpha_cond = torch.cat(alpha_conds, -1) if alpha_conds else None
    feat = O.posenc_orig(warped[..., :3], cfg.xyz_f)
    if warped.shape[-1] > 3:
        feat = torch.cat([feat, O.posenc_orig(warped[..., 3:], cfg.hyper_f)], dim=-1)
    prefix = "nerf_mlps_fine" if level == "fine" else "nerf_mlps_coarse"
    rgb, alpha = O.nerf_mlp(p, prefix, feat, alpha_cond, torch.cat(rgb_conds, -1))
    sigma = O.filter_sigma(pts, TF.softplus(alpha.squeeze(-1)), render_opts)
    return {"warped_points": warped, "rgb": rgb, "sigma": sigma, "alpha": alpha.squeeze(-1)}
