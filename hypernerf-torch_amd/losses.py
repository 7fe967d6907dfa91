"""Loss head and metrics of the reference (losses.py:4-14, metrics.py:4-20) — scalar reductions over (B,3) pixels.

`MSELoss` is one HIP launch forward (both levels, both means, their sum) and one backward (`hn_mse_loss_*`,
functional.mse_loss); the metrics `mse` and `psnr` (logging only, no gradient path in the reference) are torch
one-liners; `ssim` runs kornia's windowed SSIM in HIP (`hn_ssim_*`, ops.metrics.ssim_dssim), differentiable as kornia's;
`ms_ssim` is the five-level multi-scale SSIM the Nerfies / HyperNeRF tables report (`hn_msssim_*`), a metric only;
`lpips` is the third number of those tables, LPIPS v0.1 over a frozen AlexNet or VGG16 (`hn_lpips_*`), a metric only.
`BackgroundLoss` is HyperNeRF's background regularization, a training term that takes the model instead of rendered
rays: static points of the capture through the warp field, pulled back to where they were (`hn_bg_*`).
`DistortionLoss` is Mip-NeRF 360's distortion loss, a training term on the compositing weights of the rendered levels
that discourages floaters (`hn_distortion_*`).
GPU tensors only, like every op of the package."""
from typing import Dict, List, Optional, Sequence

import torch
from torch import nn

from . import functional as F
from .ops import lpips as _lpips_ops
from .ops import metrics


class MSELoss(nn.Module):
    """Sum over the rendered levels of mean((rgb - gt)^2): coarse always, fine when the model produced it."""

    def forward(self, inputs, targets):
        fine = inputs.get('fine')
        return F.mse_loss(inputs['coarse']['rgb'], fine['rgb'] if fine is not None else None, targets)


loss_dict = {'mse': MSELoss}


class BackgroundLoss:
    """HyperNeRF's background regularization (on by default in its configs): a batch of the capture's static background
    points (`NerfiesDataset.background_points`) goes through the warp field under randomly chosen warp embeddings and a
    robust loss pulls warp(p) back to p, so that the photometric loss cannot drag the static background around.  Per call

        i_n, k_n uniform over the M points / the K warp ids     p_n = points[i_n] + noise_std * normal(0, 1)
        w_n = warp_field(p_n, warp_embed(ids[k_n]))[..., :3]    x_n = |w_n - p_n|^2 / scale^2
        loss = mean_n 2 x_n / (x_n + 4)                         (Barron's general loss at alpha = -2, Geman-McClure)

    as four launches around the warp field's own: the draws (functional.random_draws), the sampler (hn_bg_sample), the
    embedding gather, and behind the field the loss head (hn_bg_loss_forward_grad).  Points are drawn WITH replacement
    (upstream walks a shuffled stream): that is what a draw inside a captured graph gives.  The defaults are upstream's.
    `TrainStep(..., background_loss=BackgroundLoss(ds.background_points, ds.warp_ids))` adds `weight` times the term to
    every step."""

    def __init__(self, points: torch.Tensor, warp_ids, batch_size: int = 16384, noise_std: float = 0.001,
                 scale: float = 0.001, weight: float = 1.0):
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
            shape = tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__
            raise ValueError(f"BackgroundLoss: points must be an (M, 3) tensor, got {shape}")
        if points.shape[0] == 0:
            raise ValueError("BackgroundLoss: no background points")
        if int(batch_size) <= 0:
            raise ValueError(f"BackgroundLoss: batch_size must be positive, got {batch_size}")
        if not float(scale) > 0:
            raise ValueError(f"BackgroundLoss: scale must be positive, got {scale}")
        if not float(noise_std) >= 0:
            raise ValueError(f"BackgroundLoss: noise_std must not be negative, got {noise_std}")
        ids = [int(i) for i in (warp_ids.reshape(-1).tolist() if isinstance(warp_ids, torch.Tensor) else warp_ids)]
        if not ids:
            raise ValueError("BackgroundLoss: no warp ids")
        if len(set(ids)) != len(ids) or min(ids) < 0:
            raise ValueError("BackgroundLoss: warp_ids must be distinct and non-negative")
        if points.shape[0] > F.BG_MAX_ROWS or len(ids) > F.BG_MAX_ROWS:
            raise ValueError(f"BackgroundLoss: at most 2^24 points and warp ids (a 24-bit uniform reaches no further), "
                             f"got {points.shape[0]} and {len(ids)}")
        self.points = points.detach().to(torch.float32).contiguous()
        self.warp_ids = torch.tensor(ids, dtype=torch.int64, device=points.device)
        self.max_id = max(ids)
        self.batch_size, self.noise_std, self.scale, self.weight = int(batch_size), float(noise_std), float(scale), float(weight)
        self.last_sample = None       # (points (N, 3), ids (N,)) of the latest call (graph replays overwrite them in place)

    def __call__(self, model, rng: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """The unweighted loss of one fresh batch.  rng = {'bg_u': (batch_size, 2) uniforms, 'bg_n': (batch_size, 3)
        normals} replaces the draw launch (parity runs share the draws with the CPU oracle this way)."""
        if not getattr(model, 'use_warp', False):
            raise ValueError("BackgroundLoss: the model has no warp field (use_warp=False)")
        if self.max_id >= model.warp_embed.num_embeddings:
            raise ValueError(f"BackgroundLoss: warp id {self.max_id} is outside the model's warp embedding table of "
                             f"{model.warp_embed.num_embeddings} rows")
        n = self.batch_size
        if rng is not None:
            u, nrm = rng['bg_u'], rng['bg_n']
            if tuple(u.shape) != (n, 2) or tuple(nrm.shape) != (n, 3):
                raise ValueError(f"BackgroundLoss: rng 'bg_u' ({n}, 2) and 'bg_n' ({n}, 3), got {tuple(u.shape)} and "
                                 f"{tuple(nrm.shape)}")
        else:
            u, nrm = F.random_draws([((n, 2), 'uniform'), ((n, 3), 'normal')], self.points.device)
        p, ids = F.bg_sample(self.points, self.warp_ids, u, nrm, self.noise_std)
        self.last_sample = (p, ids)
        extra = {'nerf_alpha': None, 'warp_alpha': None, 'hyper_alpha': None, 'hyper_sheet_alpha': None}
        warped = model.warp_field.warp(p, model.warp_embed(ids), extra)
        if warped.shape[-1] != 3:         # a field that appends further coordinates: the loss is on the spatial ones
            warped = warped[..., :3]
        return F.bg_loss(warped, p, self.scale)


class DistortionLoss:
    """Mip-NeRF 360's distortion loss (Barron et al. 2022, eq. 15): per ray, with s the depth normalised to [0, 1]
    between near and far, sample i owning the interval up to the next sample (midpoint m_i, width d_i) and the last
    sample a point mass at its own depth,

        L_ray = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i          loss = mean over rays, summed over `levels`

    a penalty on compositing weights that are spread out or split along the ray: what floaters are made of.  The
    weights are the level's `results[level]['weights']`, the depths `model.last_sampling` ('z_coarse', 'z_fine': the
    same sorted order); one launch per level (functional.distortion_loss).  `spacing=None` follows the model
    ('disparity' with use_linear_disparity, else 'linear'); `near` / `far` default to the model's.  weight = 0.01 is the
    paper's lambda.  `TrainStep(..., distortion_loss=DistortionLoss())` adds `weight` times the term to every step."""

    LEVELS = ('coarse', 'fine')

    def __init__(self, weight: float = 0.01, levels: Sequence[str] = ('fine',), spacing: Optional[str] = None,
                 near: Optional[float] = None, far: Optional[float] = None):
        levels = (levels,) if isinstance(levels, str) else tuple(levels)
        if not levels:
            raise ValueError("DistortionLoss: no levels")
        bad = [lv for lv in levels if lv not in self.LEVELS]
        if bad or len(set(levels)) != len(levels):
            raise ValueError(f"DistortionLoss: levels must be distinct names out of {self.LEVELS}, got {levels}")
        if spacing is not None and spacing not in F.SPACINGS:
            raise ValueError(f"DistortionLoss: spacing must be None or one of {F.SPACINGS}, got {spacing!r}")
        if not float(weight) >= 0:
            raise ValueError(f"DistortionLoss: weight must not be negative, got {weight}")
        self.weight, self.levels, self.spacing = float(weight), levels, spacing
        self.near = None if near is None else float(near)
        self.far = None if far is None else float(far)

    def per_level(self, model, results, root: float = 1.0) -> List[torch.Tensor]:
        """The unweighted loss of every level in `levels`, in that order.  `root`: the root gradient the caller will
        back-propagate each of them with (functional.backward_all): the forward launch then writes that gradient."""
        sampling = getattr(model, 'last_sampling', None)
        if sampling is None:
            raise ValueError("DistortionLoss: the model has kept no depths (model.last_sampling: a forward with fine "
                             "samples comes first)")
        spacing = self.spacing or ('disparity' if getattr(model, 'use_linear_disparity', False) else 'linear')
        near = model.near if self.near is None else self.near
        far = model.far if self.far is None else self.far
        out = []
        for level in self.levels:
            if level not in results:
                raise ValueError(f"DistortionLoss: the model rendered no '{level}' level")
            weights, z = results[level]['weights'], sampling['z_' + level]
            if z.shape != weights.shape:
                raise ValueError(f"DistortionLoss: '{level}' weights {tuple(weights.shape)} and depths {tuple(z.shape)} "
                                 f"are not of one forward pass")
            out.append(F.distortion_loss(weights, z, near, far, spacing, root=root))
        return out

    def __call__(self, model, results) -> torch.Tensor:
        """The unweighted sum over `levels` of the model's latest forward pass (`results` = what it returned)."""
        terms = self.per_level(model, results)
        total = terms[0]
        for t in terms[1:]:
            total = total + t
        return total


def mse(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """metrics.py:4-9: squared error, optionally restricted to a boolean mask, mean-reduced unless told otherwise."""
    sq = torch.square(image_pred - image_gt)
    if valid_mask is not None:
        sq = sq[valid_mask]
    return sq.mean() if reduction == 'mean' else sq


def psnr(image_pred, image_gt, valid_mask=None, reduction='mean'):
    """metrics.py:11-13."""
    return -10.0 * torch.log10(mse(image_pred, image_gt, valid_mask, reduction))


def ssim(image_pred, image_gt, reduction='mean'):
    """metrics.py:15-20: 1 - 2 * dssim(pred, gt, window 3), in [-1, 1]; image_pred and image_gt (N, 3, H, W) (the reference
    documents (1, 3, H, W)), any strides.  dssim is kornia's ssim loss (ops.metrics.ssim_dssim, two HIP launches)."""
    return 1 - 2 * metrics.ssim_dssim(image_pred, image_gt, 3, reduction=reduction)


def ms_ssim(image_pred, image_gt, reduction='mean'):
    """Multi-scale SSIM of images in [0, 1] (the NumPy `MultiScaleSSIM` that HyperNeRF's compute_multiscale_ssim restates,
    max_val 1): per image prod_{l<4} cs_l^w_l * ssim_4^w_4 over a five-level pyramid (ops.metrics.msssim_levels), weights
    ops.metrics.MSSSIM_WEIGHTS.  image_pred and image_gt (N, C, H, W) fp32 on the GPU, any strides, any H, W >= 1.
    'none' returns the (N,) values, 'mean' their average.  A negative cs_l or ssim_4 gives NaN, as it does in NumPy.
    A metric only: there is no backward and the result never requires grad."""
    if reduction not in ('mean', 'none'):
        raise ValueError(f"ms_ssim: reduction must be 'mean' or 'none', got {reduction!r}")
    levels = metrics.msssim_levels(image_pred, image_gt)
    with torch.no_grad():
        # scalar exponents: no host-to-device copy, so the product is safe inside a stream capture too
        last = metrics.MSSSIM_LEVELS - 1
        out = levels[:, last, 0].pow(metrics.MSSSIM_WEIGHTS[last])
        for l in range(last):
            out = out * levels[:, l, 1].pow(metrics.MSSSIM_WEIGHTS[l])
    return out.mean() if reduction == 'mean' else out


def load_lpips(net, backbone_path, lin_path=None, device='cuda'):
    """The LPIPS weights of `net` ('alex' or 'vgg') from the user's files, on `device` (ops.lpips.load_lpips_weights):
    a torchvision backbone checkpoint and the lpips package's lin weights, or one saved `lpips.LPIPS(...).state_dict()`.
    Nothing is downloaded.  The result is what `lpips` and `evaluate_images(..., lpips=...)` take."""
    return _lpips_ops.load_lpips_weights(net, backbone_path, lin_path).to(device)


def lpips(image_pred, image_gt, weights, reduction='mean'):
    """LPIPS v0.1 (Zhang et al. 2018; the lpips package with normalize=True, spatial=False, eval mode) of images in
    [0, 1]: the sum of the five layer terms of ops.lpips.lpips_layers.  image_pred and image_gt (N, 3, H, W) fp32 on the
    GPU, any strides, sides of at least ops.lpips.lpips_min_side(weights.net); weights: load_lpips' result on the images'
    device.  'none' returns the (N,) values, 'mean' their average.  A metric only: there is no backward and the result
    never requires grad."""
    if reduction not in ('mean', 'none'):
        raise ValueError(f"lpips: reduction must be 'mean' or 'none', got {reduction!r}")
    layers = _lpips_ops.lpips_layers(image_pred, image_gt, weights)
    with torch.no_grad():
        out = layers[:, 0]
        for l in range(1, _lpips_ops.LPIPS_LAYERS):      # a fixed order: the same bits run to run
            out = out + layers[:, l]
    return out.mean() if reduction == 'mean' else out
