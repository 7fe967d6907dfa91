"""Loss head and metrics of the reference (losses.py:4-14, metrics.py:4-20) — scalar reductions over (B,3) pixels.

`MSELoss` is one HIP launch forward (both levels, both means, their sum) and one backward (`hn_mse_loss_*`,
functional.mse_loss); the metrics `mse` and `psnr` (logging only, no gradient path in the reference) are torch
one-liners; `ssim` runs kornia's windowed SSIM in HIP (`hn_ssim_*`, functional.ssim_dssim), differentiable as kornia's;
`ms_ssim` is the five-level multi-scale SSIM the Nerfies / HyperNeRF tables report (`hn_msssim_*`), a metric only.
GPU tensors only, like every op of the package."""
import torch
from torch import nn

from . import functional as F


class MSELoss(nn.Module):
    """Sum over the rendered levels of mean((rgb - gt)^2): coarse always, fine when the model produced it."""

    def forward(self, inputs, targets):
        fine = inputs.get('fine')
        return F.mse_loss(inputs['coarse']['rgb'], fine['rgb'] if fine is not None else None, targets)


loss_dict = {'mse': MSELoss}


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
    documents (1, 3, H, W)), any strides.  dssim is kornia's ssim loss (functional.ssim_dssim, two HIP launches)."""
    return 1 - 2 * F.ssim_dssim(image_pred, image_gt, 3, reduction=reduction)


def ms_ssim(image_pred, image_gt, reduction='mean'):
    """Multi-scale SSIM of images in [0, 1] (the NumPy `MultiScaleSSIM` that HyperNeRF's compute_multiscale_ssim restates,
    max_val 1): per image prod_{l<4} cs_l^w_l * ssim_4^w_4 over a five-level pyramid (functional.msssim_levels), weights
    functional.MSSSIM_WEIGHTS.  image_pred and image_gt (N, C, H, W) fp32 on the GPU, any strides, any H, W >= 1.
    'none' returns the (N,) values, 'mean' their average.  A negative cs_l or ssim_4 gives NaN, as it does in NumPy.
    A metric only: there is no backward and the result never requires grad."""
    if reduction not in ('mean', 'none'):
        raise ValueError(f"ms_ssim: reduction must be 'mean' or 'none', got {reduction!r}")
    levels = F.msssim_levels(image_pred, image_gt)
    with torch.no_grad():
        # scalar exponents: no host-to-device copy, so the product is safe inside a stream capture too
        last = F.MSSSIM_LEVELS - 1
        out = levels[:, last, 0].pow(F.MSSSIM_WEIGHTS[last])
        for l in range(last):
            out = out * levels[:, l, 1].pow(F.MSSSIM_WEIGHTS[l])
    return out.mean() if reduction == 'mean' else out
