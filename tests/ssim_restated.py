"""Test infrastructure: the SSIM of the reference's metrics.py:15-20 (kornia 0.6.1's ssim loss, `dssim`) restated in
float64 torch on the CPU, from the contract: the 1-D Gaussian window (sigma 1.5, normalised), its outer product as the
2-D window, F.pad(mode='reflect') by window // 2 and a grouped conv2d (kornia's filter2d), the five moments, the map
S = ((2 mux muy + C1)(2 sxy + C2)) / ((mux^2 + muy^2 + C1)(sxx + syy + C2) + eps), dssim = clamp((1 - S) / 2, 0, 1),
then the reduction.  Differentiable with torch.autograd, so it is also the reference for the HIP backward.
"""
import torch
import torch.nn.functional as F


def window1d(window_size, dtype=torch.float32):
    """kornia's get_gaussian_kernel1d(window_size, 1.5): computed in `dtype` (float32 = the weights kornia, and the
    kernels, use), returned as float64."""
    x = torch.arange(window_size, dtype=dtype) - window_size // 2
    g = torch.exp(-x.pow(2.0) / float(2 * 1.5 ** 2))
    return (g / g.sum()).double()


def filt(img, window_size, weights=None):
    w1 = window1d(window_size) if weights is None else weights.double()
    k = torch.outer(w1, w1)
    c = img.shape[1]
    r = window_size // 2
    padded = F.pad(img, [r, r, r, r], mode="reflect")
    return F.conv2d(padded, k.expand(c, 1, window_size, window_size), groups=c)


def ssim_map(x, y, window_size=3, max_val=1.0, eps=1e-12, weights=None):
    """S per pixel of (N, C, H, W) images (computed in float64)."""
    x, y = x.double(), y.double()
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mu1, mu2 = filt(x, window_size, weights), filt(y, window_size, weights)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = filt(x * x, window_size, weights) - mu1_sq
    s2 = filt(y * y, window_size, weights) - mu2_sq
    s12 = filt(x * y, window_size, weights) - mu1_mu2
    num = (2.0 * mu1_mu2 + c1) * (2.0 * s12 + c2)
    den = (mu1_sq + mu2_sq + c1) * (s1 + s2 + c2)
    return num / (den + eps)


def dssim(x, y, window_size=3, max_val=1.0, eps=1e-12, reduction="mean", weights=None):
    loss = torch.clamp((1.0 - ssim_map(x, y, window_size, max_val, eps, weights)) / 2, min=0, max=1)
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss


def ssim(image_pred, image_gt, reduction="mean"):
    """metrics.py:15-20."""
    return 1 - 2 * dssim(image_pred, image_gt, 3, reduction=reduction)
