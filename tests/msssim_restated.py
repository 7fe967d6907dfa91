"""Test infrastructure: multi-scale SSIM (the NumPy `MultiScaleSSIM` that HyperNeRF's compute_multiscale_ssim restates,
max_val 1) restated in torch on the CPU, from the contract: per level the window of size min(11, h, w) with
sigma = size * 1.5 / 11 (half-integer offsets for an even size), the five moments as VALID conv2d correlations with the
outer product of the 1-D taps, ssim_l = mean(((2 mu1 mu2 + c1) v1) / ((mu1^2 + mu2^2 + c1) v2)), cs_l = mean(v1 / v2)
over all valid positions and channels of one image, then the edge-replicated 2 x 2 box mean as the next level's images.
float64 unless told otherwise (float32: the reference run the GPU test derives its tolerance from).
"""
import torch
import torch.nn.functional as F

LEVELS = 5
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window1d(size, filter_size=11, filter_sigma=1.5):
    """float64 taps: exp(-x^2 / (2 sigma^2)), sigma = size * 1.5 / 11, x centred on the window, normalised."""
    sigma = size * filter_sigma / filter_size
    x = torch.arange(size, dtype=torch.float64) - (size - 1) / 2.0
    g = torch.exp(-(x ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def valid_filter(img, taps):
    """(N, C, H, W) -> (N, C, H - size + 1, W - size + 1): correlation with outer(taps, taps), no padding."""
    c, size = img.shape[1], taps.numel()
    k = torch.outer(taps, taps).to(img.dtype)
    return F.conv2d(img, k.expand(c, 1, size, size).contiguous(), groups=c)


def downsample(img):
    """2 x 2 box mean with stride 2, an index past the edge replaced by the edge pixel: (ceil(H/2), ceil(W/2))."""
    h, w = img.shape[-2:]
    padded = F.pad(img, [0, w % 2, 0, h % 2], mode="replicate")
    return F.avg_pool2d(padded, 2)


def level_values(x, y, dtype=torch.float64):
    """(ssim_l, cs_l) of one level per image: two (N,) tensors."""
    size = min(11, x.shape[-2], x.shape[-1])
    taps = window1d(size).to(dtype)
    mu1, mu2 = valid_filter(x, taps), valid_filter(y, taps)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11 = valid_filter(x * x, taps) - mu11
    s22 = valid_filter(y * y, taps) - mu22
    s12 = valid_filter(x * y, taps) - mu12
    v1 = 2.0 * s12 + C2
    v2 = s11 + s22 + C2
    ssim = (((2.0 * mu12 + C1) * v1) / ((mu11 + mu22 + C1) * v2)).mean(dim=(1, 2, 3))
    cs = (v1 / v2).mean(dim=(1, 2, 3))
    return ssim, cs


def levels(pred, gt, dtype=torch.float64):
    """(N, 5, 2) in `dtype`: [..., 0] = ssim_l, [..., 1] = cs_l of (N, C, H, W) images."""
    x, y = pred.to(dtype), gt.to(dtype)
    out = []
    for _ in range(LEVELS):
        out.append(torch.stack(level_values(x, y, dtype), dim=-1))
        x, y = downsample(x), downsample(y)
    return torch.stack(out, dim=1)


def product(lv):
    """(N,): prod_{l<4} cs_l^w_l * ssim_4^w_4; a negative base gives NaN, as in NumPy."""
    w = torch.tensor(WEIGHTS, dtype=lv.dtype)
    terms = torch.cat([lv[:, :LEVELS - 1, 1], lv[:, LEVELS - 1:, 0]], dim=1)
    return torch.pow(terms, w).prod(dim=1)


def ms_ssim(pred, gt, dtype=torch.float64):
    return product(levels(pred, gt, dtype))
