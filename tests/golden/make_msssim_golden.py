"""Writes tests/golden/g25_msssim.npz: multi-scale SSIM of a few small image pairs, computed in float64 with NumPy and
SciPy the way the original algorithm is stated (a 2-D Gaussian window of size min(11, h, w) applied with
scipy.signal.fftconvolve in 'valid' mode, a 2 x 2 box filter applied with scipy.ndimage.convolve in 'reflect' mode and
every second pixel kept).  It shares no code with tests/msssim_restated.py (torch conv2d, separable window, replicate
padding + average pooling): the point is an independent implementation.  Images are (H, W, C) in [0, 1], max_val = 1.

    python tests/golden/make_msssim_golden.py          # needs scipy; the stored file is what the tests read
"""
import os

import numpy as np
from scipy import ndimage, signal

WEIGHTS = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
K1, K2, MAX_VAL, FILTER_SIZE, FILTER_SIGMA = 0.01, 0.03, 1.0, 11, 1.5


def gauss2d(size, sigma):
    """Normalised 2-D Gaussian on a size x size grid centred on the window (half-integer coordinates for even sizes)."""
    coords = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    yy, xx = np.meshgrid(coords, coords, indexing="ij")
    g = np.exp(-(xx ** 2 + yy ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def level(a, b):
    """(ssim, cs) of one scale of (H, W, C) float64 images."""
    h, w, _ = a.shape
    size = min(FILTER_SIZE, h, w)
    sigma = size * FILTER_SIGMA / FILTER_SIZE
    win = gauss2d(size, sigma)[:, :, None]
    mu1 = signal.fftconvolve(a, win, mode="valid")
    mu2 = signal.fftconvolve(b, win, mode="valid")
    s11 = signal.fftconvolve(a * a, win, mode="valid") - mu1 * mu1
    s22 = signal.fftconvolve(b * b, win, mode="valid") - mu2 * mu2
    s12 = signal.fftconvolve(a * b, win, mode="valid") - mu1 * mu2
    c1, c2 = (K1 * MAX_VAL) ** 2, (K2 * MAX_VAL) ** 2
    v1 = 2.0 * s12 + c2
    v2 = s11 + s22 + c2
    ssim = np.mean(((2.0 * mu1 * mu2 + c1) * v1) / ((mu1 * mu1 + mu2 * mu2 + c1) * v2))
    return ssim, np.mean(v1 / v2)


def halve(img):
    box = np.ones((2, 2, 1)) / 4.0
    return ndimage.convolve(img, box, mode="reflect")[::2, ::2, :]


def ms_ssim_levels(a, b):
    """((5, 2) array of (ssim_l, cs_l), product)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    vals = []
    for _ in range(WEIGHTS.size):
        vals.append(level(a, b))
        a, b = halve(a), halve(b)
    vals = np.array(vals)
    with np.errstate(invalid="ignore"):
        prod = np.prod(vals[:-1, 1] ** WEIGHTS[:-1]) * vals[-1, 0] ** WEIGHTS[-1]
    return vals, prod


def smooth_pair(rng, h, w, c, sigma):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = 0.5 + 0.35 * np.sin(0.31 * xx + 0.17 * yy)[:, :, None] * np.cos(0.9 * np.arange(c) + 0.05 * yy[:, :, None])
    gt = np.clip(base + 0.05 * rng.standard_normal((h, w, c)), 0, 1).astype(np.float32)
    pred = np.clip(gt + sigma * rng.standard_normal((h, w, c)), 0, 1).astype(np.float32)
    return pred, gt


def main():
    rng = np.random.default_rng(25)
    cases = {
        "s5x7": smooth_pair(rng, 5, 7, 3, 0.1),
        "s16x16": smooth_pair(rng, 16, 16, 3, 0.02),
        "s23x40": smooth_pair(rng, 23, 40, 1, 0.3),
        "s33x29": smooth_pair(rng, 33, 29, 3, 0.1),
        "n16x13": (rng.random((16, 13, 3)).astype(np.float32), rng.random((16, 13, 3)).astype(np.float32)),
    }
    out = {"names": np.array(sorted(cases))}
    for name, (pred, gt) in cases.items():
        vals, prod = ms_ssim_levels(pred, gt)
        out[name + "_pred"], out[name + "_gt"], out[name + "_levels"], out[name + "_product"] = pred, gt, vals, prod
        print(name, vals.round(4).tolist(), float(prod))
    # the 1-D statement of the downsample: the row 0 .. 6 gives 0.5, 2.5, 4.5, 6
    row = np.tile(np.arange(7, dtype=np.float64)[None, :, None], (2, 1, 1))
    out["row7_halved"] = halve(row)[0, :, 0]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g25_msssim.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
