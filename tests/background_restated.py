"""The background regularization restated without the package: the sampler in float32 NumPy (the kernel rounds every
operation on its own, so this is bit-exact), the loss and its gradient in float64 NumPy, and the loss once more in torch
for the end-to-end oracle (CPU autograd through the oracle's warp field).

    i_n = min(int(u[n, 0] * M), M - 1)      k_n = min(int(u[n, 1] * K), K - 1)
    p_n = points[i_n] + noise_std * nrm[n]  ids_n = ids[k_n]
    x_n = |w_n - p_n|^2 / scale^2           loss = mean_n 2 x_n / (x_n + 4)
    d loss / d w_n = 16 (w_n - p_n) / (scale^2 (x_n + 4)^2 N)

(Barron's general robust loss at alpha = -2, Geman-McClure, on the squared residual, as HyperNeRF's training loop
computes its background loss.)"""
import numpy as np
import torch


def sample(points, ids, u, nrm, noise_std):
    """float32: (out_points (N, 3), out_ids (N,), row index (N,), id index (N,))."""
    points, u, nrm = (np.asarray(a, dtype=np.float32) for a in (points, u, nrm))
    ids = np.asarray(ids, dtype=np.int64)
    m, k = points.shape[0], ids.shape[0]
    i = np.minimum((u[:, 0] * np.float32(m)).astype(np.int64), m - 1)
    j = np.minimum((u[:, 1] * np.float32(k)).astype(np.int64), k - 1)
    noise = (np.float32(noise_std) * nrm).astype(np.float32)
    return (points[i] + noise).astype(np.float32), ids[j], i, j


def loss(warped, points, scale):
    """float64 scalar."""
    d = np.asarray(warped, dtype=np.float64) - np.asarray(points, dtype=np.float64)
    x = (d * d).sum(-1) / (float(scale) ** 2)
    return float(np.mean(2.0 * x / (x + 4.0)))


def grad(warped, points, scale, g=1.0):
    """float64 (N, 3): g * d loss / d warped."""
    d = np.asarray(warped, dtype=np.float64) - np.asarray(points, dtype=np.float64)
    s2 = float(scale) ** 2
    x = (d * d).sum(-1, keepdims=True) / s2
    return float(g) * 16.0 * d / (s2 * (x + 4.0) ** 2 * d.shape[0])


def loss_torch(warped: torch.Tensor, points: torch.Tensor, scale: float) -> torch.Tensor:
    """The same loss on torch tensors, differentiable (the oracle's end of the end-to-end comparison)."""
    d = warped - points.detach()
    x = (d * d).sum(-1) / (float(scale) ** 2)
    return (2.0 * x / (x + 4.0)).mean()
