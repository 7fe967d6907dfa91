"""Float64 restatement of the distortion loss (Mip-NeRF 360, Barron et al. 2022, eq. 15) as the package defines it: the
plain O(S^2) double loop and its analytic gradient, in both spacings, plus the same loss in torch ops for autograd.

For one ray with sorted depths z_0 <= ... <= z_{S-1} and weights w_i:
    s_i = (z_i - near) / (far - near)                       'linear'
    s_i = (1/z_i - 1/near) / (1/far - 1/near)               'disparity'
    i < S-1: d_i = s_{i+1} - s_i, m_i = (s_i + s_{i+1}) / 2;    the last sample: d = 0, m = s_{S-1}
    L_ray = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
    dL_ray/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i d_i
"""
import numpy as np
import torch


def normalised(z, near, far, spacing):
    z = np.asarray(z, dtype=np.float64)
    near, far = float(near), float(far)
    if spacing == 'linear':
        return (z - near) / (far - near)
    if spacing == 'disparity':
        return (1.0 / z - 1.0 / near) / (1.0 / far - 1.0 / near)
    raise ValueError(spacing)


def intervals(z, near, far, spacing):
    """(m, d) of one ray: midpoints and widths, the last sample a point mass at its own depth."""
    s = normalised(z, near, far, spacing)
    m, d = s.copy(), np.zeros_like(s)
    m[:-1] = (s[:-1] + s[1:]) / 2
    d[:-1] = s[1:] - s[:-1]
    return m, d


def ray_loss(w, z, near, far, spacing='linear'):
    """L_ray by the plain double loop."""
    w = np.asarray(w, dtype=np.float64)
    m, d = intervals(z, near, far, spacing)
    total = 0.0
    for i in range(len(w)):
        for j in range(len(w)):
            total += w[i] * w[j] * abs(m[i] - m[j])
        total += w[i] * w[i] * d[i] / 3.0
    return total


def ray_grad(w, z, near, far, spacing='linear'):
    """dL_ray/dw, the analytic form by the plain loop."""
    w = np.asarray(w, dtype=np.float64)
    m, d = intervals(z, near, far, spacing)
    g = np.zeros_like(w)
    for i in range(len(w)):
        acc = 0.0
        for j in range(len(w)):
            acc += w[j] * abs(m[i] - m[j])
        g[i] = 2.0 * acc + 2.0 * w[i] * d[i] / 3.0
    return g


def ray_loss_grad_outer(w, z, near, far, spacing='linear'):
    """(L_ray, dL_ray/dw) of one ray: the same O(S^2) sums over the full |m_i - m_j| matrix (NumPy instead of the Python
    loops, for the batches the GPU tests compare against)."""
    w = np.asarray(w, dtype=np.float64)
    m, d = intervals(z, near, far, spacing)
    inner = np.abs(m[:, None] - m[None, :]) @ w
    return float(w @ inner + (w * w * d).sum() / 3.0), 2.0 * inner + 2.0 * w * d / 3.0


def per_ray(w, z, near, far, spacing='linear'):
    """(B,) L_ray of a (B, S) batch."""
    return np.array([ray_loss_grad_outer(wr, zr, near, far, spacing)[0] for wr, zr in zip(np.asarray(w), np.asarray(z))])


def loss(w, z, near, far, spacing='linear'):
    return float(per_ray(w, z, near, far, spacing).mean())


def grad_rays(w, z, near, far, spacing='linear'):
    """(B, S) dL_ray/dw per ray — the gradient of the mean times B."""
    return np.stack([ray_loss_grad_outer(wr, zr, near, far, spacing)[1] for wr, zr in zip(np.asarray(w), np.asarray(z))])


def loss_torch(w, z, near, far, spacing='linear'):
    """The mean over rays in torch ops (the O(S^2) form; differentiable in w), in w's dtype."""
    z = z.to(w.dtype)
    if spacing == 'linear':
        s = (z - near) / (far - near)
    else:
        s = (1.0 / z - 1.0 / near) / (1.0 / far - 1.0 / near)
    m = torch.cat([(s[:, :-1] + s[:, 1:]) / 2, s[:, -1:]], dim=1)
    d = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, -1:])], dim=1)
    both = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2))
    return (both + (w * w * d).sum(1) / 3.0).mean()
