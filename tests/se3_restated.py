"""The SE(3) exponential-map warp (csrc/hn_render.hip, hn_se3_forward_kernel / hn_se3_backward_kernel) restated in plain
torch on the CPU, without the package, in any float dtype.  With theta = |w|, t = theta^2 = w . w:

    y = p + A (w x p) + B (w x (w x p)) + v + B (w x v) + C (w x (w x v))
    A = sin(theta) / theta        B = (1 - cos(theta)) / theta^2        C = (theta - sin(theta)) / theta^3

which is Rodrigues' formula and Modern Robotics eq. 3.88 for the screw (w, v) / theta turned by theta, written without the
division by theta: A, B, C are even, entire functions of theta (A -> 1, B -> 1/2, C -> 1/6), so theta = 0 is the pure
translation y = p + v.  The gradient of sum(g * y), with ga = g x w:

    d p = g + A ga + B (ga x w)                    d v = g + B ga + C (ga x w)
    d w = A (p x g) + B (q x g + p x ga + v x g) + C (m x g + v x ga) + s w        q = w x p, r = w x q, m = w x v, n = w x m
    s   = A1 (q . g) + B1 (r . g + m . g) + C1 (n . g)                              X1 = X'(theta) / theta

Below the switch point (theta < 1 in float32, theta < 1e-2 in float64) every coefficient is its Taylor series in t,
TERMS terms by Horner:

    A = sum_k (-t)^k / (2k+1)!      B = sum_k (-t)^k / (2k+2)!      C = sum_k (-t)^k / (2k+3)!          k = 0 ...
    X1 = - sum_k 2(k+1) (-t)^k / (2k+2+j)!      j = 1, 2, 3 for A, B, C

above it the closed forms through the half angle (sh, ch = sin, cos of theta / 2), none of which subtracts two nearly equal
numbers unless theta is small:

    sin = 2 sh ch    A = sin / theta    B = 2 sh^2 / t    C = (theta - sin) / (t theta)
    A1 = (1 - 2 sh^2 - A) / t          B1 = (A - 2 B) / t                C1 = (B - 3 C) / t

Float64 needs the series too: (theta - sin) / theta^3 and (B - 3 C) / t lose 1 / theta^2 of the precision, and the older form
(1 - cos(theta)) / theta . (v / theta x g) of the same map is off by 3e-5 at theta = 1e-6 even in float64.

`apply(..., dtype=torch.float64)` is the oracle of tests/test_gpu_se3.py; `apply(..., dtype=torch.float32)` runs the same
formulas with every operation rounded to float32 (what the kernel does: the library is built without FMA contraction);
tests/test_se3_host.py proves both."""
import math

import numpy as np
import torch

import hashprng as H

TERMS = 7
SWITCH = {torch.float32: 1.0, torch.float64: 1e-2}
NAMES = ("y", "d w", "d v", "d points")
COEF_NAMES = ("A", "B", "C", "A1", "B1", "C1")


def series_coefficients(j, derivative):
    """The TERMS Taylor coefficients (Python floats, for (-t)^0, (-t)^1, ...) of A, B, C (j = 1, 2, 3) or of A1, B1, C1."""
    if derivative:
        return [-2.0 * (k + 1) / math.factorial(2 * k + 2 + j) for k in range(TERMS)]
    return [1.0 / math.factorial(2 * k + j) for k in range(TERMS)]


def _horner(t, coefs):
    acc = torch.full_like(t, coefs[-1])
    for c in reversed(coefs[:-1]):
        acc = c - acc * t                       # sum_k c_k (-t)^k
    return acc


def coefficients(t, switch=None):
    """(A, B, C, A1, B1, C1) at t = theta^2, in t's dtype; differentiable (the branch not taken sees t = 1, so that no
    0 * inf reaches autograd)."""
    switch = SWITCH[t.dtype] if switch is None else switch
    series = [_horner(t, series_coefficients(j, d)) for d in (False, True) for j in (1, 2, 3)]
    small = t < switch * switch
    ts = torch.where(small, torch.ones_like(t), t)
    th = torch.sqrt(ts)
    sh, ch = torch.sin(0.5 * th), torch.cos(0.5 * th)
    sn = 2.0 * sh * ch
    hv = 2.0 * sh * sh                          # 1 - cos(theta)
    a = sn / th
    b = hv / ts
    c = (th - sn) / (ts * th)
    closed = [a, b, c, ((1.0 - hv) - a) / ts, (a - 2.0 * b) / ts, (b - 3.0 * c) / ts]
    return tuple(torch.where(small, s, f) for s, f in zip(series, closed))


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])[..., None]


def _cast(dtype, *arrays):
    return tuple(torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).detach().to(dtype) for a in arrays)


def forward(w, v, p, switch=None):
    """y for tensors of one float dtype; differentiable w.r.t. all three."""
    a, b, c, _, _, _ = coefficients(_dot(w, w), switch)
    q, m = _cross(w, p), _cross(w, v)
    return p + (a * q + b * _cross(w, q)) + (v + (b * m + c * _cross(w, m)))


def apply(w, v, p, g, dtype=torch.float64, switch=None):
    """(y, d w, d v, d points) of sum(g * y), every operation in `dtype`, the gradients from the formulas above."""
    w, v, p, g = _cast(dtype, w, v, p, g)
    with torch.no_grad():
        a, b, c, a1, b1, c1 = coefficients(_dot(w, w), switch)
        q, m = _cross(w, p), _cross(w, v)
        r, n = _cross(w, q), _cross(w, m)
        y = p + (a * q + b * r) + (v + (b * m + c * n))
        ga = _cross(g, w)
        gaa = _cross(ga, w)
        d_p = g + (a * ga + b * gaa)
        d_v = g + (b * ga + c * gaa)
        s = a1 * _dot(q, g) + b1 * (_dot(r, g) + _dot(m, g)) + c1 * _dot(n, g)
        d_w = a * _cross(p, g) + b * ((_cross(q, g) + _cross(p, ga)) + _cross(v, g)) \
            + c * (_cross(m, g) + _cross(v, ga)) + s * w
    return y, d_w, d_v, d_p


def autograd(w, v, p, g, dtype=torch.float64, switch=None, fn=None):
    """The same four tensors by torch autograd through `fn(w, v, p)` (default: the forward above)."""
    w, v, p, g = _cast(dtype, w, v, p, g)
    w, v, p = (x.clone().requires_grad_(True) for x in (w, v, p))
    y = forward(w, v, p, switch) if fn is None else fn(w, v, p)
    (y * g).sum().backward()
    return y.detach(), w.grad, v.grad, p.grad


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_se3_host.py and tests/test_gpu_se3.py
# ----------------------------------------------------------------------------------------------------------------------
ROWS = 4096
SIGMA_W = (0.0, 1e-25, 1e-6, 1e-4, 3e-4, 1e-3, 1e-2, 0.1, 0.5, 1.0, math.pi / 1.7, 2.0 * math.pi / 1.7, 20.0)
BANDS = tuple(dict.fromkeys((sw, sv) for sw in SIGMA_W for sv in (sw, 0.3, 0.0)))        # (sigma_w, sigma_v), no pair twice
GPU_BOUND_MODERATE, GPU_BOUND_LARGE = 1e-5, 5e-5
SWEEP_LO, SWEEP_HI = 1e-8, 10.0
SWEEP_AXIS = (2.0 / 7.0, -3.0 / 7.0, 6.0 / 7.0)
SWEEP_V, SWEEP_P, SWEEP_G = (0.3, -0.2, 0.1), (0.5, -0.7, 0.2), (1.0, -2.0, 0.5)


def gpu_bound(sigma_w):
    """max |err| / max |ref| allowed to the kernels, per band and per output."""
    return GPU_BOUND_MODERATE if sigma_w <= 4.0 else GPU_BOUND_LARGE


def band_inputs(sigma_w, sigma_v, rows=ROWS, seed=61):
    """float32 (w, v, p, g) of one band: w ~ sigma_w N(0, 1), v ~ sigma_v N(0, 1), p uniform in [-1, 1]^3, g ~ N(0, 1)."""
    tag = f"{sigma_w!r}/{sigma_v!r}"
    w = H.normal(seed, "se3 w " + tag, (rows, 3)) * np.float32(sigma_w)
    v = H.normal(seed, "se3 v " + tag, (rows, 3)) * np.float32(sigma_v)
    return w, v, H.uniform(seed, "se3 p " + tag, (rows, 3), -1.0, 1.0), H.normal(seed, "se3 g " + tag, (rows, 3))


def sweep_thetas(rows=ROWS):
    """float64 thetas, log-uniform from SWEEP_LO to SWEEP_HI."""
    return torch.logspace(math.log10(SWEEP_LO), math.log10(SWEEP_HI), rows, dtype=torch.float64)


def sweep_inputs(rows=ROWS, dtype=torch.float32):
    """(theta, w, v, p, g): w = theta * SWEEP_AXIS rounded to `dtype`, the other three the same in every row."""
    th = sweep_thetas(rows)
    w = (th[:, None] * torch.tensor(SWEEP_AXIS, dtype=torch.float64)).to(dtype)
    v, p, g = (torch.tensor(x, dtype=dtype).expand(rows, 3).contiguous() for x in (SWEEP_V, SWEEP_P, SWEEP_G))
    return th, w, v, p, g


def sweep_decades(theta):
    """[(label, row mask)] for the decades of the sweep."""
    n = int(round(math.log10(SWEEP_HI / SWEEP_LO)))
    idx = torch.clamp(torch.floor(torch.log10(theta / SWEEP_LO) + 1e-9), 0, n - 1).long()
    return [(f"theta from {SWEEP_LO * 10.0 ** k:.0e} to {SWEEP_LO * 10.0 ** (k + 1):.0e}", idx == k) for k in range(n)]


def band_errors(got, ref, g):
    """Per output: (max |got - ref| over the band, the scale it is judged against, whether that scale is the band's own
    max |ref|).  A reference that is identically zero in the band is judged absolutely, against max |g|."""
    out = []
    for a, b in zip(got, ref):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        err = float((a - b).abs().max()) if bool(torch.isfinite(a).all()) else float("inf")
        scale = float(b.abs().max())
        out.append((err, scale, True) if scale > 0.0 else (err, float(torch.as_tensor(g).double().abs().max()), False))
    return out
