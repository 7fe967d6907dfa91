"""Gradient clipping as csrc/hn_optim.hip states it (hn_grad_norm / hn_grad_scale), restated in float64 NumPy:
torch.nn.utils.clip_grad_value_ and then torch.nn.utils.clip_grad_norm_ (2-norm, error_if_nonfinite=False) of the gradient
that counts, grad_scale * g.  clamp(s*g, +-v) = s * clamp(g, +-v/s), so everything is written on the RAW buffer g with
the threshold v' = float32(v / s):

    c = clamp(g, +-v')                       by comparisons, as torch's clamp: a NaN stays NaN
    total_norm = s * sqrt(sum c^2)           the norm of the value-clipped gradient that counts
    coef = max_norm / (total_norm + 1e-6)
    coef_clamped = coef clamped to at most 1, torch.clamp(max=1.0): a NaN stays NaN
    buffer = c * coef_clamped                what the raw buffer holds afterwards (the step launch applies s later)

`None` for max_norm or clip_value switches that clip off (the kernels take +inf)."""
import numpy as np


def threshold(clip_value, grad_scale=1.0):
    """v' as the entry points compute it: the division in double, rounded to float32 once."""
    if clip_value is None:
        return np.float32(np.inf)
    return np.float32(np.float64(clip_value) / np.float64(grad_scale))


def clamp(g, vp):
    """clamp(g, +-vp) by comparisons; g any float array, returned in g's dtype."""
    g = np.asarray(g)
    vp = g.dtype.type(vp)
    return np.where(g > vp, vp, np.where(g < -vp, -vp, g))


def clamp_coef(coef):
    """torch.clamp(coef, max=1.0): NaN > 1 is false, so a NaN stays NaN."""
    return 1.0 if coef > 1.0 else coef


def coef_of(total_norm, max_norm):
    """(coef, coef_clamped) in float64 from a total norm; without a norm clip the factor is 1 whatever the norm."""
    if max_norm is None:
        return np.float64(np.inf), 1.0
    with np.errstate(all="ignore"):
        coef = np.float64(max_norm) / (np.float64(total_norm) + 1e-6)
    return coef, clamp_coef(coef)


def clip(g, max_norm=None, clip_value=None, grad_scale=1.0):
    """g: the raw gradient buffer (any shape, any float dtype).  Returns a dict of float64 results: 'clamped' (c),
    'total_norm', 'coef', 'coef_clamped' and 'buffer' (c * coef_clamped, in g's shape)."""
    g64 = np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        c = clamp(g64, np.float64(threshold(clip_value, grad_scale)))
        total = np.float64(grad_scale) * np.sqrt(np.sum(c * c))
        coef, cc = coef_of(total, max_norm)
        buf = c * cc
    return {"clamped": c, "total_norm": float(total), "coef": float(coef), "coef_clamped": float(cc), "buffer": buf}
