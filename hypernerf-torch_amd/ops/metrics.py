"""SSIM and multi-scale SSIM of images on the GPU (csrc/hn_metrics.hip, csrc/hn_msssim.hip; their shared tile, passes and
sums: csrc/hn_window.h)."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from .. import _lib as L

__all__ = ["SSIM_MAX_WINDOW", "ssim_window", "ssim_dssim", "MSSSIM_LEVELS", "MSSSIM_MAX_SIZE", "MSSSIM_WEIGHTS",
           "msssim_window", "msssim_pyramid", "msssim_workspace_bytes", "msssim_levels"]


def _check_pair(name, pred, gt, reflect_radius=None):
    """What both metrics ask of their images: two float32 (N, C, H, W) tensors of one shape, not empty, and (SSIM) sides
    that reflect padding by `reflect_radius` allows."""
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
        raise ValueError(f"{name}: pred and gt must be tensors")
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"{name}: pred and gt must both be (N, C, H, W) of one shape, got {tuple(pred.shape)} and "
                         f"{tuple(gt.shape)}")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError(f"{name}: pred and gt must be float32")
    h, w = pred.shape[2], pred.shape[3]
    if reflect_radius is not None and (h <= reflect_radius or w <= reflect_radius):
        raise ValueError(f"{name}: H and W must be larger than window_size // 2 = {reflect_radius} (reflect padding), "
                         f"got {h} x {w}")
    if pred.numel() == 0:
        raise ValueError(f"{name}: empty images")


# --------------------------------------------------------------------------------------------
# SSIM (metrics.py:15-20: kornia's ssim loss)
# --------------------------------------------------------------------------------------------
SSIM_MAX_WINDOW = 2 * L.HN_SSIM_MAX_R + 1    # hn_ssim_*: odd windows 3 .. 15
_SSIM_WINDOWS: Dict[int, C.Array] = {}


def ssim_window(window_size: int) -> torch.Tensor:
    """kornia's get_gaussian_kernel1d(window_size, 1.5) (kornia/filters/kernels.py `gaussian`), computed by torch in
    fp32 on the CPU: the kernels take these weights as they are."""
    x = torch.arange(window_size).float() - window_size // 2
    if window_size % 2 == 0:
        x = x + 0.5
    g = torch.exp(-x.pow(2.0) / float(2 * 1.5 ** 2))
    return g / g.sum()


def _ssim_window_host(window_size: int):
    buf = _SSIM_WINDOWS.get(window_size)
    if buf is None:
        buf = _SSIM_WINDOWS[window_size] = (C.c_float * window_size)(*ssim_window(window_size).tolist())
    return buf


def _ssim_check(pred, gt, window_size, reduction):
    if not isinstance(window_size, int) or window_size < 3 or window_size % 2 == 0:
        raise ValueError(f"ssim: window_size must be an odd integer >= 3, got {window_size!r}")
    if window_size > SSIM_MAX_WINDOW:
        raise ValueError(f"ssim: window_size {window_size} is above the kernels' limit of {SSIM_MAX_WINDOW}")
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"ssim: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    _check_pair("ssim", pred, gt, reflect_radius=window_size // 2)


class _SsimFn(torch.autograd.Function):
    """The dssim map (`none`) or its sum (`mean` / `sum`): hn_ssim_forward / hn_ssim_backward."""

    @staticmethod
    def forward(ctx, pred, gt, window_size, c1, c2, eps, want_map):
        L.load()
        x, y = pred.detach(), gt.detach()
        n, c, h, w = x.shape
        args = (L.ptr(x), (C.c_int64 * 4)(*x.stride()), L.ptr(y), (C.c_int64 * 4)(*y.stride()), n, c, h, w,
                _ssim_window_host(window_size), window_size, c1, c2, eps)
        if want_map:
            out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
            L.launch("hn_ssim_forward", *args, L.ptr(out), None, None, L.stream_handle())
        else:
            nbytes = C.c_int64(0)
            L.check(L.load().hn_ssim_workspace_bytes(n, c, h, w, window_size, C.byref(nbytes)), "hn_ssim_workspace_bytes")
            ws = torch.empty(nbytes.value // 4, dtype=torch.float32, device=x.device)
            out = torch.empty((), dtype=torch.float32, device=x.device)
            L.launch("hn_ssim_forward", *args, None, L.ptr(out), L.ptr(ws), L.stream_handle())
        ctx.save_for_backward(x, y)
        ctx.cfg = (window_size, c1, c2, eps, want_map)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        window_size, c1, c2, eps, want_map = ctx.cfg
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return (None,) * 7
        if not need_x:          # S is symmetric in its two images: d/dgt is d/dpred with the roles swapped
            x, y = y, x
        n, c, h, w = x.shape
        g = g.detach().float().contiguous()
        d_first = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        d_second = torch.empty_like(d_first) if (need_x and need_y) else None
        L.launch("hn_ssim_backward", L.ptr(x), (C.c_int64 * 4)(*x.stride()), L.ptr(y), (C.c_int64 * 4)(*y.stride()),
                 n, c, h, w, _ssim_window_host(window_size), window_size, c1, c2, eps,
                 None if want_map else L.ptr(g), L.ptr(g) if want_map else None, L.ptr(d_first), L.ptr(d_second),
                 L.stream_handle())
        if need_x:
            return d_first, d_second, None, None, None, None, None
        return None, d_first, None, None, None, None, None


def ssim_dssim(pred: torch.Tensor, gt: torch.Tensor, window_size: int = 3, max_val: float = 1.0, eps: float = 1e-12,
               reduction: str = 'mean') -> torch.Tensor:
    """kornia's structural dissimilarity (kornia.losses.ssim_loss, 0.6.1): clamp((1 - SSIM) / 2, 0, 1) of (N, C, H, W)
    fp32 images on the GPU, the 2-D Gaussian window (sigma 1.5) over reflect padding, reduced by 'mean', 'sum' or
    'none' (the per-pixel map).  Any element strides (e.g. an (H, W, 3) image as `permute(2, 0, 1)[None]`).
    Differentiable in both images; the sum is bit-reproducible run to run."""
    _ssim_check(pred, gt, window_size, reduction)
    L.require_gpu(pred, gt)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    out = _SsimFn.apply(pred, gt, window_size, c1, c2, float(eps), reduction == 'none')
    if reduction == 'mean':
        out = out / pred.numel()
    return out


# --------------------------------------------------------------------------------------------
# multi-scale SSIM (the metric the Nerfies / HyperNeRF tables report)
# --------------------------------------------------------------------------------------------
MSSSIM_LEVELS = L.HN_MS_LEVELS
MSSSIM_MAX_SIZE = L.HN_MS_MAX_SIZE    # hn_msssim_forward: window sizes 1 .. 11
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_MSSSIM_TILE_W, _MSSSIM_TILE_H = 32, 16
_MSSSIM_PLANS: Dict[tuple, tuple] = {}


def msssim_window(size: int) -> torch.Tensor:
    """The 1-D taps of one level's window, float64: exp(-x^2 / (2 sigma^2)) with sigma = size * 1.5 / 11 at the integer
    offsets -(size//2) .. size//2 (odd size) or the half-integer offsets -(size/2) + 0.5 .. size/2 - 0.5 (even size),
    normalised to sum 1.  Their outer product is the normalised 2-D Gaussian of the original exactly."""
    sigma = size * 1.5 / MSSSIM_MAX_SIZE
    x = torch.arange(size, dtype=torch.float64) - (size - 1) / 2.0
    g = torch.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


def msssim_pyramid(h: int, w: int):
    """[(h_l, w_l, size_l)] of the five levels: sides halve rounding up, size_l = min(11, h_l, w_l)."""
    out = []
    for _ in range(MSSSIM_LEVELS):
        out.append((h, w, min(MSSSIM_MAX_SIZE, h, w)))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def msssim_workspace_bytes(n: int, c: int, h: int, w: int) -> int:
    """hn_msssim_workspace_bytes in Python: the planes of levels 1 .. 4 of both images, then two partial sums per
    32 x 16 tile of every plane of levels 0 .. 4, in floats, rounded up to 16 bytes."""
    pyr = msssim_pyramid(h, w)
    floats = sum(2 * n * c * hl * wl for hl, wl, _ in pyr[1:])
    floats += sum(2 * n * c * (-(-wl // _MSSSIM_TILE_W)) * (-(-hl // _MSSSIM_TILE_H)) for hl, wl, _ in pyr)
    return (floats * 4 + 15) // 16 * 16


def _msssim_plan(n, c, h, w):
    """(taps, sizes, workspace floats) of a shape: host arrays built once (float64 taps rounded to fp32)."""
    plan = _MSSSIM_PLANS.get((n, c, h, w))
    if plan is None:
        sizes = [s for _, _, s in msssim_pyramid(h, w)]
        taps = (C.c_float * (MSSSIM_LEVELS * MSSSIM_MAX_SIZE))()
        for l, s in enumerate(sizes):
            for i, v in enumerate(msssim_window(s).tolist()):
                taps[l * MSSSIM_MAX_SIZE + i] = v
        nbytes = C.c_int64(0)
        L.check(L.load().hn_msssim_workspace_bytes(n, c, h, w, C.byref(nbytes)), "hn_msssim_workspace_bytes")
        plan = _MSSSIM_PLANS[(n, c, h, w)] = (taps, (C.c_int * MSSSIM_LEVELS)(*sizes), nbytes.value // 4)
    return plan


@torch.no_grad()
def msssim_levels(pred: torch.Tensor, gt: torch.Tensor, max_val: float = 1.0) -> torch.Tensor:
    """(N, 5, 2) fp32: per image and pyramid level the mean SSIM and the mean contrast-structure term of multi-scale
    SSIM (hn_msssim_forward: one launch per level and one that adds the tiles' sums, bit-reproducible).  pred / gt:
    (N, C, H, W) fp32 on the GPU, any element strides, any H, W >= 1 (the window shrinks to min(11, h, w)).  A metric:
    the result carries no gradient.  The host plan (taps, sizes, workspace size) is cached per shape; the workspace
    itself comes from torch's allocator at every call, as ssim_dssim's does, so a call captured in a HIP graph takes it
    from the graph's pool and the host arrays are consumed at the launch."""
    _check_pair("ms_ssim", pred, gt)
    L.require_gpu(pred, gt)
    x, y = pred.detach(), gt.detach()
    n, c, h, w = x.shape
    taps, sizes, ws_floats = _msssim_plan(n, c, h, w)
    ws = torch.empty(ws_floats, dtype=torch.float32, device=x.device)
    out = torch.empty((n, MSSSIM_LEVELS, 2), dtype=torch.float32, device=x.device)
    L.launch("hn_msssim_forward", L.ptr(x), (C.c_int64 * 4)(*x.stride()), L.ptr(y), (C.c_int64 * 4)(*y.stride()),
             n, c, h, w, taps, sizes, (0.01 * max_val) ** 2, (0.03 * max_val) ** 2, L.ptr(out), L.ptr(ws),
             L.stream_handle())
    return out
