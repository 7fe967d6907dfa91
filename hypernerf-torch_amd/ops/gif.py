"""GIF of the evaluated frames, depth image of the validation step (csrc/hn_gif.hip): the colour histogram and the
palette map that quantise frames on the device, the library's host LZW coder, the depth colour map."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib as L

__all__ = ["HIST_BINS", "color_histogram", "palette_map", "gif_lzw", "depth_colormap"]

HIST_BINS = L.HN_HIST_BINS


def _check_pixels(pixels, what: str) -> torch.Tensor:
    if not isinstance(pixels, torch.Tensor) or pixels.dtype != torch.uint8 or pixels.dim() < 1 or pixels.shape[-1] != 3:
        raise ValueError(f"{what}: pixels must be a (..., 3) uint8 tensor")
    if pixels.numel() == 0 or pixels.numel() // 3 > 2 ** 31:
        raise ValueError(f"{what}: 1 .. 2**31 pixels, got {pixels.numel() // 3}")
    L.require_gpu(pixels)
    return pixels.detach().contiguous()


@torch.no_grad()
def color_histogram(pixels: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(2^18, 4) int64 table of the packed 8-bit RGB `pixels` (..., 3): cell (r>>2)<<12 | (g>>2)<<6 | b>>2 holds
    [pixels, sum r, sum g, sum b] (hn_color_hist: integer adds, exact and independent of their order).  `out`: a table to
    ADD to (several frames, one table); a fresh zeroed one otherwise."""
    px = _check_pixels(pixels, "color_histogram")
    if out is None:
        out = torch.zeros((HIST_BINS, 4), dtype=torch.int64, device=px.device)
    elif (out.dtype != torch.int64 or tuple(out.shape) != (HIST_BINS, 4) or not out.is_contiguous()
          or out.device != px.device):
        raise ValueError(f"color_histogram: out must be a contiguous ({HIST_BINS}, 4) int64 tensor on {px.device}")
    L.load()
    with torch.cuda.device(px.device):
        L.launch("hn_color_hist", L.ptr(px), px.numel() // 3, L.ptr(out), L.stream_handle())
    return out


@torch.no_grad()
def palette_map(pixels: torch.Tensor, palette: torch.Tensor) -> torch.Tensor:
    """(...,) uint8: for every packed RGB pixel of `pixels` (..., 3) the index of the nearest of the 1..256 entries of
    `palette` (K, 3) uint8 in squared RGB distance, the smallest index among equals (hn_palette_map)."""
    if (not isinstance(palette, torch.Tensor) or palette.dtype != torch.uint8 or palette.dim() != 2
            or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256):
        raise ValueError("palette_map: palette must be a (1..256, 3) uint8 tensor")
    px = _check_pixels(pixels, "palette_map")
    pal = palette.detach().to(px.device).contiguous()
    out = torch.empty(px.shape[:-1], dtype=torch.uint8, device=px.device)
    L.load()
    with torch.cuda.device(px.device):
        L.launch("hn_palette_map", L.ptr(px), px.numel() // 3, L.ptr(pal), pal.shape[0], L.ptr(out), L.stream_handle())
    return out


def gif_lzw(indices) -> bytes:
    """The raw code bytes of GIF's LZW (minimum code size 8) of a uint8 index stream — array, tensor or bytes, on the
    host (hn_gif_lzw: host C++ in the library; no GPU is involved)."""
    import numpy as np
    if isinstance(indices, torch.Tensor):
        indices = indices.detach().cpu().numpy()
    if isinstance(indices, (bytes, bytearray)):
        indices = np.frombuffer(bytes(indices), dtype=np.uint8)
    a = np.asarray(indices)
    if a.dtype != np.uint8:
        raise ValueError(f"gif_lzw: indices must be uint8, got {a.dtype}")
    a = np.ascontiguousarray(a).reshape(-1)
    n = a.size
    # at most n + 2 codes and one clear per 3838 of them, 12 bits each
    cap = ((n + 3 + n // 3838 + 1) * 12 + 7) // 8
    out = np.empty(cap, dtype=np.uint8)
    out_len = C.c_longlong(0)
    L.check(L.load().hn_gif_lzw(a.ctypes.data if n else None, n, out.ctypes.data, cap, C.byref(out_len)), "hn_gif_lzw")
    return out[:out_len.value].tobytes()


@torch.no_grad()
def depth_colormap(depth: torch.Tensor, lut: torch.Tensor, return_range: bool = False):
    """(H, W, 3) uint8 = lut[(uint8)(255 * (d - min) / (max - min + 1e-8))] of d = nan_to_num(depth), depth (H, W) fp32
    and lut (256, 3) uint8: the array visualize_depth colours (utils/visualization.py:10-16) — hn_depth_range, then
    hn_depth_colormap reading the range from the device, no host synchronisation.  A NaN quotient (both infinities in
    one map) gives index 0.  `return_range`: also the (2,) fp32 device tensor [min, max]."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.dim() != 2 or depth.numel() == 0:
        raise ValueError("depth_colormap: depth must be a non-empty (H, W) float32 tensor")
    if (not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3)):
        raise ValueError("depth_colormap: lut must be a (256, 3) uint8 tensor")
    L.require_gpu(depth)
    d = depth.detach().contiguous()
    table = lut.detach().to(d.device).contiguous()
    rng = torch.empty(2, dtype=torch.float32, device=d.device)
    out = torch.empty(tuple(d.shape) + (3,), dtype=torch.uint8, device=d.device)
    L.load()
    with torch.cuda.device(d.device):
        stream = L.stream_handle()
        L.launch("hn_depth_range", L.ptr(d), d.numel(), L.ptr(rng), stream)
        L.launch("hn_depth_colormap", L.ptr(d), d.numel(), L.ptr(rng), L.ptr(table), L.ptr(out), stream)
    return (out, rng) if return_range else out
