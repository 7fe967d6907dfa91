"""The data path on the device (csrc/hn_data.hip): ray generation, in-graph batch gathers, the RGBA white blend and
Pillow's LANCZOS resize restated byte for byte."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import _lib as L

__all__ = ["NERFIES_CAM_FLOATS", "generate_rays", "ray_batch", "ray_batch_rgba", "generate_rays_nerfies",
           "ray_batch_nerfies", "blend_white_u8", "resize_lanczos_u8", "premultiply_u8", "resize_lanczos_rgba8"]


# --------------------------------------------------------------------------------------------
# on-device ray generation
# --------------------------------------------------------------------------------------------
def _generate_rays(entry: str, h: int, w: int, name: str, table: torch.Tensor, shape: tuple, before: tuple, after: tuple,
                   near: float, far: float, image_id: Optional[int]) -> torch.Tensor:
    """Allocate the (h*w, 8|9) rows of one image and launch `entry` over them; `table` (the pose or camera record, of
    `shape`) sits between the entry's own arguments `before` and `after`."""
    L.require_gpu(table)
    L.load()
    if tuple(table.shape) != shape:
        raise L.HnError(f"{name} must be {shape}")
    t = table.detach().contiguous().float()
    cols = 9 if image_id is not None else 8
    rays = torch.empty(h * w, cols, dtype=torch.float32, device=table.device)
    L.launch(entry, h, w, *before, L.ptr(t), *after, near, far, float(image_id or 0), cols, L.ptr(rays), L.stream_handle())
    return rays


def generate_rays(h: int, w: int, focal: float, c2w: torch.Tensor, near: float, far: float, ndc: bool = False,
                  ndc_near: float = 1.0, image_id: Optional[int] = None) -> torch.Tensor:
    """(h*w, 8|9) ray rows [o, d, near, far(, image id)] of one image, generated on the GPU
    (reference: datasets/ray_utils.py get_ray_directions / get_rays / get_ndc_rays, datasets/llff.py:244-264)."""
    return _generate_rays("hn_generate_rays", h, w, "c2w", c2w, (3, 4), (focal,), (int(ndc), ndc_near), near, far,
                          image_id)


def _ray_batch(entry: str, channels: int, table_row: tuple, before: tuple, after: tuple, perm, state, batch, h, w, table,
               px8, rays, rgbs, near, far, image_ids) -> None:
    """Validate and launch one gather entry: `table` is the per-image pose or camera table, (n_images, *table_row),
    between the entry's own arguments `before` and `after`; `px8` the (n_images, h, w, channels) uint8 stack."""
    L.require_gpu(perm, state, table, px8, rays, rgbs, image_ids)
    L.load()
    cols = rays.shape[1]
    n_img = px8.shape[0]
    ok = (perm.dtype == torch.int64 and perm.is_contiguous() and state.dtype == torch.int64 and state.numel() >= 3
          and table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (n_img,) + table_row
          and px8.dtype == torch.uint8 and px8.is_contiguous() and tuple(px8.shape[1:]) == (h, w, channels)
          and rays.dtype == torch.float32 and rays.is_contiguous() and cols in (8, 9) and rays.shape[0] >= batch
          and rgbs.dtype == torch.float32 and rgbs.is_contiguous() and tuple(rgbs.shape[1:]) == (3,)
          and rgbs.shape[0] >= batch and 0 < batch and perm.numel() > 0
          and (cols == 8 or (image_ids is not None and image_ids.dtype == torch.float32 and image_ids.numel() >= n_img)))
    if not ok:
        raise L.HnError(f"{entry[3:]}: bad shapes / dtypes")
    L.launch(entry, L.ptr(perm), perm.numel(), L.ptr(state), batch, px8.numel() // channels, h, w, *before, L.ptr(table),
             L.ptr(image_ids if cols == 9 else None), *after, near, far, cols, L.ptr(px8), L.ptr(rays), L.ptr(rgbs),
             L.stream_handle())


def ray_batch(perm: torch.Tensor, state: torch.Tensor, batch: int, h: int, w: int, focal: float, c2w: torch.Tensor,
              rgb8: torch.Tensor, rays: torch.Tensor, rgbs: torch.Tensor, near: float, far: float, ndc: bool = False,
              ndc_near: float = 1.0, image_ids: Optional[torch.Tensor] = None) -> None:
    """One training batch gathered on the GPU (hn_ray_batch): rows perm[cursor : cursor + batch] of the dataset whose
    rays are the pixels of `rgb8` ((n_images, h, w, 3) uint8) seen through `c2w` ((n_images, 3, 4) fp32), written into
    rays[:batch] ((B, 8|9) fp32, column 8 = image_ids[slot] when rays has 9 columns) and rgbs[:batch] ((B, 3) fp32).
    `state` (3 int64 words: cursor, arrival counter, error flag) is advanced by `batch` on the device: no host sync.
    A row whose position lies past the permutation, or whose index lies outside the dataset, is written as NaN and sets
    the error flag."""
    _ray_batch("hn_ray_batch", 3, (3, 4), (focal,), (int(ndc), ndc_near), perm, state, batch, h, w, c2w, rgb8, rays, rgbs,
               near, far, image_ids)


def ray_batch_rgba(perm: torch.Tensor, state: torch.Tensor, batch: int, h: int, w: int, focal: float,
                   c2w: torch.Tensor, rgba8: torch.Tensor, rays: torch.Tensor, rgbs: torch.Tensor, near: float,
                   far: float, ndc: bool = False, ndc_near: float = 1.0,
                   image_ids: Optional[torch.Tensor] = None) -> None:
    """`ray_batch` over an RGBA stack ((n_images, h, w, 4) uint8, hn_ray_batch_rgba): rgbs[:batch] is each pixel
    blended onto white as `blend_white_u8` computes it, in the same launch."""
    _ray_batch("hn_ray_batch_rgba", 4, (3, 4), (focal,), (int(ndc), ndc_near), perm, state, batch, h, w, c2w, rgba8, rays,
               rgbs, near, far, image_ids)


NERFIES_CAM_FLOATS = L.HN_NERFIES_CAM_FLOATS    # hn_kernels.h: orientation 9, position 3, f, aspect, skew, cx, cy, k1 k2 k3, p1 p2, 2 zeros


def generate_rays_nerfies(h: int, w: int, cam: torch.Tensor, near: float, far: float,
                          image_id: Optional[int] = None) -> torch.Tensor:
    """(h*w, 8|9) ray rows [o, d, near, far(, image id)] of one image of a Nerfies-format capture, generated on the GPU
    (hn_generate_rays_nerfies) from its camera record `cam` ((24,) fp32, datasets.nerfies.camera_record): pixel
    centres at (i + 0.5, j + 0.5), principal point, skew, pixel aspect ratio, and 10 Newton steps that undo the radial
    and tangential distortion."""
    return _generate_rays("hn_generate_rays_nerfies", h, w, "cam", cam, (NERFIES_CAM_FLOATS,), (), (), near, far,
                          image_id)


def ray_batch_nerfies(perm: torch.Tensor, state: torch.Tensor, batch: int, h: int, w: int, cams: torch.Tensor,
                      rgb8: torch.Tensor, rays: torch.Tensor, rgbs: torch.Tensor, near: float, far: float,
                      image_ids: Optional[torch.Tensor] = None) -> None:
    """`ray_batch` over a Nerfies-format capture (hn_ray_batch_nerfies): `cams` is the (n_images, 24) fp32 table of
    camera records and rays[:batch] holds the rows `generate_rays_nerfies` writes for those pixels, bit for bit (one
    device function); perm, state, rgb8, rgbs, image_ids and the NaN rows are `ray_batch`'s."""
    _ray_batch("hn_ray_batch_nerfies", 3, (NERFIES_CAM_FLOATS,), (), (), perm, state, batch, h, w, cams, rgb8, rays,
               rgbs, near, far, image_ids)


def blend_white_u8(rgba8: torch.Tensor, with_mask: bool = False):
    """(..., 4) uint8 RGBA -> (N, 3) fp32 `rgb * a + (1 - a)` on u8 / 255 values, bit for bit the reference's blend
    (datasets/blender.py:58; hn_blend_white_u8: a multiply, a subtraction and an addition, each rounded).  With
    `with_mask` also the (N,) bool mask a > 0 (blender.py:93): returns (rgbs, mask)."""
    L.require_gpu(rgba8)
    L.load()
    if rgba8.dtype != torch.uint8 or rgba8.dim() < 1 or rgba8.shape[-1] != 4 or rgba8.numel() == 0:
        raise L.HnError("blend_white_u8: (..., 4) uint8")
    x = rgba8.contiguous()
    n = x.numel() // 4
    rgbs = torch.empty((n, 3), dtype=torch.float32, device=x.device)
    mask = torch.empty(n, dtype=torch.bool, device=x.device) if with_mask else None
    L.launch("hn_blend_white_u8", L.ptr(x), n, L.ptr(rgbs), L.ptr(mask), L.stream_handle())
    return (rgbs, mask) if with_mask else rgbs


_RESAMPLE_TABLES: Dict[tuple, tuple] = {}


def _resample_tables(in_size: int, out_size: int, device):
    key = (in_size, out_size, str(device))
    t = _RESAMPLE_TABLES.get(key)
    if t is None:
        from ..datasets.image_io import lanczos_tables
        bounds, kk, ksize = lanczos_tables(in_size, out_size)
        if not ((bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 0).all() and (bounds.sum(1) <= in_size).all()
                and (bounds[:, 1] <= ksize).all()):
            raise L.HnError("resize: coefficient bounds outside the input")
        t = _RESAMPLE_TABLES[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize)
    return t


def resize_lanczos_u8(img: torch.Tensor, size) -> torch.Tensor:
    """Pillow's `Image.resize(size, Image.LANCZOS)` of an 8-bit (H, W, C) image on the GPU, byte for byte: the
    horizontal pass first (uint8 intermediate), then the vertical one; a pass whose axis keeps its length is skipped.
    size = (width, height) as Pillow takes it."""
    L.require_gpu(img)
    L.load()
    if img.dtype != torch.uint8 or img.dim() != 3 or not 1 <= img.shape[2] <= 4:
        raise L.HnError("resize_lanczos_u8: (H, W, C) uint8, C <= 4")
    out_w, out_h = int(size[0]), int(size[1])
    if out_w <= 0 or out_h <= 0:
        raise L.HnError("resize_lanczos_u8: the size must be positive")
    x = img.contiguous()
    h, w, c = x.shape
    if out_w != w:
        bounds, kk, ksize = _resample_tables(w, out_w, x.device)
        y = torch.empty((h, out_w, c), dtype=torch.uint8, device=x.device)
        L.launch("hn_resample_u8", L.ptr(x), h, w, c, out_w, 0, L.ptr(bounds), L.ptr(kk), ksize, L.ptr(y), L.stream_handle())
        x, w = y, out_w
    if out_h != h:
        bounds, kk, ksize = _resample_tables(h, out_h, x.device)
        y = torch.empty((out_h, w, c), dtype=torch.uint8, device=x.device)
        L.launch("hn_resample_u8", L.ptr(x), h, w, c, out_h, 1, L.ptr(bounds), L.ptr(kk), ksize, L.ptr(y), L.stream_handle())
        x = y
    return x if x is not img else x.clone()


def premultiply_u8(img: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Pillow's RGBA -> RGBa conversion of an (H, W, 4) uint8 image (hn_premultiply_u8), or with `inverse` RGBa ->
    RGBA: both round, alpha stays."""
    L.require_gpu(img)
    L.load()
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 4 or img.numel() == 0:
        raise L.HnError("premultiply_u8: (H, W, 4) uint8")
    x = img.contiguous()
    out = torch.empty_like(x)
    L.launch("hn_premultiply_u8", L.ptr(x), x.numel() // 4, int(inverse), L.ptr(out),
             L.stream_handle())
    return out


def resize_lanczos_rgba8(img: torch.Tensor, size) -> torch.Tensor:
    """Pillow's `Image.resize(size, Image.LANCZOS)` of an 8-bit RGBA (H, W, 4) image on the GPU, byte for byte: Pillow
    resamples such an image in premultiplied alpha, so the colour bytes are premultiplied, the four channels go
    through the passes of `resize_lanczos_u8`, and the colours are divided by the new alpha.  At equal size Pillow
    returns a copy, without that round trip (it would change bytes).  size = (width, height)."""
    L.require_gpu(img)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 4:
        raise L.HnError("resize_lanczos_rgba8: (H, W, 4) uint8")
    out_w, out_h = int(size[0]), int(size[1])
    if (out_h, out_w) == tuple(img.shape[:2]):
        return img.clone(memory_format=torch.contiguous_format)
    return premultiply_u8(resize_lanczos_u8(premultiply_u8(img), (out_w, out_h)), inverse=True)
