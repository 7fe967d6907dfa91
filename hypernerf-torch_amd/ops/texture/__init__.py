"""Texture atlas (csrc/hn_texture.hip): the class of every face, the cell layout, the rasteriser of the
atlas texels into 3-D and the sampler that shades a traced image from a texture; and the host arithmetic between them:
argument checks, cells per side, the atlas size."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _lib as L
from ..checks import INT32_MAX, check_mesh_faces, check_points, check_rays
from ..mesh_render import check_shading

__all__ = ["TEX_MIN_SIDE", "TEX_MAX_SIDE", "TEX_MAX_ATLAS", "TEX_GUTTER", "TEX_CLASSES", "TEX_FILTERS", "check_cells_arg",
           "check_texel", "check_max_size", "class_cells", "atlas_size", "check_atlas_fits", "check_atlas", "check_texture", "face_classes",
           "atlas_layout", "atlas_rasterize", "texture_shade"]

# mirrors of csrc/hn_texture.hip's limits (no macros in the header: its set of constants is that of ABI 340)
TEX_MIN_SIDE = 16          # the smallest cell side
TEX_MAX_SIDE = 1024        # the largest
TEX_MAX_ATLAS = 16384      # atlas sides
TEX_GUTTER = 7             # a cell of side s holds charts of L = s - 7 texels
TEX_CLASSES = 7            # sides 1024 >> q, q = 0 .. 6
TEX_FILTERS = {'nearest': 0, 'bilinear': 1}


def _pow2(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool) and x > 0 and (int(x) & (int(x) - 1)) == 0


def check_cells_arg(min_cell, max_cell, what: str) -> Tuple[int, int]:
    """(min_cell, max_cell) as ints: powers of two with 16 <= min_cell <= max_cell <= 1024, or ValueError."""
    if not _pow2(min_cell) or not _pow2(max_cell):
        raise ValueError(f"{what}: min_cell and max_cell must be powers of two, got {min_cell!r} and {max_cell!r}")
    if not TEX_MIN_SIDE <= int(min_cell) <= int(max_cell) <= TEX_MAX_SIDE:
        raise ValueError(f"{what}: cell sides must satisfy {TEX_MIN_SIDE} <= min_cell <= max_cell <= {TEX_MAX_SIDE}, "
                         f"got {min_cell} and {max_cell}")
    return int(min_cell), int(max_cell)


def check_texel(texel, what: str) -> float:
    """The texel length as the float32 the kernels take, positive and finite, or ValueError."""
    try:
        with np.errstate(over="ignore"):
            t = float(np.float32(float(texel)))
    except (TypeError, ValueError):
        t = float("nan")
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"{what}: texel must be a positive finite float32 length, got {texel!r}")
    return t


def check_max_size(max_size, what: str, name: str = "max_size") -> int:
    if isinstance(max_size, bool) or not isinstance(max_size, (int, np.integer)) or not 1 <= int(max_size) <= TEX_MAX_ATLAS:
        raise ValueError(f"{what}: {name} must be an int in 1 .. {TEX_MAX_ATLAS}, got {max_size!r}")
    return int(max_size)


def class_cells(hist: Sequence[int]) -> Tuple[list, list]:
    """(first sorted rank, first cell) of every side 1024 >> q, q = 0 .. 6, each with the total appended (8 entries), from
    hist[k] = the faces of side 2**k (k = 0 .. 10): faces in descending side order, two to a cell."""
    ranks, cells = [0], [0]
    for q in range(TEX_CLASSES):
        n = int(hist[10 - q])
        ranks.append(ranks[-1] + n)
        cells.append(cells[-1] + (n + 1) // 2)
    return ranks, cells


def atlas_size(hist: Sequence[int], min_cell: int) -> Tuple[int, int]:
    """(W_t, H_t) of the atlas of the faces counted in hist (class_cells): the cells' areas in units of min_cell^2 add up
    to `total`; W_t = min_cell * 2^m with the smallest m whose square 4^m holds it, H_t = W_t / 2 when m >= 1 and the total
    fits the first half of the Z-order (2 total <= 4^m), else W_t.  An empty mesh gets one empty cell's worth."""
    _, cells = class_cells(hist)
    total = sum((cells[q + 1] - cells[q]) * ((TEX_MAX_SIDE >> q) // min_cell) ** 2 for q in range(TEX_CLASSES)
                if (TEX_MAX_SIDE >> q) >= min_cell)
    m = 0
    while 4 ** m < total:
        m += 1
    w = min_cell << m
    return w, (w // 2 if m >= 1 and 2 * total <= 4 ** m else w)


def check_atlas_fits(hist: Sequence[int], min_cell: int, max_size: int, what: str) -> Tuple[int, int]:
    """atlas_size(hist, min_cell), or ValueError naming it when it is wider than max_size."""
    w, h = atlas_size(hist, min_cell)
    if w > max_size:
        raise ValueError(f"{what}: the atlas needs {w} x {h} texels, max_size is {max_size}: use a larger texel "
                         "(atlas_texel_for_size finds one) or raise max_size")
    return w, h


@torch.no_grad()
def face_classes(vertices: torch.Tensor, faces: torch.Tensor, texel: float, min_cell: int, max_cell: int, what: str):
    """(class (F,) int32 = log2 of every face's cell side, keys (F,) int64, hist = the faces per class as 11 host ints) of
    hn_tex_classify; F >= 1.  ONE host read: the histogram and the error flag.  ValueError: a vertex id outside [0, V)."""
    dev, v, n_faces = vertices.device, vertices.shape[0], faces.shape[0]
    if v == 0:
        raise ValueError(f"{what}: faces hold a vertex id outside [0, 0)")
    L.load()
    with torch.cuda.device(dev):
        cls = torch.empty(n_faces, dtype=torch.int32, device=dev)
        keys = torch.empty(n_faces, dtype=torch.int64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        L.launch("hn_tex_classify", L.ptr(vertices), v, L.ptr(faces), n_faces, texel, min_cell, max_cell, L.ptr(cls),
                 L.ptr(keys), L.ptr(err), L.stream_handle())
        read = torch.cat([torch.bincount(cls.long(), minlength=11)[:11], err.to(torch.int64)]).tolist()
    if read[11]:
        raise ValueError(f"{what}: faces hold a vertex id outside [0, {v})")
    return cls, keys, read[:11]


@torch.no_grad()
def atlas_layout(keys: torch.Tensor, hist: Sequence[int], min_cell: int):
    """(cell_start (n_cells, 2), cell_side (n_cells,), cell_face (n_cells, 2), all int32, uv (F, 3, 2) fp32) of the faces
    with face_classes' keys and histogram: one torch.sort of the keys (they are unique), then hn_tex_layout."""
    dev, n_faces = keys.device, keys.shape[0]
    ranks, cells = class_cells(hist)
    n_cells = cells[-1]
    with torch.cuda.device(dev):
        ordered = torch.sort(keys).values
        cell_start = torch.empty((n_cells, 2), dtype=torch.int32, device=dev)
        cell_side = torch.empty(n_cells, dtype=torch.int32, device=dev)
        cell_face = torch.empty((n_cells, 2), dtype=torch.int32, device=dev)
        uv = torch.empty((n_faces, 3, 2), dtype=torch.float32, device=dev)
        L.launch("hn_tex_layout", L.ptr(ordered), n_faces, (C.c_int64 * (TEX_CLASSES + 1))(*ranks), min_cell, n_cells,
                 L.ptr(cell_start), L.ptr(cell_side), L.ptr(cell_face), L.ptr(uv), L.stream_handle())
    return cell_start, cell_side, cell_face, uv


def check_atlas(atlas, n_faces: Optional[int], what: str) -> Dict:
    """The atlas dict texture_atlas returns, checked as far as the host can, or ValueError."""
    try:
        uv, (w, h), cell_start, cell_side, cell_face = (atlas[k] for k in ('uv', 'size', 'cell_start', 'cell_side', 'cell_face'))
        min_cell, cells = int(atlas['min_cell']), [int(c) for c in atlas['class_cells']]
        w, h, n_cells = int(w), int(h), cell_side.shape[0]
        ok = (uv.dtype == torch.float32 and uv.dim() == 3 and tuple(uv.shape[1:]) == (3, 2) and uv.is_contiguous()
              and cell_start.dtype == cell_side.dtype == cell_face.dtype == torch.int32
              and tuple(cell_start.shape) == (n_cells, 2) and tuple(cell_face.shape) == (n_cells, 2) and cell_face.is_contiguous()
              and len(cells) == TEX_CLASSES + 1 and cells[0] == 0 and cells[-1] == n_cells
              and all(a <= b for a, b in zip(cells, cells[1:])) and _pow2(min_cell) and TEX_MIN_SIDE <= min_cell <= TEX_MAX_SIDE
              and 1 <= w <= TEX_MAX_ATLAS and 1 <= h <= TEX_MAX_ATLAS and w % min_cell == 0 and h % min_cell == 0
              and len({uv.device, cell_start.device, cell_side.device, cell_face.device}) == 1)
    except (KeyError, TypeError, ValueError, AttributeError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: atlas must be the dict texture_atlas returns")
    if n_faces is not None and uv.shape[0] != n_faces:
        raise ValueError(f"{what}: the atlas lays out {uv.shape[0]} faces, the mesh has {n_faces}")
    return atlas


def check_texture(texture, atlas, what: str, dtypes=(torch.uint8, torch.float32)) -> torch.Tensor:
    """An (H_t, W_t, 3) texture of the atlas in one of `dtypes`, contiguous, or ValueError."""
    w, h = (int(x) for x in atlas['size'])
    names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
    if not isinstance(texture, torch.Tensor) or texture.dtype not in dtypes:
        raise ValueError(f"{what}: texture must be a {names} tensor, got "
                         f"{texture.dtype if isinstance(texture, torch.Tensor) else type(texture).__name__}")
    if tuple(texture.shape) != (h, w, 3):
        raise ValueError(f"{what}: texture is {tuple(texture.shape)}, the atlas is ({h}, {w}, 3)")
    return texture.detach().contiguous()


@torch.no_grad()
def atlas_rasterize(vertices: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor], atlas: Dict):
    """{'owner': (H_t, W_t) int32, 'position': (H_t, W_t, 3) fp32, 'normal': (H_t, W_t, 3) fp32} of hn_tex_rasterize: per
    texel the face whose chart owns it (-1: nobody), the point of that face's plane under the texel centre (extrapolated
    outside the triangle, never clamped) and the unit normal there; zeros where nobody owns the texel."""
    what = "atlas_rasterize"
    vertices = check_points(vertices, what, "vertices")
    faces = check_mesh_faces(faces, what)
    v, n_faces = vertices.shape[0], faces.shape[0]
    if normals is not None:
        normals = check_points(normals, what, "normals", v)
    atlas = check_atlas(atlas, n_faces, what)
    cell_face = atlas['cell_face']
    L.require_gpu(vertices, faces, normals, cell_face)
    dev = vertices.device
    if any(t.device != dev for t in (faces, cell_face) + (() if normals is None else (normals,))):
        raise ValueError(f"{what}: the mesh and the atlas must live on one device")
    (w, h), n_cells = atlas['size'], cell_face.shape[0]
    if n_cells and v == 0:
        raise ValueError(f"{what}: faces hold a vertex id outside [0, 0)")
    out = {'owner': torch.empty((h, w), dtype=torch.int32, device=dev),
           'position': torch.empty((h, w, 3), dtype=torch.float32, device=dev),
           'normal': torch.empty((h, w, 3), dtype=torch.float32, device=dev)}
    L.load()
    with torch.cuda.device(dev):
        L.launch("hn_tex_rasterize", L.ptr(vertices) if n_cells else None, v, L.ptr(faces) if n_cells else None, n_faces,
                 L.ptr(normals) if n_cells else None, L.ptr(cell_face) if n_cells else None, n_cells,
                 (C.c_int64 * (TEX_CLASSES + 1))(*[int(c) for c in atlas['class_cells']]), int(atlas['min_cell']), int(h), int(w),
                 L.ptr(out['owner']), L.ptr(out['position']), L.ptr(out['normal']), L.stream_handle())
    return out


@torch.no_grad()
def texture_shade(vertices: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor], atlas: Dict,
                  texture: torch.Tensor, rays: torch.Tensor, face: torch.Tensor, bary: torch.Tensor,
                  shading: str = 'headlight', ambient: float = 0.3, background=(1.0, 1.0, 1.0),
                  filter: str = 'bilinear') -> Dict[str, torch.Tensor]:
    """{'normal': (P, 3) fp32, 'rgb': (P, 3) fp32, 'rgb8': (P, 3) uint8} of the pixels mesh_trace resolved (hn_tex_shade):
    ops.mesh_render.mesh_shade with the colour fetched from `texture` (H_t, W_t, 3) uint8 (/ 255) or fp32 at (u, v) = the
    pixel's barycentric mix of the face's atlas corners, clamped to the chart's bounding box; filter 'bilinear' (the four
    texels around (u, v), all inside the face's own chart) or 'nearest' (the one under it)."""
    what = "texture_shade"
    vertices = check_points(vertices, what, "vertices")
    faces = check_mesh_faces(faces, what)
    v, n_faces = vertices.shape[0], faces.shape[0]
    if normals is not None:
        normals = check_points(normals, what, "normals", v)
    atlas = check_atlas(atlas, n_faces, what)
    texture = check_texture(texture, atlas, what)
    if filter not in TEX_FILTERS:
        raise ValueError(f"{what}: filter must be one of {tuple(TEX_FILTERS)}, got {filter!r}")
    headlight, ambient, background, _ = check_shading(shading, ambient, background, (0.0, 0.0, 0.0), what)
    if not isinstance(face, torch.Tensor) or face.dim() != 1 or face.dtype != torch.int32:
        raise ValueError(f"{what}: face must be a (P,) int32 tensor")
    n = face.shape[0]
    if not isinstance(bary, torch.Tensor) or tuple(bary.shape) != (n, 3) or bary.dtype != torch.float32:
        raise ValueError(f"{what}: bary must be a ({n}, 3) float32 tensor")
    if n > INT32_MAX:
        raise ValueError(f"{what}: {n} pixels exceed 2**31 - 1 = {INT32_MAX}")
    rays = check_rays(rays, n, what)
    face, bary, uv = face.detach().contiguous(), bary.detach().contiguous(), atlas['uv']
    L.require_gpu(vertices, faces, normals, uv, texture, rays, face, bary)
    dev = face.device
    if any(t.device != dev for t in (vertices, faces, uv, texture, rays, bary) + (() if normals is None else (normals,))):
        raise ValueError(f"{what}: every tensor must live on one device")
    out = {'normal': torch.empty((n, 3), dtype=torch.float32, device=dev),
           'rgb': torch.empty((n, 3), dtype=torch.float32, device=dev),
           'rgb8': torch.empty((n, 3), dtype=torch.uint8, device=dev)}
    if n:
        L.load()
        with torch.cuda.device(dev):
            L.launch("hn_tex_shade", L.ptr(vertices) if v else None, v, L.ptr(faces) if n_faces else None, n_faces,
                     L.ptr(normals) if v else None, L.ptr(uv) if n_faces else None, L.ptr(texture),
                     1 if texture.dtype == torch.uint8 else 2, texture.shape[0], texture.shape[1], TEX_FILTERS[filter],
                     L.ptr(rays), rays.shape[1], n, L.ptr(face), L.ptr(bary), headlight, ambient, background,
                     L.ptr(out['normal']), L.ptr(out['rgb']), L.ptr(out['rgb8']), L.stream_handle())
    return out
