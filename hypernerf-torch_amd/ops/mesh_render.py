"""Mesh rendering by ray casting (csrc/hn_mesh_render.hip): projection, tile binning, tracing, shading."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from .. import _lib as L
from .checks import INT32_MAX, check_camera, check_mesh_faces, check_points, check_rays

__all__ = ["MESH_TILE", "MESH_MAX_SIDE", "SHADINGS", "check_image_wh", "mesh_project", "mesh_tile_pairs",
           "group_tile_pairs", "mesh_bins", "mesh_trace", "check_shading", "mesh_shade"]

MESH_TILE = L.HN_MESH_TILE    # pixels per tile side of hn_mesh_trace
MESH_MAX_SIDE = L.HN_MESH_MAX_SIDE    # image sides the mesh renderer takes


def check_image_wh(image_wh, what: str):
    """(W, H) as two ints within 1 .. 65535, or ValueError."""
    try:
        w, h = (int(v) for v in image_wh)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: image_wh must be (W, H), got {image_wh!r}") from None
    if not (1 <= w <= MESH_MAX_SIDE and 1 <= h <= MESH_MAX_SIDE):
        raise ValueError(f"{what}: image sides must be 1 .. {MESH_MAX_SIDE}, got {w} x {h}")
    return w, h


@torch.no_grad()
def mesh_project(vertices: torch.Tensor, camera: torch.Tensor):
    """(pix (V, 2) fp32, flags (V,) int32) of vertices (V, 3) fp32 through the forward model of the 24-float camera record
    (hn_mesh_project): pixel coordinates with pixel (i, j) covering [i, i + 1) x [j, j + 1); flag 1 for z <= 1e-6 in the
    camera frame, 2 where the radial distortion folds or a coordinate is not finite (pix is then (0, 0))."""
    vertices = check_points(vertices, "mesh_project", "vertices")
    camera = check_camera(camera, "mesh_project")
    L.require_gpu(vertices)
    v, dev = vertices.shape[0], vertices.device
    pix = torch.empty((v, 2), dtype=torch.float32, device=dev)
    flags = torch.empty(v, dtype=torch.int32, device=dev)
    if v:
        L.load()
        camera = camera.to(dev)
        with torch.cuda.device(dev):
            L.launch("hn_mesh_project", L.ptr(vertices), v, L.ptr(camera), L.ptr(pix), L.ptr(flags), L.stream_handle())
    return pix, flags


@torch.no_grad()
def mesh_tile_pairs(vertices: torch.Tensor, faces: torch.Tensor, camera: torch.Tensor, image_wh, pix: torch.Tensor,
                    vflags: torch.Tensor, fill: bool = True):
    """(pair_tile, pair_face): two (n_pairs,) int32 tensors, the (tile, face) pairs of the W x H image in ascending face
    order, a face's tiles row by row — hn_mesh_bin_count, torch.cumsum, ONE host read (the pair count and the error
    flag), hn_mesh_bin_fill.  vertices (V >= 1, 3), faces (F >= 1, 3), camera on their device; pix / vflags: mesh_project's.
    fill=False stops after the read and returns None (the ids are checked).  ValueError: a face holds a vertex id
    outside [0, V); more than 2**31 - 1 pairs."""
    w, h = image_wh
    dev, v, n_faces = vertices.device, vertices.shape[0], faces.shape[0]
    with torch.cuda.device(dev):
        stream = L.stream_handle()
        counts = torch.empty(n_faces, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        L.launch("hn_mesh_bin_count", L.ptr(faces), n_faces, L.ptr(vertices), L.ptr(pix), L.ptr(vflags), v, L.ptr(camera),
                 h, w, L.ptr(counts), L.ptr(err), stream)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        n_pairs, bad = torch.stack([ends[-1], err[0].to(torch.int64)]).tolist()
        if bad:
            raise ValueError(f"mesh_bins: faces hold a vertex id outside [0, {v})")
        if not fill:
            return None
        if n_pairs > INT32_MAX:
            raise ValueError(f"mesh_bins: {n_pairs} (tile, face) pairs exceed 2**31 - 1 = {INT32_MAX}")
        pair_tile = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        pair_face = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        if n_pairs:
            L.launch("hn_mesh_bin_fill", L.ptr(faces), n_faces, L.ptr(vertices), L.ptr(pix), L.ptr(vflags), v, L.ptr(camera),
                     h, w, L.ptr(ends), n_pairs, L.ptr(pair_tile), L.ptr(pair_face), stream)
    return pair_tile, pair_face


@torch.no_grad()
def group_tile_pairs(pair_tile: torch.Tensor, pair_face: torch.Tensor, n_tiles: int):
    """(tile_begin, tile_end, pair_face grouped by tile): a stable torch.sort on the tile key — the faces of a tile stay in
    ascending order — and one torch.searchsorted for where every tile begins, as simplify_faces groups its keys."""
    sorted_tile, order = torch.sort(pair_tile, stable=True)
    starts = torch.searchsorted(sorted_tile, torch.arange(n_tiles + 1, dtype=torch.int32, device=pair_tile.device))
    return starts[:-1].contiguous(), starts[1:].contiguous(), pair_face[order].contiguous()


@torch.no_grad()
def mesh_bins(vertices: torch.Tensor, faces: torch.Tensor, camera: torch.Tensor, image_wh, binning: bool = True):
    """(tile_begin, tile_end, pair_face): the faces every 16 x 16 tile of the W x H image must test are
    pair_face[tile_begin[T] : tile_end[T]] (int64 bounds, int32 face ids ascending within a tile), tile T = ty * ceil(W / 16)
    + tx: mesh_project, mesh_tile_pairs (one host read), group_tile_pairs.  binning=False: every tile gets every face (no
    fill, no sort; the ids are checked all the same).  ValueError: a face holds a vertex id outside [0, V); more than
    2**31 - 1 pairs."""
    what = "mesh_bins"
    vertices = check_points(vertices, what, "vertices")
    faces = check_mesh_faces(faces, what)
    camera = check_camera(camera, what)
    w, h = check_image_wh(image_wh, what)
    L.require_gpu(vertices, faces)
    dev = vertices.device
    v, n_faces = vertices.shape[0], faces.shape[0]
    n_tiles = ((w + MESH_TILE - 1) // MESH_TILE) * ((h + MESH_TILE - 1) // MESH_TILE)
    none = torch.zeros(n_tiles, dtype=torch.int64, device=dev)
    if n_faces == 0:
        return none, none, torch.zeros(0, dtype=torch.int32, device=dev)
    if v == 0:
        raise ValueError(f"{what}: faces hold a vertex id outside [0, 0)")
    L.load()
    camera = camera.to(dev)
    pix, vflags = mesh_project(vertices, camera)
    pairs = mesh_tile_pairs(vertices, faces, camera, (w, h), pix, vflags, fill=bool(binning))
    if pairs is None:
        return none, torch.full((n_tiles,), n_faces, dtype=torch.int64, device=dev), \
            torch.arange(n_faces, dtype=torch.int32, device=dev)
    if pairs[0].numel() == 0:
        return none, none, pairs[1]
    return group_tile_pairs(pairs[0], pairs[1], n_tiles)


@torch.no_grad()
def mesh_trace(vertices: torch.Tensor, faces: torch.Tensor, rays: torch.Tensor, camera: torch.Tensor, image_wh,
               binning: bool = True, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """{'face': (H*W,) int32, 'depth': (H*W,) fp32, 'bary': (H*W, 3) fp32} of the mesh seen along rays (H*W, >= 6) fp32
    (row p = pixel p: origin, unit direction): the nearest face every ray crosses by the ray-casting definition of
    csrc/hn_mesh_render.hip (-1 / 0 / zeros where it crosses none).  `camera` only bins the faces (mesh_bins);
    binning=False tests every face at every pixel and gives the same bits (but for stray hits of near-degenerate faces,
    DESIGN.md 3.11).  `out`: contiguous tensors of those shapes to
    write into; a ValueError (a vertex id outside [0, V)) leaves them untouched."""
    what = "mesh_trace"
    vertices = check_points(vertices, what, "vertices")
    faces = check_mesh_faces(faces, what)
    w, h = check_image_wh(image_wh, what)
    n = h * w
    rays = check_rays(rays, n, what)
    L.require_gpu(vertices, faces, rays)
    dev = vertices.device
    shapes = {'face': ((n,), torch.int32), 'depth': ((n,), torch.float32), 'bary': ((n, 3), torch.float32)}
    if out is not None:
        for k, (shape, dtype) in shapes.items():
            t = out.get(k)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() \
                    or t.device != dev:
                raise ValueError(f"{what}: out['{k}'] must be a contiguous {shape} {dtype} tensor on {dev}")
    tile_begin, tile_end, pair_face = mesh_bins(vertices, faces, camera, (w, h), binning)
    if out is None:
        out = {k: torch.empty(shape, dtype=dtype, device=dev) for k, (shape, dtype) in shapes.items()}
    n_pairs = pair_face.shape[0]
    L.load()
    with torch.cuda.device(dev):
        L.launch("hn_mesh_trace", L.ptr(vertices) if n_pairs else None, vertices.shape[0], L.ptr(faces) if n_pairs else None,
                 faces.shape[0], L.ptr(rays), rays.shape[1], h, w, L.ptr(tile_begin), L.ptr(tile_end),
                 L.ptr(pair_face) if n_pairs else None, n_pairs, L.ptr(out['face']), L.ptr(out['depth']), L.ptr(out['bary']),
                 L.stream_handle())
    return {k: out[k] for k in shapes}


SHADINGS = ('headlight', 'none')


def check_shading(shading, ambient, background, base_color, what: str):
    """(headlight flag, ambient, background, base_color as (c_float * 3)) or ValueError: colours and ambient in [0, 1]."""
    if shading not in SHADINGS:
        raise ValueError(f"{what}: shading must be one of {SHADINGS}, got {shading!r}")
    try:
        ambient = float(ambient)
    except (TypeError, ValueError):
        ambient = float("nan")
    if not 0.0 <= ambient <= 1.0:
        raise ValueError(f"{what}: ambient must lie in [0, 1]")
    cols = []
    for name, col in (("background", background), ("base_color", base_color)):
        try:
            vals = [float(x) for x in col]
        except (TypeError, ValueError):
            vals = []
        if len(vals) != 3 or not all(0.0 <= x <= 1.0 for x in vals):
            raise ValueError(f"{what}: {name} must be three numbers in [0, 1], got {col!r}")
        cols.append((C.c_float * 3)(*vals))
    return int(shading == 'headlight'), ambient, cols[0], cols[1]


@torch.no_grad()
def mesh_shade(vertices: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor], colors: Optional[torch.Tensor],
               rays: torch.Tensor, face: torch.Tensor, bary: torch.Tensor, shading: str = 'headlight', ambient: float = 0.3,
               background=(1.0, 1.0, 1.0), base_color=(0.8, 0.8, 0.8)) -> Dict[str, torch.Tensor]:
    """{'normal': (P, 3) fp32, 'rgb': (P, 3) fp32, 'rgb8': (P, 3) uint8} of the pixels mesh_trace resolved (hn_mesh_shade):
    the normalised interpolated vertex normal (the face normal without `normals`), the interpolated vertex colour
    (uint8 / 255, fp32 as it is, `base_color` without `colors`) times ambient + (1 - ambient) |N . d| ('headlight') or 1
    ('none'), clamped to [0, 1]; rgb8 = floor(255 rgb + 0.5); `background` and a zero normal where face is -1."""
    what = "mesh_shade"
    vertices = check_points(vertices, what, "vertices")
    faces = check_mesh_faces(faces, what)
    v, n_faces = vertices.shape[0], faces.shape[0]
    if normals is not None:
        normals = check_points(normals, what, "normals", v)
    kind = 0
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (v, 3) or colors.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"{what}: colors must be a ({v}, 3) uint8 or float32 tensor")
        colors = colors.detach().contiguous()
        kind = 1 if colors.dtype == torch.uint8 else 2
    headlight, ambient, background, base_color = check_shading(shading, ambient, background, base_color, what)
    if not isinstance(face, torch.Tensor) or face.dim() != 1 or face.dtype != torch.int32:
        raise ValueError(f"{what}: face must be a (P,) int32 tensor")
    n = face.shape[0]
    if not isinstance(bary, torch.Tensor) or tuple(bary.shape) != (n, 3) or bary.dtype != torch.float32:
        raise ValueError(f"{what}: bary must be a ({n}, 3) float32 tensor")
    rays = check_rays(rays, n, what)
    face, bary = face.detach().contiguous(), bary.detach().contiguous()
    L.require_gpu(vertices, faces, normals, colors, rays, face, bary)
    dev = face.device
    out = {'normal': torch.empty((n, 3), dtype=torch.float32, device=dev),
           'rgb': torch.empty((n, 3), dtype=torch.float32, device=dev),
           'rgb8': torch.empty((n, 3), dtype=torch.uint8, device=dev)}
    if n:
        L.load()
        with torch.cuda.device(dev):
            L.launch("hn_mesh_shade", L.ptr(vertices) if v else None, v, L.ptr(faces) if n_faces else None, n_faces,
                     L.ptr(normals) if v else None, L.ptr(colors) if v else None, kind, L.ptr(rays), rays.shape[1], n,
                     L.ptr(face), L.ptr(bary), headlight, ambient, base_color, background,
                     L.ptr(out['normal']), L.ptr(out['rgb']), L.ptr(out['rgb8']), L.stream_handle())
    return out
