"""Geometry out of a trained field (csrc/hn_geometry.hip): lattice points, the isosurface by marching tetrahedra,
connected components of a mesh and its compaction, view directions of its vertices; and depth fusion on the same lattice
(csrc/hn_fusion.hip): depth images into a TSDF volume, the faces of its mesh that lie in observed cells; and the distance
between meshes (csrc/hn_mesh_distance.hip): area-weighted surface samples, a grid of cells over a mesh, the nearest point
of the mesh from query points."""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib as L
from .checks import INT32_MAX, check_faces, check_mesh_faces, check_points
from .data import NERFIES_CAM_FLOATS
from .simplify import vertex_extent

__all__ = ["ISO_BLOCK", "check_lattice", "grid_points", "density_activate", "extract_isosurface", "mesh_components",
           "component_sizes", "gather_rows", "compact_mesh", "compact_kept", "vertex_viewdirs", "check_volume", "tsdf_integrate",
           "tsdf_face_keep", "MD_MAX_RES", "MD_TRI_FLOATS", "MD_WEIGHT_BITS", "GRID_DENSITY", "check_grid_resolution", "check_max_distance",
           "default_grid_resolution", "surface_cdf", "sample_faces", "distance_grid", "grid_query"]

ISO_BLOCK = L.HN_ISO_BLOCK    # lattice points (cells) per workgroup of the hn_iso_* passes


def check_lattice(shape, bounds, what: str):
    """(nx, ny, nz) and the six bounds of a lattice as the hn_geometry entry points accept them, or ValueError."""
    try:
        nx, ny, nz = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the lattice must have three sides, got {shape!r}") from None
    if min(nx, ny, nz) < 2:
        raise ValueError(f"{what}: every side of the lattice needs at least 2 points, got {(nx, ny, nz)}")
    if 7 * nx * ny * nz > INT32_MAX:
        raise ValueError(f"{what}: 7 * {nx} * {ny} * {nz} = {7 * nx * ny * nz} edge slots exceed the int32 limit "
                         f"2**31 - 1 = {INT32_MAX} of the mesh indices")
    try:
        bounds = tuple(float(v) for v in bounds)
    except (TypeError, ValueError):
        bounds = ()
    if len(bounds) != 6:
        raise ValueError(f"{what}: bounds must be (xmin, xmax, ymin, ymax, zmin, zmax), got {bounds!r}")
    if not all(hi > lo for lo, hi in zip(bounds[0::2], bounds[1::2])):
        raise ValueError(f"{what}: bounds need hi > lo on every axis, got {bounds}")
    return (nx, ny, nz), bounds


@torch.no_grad()
def grid_points(shape, bounds, start: int, count: int, device) -> torch.Tensor:
    """(count, 3) fp32: lattice points start .. start + count - 1 of the (nx, ny, nz) lattice over `bounds`
    (hn_grid_points), p = (i*ny + j)*nz + k at lo + (i, j, k) * (hi - lo)/(n - 1); indices past the lattice repeat its last
    point.  float32 NumPy gives the same bits."""
    (nx, ny, nz), bounds = check_lattice(shape, bounds, "grid_points")
    if not 0 <= start < nx * ny * nz or not 0 < count <= INT32_MAX:
        raise ValueError(f"grid_points: start {start} / count {count} outside the lattice of {nx * ny * nz} points")
    device = torch.device(device)
    if device.type != "cuda":
        raise L.HnError("hypernerf_torch_amd runs on MI355X only: grid_points needs a GPU device")
    L.load()
    out = torch.empty((count, 3), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        L.launch("hn_grid_points", nx, ny, nz, (C.c_float * 6)(*bounds), start, count, L.ptr(out),
                 L.stream_handle())
    return out


@torch.no_grad()
def density_activate(raw: torch.Tensor, points: torch.Tensor, render_opts=None) -> torch.Tensor:
    """Raw densities (...,) of points (..., 3) -> Softplus, then filter_sigma (dust threshold, bounding box) exactly as the
    compositing kernel applies them (hn_density_activate), as fp32 of raw's shape."""
    L.require_gpu(raw, points)
    L.load()
    raw = raw.detach().float().contiguous()
    has_dust, dust, box = 0, 0.0, None
    if render_opts is not None:
        if 'dust_threshold' in render_opts:
            has_dust, dust = 1, float(render_opts.get('dust_threshold', 0.0))
        if 'bounding_box' in render_opts:
            box = (C.c_float * 6)(*(float(v) for v in render_opts['bounding_box']))
            points = points.detach().float().contiguous()
            if points.shape != raw.shape + (3,):
                raise ValueError(f"density_activate: points {tuple(points.shape)} do not match raw {tuple(raw.shape)}")
    out = torch.empty_like(raw)
    if raw.numel():
        L.launch("hn_density_activate", L.ptr(raw), L.ptr(points) if box is not None else None, raw.numel(),
                 has_dust, dust, box, L.ptr(out), L.stream_handle())
    return out


@torch.no_grad()
def extract_isosurface(grid: torch.Tensor, iso: float, bounds) -> Dict[str, torch.Tensor]:
    """Indexed triangle mesh of the surface grid = iso by marching tetrahedra (hn_iso_*): grid (nx, ny, nz) fp32,
    C-contiguous, on the GPU, its points spread over bounds (xmin, xmax, ymin, ymax, zmin, zmax) ->
    {'vertices': (V, 3) fp32, 'normals': (V, 3) fp32 unit (from inside, grid >= iso, to outside), 'faces': (F, 3) int32}.
    Vertices ascend with their edge slot, faces with cell, tetrahedron, triangle: the same grid gives the same arrays on
    every run.  An empty surface gives zero-length tensors.  Working memory: 28 bytes of edge slots + 1 of marks per
    lattice point.  Two host synchronisations (the vertex and the face count size the outputs)."""
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
        raise ValueError("extract_isosurface: grid must be a (nx, ny, nz) tensor")
    (nx, ny, nz), bounds = check_lattice(grid.shape, bounds, "extract_isosurface")
    if grid.dtype != torch.float32:
        raise ValueError(f"extract_isosurface: grid must be float32, got {grid.dtype}")
    if not grid.is_contiguous():
        raise ValueError("extract_isosurface: grid must be C-contiguous")
    if not grid.is_cuda:
        raise ValueError("extract_isosurface: grid must live on the GPU (there is no CPU fallback)")
    L.load()
    f = grid.detach()
    dev = f.device
    empty = {'vertices': torch.zeros((0, 3), dtype=torch.float32, device=dev),
             'normals': torch.zeros((0, 3), dtype=torch.float32, device=dev),
             'faces': torch.zeros((0, 3), dtype=torch.int32, device=dev)}
    n = nx * ny * nz
    iso = float(iso)
    with torch.cuda.device(dev):
        stream = L.stream_handle()
        # pass A: marks and per-workgroup counts; the scan of the counts is torch's
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        counts = torch.empty((n + ISO_BLOCK - 1) // ISO_BLOCK, dtype=torch.int32, device=dev)
        L.launch("hn_iso_mark", L.ptr(f), nx, ny, nz, iso, L.ptr(mask), L.ptr(counts), stream)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        n_vertices = int(ends[-1])
        if n_vertices == 0:
            return empty
        # pass B
        vertices = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
        slots = torch.empty(7 * n, dtype=torch.int32, device=dev)
        offsets = ends - counts
        L.launch("hn_iso_vertices", L.ptr(f), nx, ny, nz, (C.c_float * 6)(*bounds), iso, L.ptr(mask),
                 L.ptr(offsets), L.ptr(vertices), L.ptr(normals), L.ptr(slots), stream)
        # pass C: count, scan, emit
        n_cells = (nx - 1) * (ny - 1) * (nz - 1)
        fcounts = torch.empty((n_cells + ISO_BLOCK - 1) // ISO_BLOCK, dtype=torch.int32, device=dev)
        L.launch("hn_iso_faces", L.ptr(f), nx, ny, nz, iso, None, None, L.ptr(fcounts), None, stream)
        fends = torch.cumsum(fcounts, 0, dtype=torch.int64)
        n_faces = int(fends[-1])
        if n_faces > INT32_MAX:
            raise ValueError(f"extract_isosurface: {n_faces} faces exceed the int32 limit 2**31 - 1 = {INT32_MAX}")
        faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
        if n_faces:
            foffsets = fends - fcounts
            L.launch("hn_iso_faces", L.ptr(f), nx, ny, nz, iso, L.ptr(slots), L.ptr(foffsets), None,
                     L.ptr(faces), stream)
    return {'vertices': vertices, 'normals': normals, 'faces': faces}


@torch.no_grad()
def mesh_components(faces: torch.Tensor, num_vertices: int, out: Optional[torch.Tensor] = None,
                    return_rounds: bool = False):
    """labels (V,) int32 of the mesh faces (F, 3) int32 over V vertices: the SMALLEST vertex id of the vertex's connected
    component (two vertices are connected when a face holds both; an unreferenced vertex is its own component) — a
    definition that no scheduling can change, so two runs give the same bits (hn_cc_init / hn_cc_round: hook and
    pointer-jump rounds with integer atomicMin).  One host read of two ints per round; the loop is capped at V + 1 rounds
    (min-label propagation needs at most V - 1 that change something, every round here does at least its step) and a
    RuntimeError names the cap if it is ever exceeded.  A vertex id outside [0, V) is a ValueError; nothing is written
    outside the label array.  `out`: a contiguous (V,) int32 tensor to label in place.  `return_rounds`: (labels, rounds
    run, the last one included that changed nothing)."""
    faces, v = check_faces(faces, num_vertices, "mesh_components")
    dev = faces.device
    if out is None:
        out = torch.empty(v, dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or out.shape != (v,) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"mesh_components: out must be a contiguous ({v},) int32 tensor on {dev}")
    n_faces = faces.shape[0]
    rounds = 0
    if v == 0 and n_faces == 0:
        return (out, rounds) if return_rounds else out
    L.load()
    cap = v + 1
    with torch.cuda.device(dev):
        stream = L.stream_handle()
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        L.launch("hn_cc_init", L.ptr(faces) if n_faces else None, n_faces, L.ptr(out) if v else None, v,
                 L.ptr(flags), stream)
        if n_faces == 0:
            return (out, rounds) if return_rounds else out
        if v == 0:
            raise ValueError("mesh_components: faces hold a vertex id outside [0, 0)")
        while True:
            rounds += 1
            if rounds > cap:
                raise RuntimeError(f"mesh_components: no fixed point after the cap of V + 1 = {cap} rounds")
            L.launch("hn_cc_round", L.ptr(faces), n_faces, L.ptr(out), v, rounds, L.ptr(flags), stream)
            err, changed = flags.tolist()
            if err:
                raise ValueError(f"mesh_components: faces hold a vertex id outside [0, {v})")
            if changed != rounds:
                break
    return (out, rounds) if return_rounds else out


@torch.no_grad()
def component_sizes(labels: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """(V,) int32: the number of faces of every component at index = its label (mesh_components), zero elsewhere
    (hn_cc_sizes: integer atomic adds, whose sum does not depend on their order).  No host synchronisation: an id or a
    label outside [0, V) is skipped (mesh_components refuses such faces first)."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype != torch.int32:
        raise ValueError("component_sizes: labels must be a (V,) int32 tensor")
    faces, v = check_faces(faces, labels.shape[0], "component_sizes")
    L.require_gpu(labels)
    sizes = torch.zeros(v, dtype=torch.int32, device=faces.device)
    if v and faces.shape[0]:
        L.load()
        with torch.cuda.device(faces.device):
            flags = torch.zeros(2, dtype=torch.int32, device=faces.device)
            L.launch("hn_cc_sizes", L.ptr(labels.detach().contiguous()), L.ptr(faces), faces.shape[0], v,
                     L.ptr(sizes), L.ptr(flags), L.stream_handle())
    return sizes


@torch.no_grad()
def gather_rows(src: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """src[index] along the first dimension for an int32 index (hn_gather_rows): any dtype, any trailing shape."""
    L.require_gpu(src, index)
    src = src.detach().contiguous()
    n = index.shape[0]
    out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if out.numel():
        L.load()
        row_bytes = out.numel() // n * out.element_size()
        with torch.cuda.device(src.device):
            L.launch("hn_gather_rows", L.ptr(src), src.shape[0], L.ptr(index), n, row_bytes, L.ptr(out),
                     L.stream_handle())
    return out


@torch.no_grad()
def compact_mesh(faces: torch.Tensor, labels: torch.Tensor, keep_comp: torch.Tensor):
    """(vertex_index (V',) int32, faces (F', 3) int32): the vertices whose component is kept (keep_comp: (V,) bool or
    uint8 indexed by label) in their old order, and the faces of those components in their old order, re-indexed
    (hn_mesh_keep, two torch.cumsum scans, hn_mesh_compact).  One host read (both counts at once) sizes the outputs."""
    faces, v = check_faces(faces, labels.shape[0], "compact_mesh")
    dev = faces.device
    n_faces = faces.shape[0]
    if v == 0:
        return torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev)
    L.load()
    keep_comp = keep_comp.to(torch.uint8).contiguous()
    with torch.cuda.device(dev):
        stream = L.stream_handle()
        vkeep = torch.empty(v, dtype=torch.int32, device=dev)
        fkeep = torch.empty(max(n_faces, 1), dtype=torch.int32, device=dev)
        if n_faces == 0:
            fkeep.zero_()
        L.launch("hn_mesh_keep", L.ptr(labels.contiguous()), L.ptr(faces) if n_faces else None, L.ptr(keep_comp),
                 v, n_faces, L.ptr(vkeep), L.ptr(fkeep), stream)
    return compact_kept(faces, vkeep, fkeep)


@torch.no_grad()
def compact_kept(faces: torch.Tensor, vkeep: torch.Tensor, fkeep: torch.Tensor):
    """(vertex_index (V',) int32, faces (F', 3) int32) of faces (F, 3) int32 and the 0 / 1 int32 marks vkeep (V >= 1,) and
    fkeep (max(F, 1),): the kept vertices and faces in their old order, the faces re-indexed (two torch.cumsum scans,
    hn_mesh_compact).  Every vertex of a kept face must be kept.  One host read (both counts at once) sizes the outputs."""
    dev, v, n_faces = faces.device, vkeep.shape[0], faces.shape[0]
    with torch.cuda.device(dev):
        vscan = torch.cumsum(vkeep, 0, dtype=torch.int32)
        fscan = torch.cumsum(fkeep, 0, dtype=torch.int32)
        n_v, n_f = torch.stack([vscan[-1], fscan[-1]]).tolist()
        vertex_index = torch.empty(n_v, dtype=torch.int32, device=dev)
        faces_out = torch.empty((n_f, 3), dtype=torch.int32, device=dev)
        if n_v:
            L.launch("hn_mesh_compact", L.ptr(faces) if n_faces else None, L.ptr(vscan), L.ptr(fscan), v, n_faces,
                     n_v, n_f, L.ptr(vertex_index), L.ptr(faces_out) if n_f else None, L.stream_handle())
    return vertex_index, faces_out


@torch.no_grad()
def vertex_viewdirs(vertices: torch.Tensor, normals: Optional[torch.Tensor], start: int, count: int,
                    camera=None) -> torch.Tensor:
    """(count, 3) fp32 unit directions for vertices start .. start + count - 1 (hn_vertex_viewdirs; rows past the mesh
    repeat its last vertex): -normal/|normal| when `camera` is None, else (v - camera)/|v - camera| for the three host
    floats `camera`; a zero length gives (0, 0, 1).  float32 NumPy gives the same values to a few roundings."""
    L.require_gpu(vertices, normals)
    ref = vertices if camera is not None else normals
    if ref is None or ref.dim() != 2 or ref.shape[1] != 3 or ref.dtype != torch.float32:
        raise ValueError("vertex_viewdirs: vertices / normals must be (V, 3) float32")
    v = ref.shape[0]
    if not 0 <= start < v or not 0 < count <= INT32_MAX:
        raise ValueError(f"vertex_viewdirs: start {start} / count {count} outside the mesh of {v} vertices")
    L.load()
    ref = ref.detach().contiguous()
    out = torch.empty((count, 3), dtype=torch.float32, device=ref.device)
    cam = None if camera is None else (C.c_float * 3)(*(float(x) for x in camera))
    with torch.cuda.device(ref.device):
        L.launch("hn_vertex_viewdirs", L.ptr(ref) if camera is not None else None,
                 L.ptr(ref) if camera is None else None, v, start, count, cam, L.ptr(out),
                 L.stream_handle())
    return out


# ---- depth fusion (csrc/hn_fusion.hip) -----------------------------------------------------------------------------------
def check_volume(t, what: str, name: str, shape=None) -> torch.Tensor:
    """A (nx, ny, nz) float32 C-contiguous volume as the hn_tsdf entry points take it (of `shape` when given), or
    ValueError.  The device is the caller's to check, after its other arguments."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError(f"{what}: {name} must be a (nx, ny, nz) tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, the lattice {tuple(shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be C-contiguous")
    return t.detach()


@torch.no_grad()
def tsdf_integrate(tsdf: torch.Tensor, weight: torch.Tensor, bounds, cams: torch.Tensor, depths: torch.Tensor,
                   trunc: float) -> None:
    """Folds depths (N, H, W) fp32 seen through the camera records cams (N, 24) fp32 into the volumes tsdf and weight
    ((nx, ny, nz) fp32, C-contiguous, zeroed before the first batch), IN PLACE (hn_tsdf_integrate; DESIGN.md 3.12 holds the
    definition): per lattice point and view, in the order of the views, the point is projected by the forward camera
    model, the depth D of the pixel it falls into is read (nearest pixel; +inf = the ray hit nothing, not > 0 = nothing
    known), s = D - |x - camera|, and unless s < -trunc, tsdf = (weight * tsdf + min(1, s / trunc)) / (weight + 1) and
    weight += 1.  Depths are distances along the unit ray from the camera position.  Everything on the GPU of the volumes;
    no host synchronisation; two runs, and the same views in several batches, give the same bits."""
    what = "tsdf_integrate"
    tsdf = check_volume(tsdf, what, "tsdf")
    weight = check_volume(weight, what, "weight", tsdf.shape)
    (nx, ny, nz), bounds = check_lattice(tsdf.shape, bounds, what)
    if not isinstance(cams, torch.Tensor) or cams.dim() != 2 or cams.shape[1] != NERFIES_CAM_FLOATS \
            or cams.dtype != torch.float32:
        raise ValueError(f"{what}: cams must be a (N, {NERFIES_CAM_FLOATS}) float32 tensor of camera records")
    n = cams.shape[0]
    if n < 1:
        raise ValueError(f"{what}: cams holds no camera")
    if not isinstance(depths, torch.Tensor) or depths.dim() != 3 or depths.dtype != torch.float32:
        raise ValueError(f"{what}: depths must be a (N, H, W) float32 tensor")
    if depths.shape[0] != n:
        raise ValueError(f"{what}: depths holds {depths.shape[0]} images for {n} cameras")
    h, w = int(depths.shape[1]), int(depths.shape[2])
    if not (1 <= w <= L.HN_MESH_MAX_SIDE and 1 <= h <= L.HN_MESH_MAX_SIDE):
        raise ValueError(f"{what}: the image sides of depths must be 1 .. {L.HN_MESH_MAX_SIDE}, got {w} x {h}")
    try:
        trunc = float(trunc)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: trunc must be a number, got {trunc!r}") from None
    if not (math.isfinite(trunc) and trunc > 0.0):
        raise ValueError(f"{what}: trunc must be positive and finite, got {trunc}")
    if not (tsdf.is_cuda and weight.is_cuda and cams.is_cuda and depths.is_cuda):
        raise ValueError(f"{what}: tsdf, weight, cams and depths must live on the GPU (there is no CPU fallback)")
    if cams.device != tsdf.device or depths.device != tsdf.device or weight.device != tsdf.device:
        raise ValueError(f"{what}: tsdf, weight, cams and depths must live on one device")
    L.load()
    cams, depths = cams.detach().contiguous(), depths.detach().contiguous()
    with torch.cuda.device(tsdf.device):
        L.launch("hn_tsdf_integrate", L.ptr(tsdf), L.ptr(weight), nx, ny, nz, (C.c_float * 6)(*bounds), L.ptr(cams),
                 L.ptr(depths), n, h, w, trunc, L.stream_handle())


@torch.no_grad()
def tsdf_face_keep(vertices: torch.Tensor, faces: torch.Tensor, weight: torch.Tensor, bounds):
    """(fkeep (F,) int32, vkeep (V,) int32), 0 / 1: a face of a mesh extracted on the lattice of `weight` ((nx, ny, nz)
    fp32 over `bounds`) is kept iff all eight lattice points of the cell that holds its centroid ((a + b) + c) / 3 have
    weight > 0, a vertex iff a kept face references it (hn_tsdf_face_keep).  A face with a vertex id outside [0, V) is
    dropped.  No host synchronisation; the scans and hn_mesh_compact that follow are the caller's."""
    what = "tsdf_face_keep"
    vertices = check_points(vertices, what, "vertices")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{what}: faces must be a (F, 3) int32 tensor")
    weight = check_volume(weight, what, "weight")
    (nx, ny, nz), bounds = check_lattice(weight.shape, bounds, what)
    if not (vertices.is_cuda and faces.is_cuda and weight.is_cuda):
        raise ValueError(f"{what}: vertices, faces and weight must live on the GPU (there is no CPU fallback)")
    faces, v = check_faces(faces, vertices.shape[0], what)
    if vertices.device != faces.device or weight.device != faces.device:
        raise ValueError(f"{what}: vertices, faces and weight must live on one device")
    dev, n_faces = faces.device, faces.shape[0]
    fkeep = torch.empty(n_faces, dtype=torch.int32, device=dev)
    vkeep = torch.zeros(v, dtype=torch.int32, device=dev)
    if n_faces and v:
        L.load()
        with torch.cuda.device(dev):
            L.launch("hn_tsdf_face_keep", L.ptr(faces), n_faces, L.ptr(vertices), v, L.ptr(weight), nx, ny, nz,
                     (C.c_float * 6)(*bounds), L.ptr(fkeep), L.ptr(vkeep), L.stream_handle())
    else:
        fkeep.zero_()
    return fkeep, vkeep


# ---- mesh-to-mesh distance (csrc/hn_mesh_distance.hip) ---------------------------------------------------------------------
# mirrors of csrc/hn_mesh_distance.hip's limits (no macros in the header: its set of constants is that of ABI 340)
MD_MAX_RES = 256          # grid cells per axis of the distance grid
MD_TRI_FLOATS = 12        # floats per packed triangle
MD_WEIGHT_BITS = 24       # the largest face has the integer weight 2**24
GRID_DENSITY = 0.5    # default_grid_resolution: cells along the longest axis per sqrt(faces) (DESIGN.md 3.13 has the numbers)


def check_grid_resolution(resolution, what: str):
    """(rx, ry, rz) from an int or three ints, each 1 .. MD_MAX_RES, or ValueError."""
    if isinstance(resolution, numbers.Integral) and not isinstance(resolution, bool):
        res = (int(resolution),) * 3
    else:
        try:
            vals = list(resolution)
        except TypeError:
            vals = []
        res = tuple(int(r) for r in vals) if all(isinstance(r, numbers.Integral) and not isinstance(r, bool) for r in vals) \
            else ()
    if len(res) != 3 or not all(1 <= r <= MD_MAX_RES for r in res):
        raise ValueError(f"{what}: grid_resolution must be an int or three ints in 1 .. {MD_MAX_RES}, got {resolution!r}")
    return res


def check_max_distance(max_distance, what: str) -> float:
    """max_distance as the float hn_md_query takes (-1.0 for None: no limit), or ValueError when negative or NaN."""
    if max_distance is None:
        return -1.0
    try:
        d = float(max_distance)
    except (TypeError, ValueError):
        d = float("nan")
    if not d >= 0.0:
        raise ValueError(f"{what}: max_distance must be a number >= 0 or None, got {max_distance!r}")
    return d


def default_grid_resolution(n_faces: int, lo, hi):
    """(rx, ry, rz): round(GRID_DENSITY * sqrt(F)) cells along the longest side of the box lo .. hi, the other axes in
    proportion to their sides (cells about cubic), each clamped to 1 .. MD_MAX_RES; a side of zero length gets 1."""
    ext = [max(float(h) - float(l), 0.0) for l, h in zip(lo, hi)]
    longest = max(ext)
    along = GRID_DENSITY * math.sqrt(max(int(n_faces), 1))
    if not longest > 0.0:
        return (1, 1, 1)
    return tuple(min(MD_MAX_RES, max(1, int(round(along * e / longest)))) for e in ext)


def _check_mesh(vertices, faces, what: str):
    vertices = check_points(vertices, what, "vertices")
    faces = check_mesh_faces(faces, what)
    if vertices.shape[0] > INT32_MAX or faces.shape[0] > INT32_MAX:
        raise ValueError(f"{what}: {vertices.shape[0]} vertices / {faces.shape[0]} faces exceed 2**31 - 1 = {INT32_MAX}")
    return vertices, faces


@torch.no_grad()
def surface_cdf(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """(F,) int64: the inclusive scan of the integer face weights w_f = (int64)((a2_f / max a2) * 2**24), a2_f = twice the
    area of face f in fp32 (hn_md_face_weights; 0 where not finite) — what sample_faces draws its faces from.  The maximum,
    the quotient and the scan are torch's: an fp32 maximum and integer sums are exact, the quotient one correctly rounded
    division.  One host read (the total weight and the error flag).  ValueError: a face holds a vertex id outside
    [0, V); the total weight is 0 (no face, or none with a positive finite area)."""
    what = "surface_cdf"
    vertices, faces = _check_mesh(vertices, faces, what)
    L.require_gpu(vertices, faces)
    v, n_faces, dev = vertices.shape[0], faces.shape[0], faces.device
    if n_faces == 0:
        raise ValueError(f"{what}: the mesh has no faces")
    if v == 0:
        raise ValueError(f"{what}: faces hold a vertex id outside [0, 0)")
    L.load()
    a2 = torch.empty(n_faces, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.launch("hn_md_face_weights", L.ptr(vertices), v, L.ptr(faces), n_faces, L.ptr(a2), L.ptr(err), L.stream_handle())
    m = a2.amax()      # stays on the device: a tensor divisor is divided by, a host scalar would be multiplied by its inverse
    w = torch.where(m > 0, (a2 / m) * float(1 << MD_WEIGHT_BITS), torch.zeros_like(a2)).to(torch.int64)
    cdf = torch.cumsum(w, 0)
    total, bad = torch.stack([cdf[-1], err[0].to(torch.int64)]).tolist()
    if bad:
        raise ValueError(f"{what}: faces hold a vertex id outside [0, {v})")
    if total == 0:
        raise ValueError(f"{what}: no face has a positive finite area")
    return cdf


@torch.no_grad()
def sample_faces(vertices: torch.Tensor, faces: torch.Tensor, cdf: torch.Tensor, n: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """{'points': (n, 3) fp32, 'face': (n,) int32, 'bary': (n, 3) fp32}: n independent area-weighted points of the surface
    (hn_md_sample; cdf: surface_cdf's).  Sample k hashes (seed, k) with splitmix64 into a face (through the integer cdf)
    and two 24-bit uniforms: any machine gives the same bits, and tests/mesh_distance_restated.py restates them."""
    what = "sample_faces"
    vertices, faces = _check_mesh(vertices, faces, what)
    n_faces, v = faces.shape[0], vertices.shape[0]
    n = int(n)
    if not 1 <= n <= INT32_MAX:
        raise ValueError(f"{what}: n must be 1 .. 2**31 - 1, got {n}")
    if not isinstance(cdf, torch.Tensor) or cdf.dtype != torch.int64 or tuple(cdf.shape) != (n_faces,) or n_faces == 0:
        raise ValueError(f"{what}: cdf must be the ({n_faces},) int64 tensor surface_cdf returned for this mesh")
    L.require_gpu(vertices, faces, cdf)
    dev = faces.device
    out = {'points': torch.empty((n, 3), dtype=torch.float32, device=dev),
           'face': torch.empty(n, dtype=torch.int32, device=dev),
           'bary': torch.empty((n, 3), dtype=torch.float32, device=dev)}
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    L.load()
    with torch.cuda.device(dev):
        L.launch("hn_md_sample", L.ptr(vertices), v, L.ptr(faces), n_faces, L.ptr(cdf.contiguous()), n,
                 seed - (1 << 64) if seed >= 1 << 63 else seed, L.ptr(out['points']), L.ptr(out['face']), L.ptr(out['bary']),
                 L.stream_handle())
    return out


@torch.no_grad()
def distance_grid(vertices: torch.Tensor, faces: torch.Tensor, resolution=None) -> Dict:
    """The acceleration grid grid_query searches: rx x ry x rz cells over the box of the vertices (vertex_extent), every
    face listed in the cells of [idx(its min corner), idx(its max corner)] — hn_md_pack, hn_md_cell_count, torch.cumsum, one
    host read (the pair count and the error flag), hn_md_cell_fill, a stable torch.sort on the cell and torch.searchsorted,
    as mesh_bins builds its tiles; face ids ascend within a cell.  resolution: an int or three, None =
    default_grid_resolution; 1 lists every face in one cell (brute force).  More than 2**31 - 1 pairs halve the
    resolution and count again.  {'tri': (F, 12) fp32 packed triangles, 'cell_begin': (cells + 1,) int32, 'pair_face':
    (pairs,) int32, 'lo', 'cell': three host floats each, 'resolution': (rx, ry, rz), 'num_faces': F}.  An empty mesh
    gives a grid without pairs.  ValueError: a vertex id outside [0, V), vertices that are not finite.  Two host reads."""
    what = "distance_grid"
    vertices, faces = _check_mesh(vertices, faces, what)
    res = None if resolution is None else check_grid_resolution(resolution, what)
    L.require_gpu(vertices, faces)
    v, n_faces, dev = vertices.shape[0], faces.shape[0], faces.device
    if n_faces == 0:
        return {'tri': torch.zeros((0, MD_TRI_FLOATS), dtype=torch.float32, device=dev),
                'cell_begin': torch.zeros(2, dtype=torch.int32, device=dev),
                'pair_face': torch.zeros(0, dtype=torch.int32, device=dev), 'lo': [0.0] * 3, 'cell': [1.0] * 3,
                'resolution': (1, 1, 1), 'num_faces': 0}
    if v == 0:
        raise ValueError(f"{what}: faces hold a vertex id outside [0, 0)")
    lo, hi = (np.asarray(t, dtype=np.float32) for t in vertex_extent(vertices))      # host read 1
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(hi - lo).all()):
        raise ValueError(f"{what}: the vertices are not finite")
    if res is None:
        res = default_grid_resolution(n_faces, lo.tolist(), hi.tolist())
    res = tuple(1 if not h > l else r for r, l, h in zip(res, lo, hi))      # an axis of zero extent has one cell
    L.load()
    with torch.cuda.device(dev):
        stream = L.stream_handle()
        tri = torch.empty((n_faces, MD_TRI_FLOATS), dtype=torch.float32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        L.launch("hn_md_pack", L.ptr(vertices), v, L.ptr(faces), n_faces, L.ptr(tri), L.ptr(err), stream)
        counts = torch.empty(n_faces, dtype=torch.int32, device=dev)
        while True:
            # fp32 cell sides: the quotient of the side and the cell count, 1 where the side is zero
            cell = [float(np.float32(h - l) / np.float32(r)) if r > 1 or h > l else 1.0 for r, l, h in zip(res, lo, hi)]
            if not all(c > 0.0 for c in cell):      # a side below the smallest float32 times R
                res = tuple(1 if not c > 0.0 else r for r, c in zip(res, cell))
                continue
            lo_c, cell_c = (C.c_float * 3)(*lo.tolist()), (C.c_float * 3)(*cell)
            L.launch("hn_md_cell_count", L.ptr(tri), n_faces, lo_c, cell_c, res[0], res[1], res[2], L.ptr(counts), stream)
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            n_pairs, bad = torch.stack([ends[-1], err[0].to(torch.int64)]).tolist()      # host read 2
            if bad:
                raise ValueError(f"{what}: faces hold a vertex id outside [0, {v})")
            if n_pairs <= INT32_MAX:
                break
            if max(res) == 1:
                raise ValueError(f"{what}: {n_pairs} (cell, face) pairs exceed 2**31 - 1 = {INT32_MAX}")
            res = tuple(max(1, r // 2) for r in res)
        n_cells = res[0] * res[1] * res[2]
        if n_pairs == 0:
            raise ValueError(f"{what}: the vertices of the faces are not finite")
        pair_cell = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        pair_face = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        L.launch("hn_md_cell_fill", L.ptr(tri), n_faces, lo_c, cell_c, res[0], res[1], res[2], L.ptr(ends), n_pairs,
                 L.ptr(pair_cell), L.ptr(pair_face), stream)
        if n_cells > 1:
            sorted_cell, order = torch.sort(pair_cell, stable=True)
            cell_begin = torch.searchsorted(sorted_cell, torch.arange(n_cells + 1, dtype=torch.int32, device=dev))
            cell_begin, pair_face = cell_begin.to(torch.int32), pair_face[order].contiguous()
        else:
            cell_begin = torch.tensor([0, n_pairs], dtype=torch.int32, device=dev)
    return {'tri': tri, 'cell_begin': cell_begin.contiguous(), 'pair_face': pair_face, 'lo': lo.tolist(), 'cell': cell,
            'resolution': res, 'num_faces': n_faces}


def _check_grid(grid, what: str):
    try:
        res = check_grid_resolution(grid['resolution'], what)
        tri, cell_begin, pair_face = grid['tri'], grid['cell_begin'], grid['pair_face']
        lo, cell, n_faces = [float(x) for x in grid['lo']], [float(x) for x in grid['cell']], int(grid['num_faces'])
        ok = (tri.dtype == torch.float32 and tuple(tri.shape) == (n_faces, MD_TRI_FLOATS) and tri.is_contiguous()
              and cell_begin.dtype == torch.int32 and cell_begin.is_contiguous() and pair_face.dtype == torch.int32
              and pair_face.dim() == 1 and pair_face.is_contiguous() and len(lo) == 3 and len(cell) == 3
              and tuple(cell_begin.shape) == ((res[0] * res[1] * res[2] if n_faces else 1) + 1,))
    except (KeyError, TypeError, ValueError, AttributeError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: grid must be what distance_grid returned")
    return res, tri, cell_begin, pair_face, lo, cell, n_faces


@torch.no_grad()
def grid_query(points: torch.Tensor, grid: Dict, max_distance=None, sort_queries: bool = True) -> Dict[str, torch.Tensor]:
    """{'distance': (N,) fp32, 'face': (N,) int32, 'closest': (N, 3) fp32}: for every point of points (N, 3) fp32 the
    nearest point of the mesh behind `grid` (distance_grid's), its face (ties to the smallest id) and the distance
    (hn_md_query; DESIGN.md 3.13 holds the definition): the same bits as testing every face, whatever the resolution.
    A point that is not finite gives NaN, -1, NaN; a mesh without faces +inf, -1, NaN; with max_distance, so does every
    point farther than that from the mesh, and the search stops at that radius.  sort_queries: the queries are sorted by
    their cell (hn_md_cell_keys, torch.sort) and the kernel reads them through the permutation, so that the lanes of a wave
    walk the same cells; the results are the same bits, in the caller's order, either way.  No host synchronisation."""
    what = "grid_query"
    points = check_points(points, what, "points")
    max_d = check_max_distance(max_distance, what)
    res, tri, cell_begin, pair_face, lo, cell, n_faces = _check_grid(grid, what)
    n = points.shape[0]
    if n > INT32_MAX:
        raise ValueError(f"{what}: {n} points exceed 2**31 - 1 = {INT32_MAX}")
    L.require_gpu(points, tri)
    dev = points.device
    if tri.device != dev:
        raise ValueError(f"{what}: points and grid must live on one device")
    out = {'distance': torch.empty(n, dtype=torch.float32, device=dev), 'face': torch.empty(n, dtype=torch.int32, device=dev),
           'closest': torch.empty((n, 3), dtype=torch.float32, device=dev)}
    if n == 0:
        return out
    if n_faces == 0:
        out['distance'].fill_(float("inf"))
        out['face'].fill_(-1)
        out['closest'].fill_(float("nan"))
        return out
    L.load()
    lo_c, cell_c = (C.c_float * 3)(*lo), (C.c_float * 3)(*cell)
    with torch.cuda.device(dev):
        stream = L.stream_handle()
        perm = None
        if sort_queries and res != (1, 1, 1) and n > 1:
            keys = torch.empty(n, dtype=torch.int32, device=dev)
            L.launch("hn_md_cell_keys", L.ptr(points), n, lo_c, cell_c, res[0], res[1], res[2], L.ptr(keys), stream)
            perm = torch.sort(keys).indices
        L.launch("hn_md_query", L.ptr(points), n, L.ptr(perm), L.ptr(tri), n_faces, L.ptr(cell_begin), L.ptr(pair_face),
                 pair_face.shape[0], lo_c, cell_c, res[0], res[1], res[2], max_d, L.ptr(out['distance']), L.ptr(out['face']),
                 L.ptr(out['closest']), stream)
    return out
