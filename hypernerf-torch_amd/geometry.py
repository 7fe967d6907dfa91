"""Geometry out of a trained field: the density on a lattice at one frame, its isosurface as a triangle mesh, PLY files.

    grid = density_grid(model, bounds, 256, frame_id=12)            # (256, 256, 256) fp32 on the model's device
    mesh = extract_isosurface(grid, iso=10.0, bounds=bounds)         # {'vertices', 'normals', 'faces'}
    write_ply("frame12.ply", mesh['vertices'], mesh['faces'], mesh['normals'])

The lattice points are observation-space points of frame `frame_id`: they go through that frame's warp and hyper slice
into the template (NerfModel.query_points), so the mesh is the surface of the deforming scene at that frame.  Lattice
points are written chunk by chunk by a kernel (hn_grid_points) and never exist as one (N, 3) tensor; the isosurface is
marching tetrahedra in HIP (csrc/hn_geometry.hip).  Vertex colours are not produced: a colour needs a view direction
per point, which a lattice does not have.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import functional as F

ROW = 64      # lattice points per row of a query: one row = one "ray" of the programs (one id, one view direction)


def _resolution(resolution):
    if isinstance(resolution, (int, np.integer)):
        return (int(resolution),) * 3
    return tuple(resolution)


@torch.no_grad()
def density_grid(model, bounds, resolution, frame_id: int, level: str = 'fine', chunk: int = 1 << 20,
                 render_opts=None) -> torch.Tensor:
    """(nx, ny, nz) fp32 on the model's device: the activated density of `level` (NerfModel.query_points' sigma) at the
    points of the lattice over bounds = (xmin, xmax, ymin, ymax, zmin, zmax), point (i, j, k) at
    lo + (i, j, k) * (hi - lo)/(n - 1), in observation space of frame `frame_id` — the id fills every metadata key, as
    column 8 of a ray row does.  `resolution`: an int or (nx, ny, nz).  The lattice is queried `chunk` points at a time
    (rounded up to whole rows of 64 points; the last chunk is padded with copies of the last point, which are dropped), in
    the model's current precision; the values do not depend on `chunk`."""
    shape, bounds = F.check_lattice(_resolution(resolution), bounds, "density_grid")
    if int(chunk) < 1:
        raise ValueError(f"density_grid: chunk must be positive, got {chunk}")
    device = next(model.parameters()).device
    n = shape[0] * shape[1] * shape[2]
    rows_per_chunk = (int(chunk) + ROW - 1) // ROW
    out = torch.empty(n, dtype=torch.float32, device=device)
    ids = torch.full((rows_per_chunk,), int(frame_id), dtype=torch.int64, device=device)
    viewdirs = torch.tensor([0.0, 0.0, 1.0], device=device).expand(rows_per_chunk, 3).contiguous()
    for start in range(0, n, rows_per_chunk * ROW):
        rows = min(rows_per_chunk, (n - start + ROW - 1) // ROW)
        points = F.grid_points(shape, bounds, start, rows * ROW, device).view(rows, ROW, 3)
        metadata = {k: ids[:rows] for k in ('warp', 'camera', 'appearance', 'time')}
        sigma = model.query_points(points, metadata, level=level, viewdirs=viewdirs[:rows], render_opts=render_opts)['sigma']
        valid = min(rows * ROW, n - start)
        out[start:start + valid] = sigma.reshape(-1)[:valid]
    return out.view(shape)


def extract_isosurface(grid: torch.Tensor, iso: float, bounds) -> Dict[str, torch.Tensor]:
    """{'vertices': (V, 3) fp32, 'normals': (V, 3) fp32, 'faces': (F, 3) int32} of the surface grid = iso (marching
    tetrahedra, functional.extract_isosurface): grid (nx, ny, nz) fp32 on the GPU over `bounds`.  Normals point from
    grid >= iso towards lower values, faces wind accordingly; an empty surface gives zero-length tensors."""
    return F.extract_isosurface(grid, iso, bounds)


def extract_mesh(model, bounds, resolution, frame_id: int, iso: float = 10.0, **kw) -> Dict[str, torch.Tensor]:
    """extract_isosurface(density_grid(model, bounds, resolution, frame_id, **kw), iso, bounds)."""
    return extract_isosurface(density_grid(model, bounds, resolution, frame_id, **kw), iso, bounds)


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path, vertices, faces, normals=None) -> None:
    """Binary little-endian PLY: vertices (V, 3) as float x y z (+ nx ny nz when `normals` (V, 3) is given), faces
    (F, 3) as `list uchar int vertex_indices`.  Tensors or arrays."""
    v = _host(vertices, "<f4").reshape(-1, 3)
    f = _host(faces, "<i4").reshape(-1, 3)
    cols = [v]
    names = ["x", "y", "z"]
    if normals is not None:
        nrm = _host(normals, "<f4").reshape(-1, 3)
        if nrm.shape != v.shape:
            raise ValueError(f"write_ply: {nrm.shape[0]} normals for {v.shape[0]} vertices")
        cols.append(nrm)
        names += ["nx", "ny", "nz"]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property float {n}" for n in names]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(np.concatenate(cols, axis=1).astype("<f4").tobytes())
        fh.write(rec.tobytes())


def read_ply(path) -> Dict[str, Optional[np.ndarray]]:
    """What write_ply wrote: {'vertices': (V, 3) float32, 'normals': (V, 3) float32 | None, 'faces': (F, 3) int32}."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"read_ply: {path} is not a binary little-endian PLY file")
    counts, props, cur = {}, {}, None
    for line in lines[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            cur = w[1]
            counts[cur] = int(w[2])
            props[cur] = []
        elif w[:1] == ["property"]:
            props[cur].append(w[1:])
    names = [p[-1] for p in props.get("vertex", [])]
    if any(p[0] != "float" for p in props.get("vertex", [])) or names[:3] != ["x", "y", "z"] \
            or props.get("face") != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError(f"read_ply: {path} has a layout write_ply does not write")
    nv, nf, width = counts["vertex"], counts["face"], len(names)
    table = np.frombuffer(blob, dtype="<f4", count=nv * width, offset=end).reshape(nv, width)
    rec = np.frombuffer(blob, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nf, offset=end + 4 * nv * width)
    if nf and not (rec["n"] == 3).all():
        raise ValueError(f"read_ply: {path} has faces that are not triangles")
    if len(blob) != end + 4 * nv * width + 13 * nf:
        raise ValueError(f"read_ply: {path} has {len(blob)} bytes, its header describes {end + 4 * nv * width + 13 * nf}")
    normals = table[:, 3:6].copy() if names[3:6] == ["nx", "ny", "nz"] else None
    return {"vertices": table[:, :3].copy(), "normals": normals, "faces": rec["idx"].astype(np.int32).reshape(nf, 3)}
