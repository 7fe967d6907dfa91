"""Geometry out of a trained field: the density on a lattice at one frame, its isosurface as a triangle mesh, PLY files.

    grid = density_grid(model, bounds, 256, frame_id=12)            # (256, 256, 256) fp32 on the model's device
    mesh = extract_isosurface(grid, iso=10.0, bounds=bounds)         # {'vertices', 'normals', 'faces'}
    mesh = filter_mesh(mesh, keep_largest=1)                         # drop the floaters; + 'vertex_index'
    mesh['colors'] = vertex_colors(model, mesh['vertices'], mesh['normals'], frame_id=12)    # (V, 3) uint8
    write_ply("frame12.ply", mesh['vertices'], mesh['faces'], mesh['normals'], mesh['colors'])

The lattice points are observation-space points of frame `frame_id`: they go through that frame's warp and hyper slice
into the template (NerfModel.query_points), so the mesh is the surface of the deforming scene at that frame.  Lattice
points are written chunk by chunk by a kernel (hn_grid_points) and never exist as one (N, 3) tensor; the isosurface is
marching tetrahedra in HIP (csrc/hn_geometry.hip).

Floaters: `mesh_components` labels every vertex with the smallest vertex id of its connected component (two vertices are
connected when a face holds both; hook and pointer-jump rounds with integer atomicMin, a definition no scheduling can
change), `component_sizes` counts the faces per label, and `filter_mesh` keeps the components with at least `min_faces`
faces and / or the `keep_largest` ones with the most faces (ties to the smaller label), orders kept, faces re-indexed.

Colours: a lattice has no view direction, but a mesh vertex has a normal and a frame has a camera.  `vertex_colors`
looks at every vertex along -normal (head-on from outside) or from a camera position, (v - c)/|v - c| — a zero length
gives (0, 0, 1) — and takes the field's `rgb` at the vertex (rows of one point through NerfModel.query_points, the
directions written chunk by chunk by hn_vertex_viewdirs), as float32 or as (rgb * 255) truncated to uint8.

Simplification: marching tetrahedra emits about two triangles per surface vertex at lattice resolution.  `simplify_mesh`
collapses the vertices of every cell of a coarser lattice into one (vertex clustering, csrc/hn_simplify.hip), placed by
the members' tangent planes, and cancels the folded flaps the collapse leaves; `extract_mesh(simplify=k)` does it with
cells of k lattice spacings.  The definition fixes every summation order: two runs give the same bits.

Looking at it: `render_mesh` casts the rays of a camera of the field at the mesh (csrc/hn_mesh_render.hip, DESIGN.md
3.11) and gives face-id, depth, barycentric, normal and shaded colour images; `depth_agreement` / `mesh_depth_error`
compare its depth with the field's along the same rays, and `mesh_turntable` writes an orbit as a GIF:

    cam = camera_from_c2w(c2w, focal, W, H)            # or dataset.camera_record(idx), or orbit_cameras(...)[k]
    rays = camera_rays(cam, W, H, near, far)
    img = render_mesh(mesh, rays, cam, (W, H))          # img['rgb8'] (H, W, 3) uint8, img['depth'] (H, W)
    mesh_depth_error(model, mesh, rays, cam, (W, H))    # {'abs_mean', 'rmse', 'iou', 'n'}
    mesh_turntable(mesh, "turntable.gif", n=60)

Depth fusion: a level set of the density needs an `iso`, and a NeRF's density is no distance.  `extract_mesh_fused`
renders depth from cameras around the frame (`depth_images_from_field`), integrates the depth maps into a truncated
signed distance volume (`fuse_depth`, csrc/hn_fusion.hip) and meshes its zero level set
(`tsdf_isosurface`): what is visible defines the surface, and rays that pass through carve the floaters away.

    cams = orbit_cameras((0, 0, 0), 3.0, 60, 20.0, focal=400.0, image_wh=(W, H))
    mesh = extract_mesh_fused(model, bounds, 256, 12, cams, (W, H), near, far, keep_largest=1)

Comparing meshes: `mesh_distance` samples both surfaces by area (`sample_surface`, reproducible bit for bit), finds every
sample's exact nearest point on the other mesh (`point_mesh_distance`, csrc/hn_mesh_distance.hip, DESIGN.md 3.13: a grid
of cells prunes the search, the result is that of testing every face) and reports Chamfer, Hausdorff and precision /
recall / F-score at thresholds; `distance_colors` turns per-vertex distances into colours for write_ply.

    small = simplify_mesh(mesh, cell=0.02)
    mesh_distance(mesh, small, n_samples=1_000_000, thresholds=[0.01])    # what the simplification cost
    d = point_mesh_distance(small['vertices'], mesh)['distance']
    write_ply("error.ply", small['vertices'], small['faces'], colors=distance_colors(d, vmax=0.02))

Meshes in different frames: the distance means something only once both meshes share a frame.  `register_mesh` finds the
rigid or similarity transform that moves one onto the other by trimmed ICP (csrc/hn_registration.hip, DESIGN.md 3.15: the
nearest points come from the same grid, the sums of each iteration from one fused, bit-reproducible reduction, the solve
is float64 NumPy), `transform_mesh` applies it, and `aligned_mesh_distance` does both and then measures.

    fit = register_mesh(scan, mesh, with_scale=True, trim=0.9, init='centroid')     # fit['matrix'] (4, 4), fit['rms']
    aligned_mesh_distance(scan, mesh, register=dict(with_scale=True), thresholds=[0.01])

Taking a mesh out with its appearance: after simplify_mesh a colour per vertex keeps little of what the field knows.
`texture_atlas` gives every face a chart in one image (csrc/hn_texture.hip, DESIGN.md 3.16: two faces to a power-of-two
cell, cells packed in Z-order, no host loop over faces), `rasterize_atlas` turns its texels into points and normals,
`bake_field_texture` asks the field for their colours, `render_textured_mesh` puts the texture back on the rendered
mesh and `write_obj` writes mesh, UVs and the image for a viewer.

    small = simplify_mesh(mesh, cell=0.02)
    atlas = texture_atlas(small, atlas_texel_for_size(small, 4096), max_size=4096)
    texture = bake_field_texture(model, small, atlas, frame_id=12)        # (H_t, W_t, 3) uint8
    img = render_textured_mesh(small, atlas, texture, rays, cam, (W, H))
    write_obj("frame12.obj", small, atlas, texture)                        # + frame12.mtl, frame12.png

Rendering faster: most samples of a ray lie in air.  `occupancy_grid` turns the density lattice of a frame into one bit per
lattice cell (csrc/hn_occupancy.hip), `clip_rays` cuts every ray to the part of [near, far] between the
first and the last occupied cell it crosses and re-parametrises it so that an unchanged model samples exactly that part,
`unclip` maps depths back, and inference.render_image / evaluate_images, depth_images_from_field and extract_mesh_fused
take `occupancy=` and do all three; `OccupancyCache` builds the grid of each frame on first use.

    occ = occupancy_grid(model, bounds, 128, frame_id=12, sigma_min=0.5, dilate=1)
    occupancy_fraction(occ)                                               # the occupied share of the cells
    img = inference.render_image(model, rays, occupancy=occ)             # rays of frame 12
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ops.occupancy import (OccupancyCache, clip_rays, occupancy_fraction, occupancy_from_density, occupancy_grid,      # noqa: F401
                            occupancy_union, unclip)

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
    shape, bounds = ops.mesh.check_lattice(_resolution(resolution), bounds, "density_grid")
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
        points = ops.mesh.grid_points(shape, bounds, start, rows * ROW, device).view(rows, ROW, 3)
        metadata = {k: ids[:rows] for k in ('warp', 'camera', 'appearance', 'time')}
        sigma = model.query_points(points, metadata, level=level, viewdirs=viewdirs[:rows], render_opts=render_opts)['sigma']
        valid = min(rows * ROW, n - start)
        out[start:start + valid] = sigma.reshape(-1)[:valid]
    return out.view(shape)


def extract_isosurface(grid: torch.Tensor, iso: float, bounds) -> Dict[str, torch.Tensor]:
    """{'vertices': (V, 3) fp32, 'normals': (V, 3) fp32, 'faces': (F, 3) int32} of the surface grid = iso (marching
    tetrahedra, ops.mesh.extract_isosurface): grid (nx, ny, nz) fp32 on the GPU over `bounds`.  Normals point from
    grid >= iso towards lower values, faces wind accordingly; an empty surface gives zero-length tensors."""
    return ops.mesh.extract_isosurface(grid, iso, bounds)


def mesh_components(faces: torch.Tensor, num_vertices: int) -> torch.Tensor:
    """labels (V,) int32: the smallest vertex id of every vertex's connected component (ops.mesh.mesh_components)."""
    return ops.mesh.mesh_components(faces, num_vertices)


def component_sizes(labels: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """(V,) int32: faces per component at index = label, zero elsewhere (ops.mesh.component_sizes)."""
    return ops.mesh.component_sizes(labels, faces)


@torch.no_grad()
def filter_mesh(mesh: Dict[str, torch.Tensor], min_faces: Optional[int] = None,
                keep_largest: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The mesh without its small components.  A component (mesh_components) stays when it has at least `min_faces` faces
    and, if `keep_largest` = k is given, is among the k components with the most faces, ties going to the smaller label.
    A component without a face (an unreferenced vertex) never stays.  Kept vertices and faces keep their relative order,
    faces are re-indexed, every tensor of the dict whose first dimension is V ('vertices', 'normals', 'colors', ...) is
    compacted alike, and the result gains 'vertex_index' (V',) int32: the id every kept vertex had in `mesh`.  An empty result
    gives zero-length tensors.  With both arguments None the SAME dict comes back.
    Host synchronisations: one read of two ints per labelling round (mesh_components), then ONE read of the vertex and
    the face count, which size the outputs; which components stay is decided on the device (topk, cumsum)."""
    if min_faces is None and keep_largest is None:
        return mesh
    faces, vertices = mesh['faces'], mesh['vertices']
    v = vertices.shape[0]
    dev = faces.device
    per_vertex = [k for k, t in mesh.items() if k not in ('faces', 'vertex_index') and isinstance(t, torch.Tensor)
                  and t.dim() >= 1 and t.shape[0] == v]
    labels = ops.mesh.mesh_components(faces, v)
    sizes = ops.mesh.component_sizes(labels, faces)
    keep = sizes >= max(int(min_faces or 0), 1)
    if keep_largest is not None:
        k = int(keep_largest)
        if k <= 0:
            keep = torch.zeros_like(keep)
        elif k < v:
            # the k-th largest size t: everything above it stays, and of the components AT t the first (k - #above) by label
            t = torch.topk(sizes, k).values[-1]
            above, at = sizes > t, sizes == t
            keep &= above | (at & (torch.cumsum(at, 0) <= k - above.sum()))
    vertex_index, new_faces = ops.mesh.compact_mesh(faces, labels, keep)
    out = dict(mesh)
    for name in per_vertex:
        out[name] = ops.mesh.gather_rows(mesh[name], vertex_index)
    out['faces'] = new_faces
    out['vertex_index'] = vertex_index
    return out


@torch.no_grad()
def vertex_colors(model, vertices: torch.Tensor, normals: Optional[torch.Tensor], frame_id: int,
                  view: Union[str, Sequence[float], torch.Tensor] = 'normal', level: str = 'fine', chunk: int = 1 << 20,
                  render_opts=None, dtype=torch.uint8) -> torch.Tensor:
    """(V, 3) colours of mesh vertices at frame `frame_id`: the field's `rgb` (NerfModel.query_points) at the vertex
    position, seen along -normal/|normal| (`view='normal'`: head-on from outside) or from the camera position `view` =
    (cx, cy, cz), along (v - c)/|v - c|; a zero normal or v == c looks along (0, 0, 1).  The id fills every metadata key,
    as in density_grid.  `chunk` vertices at a time, as rows of ONE point with their own direction (hn_vertex_viewdirs
    writes a chunk of directions; the full direction tensor never exists); the values do not depend on `chunk`.
    dtype float32: that rgb; uint8: (rgb * 255) truncated on the device, the convention of inference.evaluate_images.
    A model with use_viewdirs=False ignores the direction.  Inference only; no state is left on the model."""
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"vertex_colors: dtype must be torch.uint8 or torch.float32, got {dtype}")
    if int(chunk) < 1:
        raise ValueError(f"vertex_colors: chunk must be positive, got {chunk}")
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertex_colors: vertices must be a (V, 3) tensor")
    camera = None
    if not (isinstance(view, str) and view == 'normal'):
        if isinstance(view, str):
            raise ValueError(f"vertex_colors: view must be 'normal' or a camera position (cx, cy, cz), got {view!r}")
        camera = [float(x) for x in (view.detach().cpu().reshape(-1).tolist() if isinstance(view, torch.Tensor) else view)]
        if len(camera) != 3:
            raise ValueError(f"vertex_colors: a camera position has three components, got {len(camera)}")
    elif normals is None or normals.shape != vertices.shape:
        raise ValueError("vertex_colors: view='normal' needs normals of the vertices' shape")
    device = next(model.parameters()).device
    vertices = vertices.detach().to(device=device, dtype=torch.float32).contiguous()
    if camera is None:
        normals = normals.detach().to(device=device, dtype=torch.float32).contiguous()
    v = vertices.shape[0]
    out = torch.empty((v, 3), dtype=dtype, device=device)
    chunk = min(int(chunk), max(v, 1))
    ids = torch.full((chunk,), int(frame_id), dtype=torch.int64, device=device)
    for start in range(0, v, chunk):
        n = min(chunk, v - start)
        dirs = ops.mesh.vertex_viewdirs(vertices, normals, start, n, camera)
        metadata = {k: ids[:n] for k in ('warp', 'camera', 'appearance', 'time')}
        rgb = model.query_points(vertices[start:start + n].view(n, 1, 3), metadata, level=level, viewdirs=dirs,
                                 render_opts=render_opts)['rgb'].view(n, 3)
        out[start:start + n] = rgb if dtype == torch.float32 else (rgb * 255).to(torch.uint8)
    return out


def _simplify_factor(simplify):
    """Three positive finite floats from extract_mesh's `simplify`, or ValueError."""
    k = ops.checks.float3(simplify, "extract_mesh: simplify")
    if not all(np.isfinite(x) and x > 0.0 for x in k):
        raise ValueError(f"extract_mesh: simplify must be positive and finite, got {simplify!r}")
    return k


@torch.no_grad()
def simplify_mesh(mesh: Dict[str, torch.Tensor], cell, origin=None, placement: str = 'quadric',
                  regularization: float = 0.1) -> Dict[str, torch.Tensor]:
    """The mesh simplified by vertex clustering (csrc/hn_simplify.hip; DESIGN.md holds the definition).  mesh: a dict as
    extract_isosurface / filter_mesh return it — 'vertices' (V, 3) fp32, 'faces' (F, 3) int32, optional 'normals' (V, 3)
    fp32 and 'colors' (V, 3) uint8 or fp32.  `cell`: the cell size, a float or three, positive and finite; `origin`: three
    floats, None = the per-axis minimum of the vertices.  All vertices of a cell idx_c = floor((v_c - origin_c) / cell_c)
    collapse into one: placement='mean' puts it at their mean, 'quadric' (needs 'normals') at the point of the cell
    closest to their tangent planes, pulled towards the mean by `regularization`.  Its normal is the normalised sum of the
    members' normals, its colour their mean.  Faces go through the collapse; those that degenerate leave, and so do pairs
    of opposite faces over the same three vertices (folded flaps): the directed edges of the result balance as those of
    the input did.
    Returns 'vertices', 'faces', 'normals' and 'colors' when they were given, and 'vertex_cluster' (V,) int32: the output
    vertex of every input vertex, -1 where its cluster lost all its faces.  Other keys of `mesh`, 'vertex_index'
    included, are NOT carried over (an output vertex stands for several input ones).  Output vertices ascend with their
    cell key ix | iy << 21 | iz << 42, faces with their sorted vertex triple; two runs give the same bits; an empty
    input, or one that collapses entirely, gives zero-length tensors.
    ValueError: origin above the vertices' minimum, 2**21 or more cells along an axis, vertices that are not finite.
    Host synchronisations, four: the extent of the vertices (one read of six floats), the cluster count, the output
    face count, the output vertex count."""
    what = "simplify_mesh"
    if placement not in ('quadric', 'mean'):
        raise ValueError(f"{what}: placement must be 'quadric' or 'mean', got {placement!r}")
    vertices = ops.checks.check_points(mesh.get('vertices'), what, "vertices")
    v = vertices.shape[0]
    faces = mesh.get('faces')
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{what}: faces must be a (F, 3) int32 tensor")
    normals, colors = mesh.get('normals'), mesh.get('colors')
    if normals is not None:
        normals = ops.checks.check_points(normals, what, "normals", v)
    elif placement == 'quadric':
        raise ValueError(f"{what}: placement='quadric' needs the mesh's 'normals'")
    if colors is not None and (not isinstance(colors, torch.Tensor) or colors.shape != (v, 3)
                               or colors.dtype not in (torch.uint8, torch.float32)):
        raise ValueError(f"{what}: colors must be a ({v}, 3) uint8 or float32 tensor")
    regularization = float(regularization)
    if not (np.isfinite(regularization) and regularization >= 0.0):
        raise ValueError(f"{what}: regularization must be finite and not negative, got {regularization}")
    cell_c, _ = ops.simplify.check_cells(cell, (0.0, 0.0, 0.0) if origin is None else origin, what)
    dev = vertices.device

    def empty():
        out = {'vertices': torch.zeros((0, 3), dtype=torch.float32, device=dev),
               'faces': torch.zeros((0, 3), dtype=torch.int32, device=dev),
               'vertex_cluster': torch.full((v,), -1, dtype=torch.int32, device=dev)}
        if normals is not None:
            out['normals'] = torch.zeros((0, 3), dtype=torch.float32, device=dev)
        if colors is not None:
            out['colors'] = torch.zeros((0, 3), dtype=colors.dtype, device=dev)
        return out

    if v:
        # host read 1: the extent, which the key layout (21 bits per axis, no negative index) must hold
        lo, hi = (np.asarray(t, dtype=np.float32) for t in ops.simplify.vertex_extent(vertices))
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError(f"{what}: the vertices are not finite")
        origin_f = lo if origin is None else np.asarray(ops.checks.float3(origin, f"{what}: origin"), dtype=np.float32)
        cell_f = np.asarray(list(cell_c), dtype=np.float32)
        if (origin_f > lo).any():
            raise ValueError(f"{what}: origin {origin_f.tolist()} lies above the vertices' minimum {lo.tolist()}")
        with np.errstate(all="ignore"):
            cells = np.floor((hi - origin_f) / cell_f)
        if not (cells < 2 ** ops.simplify.CELL_BITS).all():
            raise ValueError(f"{what}: the vertices span {cells.tolist()} cells from the origin; the keys hold fewer than "
                             f"2**{ops.simplify.CELL_BITS} = {2 ** ops.simplify.CELL_BITS} per axis")
        origin = origin_f.tolist()
    if not vertices.is_cuda or not faces.is_cuda:
        raise ValueError(f"{what}: the mesh must live on the GPU (there is no CPU fallback)")
    if v == 0 or faces.shape[0] == 0:
        return empty()
    clusters = ops.simplify.cluster_vertices(vertices, cell, origin)                        # host read 2: the cluster count
    n_clusters = clusters['cluster_keys'].shape[0]
    cfaces, used = ops.simplify.cluster_faces(faces, clusters['vertex_cluster'], n_clusters,
                                              return_used=True)                             # host read 3: F'
    n_faces = cfaces.shape[0]
    if n_faces == 0:
        return empty()
    rep = ops.simplify.reduce_clusters(vertices, normals, colors, clusters, cell, origin, placement, regularization)
    scan = torch.cumsum(used, 0, dtype=torch.int32)
    n_out = int(scan[-1])                                                                   # host read 4: V'
    kept = torch.empty(n_out, dtype=torch.int32, device=dev)
    out_faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    every_face = torch.arange(1, n_faces + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.launch("hn_mesh_compact", L.ptr(cfaces), L.ptr(scan), L.ptr(every_face), n_clusters, n_faces, n_out,
                 n_faces, L.ptr(kept), L.ptr(out_faces), L.stream_handle())
    out = {name: ops.mesh.gather_rows(t, kept) for name, t in rep.items()}
    out['faces'] = out_faces
    out['vertex_cluster'] = ops.simplify.relabel_vertices(clusters['vertex_cluster'], used, scan)
    return out


def _finish_mesh(mesh, model, bounds, resolution, frame_id, factor, colors, min_faces, keep_largest, kw):
    """The tail extract_mesh and extract_mesh_fused share: filter_mesh, simplify_mesh by `factor` lattice spacings (None: not
    at all), vertex_colors(view=colors) on what survived."""
    mesh = filter_mesh(mesh, min_faces=min_faces, keep_largest=keep_largest)
    if factor is not None:
        shape, b = ops.mesh.check_lattice(_resolution(resolution), bounds, "extract_mesh")
        cell = [k * (b[2 * c + 1] - b[2 * c]) / (shape[c] - 1) for c, k in enumerate(factor)]
        mesh = simplify_mesh(mesh, cell, origin=(b[0], b[2], b[4]))
    if colors is not None:
        mesh = dict(mesh)
        mesh['colors'] = vertex_colors(model, mesh['vertices'], mesh['normals'], frame_id, view=colors, **kw)
    return mesh


def extract_mesh(model, bounds, resolution, frame_id: int, iso: float = 10.0, colors=None, min_faces: Optional[int] = None,
                 keep_largest: Optional[int] = None, simplify=None, **kw) -> Dict[str, torch.Tensor]:
    """extract_isosurface(density_grid(model, bounds, resolution, frame_id, **kw), iso, bounds), then
    filter_mesh(min_faces, keep_largest) when either is given, then simplify_mesh when `simplify` = k (a float or three,
    in units of the lattice spacing) is given: cells of k * (hi - lo)/(n - 1) per axis from the lower bounds, so the
    clusters align with the lattice; then — only on what survived, along the new normals — 'colors' (V, 3) uint8 =
    vertex_colors(view=colors) when `colors` is 'normal' or a camera position, with density_grid's level / chunk /
    render_opts."""
    factor = None if simplify is None else _simplify_factor(simplify)
    mesh = extract_isosurface(density_grid(model, bounds, resolution, frame_id, **kw), iso, bounds)
    return _finish_mesh(mesh, model, bounds, resolution, frame_id, factor, colors, min_faces, keep_largest, kw)


# ---- depth fusion: a surface where the field RENDERS it (csrc/hn_fusion.hip) ----------------------------
def _refuse_ndc(ndc, what: str):
    if ndc:
        raise ValueError(f"{what}: NDC rays have no pinhole camera (the NDC transform moves origins and bends directions "
                         "per pixel) and their depth is no distance; fuse depth in world space with ndc=False rays")


def _check_cameras(cameras, what: str) -> torch.Tensor:
    """(N >= 1, 24) float32 camera records as a tensor (a host array is copied and stays on the host), or ValueError."""
    if not isinstance(cameras, torch.Tensor) and hasattr(cameras, "__array__"):
        cameras = torch.from_numpy(np.array(cameras))      # a copy: the array may be read-only
    n_floats = ops.data.NERFIES_CAM_FLOATS
    if (not isinstance(cameras, torch.Tensor) or cameras.dim() != 2 or cameras.shape[1] != n_floats
            or cameras.dtype != torch.float32 or cameras.shape[0] < 1):
        raise ValueError(f"{what}: cameras must be (N >= 1, {n_floats}) float32 camera records")
    return cameras.detach()


@torch.no_grad()
def fuse_depth(depths: torch.Tensor, cameras, bounds, resolution, trunc: Optional[float] = None,
               volume: Optional[Dict[str, torch.Tensor]] = None, *, ndc: bool = False) -> Dict[str, torch.Tensor]:
    """{'tsdf', 'weight'}: two (nx, ny, nz) fp32 volumes on the device of `depths`, the depth images (N, H, W) fp32 seen
    through `cameras` (N, 24) (camera_from_c2w, orbit_cameras, NerfiesDataset.camera_record; NDC scenes have no such
    camera) integrated into a truncated signed distance volume on the lattice of `resolution` points over `bounds`
    (ops.mesh.tsdf_integrate).  A depth is the distance along the unit ray from the camera position — what
    render_image's and render_mesh's depth are —, +inf where the ray hit nothing, anything not > 0 where nothing is
    known.  tsdf is positive in front of the surface (1 = at least `trunc` in front), negative behind it down to -1,
    and means nothing where weight (the number of views that saw the point) is 0.  trunc: 4 times the largest lattice
    spacing by default.  volume: an earlier result on the same lattice, continued IN PLACE and returned.  ndc=True (the
    scene's rays are NDC rays) is refused, as camera_from_c2w refuses it."""
    what = "fuse_depth"
    _refuse_ndc(ndc, what)
    shape, bounds = ops.mesh.check_lattice(_resolution(resolution), bounds, what)
    if not isinstance(depths, torch.Tensor) or depths.dim() != 3 or depths.dtype != torch.float32:
        raise ValueError(f"{what}: depths must be a (N, H, W) float32 tensor")
    cameras = _check_cameras(cameras, what)
    if cameras.shape[0] != depths.shape[0]:
        raise ValueError(f"{what}: {depths.shape[0]} depth images for {cameras.shape[0]} cameras")
    if trunc is None:
        trunc = 4.0 * max((bounds[2 * c + 1] - bounds[2 * c]) / (shape[c] - 1) for c in range(3))
    trunc = float(trunc)
    if not (np.isfinite(trunc) and trunc > 0.0):
        raise ValueError(f"{what}: trunc must be positive and finite, got {trunc}")
    if volume is not None:
        if not isinstance(volume, dict) or 'tsdf' not in volume or 'weight' not in volume:
            raise ValueError(f"{what}: volume must be a dict with 'tsdf' and 'weight', as fuse_depth returns it")
        for k in ('tsdf', 'weight'):
            ops.mesh.check_volume(volume[k], what, f"volume['{k}']", shape)
    if not depths.is_cuda:
        raise ValueError(f"{what}: depths must live on the GPU (there is no CPU fallback)")
    if volume is None:
        volume = {k: torch.zeros(shape, dtype=torch.float32, device=depths.device) for k in ('tsdf', 'weight')}
    ops.mesh.tsdf_integrate(volume['tsdf'], volume['weight'], bounds, cameras.to(depths.device), depths, trunc)
    return {'tsdf': volume['tsdf'], 'weight': volume['weight']}


@torch.no_grad()
def depth_images_from_field(model, cameras, image_wh, frame_id: int, near: float, far: float, acc_min: float = 0.5,
                            acc_free: float = 0.05, normalize: bool = True, level: str = 'fine',
                            chunk: int = 16384, *, ndc: bool = False, occupancy=None) -> torch.Tensor:
    """(N, H, W) fp32 depth images of the field at frame `frame_id` through `cameras` (N, 24), in fuse_depth's convention.
    Per camera: camera_rays(near, far), a ninth column holding frame_id (as the rays of a dataset carry it), then
    inference.render_image(keys=('depth', 'acc')).  Where acc >= acc_min the pixel is a surface at depth / acc
    (`normalize`: the expected distance of the mass the ray did meet) or at depth; where acc <= acc_free the ray hit
    nothing: +inf; in between nothing is known: 0.  The two thresholds are the caller's to set: they decide what counts
    as seen, and no value suits every scene.  ndc=True (a model trained on NDC rays) is refused.
    occupancy: an occupancy dict (occupancy_grid) or an OccupancyCache, asked for `frame_id`; the rays are then clipped to
    the occupied cells before they are rendered (inference.render_image's `occupancy`).  With both ends
    clipped the sample a model with use_sample_at_infinity treats as 'at infinity' sits at the exit of the last occupied
    cell, not at `far`; a lattice can miss structure thinner than a cell (sigma_min and dilate are the guard); a model
    with use_linear_disparity spaces its samples over the clipped interval.  None: the launches are unchanged."""
    from . import inference
    what = "depth_images_from_field"
    _refuse_ndc(ndc, what)
    cameras = _check_cameras(cameras, what)
    w, h = ops.mesh_render.check_image_wh(image_wh, what)
    acc_min, acc_free = float(acc_min), float(acc_free)
    if not 0.0 <= acc_free < acc_min <= 1.0:
        raise ValueError(f"{what}: the thresholds need 0 <= acc_free < acc_min <= 1, got acc_free {acc_free}, acc_min {acc_min}")
    device = next(model.parameters()).device
    occ_kw = {}
    if occupancy is not None:
        occ_kw['occupancy'] = occupancy.get(int(frame_id)) if isinstance(occupancy, OccupancyCache) else occupancy
    out = torch.empty((cameras.shape[0], h, w), dtype=torch.float32, device=device)
    for n, cam in enumerate(cameras.to(device)):
        rays = camera_rays(cam, w, h, near, far)
        rays = torch.cat([rays, torch.full((rays.shape[0], 1), float(int(frame_id)), device=device)], dim=1)
        field = inference.render_image(model, rays, chunk=chunk, level=level, keys=('depth', 'acc'), **occ_kw)
        depth, acc = field['depth'].reshape(h, w).float(), field['acc'].reshape(h, w).float()
        surface = depth / acc if normalize else depth
        out[n] = torch.where(acc >= acc_min, surface,
                             torch.where(acc <= acc_free, torch.full_like(depth, float('inf')), torch.zeros_like(depth)))
    return out


@torch.no_grad()
def tsdf_isosurface(volume: Dict[str, torch.Tensor], bounds, observed_only: bool = True) -> Dict[str, torch.Tensor]:
    """The mesh dict of the zero level set of a fuse_depth volume: extract_isosurface(g, 0.0, bounds) of the lattice
    g = -tsdf where weight > 0 and +1 elsewhere.  Space no view ever saw counts as solid, so the inside of an object
    stays filled, and the normals point out of the surface, towards the cameras.  That puts faces between seen free
    space and unseen space too (the walls of the viewing frusta); observed_only=True drops every face whose centroid
    lies in a lattice cell with a never-observed corner (ops.mesh.tsdf_face_keep), compacts the mesh as filter_mesh
    does ('vertices' and 'normals' gathered, faces re-indexed) and adds 'vertex_index' (V',) int32: the id each kept
    vertex had before.  The surface then has holes where nothing was observed.  One more host read (both counts)."""
    what = "tsdf_isosurface"
    if not isinstance(volume, dict) or 'tsdf' not in volume or 'weight' not in volume:
        raise ValueError(f"{what}: volume must be a dict with 'tsdf' and 'weight', as fuse_depth returns it")
    tsdf = ops.mesh.check_volume(volume['tsdf'], what, "volume['tsdf']")
    weight = ops.mesh.check_volume(volume['weight'], what, "volume['weight']", tsdf.shape)
    _, bounds = ops.mesh.check_lattice(tsdf.shape, bounds, what)
    if not (tsdf.is_cuda and weight.is_cuda):
        raise ValueError(f"{what}: the volume must live on the GPU (there is no CPU fallback)")
    mesh = ops.mesh.extract_isosurface(torch.where(weight > 0, -tsdf, torch.ones_like(tsdf)), 0.0, bounds)
    if not observed_only:
        return mesh
    faces, v = mesh['faces'], mesh['vertices'].shape[0]
    dev = faces.device
    if v == 0 or faces.shape[0] == 0:
        return {'vertices': mesh['vertices'][:0], 'normals': mesh['normals'][:0], 'faces': faces[:0],
                'vertex_index': torch.zeros(0, dtype=torch.int32, device=dev)}
    fkeep, vkeep = ops.mesh.tsdf_face_keep(mesh['vertices'], faces, weight, bounds)
    vertex_index, faces_out = ops.mesh.compact_kept(faces, vkeep, fkeep)
    return {'vertices': ops.mesh.gather_rows(mesh['vertices'], vertex_index),
            'normals': ops.mesh.gather_rows(mesh['normals'], vertex_index), 'faces': faces_out,
            'vertex_index': vertex_index}


def extract_mesh_fused(model, bounds, resolution, frame_id: int, cameras, image_wh, near: float, far: float,
                       trunc: Optional[float] = None, min_faces: Optional[int] = None, keep_largest: Optional[int] = None,
                       simplify=None, colors=None, *, ndc: bool = False, occupancy=None, **kw) -> Dict[str, torch.Tensor]:
    """The surface of frame `frame_id` where the field renders it, with no iso level to guess:
    tsdf_isosurface(fuse_depth(depth_images_from_field(model, cameras, image_wh, frame_id, near, far), cameras, bounds,
    resolution, trunc), bounds), then extract_mesh's tail: filter_mesh(min_faces, keep_largest), simplify_mesh by
    `simplify` lattice spacings, 'colors' = vertex_colors(view=colors).  Of **kw, acc_min / acc_free / normalize go to
    depth_images_from_field, level / chunk to it and to vertex_colors, render_opts to vertex_colors.  ndc=True is
    refused.  occupancy (a dict or an OccupancyCache) goes to depth_images_from_field: the depth maps are rendered with
    empty space skipped."""
    _refuse_ndc(ndc, "extract_mesh_fused")
    factor = None if simplify is None else _simplify_factor(simplify)
    field_kw = {k: kw[k] for k in ('acc_min', 'acc_free', 'normalize', 'level', 'chunk') if k in kw}
    color_kw = {k: kw[k] for k in ('level', 'chunk', 'render_opts') if k in kw}
    unknown = set(kw) - set(field_kw) - set(color_kw)
    if unknown:
        raise TypeError(f"extract_mesh_fused: unexpected keyword arguments {sorted(unknown)}")
    if occupancy is not None:
        field_kw['occupancy'] = occupancy
    depths = depth_images_from_field(model, cameras, image_wh, frame_id, near, far, **field_kw)
    mesh = tsdf_isosurface(fuse_depth(depths, cameras, bounds, resolution, trunc), bounds)
    return _finish_mesh(mesh, model, bounds, resolution, frame_id, factor, colors, min_faces, keep_largest, color_kw)


# ---- looking at a mesh: ray casting through the cameras the field is rendered with (csrc/hn_mesh_render.hip) ------------
def _check_render_mesh(mesh, what: str):
    """(vertices, faces, normals, colors) of a mesh dict, checked as far as the host can, or ValueError."""
    if not isinstance(mesh, dict):
        raise ValueError(f"{what}: mesh must be a dict with 'vertices' and 'faces'")
    vertices = ops.checks.check_points(mesh.get('vertices'), what, "vertices")
    faces = ops.checks.check_mesh_faces(mesh.get('faces'), what)
    v = vertices.shape[0]
    normals, colors = mesh.get('normals'), mesh.get('colors')
    if normals is not None:
        normals = ops.checks.check_points(normals, what, "normals", v)
    if colors is not None and (not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (v, 3)
                               or colors.dtype not in (torch.uint8, torch.float32)):
        raise ValueError(f"{what}: colors must be a ({v}, 3) uint8 or float32 tensor")
    return vertices, faces, normals, colors


@torch.no_grad()
def render_mesh(mesh: Dict[str, torch.Tensor], rays: torch.Tensor, camera, image_wh, shading: str = 'headlight',
                ambient: float = 0.3, background=(1.0, 1.0, 1.0), base_color=(0.8, 0.8, 0.8),
                binning: bool = True) -> Dict[str, torch.Tensor]:
    """The mesh seen through a camera of the field: {'face': (H, W) int32, -1 where no face is hit, 'depth': (H, W) fp32,
    the distance along the unit ray (0 for none), 'bary': (H, W, 3) fp32, 'normal': (H, W, 3) fp32, 'rgb': (H, W, 3) fp32,
    'rgb8': (H, W, 3) uint8} on the mesh's device.
    mesh: the dict every function here passes around ('vertices' (V, 3) fp32, 'faces' (F, 3) int32, optional 'normals'
    (V, 3) fp32 and 'colors' (V, 3) uint8 or fp32).  rays: (H*W, >= 6) fp32, row j*W + i the ray of pixel (col i, row j) —
    the tensor render_image takes.  camera: the (24,) fp32 record those rays came from (camera_from_c2w, orbit_cameras,
    NerfiesDataset.camera_record); image_wh = (W, H).
    The picture is defined by casting exactly those rays: the camera only decides which faces a 16 x 16
    tile of pixels looks at, so depth agrees with the field's rays bit for bit, lens distortion included, faces that share
    an edge never leave a pinhole between them, hits are two-sided, and binning=False (every face at every pixel) gives
    the same bits — except on the extension of a near-degenerate sliver face, where the fp32 edge test is rounding noise
    and either picture can show a stray hit (limits).  A camera that does not match the rays drops faces.
    shading: 'headlight' — colour * (ambient + (1 - ambient) |N . d|) with N the interpolated vertex normal (the face
    normal without 'normals') — or 'none'; colour: the interpolated 'colors', `base_color` without them; `background`
    where nothing is hit.  An empty mesh gives an all-background image.
    ValueError: a face with a vertex id outside [0, V); more than 2**31 - 1 (tile, face) pairs.  One host read."""
    what = "render_mesh"
    vertices, faces, normals, colors = _check_render_mesh(mesh, what)
    w, h = ops.mesh_render.check_image_wh(image_wh, what)
    camera = ops.checks.check_camera(camera, what)
    rays = ops.checks.check_rays(rays, h * w, what)
    ops.mesh_render.check_shading(shading, ambient, background, base_color, what)
    if not vertices.is_cuda or not faces.is_cuda or not rays.is_cuda:
        raise ValueError(f"{what}: the mesh and the rays must live on the GPU (there is no CPU fallback)")
    out = ops.mesh_render.mesh_trace(vertices, faces, rays, camera, (w, h), binning=bool(binning))
    out.update(ops.mesh_render.mesh_shade(vertices, faces, normals, colors, rays, out['face'], out['bary'], shading,
                                          ambient, background, base_color))
    return {k: t.view((h, w) + tuple(t.shape[1:])) for k, t in out.items()}


def camera_from_c2w(c2w, focal: float, W: int, H: int, ndc: bool = False) -> np.ndarray:
    """The (24,) fp32 camera record whose rays are the LLFF / Blender rays of the pose c2w (3, 4) with `focal`
    (ops.data.generate_rays without NDC): orientation rows c2w[:, 0], -c2w[:, 1], -c2w[:, 2] (the pose looks along -z
    with y up, the record along +z with y down), position c2w[:, 3], principal point (W/2 + 0.5, H/2 + 0.5) (a pixel
    index there is a pixel centre here), no skew, no distortion.  The pose's rotation must be orthonormal, as a pose is.
    NDC scenes are refused: a mesh in NDC space is not seen through a pinhole camera."""
    if ndc:
        raise ValueError("camera_from_c2w: NDC rays have no pinhole camera (the NDC transform moves origins and bends "
                         "directions per pixel); extract and render the mesh in world space with ndc=False rays")
    c2w = np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float64)
    if c2w.shape != (3, 4):
        raise ValueError(f"camera_from_c2w: c2w must be (3, 4), got {c2w.shape}")
    focal, W, H = float(focal), int(W), int(H)
    if not (np.isfinite(focal) and focal > 0.0) or W < 1 or H < 1:
        raise ValueError("camera_from_c2w: focal, W and H must be positive")
    rec = np.zeros(ops.data.NERFIES_CAM_FLOATS, dtype=np.float64)
    rec[0:3], rec[3:6], rec[6:9], rec[9:12] = c2w[:, 0], -c2w[:, 1], -c2w[:, 2], c2w[:, 3]
    rec[12:17] = (focal, 1.0, 0.0, W / 2 + 0.5, H / 2 + 0.5)
    return rec.astype(np.float32)


def orbit_cameras(center, radius: float, n: int, elevation: float = 0.0, up=(0.0, -1.0, 0.0), *, focal: float,
                  image_wh) -> np.ndarray:
    """(n, 24) fp32 camera records on a circle around `center`, all looking at it: camera k sits at azimuth 2 pi k / n and
    `elevation` degrees (-90 < elevation < 90) above the plane through `center` whose normal is `up`, at distance `radius`;
    `up` appears up in the image (the record's y axis points down).  focal in pixels, the principal point at the image
    centre (W/2, H/2), no skew, no distortion.  NumPy float64, rounded to fp32 at the end."""
    what = "orbit_cameras"
    c = np.asarray(ops.checks.float3(center, f"{what}: center"), dtype=np.float64)
    u = np.asarray(ops.checks.float3(up, f"{what}: up"), dtype=np.float64)
    w, h = ops.mesh_render.check_image_wh(image_wh, what)
    radius, focal, elevation, n = float(radius), float(focal), float(elevation), int(n)
    if n < 1:
        raise ValueError(f"{what}: n must be at least 1, got {n}")
    if not (np.isfinite(radius) and radius > 0.0) or not (np.isfinite(focal) and focal > 0.0):
        raise ValueError(f"{what}: radius and focal must be positive and finite")
    if not -90.0 < elevation < 90.0:
        raise ValueError(f"{what}: elevation must lie strictly between -90 and 90 degrees, got {elevation}")
    if not np.isfinite(c).all() or not np.isfinite(u).all() or not np.linalg.norm(u) > 0.0:
        raise ValueError(f"{what}: center must be finite and up a finite non-zero vector")
    u = u / np.linalg.norm(u)
    e1 = np.cross(u, np.eye(3)[int(np.argmin(np.abs(u)))])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    el = np.deg2rad(elevation)
    out = np.zeros((n, ops.data.NERFIES_CAM_FLOATS), dtype=np.float64)
    for k in range(n):
        az = 2.0 * np.pi * k / n
        pos = c + radius * (np.cos(el) * (np.cos(az) * e1 + np.sin(az) * e2) + np.sin(el) * u)
        z = (c - pos) / np.linalg.norm(c - pos)
        x = np.cross(-u, z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        out[k, 0:3], out[k, 3:6], out[k, 6:9], out[k, 9:12] = x, y, z, pos
        out[k, 12:17] = (focal, 1.0, 0.0, w / 2, h / 2)
    return out.astype(np.float32)


def camera_rays(record, W: int, H: int, near: float, far: float, device=None) -> torch.Tensor:
    """(H*W, 8) fp32 ray rows [o, d, near, far] of a (24,) camera record, generated on the GPU
    (ops.data.generate_rays_nerfies); `device`: where, the record's own device by default (a host record goes to the
    current GPU)."""
    cam = ops.checks.check_camera(record, "camera_rays")
    w, h = ops.mesh_render.check_image_wh((W, H), "camera_rays")
    if device is None and not cam.is_cuda:
        if not torch.cuda.is_available():
            L.require_gpu(cam)
        device = torch.device("cuda", torch.cuda.current_device())
    if device is not None:
        cam = cam.to(device)
    with torch.cuda.device(cam.device):
        return ops.data.generate_rays_nerfies(h, w, cam, float(near), float(far))


@torch.no_grad()
def mesh_turntable(mesh: Dict[str, torch.Tensor], path, n: int = 60, image_wh=(256, 256), elevation: float = 20.0,
                   radius: Optional[float] = None, focal: Optional[float] = None, up=(0.0, -1.0, 0.0), fps: float = 30,
                   **render_kw) -> np.ndarray:
    """An animated GIF of the mesh on a turntable: orbit_cameras around the centre of the vertices' bounding box (n
    cameras, `elevation` degrees, `up`), render_mesh(**render_kw) per camera, the rgb8 frames through
    inference.write_gif(path, frames, fps).  radius: 3 half-diagonals of the box by default; focal: by default the one at
    which the box's bounding sphere spans 0.9 of the smaller image side.  Returns the (n, 24) records."""
    from . import inference
    what = "mesh_turntable"
    vertices, _, _, _ = _check_render_mesh(mesh, what)
    w, h = ops.mesh_render.check_image_wh(image_wh, what)
    if vertices.shape[0] == 0:
        raise ValueError(f"{what}: the mesh has no vertices")
    if not vertices.is_cuda:
        raise ValueError(f"{what}: the mesh must live on the GPU (there is no CPU fallback)")
    lo, hi = (np.asarray(t, dtype=np.float64) for t in ops.simplify.vertex_extent(vertices))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"{what}: the vertices are not finite")
    half = max(0.5 * float(np.linalg.norm(hi - lo)), 1e-6)
    radius = 3.0 * half if radius is None else float(radius)
    if focal is None:
        if not radius > half:
            raise ValueError(f"{what}: radius {radius} lies inside the bounding sphere ({half}); give focal")
        focal = 0.45 * min(w, h) * np.sqrt(radius * radius - half * half) / half
    cams = orbit_cameras(0.5 * (lo + hi), radius, n, elevation, up, focal=focal, image_wh=(w, h))
    frames = []
    for rec in cams:
        cam = torch.from_numpy(rec).to(vertices.device)
        rays = camera_rays(cam, w, h, 0.0, radius + half)
        frames.append(render_mesh(mesh, rays, cam, (w, h), **render_kw)['rgb8'])
    inference.write_gif(path, frames, fps=fps)
    return cams


@torch.no_grad()
def depth_agreement(mesh_depth: torch.Tensor, mesh_face: torch.Tensor, field_depth: torch.Tensor, field_acc: torch.Tensor,
                    acc_min: float = 0.5) -> Dict[str, torch.Tensor]:
    """How well a mesh's depth image agrees with the field's: {'abs_mean', 'rmse', 'iou', 'n'} as scalars on the inputs'
    device (no host read).  The mesh covers a pixel when mesh_face >= 0, the field when field_acc >= acc_min; 'n' (int64) is
    the number of pixels both cover, 'abs_mean' and 'rmse' the mean absolute and root mean square of mesh_depth -
    field_depth over them (float64 sums; NaN when n is 0), 'iou' the intersection over the union of the two coverages
    (NaN when neither covers anything).  The four tensors hold one value per pixel, in any matching shape."""
    tensors = (mesh_depth, mesh_face, field_depth, field_acc)
    if not all(isinstance(t, torch.Tensor) for t in tensors):
        raise ValueError("depth_agreement: mesh_depth, mesh_face, field_depth and field_acc must be tensors")
    numel = mesh_depth.numel()
    if any(t.numel() != numel for t in tensors):
        raise ValueError(f"depth_agreement: the four images differ in size: {[tuple(t.shape) for t in tensors]}")
    if mesh_face.dtype.is_floating_point:
        raise ValueError("depth_agreement: mesh_face must hold integer face ids")
    md, mf, fd, fa = (t.detach().reshape(-1) for t in tensors)
    mesh_cov, field_cov = mf >= 0, fa >= float(acc_min)
    both = mesh_cov & field_cov
    n = both.sum()
    err = torch.where(both, md.double() - fd.double(), torch.zeros((), dtype=torch.float64, device=md.device))
    return {'abs_mean': err.abs().sum() / n, 'rmse': torch.sqrt((err * err).sum() / n),
            'iou': n / (mesh_cov | field_cov).sum(), 'n': n}


@torch.no_grad()
def mesh_depth_error(model, mesh: Dict[str, torch.Tensor], rays: torch.Tensor, camera, image_wh, chunk: int = 16384,
                     depth_key: str = 'depth', acc_min: float = 0.5, level: str = 'fine') -> Dict[str, torch.Tensor]:
    """depth_agreement between the mesh and the field it came from, through one camera: the field's `depth_key` and
    'acc' from inference.render_image(model, rays, chunk, level), the mesh's depth and face from render_mesh along the
    same rays.  Tells whether the iso level, min_faces and the simplification cell left the surface where the field
    renders it."""
    from . import inference
    w, h = ops.mesh_render.check_image_wh(image_wh, "mesh_depth_error")
    field = inference.render_image(model, rays, chunk=chunk, level=level, keys=(depth_key, 'acc'))
    seen = render_mesh(mesh, rays, camera, (w, h), shading='none')
    return depth_agreement(seen['depth'], seen['face'], field[depth_key], field['acc'], acc_min=acc_min)


# ---- distance between meshes (csrc/hn_mesh_distance.hip) ----------------------------------------------------
def _mesh_arrays(mesh, what: str):
    """(vertices, faces) of a mesh dict as the distance ops take them, or ValueError."""
    if not isinstance(mesh, dict) or 'vertices' not in mesh or 'faces' not in mesh:
        raise ValueError(f"{what}: a mesh is a dict with 'vertices' (V, 3) float32 and 'faces' (F, 3) int32")
    return (ops.checks.check_points(mesh['vertices'], what, "vertices"), ops.checks.check_mesh_faces(mesh['faces'], what))


@torch.no_grad()
def sample_surface(mesh: Dict[str, torch.Tensor], n: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """n independent points of the mesh's surface, uniform by area: {'points': (n, 3) fp32, 'face': (n,) int32, 'bary':
    (n, 3) fp32} with points = (b0*A + b1*B) + b2*C of the face's corners.  Sample k is a pure function of (seed, k) and
    the mesh — splitmix64 hashes, an integer table of face weights (each face's area over the largest, in 2**-24 steps:
    a face below 2**-24 of the largest, or without a finite area, is never drawn) — so every run and every machine gives
    the same bits (tests/mesh_distance_restated.py restates them in NumPy).  One host read.  ValueError: n < 1, a mesh
    without faces or without area, a vertex id outside [0, V)."""
    what = "sample_surface"
    vertices, faces = _mesh_arrays(mesh, what)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= ops.checks.INT32_MAX:
        raise ValueError(f"{what}: n must be an int in 1 .. 2**31 - 1, got {n!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"{what}: seed must be an int, got {seed!r}")
    if faces.shape[0] == 0:
        raise ValueError(f"{what}: the mesh has no faces")
    cdf = ops.mesh.surface_cdf(vertices, faces)
    return ops.mesh.sample_faces(vertices, faces, cdf, int(n), int(seed))


@torch.no_grad()
def build_distance_grid(mesh: Dict[str, torch.Tensor], grid_resolution=None) -> Dict:
    """The search structure of point_mesh_distance for `mesh`, which takes it in place of the mesh: build once, query several
    point sets.  grid_resolution: cells per axis, an int or three in 1 .. 256; 1 = one cell holding every face (brute
    force); None = round(sqrt(F) / 2) cells along the longest side of the mesh's box and cubic cells on the others
    (ops.mesh.default_grid_resolution; DESIGN.md 3.13 has the measurements behind it).  Two host reads."""
    what = "build_distance_grid"
    vertices, faces = _mesh_arrays(mesh, what)
    if grid_resolution is not None:
        ops.mesh.check_grid_resolution(grid_resolution, what)
    return ops.mesh.distance_grid(vertices, faces, grid_resolution)


@torch.no_grad()
def point_mesh_distance(points: torch.Tensor, mesh, max_distance: Optional[float] = None, grid_resolution=None,
                        sort_queries: bool = True) -> Dict[str, torch.Tensor]:
    """For every point of points (N, 3) fp32 the nearest point of the triangle mesh: {'distance': (N,) fp32, 'face': (N,)
    int32, 'closest': (N, 3) fp32} — the exact closest point of each candidate triangle by Voronoi regions, fp32 with every
    operation rounded on its own, the minimum over (squared distance, face id): ties go to the smallest face id, and the
    result is bit for bit that of testing every face, whatever the grid.  mesh: a mesh dict, or
    build_distance_grid's result (grid_resolution is then ignored).  A point that is not finite gives NaN, -1, NaN; a mesh
    without faces +inf, -1, NaN; with max_distance (>= 0) so does a point farther than that from the mesh, and the search
    stops at that radius.  sort_queries=False skips sorting the queries by cell (same bits, slower on large sets).
    Cost: a query near the surface visits a few cells; one far outside the mesh's box visits most of the grid."""
    what = "point_mesh_distance"
    points = ops.checks.check_points(points, what, "points")
    ops.mesh.check_max_distance(max_distance, what)
    if isinstance(mesh, dict) and 'cell_begin' in mesh:
        grid = mesh
    else:
        grid = build_distance_grid(mesh, grid_resolution)
    return ops.mesh.grid_query(points, grid, max_distance, bool(sort_queries))


def _distance_stats(d: torch.Tensor, taus) -> torch.Tensor:
    """[mean, mean of squares, max, share within tau ...] of fp32 distances, as float64 on their device."""
    d64 = d.double()
    parts = [d64.mean(), (d64 * d64).mean(), d64.max()] + [(d64 <= t).double().mean() for t in taus]
    return torch.stack(parts)


@torch.no_grad()
def mesh_distance(a: Dict[str, torch.Tensor], b: Dict[str, torch.Tensor], n_samples: int = 100_000, seed: int = 0,
                  thresholds=None, with_vertices: bool = False, return_distances: bool = False) -> Dict:
    """Sampled distances between two meshes: n_samples points of a (sample_surface, `seed`) to their nearest points on b, and
    n_samples of b (`seed + 1`) to a.  with_vertices appends every vertex of the sampled mesh to its samples, so that
    corners count for the maximum.  {'a_to_b': {'mean', 'rms', 'max'}, 'b_to_a': likewise, 'chamfer': (mean_ab + mean_ba)
    / 2, 'chamfer_l2': (mean(d_ab^2) + mean(d_ba^2)) / 2, 'hausdorff': max(max_ab, max_ba), 'n': (samples of a, samples of
    b)}, and with thresholds (a number or several) 'thresholds': {tau: {'precision': the share of a's samples within tau of
    b, 'recall': the share of b's within tau of a, 'fscore': 2PR / (P + R), 0 when P + R == 0}}.  Python floats: the
    reductions are torch's, float64 over the fp32 distances, read in one host read at the end.  return_distances adds
    'distances_ab' / 'distances_ba', the fp32 tensors reduced.  ValueError: a mesh without faces, n_samples < 1."""
    what = "mesh_distance"
    meshes = [_mesh_arrays(m, what) for m in (a, b)]
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or int(n_samples) < 1:
        raise ValueError(f"{what}: n_samples must be an int >= 1, got {n_samples!r}")
    if thresholds is None:
        taus = []
    else:
        try:
            taus = [float(t) for t in (thresholds if hasattr(thresholds, '__iter__') else [thresholds])]
        except (TypeError, ValueError):
            taus = [float("nan")]
        if not all(t >= 0.0 for t in taus):
            raise ValueError(f"{what}: thresholds must be numbers >= 0, got {thresholds!r}")
    for vertices, faces in meshes:
        if faces.shape[0] == 0 or vertices.shape[0] == 0:
            raise ValueError(f"{what}: a mesh without faces has no distance")
    dists = []
    for k, (src, dst) in enumerate(((a, b), (b, a))):
        pts = sample_surface(src, int(n_samples), int(seed) + k)['points']
        if with_vertices:
            pts = torch.cat([pts, meshes[k][0]], 0)
        dists.append(point_mesh_distance(pts, dst)['distance'])
    stats = torch.stack([_distance_stats(d, taus) for d in dists]).tolist()       # the one host read
    (mean_ab, sq_ab, max_ab), (mean_ba, sq_ba, max_ba) = stats[0][:3], stats[1][:3]
    out = {'a_to_b': {'mean': mean_ab, 'rms': float(np.sqrt(sq_ab)), 'max': max_ab},
           'b_to_a': {'mean': mean_ba, 'rms': float(np.sqrt(sq_ba)), 'max': max_ba},
           'chamfer': (mean_ab + mean_ba) / 2, 'chamfer_l2': (sq_ab + sq_ba) / 2, 'hausdorff': max(max_ab, max_ba),
           'n': (dists[0].shape[0], dists[1].shape[0])}
    if thresholds is not None:
        out['thresholds'] = {}
        for j, tau in enumerate(taus):
            p, r = stats[0][3 + j], stats[1][3 + j]
            out['thresholds'][tau] = {'precision': p, 'recall': r, 'fscore': 2 * p * r / (p + r) if p + r > 0 else 0.0}
    if return_distances:
        out['distances_ab'], out['distances_ba'] = dists
    return out


# ---- registration (csrc/hn_registration.hip) -----------------------------------------------------------------
def _is_grid(x) -> bool:
    return isinstance(x, dict) and 'cell_begin' in x


def _int_arg(value, what: str, name: str, least: int) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < least:
        raise ValueError(f"{what}: {name} must be an int >= {least}, got {value!r}")
    return int(value)


def _grid_corners(grid) -> torch.Tensor:
    """(3 F, 3) fp32: the corners of a distance grid's packed triangles."""
    return grid['tri'][:, :9].reshape(-1, 3)


@torch.no_grad()
def register_mesh(source, target, n_samples: int = 100_000, seed: int = 0, method: str = 'plane', with_scale: bool = False,
                  trim: float = 1.0, max_distance: Optional[float] = None, init=None, max_iterations: int = 50,
                  tol: float = 1e-5, grid_resolution=None) -> Dict:
    """The similarity transform x -> s R x + t that moves `source` onto `target` by trimmed ICP.  source: a
    mesh dict, sampled once (sample_surface(source, n_samples, seed)), or an (N, 3) fp32 point tensor; target: a mesh dict or
    build_distance_grid's result (built once, queried in every iteration).  An iteration transforms the ORIGINAL samples
    by the current transform (hn_reg_transform; the float64 transform is rounded to fp32 once per iteration, nothing
    drifts), finds their nearest points on the target (ops.mesh.grid_query with max_distance), keeps the share `trim` (0 <
    trim <= 1) of them with the smallest distances (ops.registration.trim_threshold), sums what the solve needs on the
    device (hn_reg_moments: fused, float64, the same bits on every run), reads the 38 sums (the iteration's one host read)
    and solves in float64 NumPy: method 'point' the closed form of Umeyama / Horn, 'plane' one Gauss-Newton step of the
    point-to-plane error by minimum-norm least squares; with_scale also fits s.  The step (s', R', t') composes as
    s <- s' s, R <- R' R, t <- s' R' t + t'.  It stops when the UPDATE is small — the angle of R' <= tol rad, |t'| <= tol *
    (the diagonal of the target's box) and |s' - 1| <= tol — or after max_iterations.  init: None (identity), a (4, 4)
    similarity matrix, or 'centroid' (the samples' centroid onto that of n_samples surface samples of the target, seed + 1;
    with with_scale also the ratio of their rms radii).  ICP converges to the nearest local minimum: it needs an init within
    reach, a symmetric shape has several answers, and 'point' creeps along smooth surfaces where 'plane' slides.
    {'matrix': (4, 4) float64, 'scale', 'rotation' (3, 3), 'translation' (3,), 'rms': sqrt(sum d^2 / n) of the last inlier
    set, 'inliers', 'iterations', 'converged', 'history': [{'rms', 'inliers'}] per iteration}.  ValueError: an empty mesh or
    point set, arguments out of range, an init that is no similarity (det <= 0, a non-uniform scale), fewer than 3 inliers
    (6 for 'plane', 7 with scale) in an iteration."""
    what = "register_mesh"
    R = ops.registration
    if isinstance(source, torch.Tensor):
        samples, src_mesh = ops.checks.check_points(source, what, "source"), None
        if samples.shape[0] == 0:
            raise ValueError(f"{what}: the source holds no points")
    else:
        samples, src_mesh = None, _mesh_arrays(source, what)
        if src_mesh[1].shape[0] == 0 or src_mesh[0].shape[0] == 0:
            raise ValueError(f"{what}: the source mesh has no faces")
    if _is_grid(target):
        try:
            target_faces = int(target['num_faces'])
        except (KeyError, TypeError, ValueError):
            raise ValueError(f"{what}: target must be a mesh dict or what build_distance_grid returned") from None
        if target_faces == 0:
            raise ValueError(f"{what}: the target mesh has no faces")
    else:
        tv, tf = _mesh_arrays(target, what)
        if tf.shape[0] == 0 or tv.shape[0] == 0:
            raise ValueError(f"{what}: the target mesh has no faces")
    n_samples = _int_arg(n_samples, what, "n_samples", 1)
    if n_samples > ops.checks.INT32_MAX:
        raise ValueError(f"{what}: n_samples must be at most 2**31 - 1, got {n_samples}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"{what}: seed must be an int, got {seed!r}")
    if method not in R.REG_MODES:
        raise ValueError(f"{what}: method must be 'point' or 'plane', got {method!r}")
    with_scale = bool(with_scale)
    try:
        trim_f, tol_f = float(trim), float(tol)
    except (TypeError, ValueError):
        trim_f = tol_f = float("nan")
    if not 0.0 < trim_f <= 1.0:
        raise ValueError(f"{what}: trim must be a number in (0, 1], got {trim!r}")
    if not (tol_f > 0.0 and np.isfinite(tol_f)):
        raise ValueError(f"{what}: tol must be a positive finite number, got {tol!r}")
    ops.mesh.check_max_distance(max_distance, what)
    max_iterations = _int_arg(max_iterations, what, "max_iterations", 1)
    if grid_resolution is not None:
        ops.mesh.check_grid_resolution(grid_resolution, what)
    if init is None:
        current = (1.0, np.eye(3), np.zeros(3))
    elif isinstance(init, str):
        if init != 'centroid':
            raise ValueError(f"{what}: init must be None, 'centroid' or a (4, 4) similarity matrix, got {init!r}")
        current = None
    else:
        current = R.check_similarity(init, what)

    if samples is None:
        samples = sample_surface(source, n_samples, int(seed))['points']
    L.require_gpu(samples)
    grid = target if _is_grid(target) else build_distance_grid(target, grid_resolution)
    corners = _grid_corners(grid).double()
    ok = torch.isfinite(corners).all(dim=1, keepdim=True)
    box = torch.stack([torch.where(ok, corners, torch.full_like(corners, float("inf"))).amin(0),
                       torch.where(ok, corners, torch.full_like(corners, float("-inf"))).amax(0)])
    if current is None:
        # 'centroid': the moments of both samples about the origin in float64, one host read with the box
        tgt = sample_surface({'vertices': _grid_corners(grid).contiguous(),
                              'faces': torch.arange(3 * grid['num_faces'], dtype=torch.int32, device=samples.device).reshape(-1, 3)},
                             n_samples, int(seed) + 1)['points'].double()
        src = samples.double()
        src = src[torch.isfinite(src).all(dim=1)]
        if src.shape[0] == 0:
            raise ValueError(f"{what}: the source holds no finite point")
        stats = torch.stack([box[0], box[1], src.mean(0), tgt.mean(0), (src * src).sum(1).mean().expand(3),
                             (tgt * tgt).sum(1).mean().expand(3)]).cpu().numpy()
        c_src, c_tgt = stats[2], stats[3]
        r_src, r_tgt = (float(np.sqrt(max(m2 - float(c @ c), 0.0))) for m2, c in ((stats[4][0], c_src), (stats[5][0], c_tgt)))
        s0 = r_tgt / r_src if with_scale and r_src > 0.0 and r_tgt > 0.0 else 1.0
        current = (s0, np.eye(3), c_tgt - s0 * c_src)
    else:
        stats = box.cpu().numpy()
    diagonal = float(np.linalg.norm(stats[1] - stats[0]))

    need = R.REG_MIN_INLIERS[(method, with_scale)]
    history, converged, iterations = [], False, 0
    for iterations in range(1, max_iterations + 1):
        moved = R.transform_points(samples, *current)
        query = ops.mesh.grid_query(moved, grid, max_distance)
        tau = R.trim_threshold(query['distance'], trim_f)
        sums = R.registration_moments(moved, query, grid['tri'], tau, method).cpu().numpy()      # the iteration's host read
        inliers = int(sums[0])
        if inliers < need:
            raise ValueError(f"{what}: iteration {iterations} has {inliers} inliers, fewer than the {need} that method "
                             f"{method!r}{' with scale' if with_scale else ''} solves from (max_distance {max_distance!r}, "
                             f"trim {trim!r})")
        rms = float(np.sqrt(sums[1] / inliers))
        history.append({'rms': rms, 'inliers': inliers})
        step = (R.solve_point if method == 'point' else R.solve_plane)(sums, with_scale)
        if not (np.isfinite(step[0]) and step[0] > 0.0 and np.isfinite(step[1]).all() and np.isfinite(step[2]).all()):
            raise ValueError(f"{what}: iteration {iterations} has no finite solution (its {inliers} inliers are degenerate)")
        current = R.compose_similarity(step, current)
        if (R.rotation_angle(step[1]) <= tol_f and float(np.linalg.norm(step[2])) <= tol_f * diagonal
                and abs(step[0] - 1.0) <= tol_f):
            converged = True
            break
    s, rot, t = current
    return {'matrix': R.similarity_matrix(s, rot, t), 'scale': float(s), 'rotation': np.array(rot), 'translation': np.array(t),
            'rms': history[-1]['rms'], 'inliers': history[-1]['inliers'], 'iterations': iterations, 'converged': converged,
            'history': history}


@torch.no_grad()
def transform_mesh(mesh: Dict[str, torch.Tensor], matrix) -> Dict[str, torch.Tensor]:
    """`mesh` moved by the (4, 4) similarity `matrix` (register_mesh's 'matrix'): the vertices through hn_reg_transform, the
    'normals', where the mesh has some, through its direction form (rotated, unit length; a zero normal stays zero); the
    faces, colours and every other key are carried over as they are.  ValueError: a matrix that is no similarity (det <= 0
    would turn the faces inside out)."""
    what = "transform_mesh"
    vertices, _ = _mesh_arrays(mesh, what)
    s, rot, t = ops.registration.check_similarity(matrix, what)
    normals = mesh.get('normals')
    if normals is not None:
        normals = ops.checks.check_points(normals, what, "normals", rows=vertices.shape[0])
    out = dict(mesh)
    out['vertices'] = ops.registration.transform_points(vertices, s, rot, t)
    if normals is not None:
        out['normals'] = ops.registration.transform_points(normals, 1.0, rot, np.zeros(3), direction=True)
    return out


@torch.no_grad()
def aligned_mesh_distance(a: Dict[str, torch.Tensor], b: Dict[str, torch.Tensor], register: Optional[Dict] = None,
                          **mesh_distance_kwargs) -> Dict:
    """mesh_distance after registration: register_mesh(a, b, **register), transform_mesh(a, its matrix), mesh_distance(the
    moved a, b, **mesh_distance_kwargs).  The report of mesh_distance plus 'alignment': register_mesh's result."""
    what = "aligned_mesh_distance"
    _mesh_arrays(a, what)
    _mesh_arrays(b, what)
    if register is not None and not isinstance(register, dict):
        raise ValueError(f"{what}: register must be a dict of register_mesh's keyword arguments or None, got {register!r}")
    alignment = register_mesh(a, b, **(register or {}))
    report = mesh_distance(transform_mesh(a, alignment['matrix']), b, **mesh_distance_kwargs)
    report['alignment'] = alignment
    return report


@torch.no_grad()
def distance_colors(distance: torch.Tensor, vmax: float) -> torch.Tensor:
    """(N, 3) uint8 RGB of distances (N,): inference.jet_lut() (its blue-first rows turned to red-first) at index
    (int)(255 * min(d / vmax, 1)) — 0 is the table's first entry (dark blue), vmax and above its last (dark red), and so are NaN
    and inf.  For write_ply(path, v, f, colors=distance_colors(point_mesh_distance(v, other)['distance'], vmax)): where
    two meshes differ.  Plain torch indexing, on the device of `distance`."""
    from . import inference
    if not isinstance(distance, torch.Tensor) or distance.dim() != 1 or not distance.dtype.is_floating_point:
        raise ValueError("distance_colors: distance must be a (N,) floating point tensor")
    vmax = float(vmax)
    if not (np.isfinite(vmax) and vmax > 0.0):
        raise ValueError(f"distance_colors: vmax must be positive and finite, got {vmax}")
    x = distance.detach().float() / vmax
    x = torch.where(x <= 1.0, x.clamp(min=0.0), torch.ones_like(x))          # NaN, inf and above vmax -> 1
    index = (x * 255.0).to(torch.int64)
    return inference.jet_lut().flip(1).to(distance.device)[index]


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path, vertices, faces, normals=None, colors=None) -> None:
    """Binary little-endian PLY: vertices (V, 3) as float x y z (+ nx ny nz when `normals` (V, 3) is given, + uchar
    red green blue when `colors` (V, 3) uint8 is given), faces (F, 3) as `list uchar int vertex_indices`.  Tensors or
    arrays."""
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
    table = np.concatenate(cols, axis=1).astype("<f4")
    if colors is not None:
        if isinstance(colors, torch.Tensor):
            colors = colors.detach().cpu().numpy()
        colors = np.asarray(colors)
        if colors.dtype != np.uint8:
            raise ValueError(f"write_ply: colors must be uint8, got {colors.dtype}")
        colors = colors.reshape(-1, 3)
        if colors.shape != v.shape:
            raise ValueError(f"write_ply: {colors.shape[0]} colors for {v.shape[0]} vertices")
        header += [f"property uchar {n}" for n in ("red", "green", "blue")]
        vrec = np.empty(v.shape[0], dtype=[("f", "<f4", (table.shape[1],)), ("c", "u1", (3,))])     # packed: no padding
        vrec["f"] = table
        vrec["c"] = colors
        table = vrec
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(table.tobytes())
        fh.write(rec.tobytes())


def read_ply(path) -> Dict[str, Optional[np.ndarray]]:
    """What write_ply wrote: {'vertices': (V, 3) float32, 'normals': (V, 3) float32 | None, 'faces': (F, 3) int32,
    'colors': (V, 3) uint8 | None}."""
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
    vprops = props.get("vertex", [])
    has_colors = vprops[-3:] == [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    fprops = vprops[:-3] if has_colors else vprops
    names = [p[-1] for p in fprops]
    if any(p[0] != "float" for p in fprops) or names[:3] != ["x", "y", "z"] \
            or props.get("face") != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError(f"read_ply: {path} has a layout write_ply does not write")
    nv, nf, width = counts["vertex"], counts["face"], len(names)
    stride = 4 * width + (3 if has_colors else 0)
    vrec = np.frombuffer(blob, dtype=[("f", "<f4", (width,)), ("c", "u1", (3 if has_colors else 0,))], count=nv, offset=end)
    table = vrec["f"].reshape(nv, width)
    rec = np.frombuffer(blob, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nf, offset=end + stride * nv)
    if nf and not (rec["n"] == 3).all():
        raise ValueError(f"read_ply: {path} has faces that are not triangles")
    if len(blob) != end + stride * nv + 13 * nf:
        raise ValueError(f"read_ply: {path} has {len(blob)} bytes, its header describes {end + stride * nv + 13 * nf}")
    normals = table[:, 3:6].copy() if names[3:6] == ["nx", "ny", "nz"] else None
    return {"vertices": table[:, :3].copy(), "normals": normals, "faces": rec["idx"].astype(np.int32).reshape(nf, 3),
            "colors": vrec["c"].reshape(nv, 3).copy() if has_colors else None}


# ---- taking a mesh out with its appearance: a texture atlas baked from the field (csrc/hn_texture.hip) ---
def _check_atlas_mesh(mesh, what: str):
    """(vertices, faces, normals) of a mesh dict on one GPU, or ValueError."""
    vertices, faces, normals, _ = _check_render_mesh(mesh, what)
    if not vertices.is_cuda or not faces.is_cuda or (normals is not None and not normals.is_cuda):
        raise ValueError(f"{what}: the mesh must live on the GPU (there is no CPU fallback)")
    if faces.device != vertices.device or (normals is not None and normals.device != vertices.device):
        raise ValueError(f"{what}: the mesh's tensors must live on one device")
    return vertices, faces, normals


@torch.no_grad()
def texture_atlas(mesh: Dict[str, torch.Tensor], texel: float, min_cell: int = 16, max_cell: int = 256,
                  max_size: int = 8192) -> Dict:
    """A texture atlas of the mesh with one chart per face, texels of length `texel`: {'uv': (F, 3, 2) fp32,
    the corners of every face in absolute texel coordinates (texel (i, j) has its centre at (i + 0.5, j + 0.5)), 'size':
    (W_t, H_t), 'cell_start': (n_cells, 2) int32, 'cell_side': (n_cells,) int32, 'cell_face': (n_cells, 2) int32 (-1: an
    empty half), 'texel', and 'min_cell' / 'class_cells', the cells per side that rasterize_atlas finds a texel's cell
    with} on the mesh's device.
    A face gets the smallest power-of-two cell side s in [min_cell, max_cell] whose L = s - 7 texels cover its longest edge
    (max_cell when none does: such a face is sampled more coarsely than `texel`); two faces share a square cell as the
    two right triangles of legs L along its diagonal, a 1.5-texel gutter around each, so that a bilinear fetch inside a
    chart never reads another face's texels.  Cells are packed by descending side in Z-order, without holes; W_t =
    min_cell * 2^m, H_t = W_t or W_t / 2.  Deterministic: a sort of unique keys, no atomics.  One host read.
    ValueError: cell sides that are no powers of two in 16 .. 1024; texel not positive and finite; max_size above 16384; an
    atlas wider than max_size (the message names the size needed); a face with a vertex id outside [0, V)."""
    what = "texture_atlas"
    if not isinstance(mesh, dict):
        raise ValueError(f"{what}: mesh must be a dict with 'vertices' and 'faces'")
    min_cell, max_cell = ops.texture.check_cells_arg(min_cell, max_cell, what)
    texel = ops.texture.check_texel(texel, what)
    max_size = ops.texture.check_max_size(max_size, what)
    vertices, faces, _ = _check_atlas_mesh(mesh, what)
    dev, n_faces = vertices.device, faces.shape[0]
    if n_faces == 0:
        hist = [0] * 11
        empty = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)      # noqa: E731
        cell_start, cell_side, cell_face = empty(0, 2), empty(0), empty(0, 2)
        uv = torch.zeros((0, 3, 2), dtype=torch.float32, device=dev)
    else:
        _, keys, hist = ops.texture.face_classes(vertices, faces, texel, min_cell, max_cell, what)
    size = ops.texture.check_atlas_fits(hist, min_cell, max_size, what)
    if n_faces:
        cell_start, cell_side, cell_face, uv = ops.texture.atlas_layout(keys, hist, min_cell)
    return {'uv': uv, 'size': size, 'cell_start': cell_start, 'cell_side': cell_side, 'cell_face': cell_face,
            'texel': texel, 'min_cell': min_cell, 'class_cells': tuple(ops.texture.class_cells(hist)[1])}


@torch.no_grad()
def atlas_texel_for_size(mesh: Dict[str, torch.Tensor], size: int, min_cell: int = 16, max_cell: int = 256) -> float:
    """The finest texel length of the ladder texel_k = 2^(k/2) * (longest bounding-box side / size), k = 0, 1, 2, ..., whose
    texture_atlas fits size x size.  One face classification and one host read of 12 ints per step, at most 64 steps.
    ValueError: a mesh without faces or without extent; a mesh that does not fit even with every face in a min_cell chart."""
    what = "atlas_texel_for_size"
    if not isinstance(mesh, dict):
        raise ValueError(f"{what}: mesh must be a dict with 'vertices' and 'faces'")
    min_cell, max_cell = ops.texture.check_cells_arg(min_cell, max_cell, what)
    size = ops.texture.check_max_size(size, what, "size")
    vertices, faces, _ = _check_atlas_mesh(mesh, what)
    if faces.shape[0] == 0 or vertices.shape[0] == 0:
        raise ValueError(f"{what}: the mesh has no faces")
    lo, hi = (np.asarray(t, dtype=np.float64) for t in ops.simplify.vertex_extent(vertices))
    longest = float((hi - lo).max()) if np.isfinite(lo).all() and np.isfinite(hi).all() else 0.0
    if not longest > 0.0:
        raise ValueError(f"{what}: the vertices have no finite extent")
    need = None
    for k in range(64):
        texel = ops.texture.check_texel(2.0 ** (0.5 * k) * longest / size, what)
        hist = ops.texture.face_classes(vertices, faces, texel, min_cell, max_cell, what)[2]
        need = ops.texture.atlas_size(hist, min_cell)
        if max(need) <= size:
            return texel
        if hist[min_cell.bit_length() - 1] == faces.shape[0]:
            break
    raise ValueError(f"{what}: the mesh needs {need[0]} x {need[1]} texels even with every face in a {min_cell}-texel cell; "
                     f"size is {size}")


@torch.no_grad()
def rasterize_atlas(mesh: Dict[str, torch.Tensor], atlas: Dict) -> Dict[str, torch.Tensor]:
    """The atlas texels in 3-D: {'owner': (H_t, W_t) int32, the face whose chart owns the texel or -1, 'position': (H_t, W_t,
    3) fp32, the point of the face's plane under the texel centre — extrapolated outside the triangle, so that bilinear
    sampling reproduces an affine function exactly up to the face's edges —, 'normal': (H_t, W_t, 3) fp32, the unit
    interpolated vertex normal there (the face normal without 'normals' or where the interpolation vanishes)}; zeros at
    unowned texels (hn_tex_rasterize)."""
    what = "rasterize_atlas"
    vertices, faces, normals = _check_atlas_mesh(mesh, what)
    ops.texture.check_atlas(atlas, faces.shape[0], what)
    return ops.texture.atlas_rasterize(vertices, faces, normals, atlas)


@torch.no_grad()
def bake_texture(mesh: Dict[str, torch.Tensor], atlas: Dict, color_fn, dtype=torch.uint8, fill=0) -> torch.Tensor:
    """The (H_t, W_t, 3) texture of the atlas whose owned texels hold color_fn(points (n, 3), normals (n, 3)) -> (n, 3) fp32
    in [0, 1], called ONCE on the owned texels of rasterize_atlas in row-major order; unowned texels hold `fill`.
    dtype float32: the colours as they are; uint8: (rgb * 255) truncated, the convention of vertex_colors."""
    what = "bake_texture"
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: dtype must be torch.uint8 or torch.float32, got {dtype}")
    try:
        given, fill = float(fill), (float(fill) if dtype == torch.float32 else int(fill))
        ok = bool(np.isfinite(given)) if dtype == torch.float32 else (0 <= fill <= 255 and fill == given)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: fill must be one {'finite number' if dtype == torch.float32 else 'integer in 0 .. 255'}")
    if not callable(color_fn):
        raise ValueError(f"{what}: color_fn must be callable")
    rast = rasterize_atlas(mesh, atlas)
    (w, h), dev = atlas['size'], rast['owner'].device
    index = torch.nonzero(rast['owner'].view(-1) >= 0).view(-1)
    n = index.shape[0]
    texture = torch.full((h, w, 3), fill, dtype=dtype, device=dev)
    colors = color_fn(rast['position'].view(-1, 3)[index], rast['normal'].view(-1, 3)[index])
    if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (n, 3) or colors.dtype != torch.float32 \
            or colors.device != dev:
        raise ValueError(f"{what}: color_fn must return a ({n}, 3) float32 tensor on {dev}")
    texture.view(-1, 3)[index] = colors if dtype == torch.float32 else (colors * 255).to(torch.uint8)
    return texture


@torch.no_grad()
def bake_field_texture(model, mesh: Dict[str, torch.Tensor], atlas: Dict, frame_id: int,
                       view: Union[str, Sequence[float], torch.Tensor] = 'normal', level: str = 'fine', chunk: int = 1 << 20,
                       render_opts=None, dtype=torch.uint8) -> torch.Tensor:
    """bake_texture with the field's colour at frame `frame_id`: vertex_colors(model, points, normals, frame_id, view=...) at
    every owned texel's point, seen along -normal or from the camera position `view`.  The mesh lives on the model's
    device.  The values do not depend on `chunk`; no state is left on the model."""
    if int(chunk) < 1:
        raise ValueError(f"bake_field_texture: chunk must be positive, got {chunk}")

    def color_fn(points, normals):
        return vertex_colors(model, points, normals, frame_id, view=view, level=level, chunk=chunk, render_opts=render_opts,
                             dtype=torch.float32)
    return bake_texture(mesh, atlas, color_fn, dtype=dtype)


@torch.no_grad()
def render_textured_mesh(mesh: Dict[str, torch.Tensor], atlas: Dict, texture: torch.Tensor, rays: torch.Tensor, camera,
                         image_wh, shading: str = 'headlight', ambient: float = 0.3, background=(1.0, 1.0, 1.0),
                         filter: str = 'bilinear', binning: bool = True) -> Dict[str, torch.Tensor]:
    """render_mesh with the colour from a texture: the same keys and shapes, the same face / depth / bary / normal images
    (ops.mesh_render.mesh_trace), and rgb / rgb8 from `texture` (H_t, W_t, 3) uint8 or fp32 fetched at the hit point's atlas
    coordinates (hn_tex_shade), filter 'bilinear' or 'nearest'; the mesh's 'colors' are not looked at.  No mip levels: a
    minified texture aliases.  One chart per face: magnified bilinear filtering does not blend across face edges."""
    what = "render_textured_mesh"
    vertices, faces, normals, _ = _check_render_mesh(mesh, what)
    w, h = ops.mesh_render.check_image_wh(image_wh, what)
    camera = ops.checks.check_camera(camera, what)
    rays = ops.checks.check_rays(rays, h * w, what)
    ops.mesh_render.check_shading(shading, ambient, background, (0.0, 0.0, 0.0), what)
    ops.texture.check_atlas(atlas, faces.shape[0], what)
    texture = ops.texture.check_texture(texture, atlas, what)
    if filter not in ops.texture.TEX_FILTERS:
        raise ValueError(f"{what}: filter must be one of {tuple(ops.texture.TEX_FILTERS)}, got {filter!r}")
    if not vertices.is_cuda or not faces.is_cuda or not rays.is_cuda or not texture.is_cuda:
        raise ValueError(f"{what}: the mesh, the texture and the rays must live on the GPU (there is no CPU fallback)")
    out = ops.mesh_render.mesh_trace(vertices, faces, rays, camera, (w, h), binning=bool(binning))
    out.update(ops.texture.texture_shade(vertices, faces, normals, atlas, texture, rays, out['face'], out['bary'], shading,
                                         ambient, background, filter))
    return {k: t.view((h, w) + tuple(t.shape[1:])) for k, t in out.items()}


def write_obj(path, mesh: Dict, atlas: Dict, texture) -> None:
    """A textured Wavefront OBJ: `name.obj` (path), `name.mtl` and `name.png` beside it.  The .obj holds `mtllib`, `v` per
    vertex, `vn` per vertex when the mesh has 'normals', three `vt` per face — u = x / W_t, v = 1 - y / H_t of atlas['uv'],
    exact in the decimal digits written — `usemtl` and `f a/ta/na b/tb/nb c/tc/nc` (`a/ta` without normals), 1-based; the
    .mtl one material with `map_Kd name.png`; the .png the texture (H_t, W_t, 3) uint8 through inference.write_png, row 0
    on top.  Tensors or arrays, host or device.  ValueError: a path that does not end in .obj, a texture that is not
    uint8 or not of the atlas's size, a uv table that is not (F, 3, 2)."""
    import os
    from . import inference
    what = "write_obj"
    path = os.fspath(path)
    if not path.lower().endswith(".obj"):
        raise ValueError(f"{what}: path must end in .obj, got {path!r}")
    if not isinstance(mesh, dict) or not isinstance(atlas, dict) or 'uv' not in atlas or 'size' not in atlas:
        raise ValueError(f"{what}: mesh must be a mesh dict and atlas the dict texture_atlas returns")
    tex = texture.detach().cpu().numpy() if isinstance(texture, torch.Tensor) else np.asarray(texture)
    if tex.dtype != np.uint8:
        raise ValueError(f"{what}: texture must be uint8 (bake with dtype=torch.uint8), got {tex.dtype}")
    w, h = (int(x) for x in atlas['size'])
    if tex.shape != (h, w, 3):
        raise ValueError(f"{what}: texture is {tuple(tex.shape)}, the atlas is ({h}, {w}, 3)")
    v = _host(mesh['vertices'], np.float32).reshape(-1, 3)
    f = _host(mesh['faces'], np.int32).reshape(-1, 3)
    uv = _host(atlas['uv'], np.float32)
    if uv.shape != (f.shape[0], 3, 2):
        raise ValueError(f"{what}: the atlas lays out {uv.shape[0]} faces, the mesh has {f.shape[0]}")
    nrm = mesh.get('normals')
    if nrm is not None:
        nrm = _host(nrm, np.float32).reshape(-1, 3)
        if nrm.shape != v.shape:
            raise ValueError(f"{what}: {nrm.shape[0]} normals for {v.shape[0]} vertices")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"{what}: faces hold a vertex id outside [0, {v.shape[0]})")
    base = path[:-4]
    name = os.path.basename(base)
    # float32 survives nine significant digits; u and v are dyadic in float64 when the sides are powers of two
    lines = [f"mtllib {name}.mtl"]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    if nrm is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(r) for r in nrm.tolist()]
    u64 = uv.reshape(-1, 2).astype(np.float64)
    lines += ["vt %.17g %.17g" % (x / w, 1.0 - y / h) for x, y in u64.tolist()]
    lines.append(f"usemtl {name}")
    corner = "%d/%d/%d" if nrm is not None else "%d/%d"
    for k, (a, b, c) in enumerate(f.tolist()):
        ids = ((a + 1, 3 * k + 1, a + 1), (b + 1, 3 * k + 2, b + 1), (c + 1, 3 * k + 3, c + 1))
        lines.append("f " + " ".join(corner % (t if nrm is not None else t[:2]) for t in ids))
    with open(path, "w", encoding="ascii") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(base + ".mtl", "w", encoding="ascii") as fh:
        fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    inference.write_png(base + ".png", tex)


def read_obj(path) -> Dict:
    """What write_obj wrote: {'vertices': (V, 3) float32, 'normals': (V, 3) float32 | None, 'faces': (F, 3) int32, 'vt':
    (F, 3, 2) float64 as written, 'uv': (F, 3, 2) float32, vt mapped back to texel coordinates (u W_t, (1 - v) H_t),
    'texture': (H_t, W_t, 3) uint8, 'size': (W_t, H_t), 'mtl': the .mtl's file name, 'map_Kd': the image's file name}.  Standard
    library and NumPy only."""
    import os
    from . import inference
    what = "read_obj"
    path = os.fspath(path)
    v, vn, vt, faces, mtl, used = [], [], [], [], None, None
    with open(path, "r", encoding="ascii") as fh:
        for line in fh:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:4]])
            elif w[0] == "vn":
                vn.append([float(x) for x in w[1:4]])
            elif w[0] == "vt":
                vt.append([float(x) for x in w[1:3]])
            elif w[0] == "f":
                faces.append([[int(x) for x in c.split("/")] for c in w[1:]])
            elif w[0] == "mtllib":
                mtl = w[1]
            elif w[0] == "usemtl":
                used = w[1]
    n_f = len(faces)
    corners = np.asarray(faces, dtype=np.int64).reshape(n_f, 3, -1) if n_f else np.zeros((0, 3, 3 if vn else 2), dtype=np.int64)
    if mtl is None or used is None or len(vt) != 3 * n_f or corners.shape[2] != (3 if vn else 2) \
            or not (corners[:, :, 1].reshape(-1) == np.arange(1, 3 * n_f + 1)).all() \
            or (vn and (len(vn) != len(v) or not (corners[:, :, 2] == corners[:, :, 0]).all())):
        raise ValueError(f"{what}: {path} has a layout write_obj does not write")
    image = None
    with open(os.path.join(os.path.dirname(path), mtl), "r", encoding="ascii") as fh:
        for line in fh:
            w = line.split()
            if w[:1] == ["map_Kd"]:
                image = w[1]
    if image is None:
        raise ValueError(f"{what}: {mtl} names no map_Kd image")
    texture = inference.read_png(os.path.join(os.path.dirname(path), image))
    h_t, w_t = texture.shape[:2]
    vt = np.asarray(vt, dtype=np.float64).reshape(n_f, 3, 2)
    uv = np.stack([vt[..., 0] * w_t, (1.0 - vt[..., 1]) * h_t], axis=-1).astype(np.float32)
    return {"vertices": np.asarray(v, dtype=np.float32).reshape(-1, 3),
            "normals": np.asarray(vn, dtype=np.float32).reshape(-1, 3) if vn else None,
            "faces": (corners[:, :, 0] - 1).astype(np.int32), "vt": vt, "uv": uv, "texture": texture, "size": (w_t, h_t),
            "mtl": mtl, "map_Kd": image}
