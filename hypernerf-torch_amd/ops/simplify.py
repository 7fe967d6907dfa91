"""Mesh simplification by vertex clustering (csrc/hn_simplify.hip)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from .. import _lib as L
from .checks import INT32_MAX, check_faces, check_points, float3

__all__ = ["CELL_BITS", "EXTENT_TILE", "check_cells", "vertex_extent", "cluster_vertices", "reduce_clusters",
           "cluster_faces", "relabel_vertices"]

CELL_BITS = L.HN_SIMPLIFY_BITS    # bits per axis of a cell key: fewer than 2**21 cells along every axis


def check_cells(cell, origin, what: str):
    """(cell, origin) as two (c_float * 3) host arrays, or ValueError: every cell side positive and finite (also once
    rounded to float32), every origin finite."""
    import math
    cell = (C.c_float * 3)(*float3(cell, f"{what}: cell"))
    origin = (C.c_float * 3)(*float3(origin, f"{what}: origin"))
    if not all(math.isfinite(c) and c > 0.0 for c in cell):
        raise ValueError(f"{what}: every cell side must be positive and finite, got {list(cell)}")
    if not all(math.isfinite(o) for o in origin):
        raise ValueError(f"{what}: origin must be finite, got {list(origin)}")
    return cell, origin


EXTENT_TILE = L.HN_EXTENT_TILE    # vertices per workgroup of hn_simplify_extent


@torch.no_grad()
def vertex_extent(vertices: torch.Tensor):
    """(lo, hi): two lists of three host floats, the per-axis minimum and maximum of vertices (V >= 1, 3) fp32
    (hn_simplify_extent: one partial per 2048 vertices, the partials reduced by torch; NaN where a coordinate is NaN).
    One host read.  A CPU tensor is read with torch: simplify_mesh checks its arguments in full before it refuses a mesh
    that does not live on the GPU."""
    vertices = check_points(vertices, "vertex_extent", "vertices")
    v = vertices.shape[0]
    if v == 0:
        raise ValueError("vertex_extent: no vertices")
    if not vertices.is_cuda:
        return tuple(t.tolist() for t in torch.aminmax(vertices, dim=0))
    L.load()
    blocks = (v + EXTENT_TILE - 1) // EXTENT_TILE
    partial = torch.empty((blocks, 2, 3), dtype=torch.float32, device=vertices.device)
    with torch.cuda.device(vertices.device):
        L.launch("hn_simplify_extent", L.ptr(vertices), v, L.ptr(partial), blocks, L.stream_handle())
    lo, hi = torch.stack([partial[:, 0].amin(dim=0), partial[:, 1].amax(dim=0)]).tolist()
    return lo, hi


@torch.no_grad()
def cluster_vertices(vertices: torch.Tensor, cell, origin) -> Dict[str, torch.Tensor]:
    """The clusters of `vertices` (V, 3) fp32 on the lattice of cells `cell` (a float or three) from `origin` (three
    floats): {'keys': (V,) int64 = ix | iy << 21 | iz << 42 with idx_c = floorf((v_c - origin_c) / cell_c) in fp32
    (hn_simplify_keys), 'cluster_keys': (C,) int64, the distinct keys ascending, 'vertex_cluster': (V,) int32, 'order':
    (V,) int32, the vertex ids by (key, id) — the members of cluster c are order[starts[c] : starts[c + 1]], 'starts':
    (C + 1,) int32}.  The sort and the run lengths are torch's (a stable sort of integers).  The caller has checked the
    extent (0 <= idx < 2**21; simplify_mesh does); an index outside is clamped.  One host read: the cluster count."""
    vertices = check_points(vertices, "cluster_vertices", "vertices")
    cell, origin = check_cells(cell, origin, "cluster_vertices")
    L.require_gpu(vertices)
    v, dev = vertices.shape[0], vertices.device
    if v > INT32_MAX:
        raise ValueError(f"cluster_vertices: {v} vertices exceed 2**31 - 1 = {INT32_MAX}")
    keys = torch.empty(v, dtype=torch.int64, device=dev)
    if v == 0:
        return {'keys': keys, 'cluster_keys': keys, 'vertex_cluster': torch.empty(0, dtype=torch.int32, device=dev),
                'order': torch.empty(0, dtype=torch.int32, device=dev), 'starts': torch.zeros(1, dtype=torch.int32, device=dev)}
    L.load()
    with torch.cuda.device(dev):
        L.launch("hn_simplify_keys", L.ptr(vertices), v, origin, cell, L.ptr(keys), L.stream_handle())
    sorted_keys, order = torch.sort(keys, stable=True)
    cluster_keys, inverse, counts = torch.unique_consecutive(sorted_keys, return_inverse=True, return_counts=True)
    vertex_cluster = torch.empty(v, dtype=torch.int32, device=dev)
    vertex_cluster[order] = inverse.to(torch.int32)
    starts = torch.zeros(cluster_keys.shape[0] + 1, dtype=torch.int32, device=dev)
    starts[1:] = torch.cumsum(counts, 0)
    return {'keys': keys, 'cluster_keys': cluster_keys, 'vertex_cluster': vertex_cluster, 'order': order.to(torch.int32),
            'starts': starts}


@torch.no_grad()
def reduce_clusters(vertices: torch.Tensor, normals: Optional[torch.Tensor], colors: Optional[torch.Tensor],
                    clusters: Dict[str, torch.Tensor], cell, origin, placement: str = 'quadric',
                    regularization: float = 0.1) -> Dict[str, torch.Tensor]:
    """The representative of EVERY cluster of cluster_vertices, before any is dropped (hn_simplify_reduce, one work-item
    per cluster walking its members in ascending vertex id): {'vertices': (C, 3) fp32, 'normals': (C, 3) fp32 when
    given, 'colors': (C, 3) uint8 or fp32 when given}.  placement 'mean': the sequential fp32 mean; 'quadric': the mean
    plus the step that minimises sum (n_i . (x - p_i))^2 + regularization * k * |x - mean|^2, clamped into the cell
    (needs normals).  Every operation fp32 and rounded on its own, in the order tests/simplify_restated.py states."""
    if placement not in ('quadric', 'mean'):
        raise ValueError(f"reduce_clusters: placement must be 'quadric' or 'mean', got {placement!r}")
    import math
    regularization = float(regularization)
    if not (math.isfinite(regularization) and regularization >= 0.0):
        raise ValueError(f"reduce_clusters: regularization must be finite and not negative, got {regularization}")
    vertices = check_points(vertices, "reduce_clusters", "vertices")
    v, dev = vertices.shape[0], vertices.device
    if normals is not None:
        normals = check_points(normals, "reduce_clusters", "normals", v)
    elif placement == 'quadric':
        raise ValueError("reduce_clusters: placement='quadric' needs normals")
    kind = 0
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or colors.shape != (v, 3) or colors.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"reduce_clusters: colors must be a ({v}, 3) uint8 or float32 tensor")
        colors = colors.detach().contiguous()
        kind = 1 if colors.dtype == torch.uint8 else 2
    cell, origin = check_cells(cell, origin, "reduce_clusters")
    L.require_gpu(vertices, normals, colors)
    order, starts, cluster_keys = (clusters[k].contiguous() for k in ('order', 'starts', 'cluster_keys'))
    n_clusters = cluster_keys.shape[0]
    if order.dtype != torch.int32 or starts.dtype != torch.int32 or cluster_keys.dtype != torch.int64 \
            or order.shape != (v,) or starts.shape != (n_clusters + 1,) or n_clusters > v:
        raise ValueError("reduce_clusters: clusters must be what cluster_vertices returned for these vertices")
    out = {'vertices': torch.empty((n_clusters, 3), dtype=torch.float32, device=dev)}
    if normals is not None:
        out['normals'] = torch.empty((n_clusters, 3), dtype=torch.float32, device=dev)
    if colors is not None:
        out['colors'] = torch.empty((n_clusters, 3), dtype=colors.dtype, device=dev)
    if n_clusters:
        L.load()
        with torch.cuda.device(dev):
            L.launch("hn_simplify_reduce", L.ptr(vertices), L.ptr(normals), L.ptr(colors), kind, L.ptr(order), L.ptr(starts),
                     L.ptr(cluster_keys), n_clusters, v, origin, cell, regularization, 1 if placement == 'quadric' else 0,
                     L.ptr(out['vertices']), L.ptr(out.get('normals')), L.ptr(out.get('colors')), L.stream_handle())
    return out


@torch.no_grad()
def cluster_faces(faces: torch.Tensor, vertex_cluster: torch.Tensor, num_clusters: int, return_used: bool = False):
    """(F', 3) int32 faces over CLUSTER ids: every face of `faces` (F, 3) int32 goes through vertex_cluster (V,) int32; a
    face with two equal ids is dropped; per set {a < b < c}, net = #(a, b, c) - #(a, c, b) among the rest, and |net| copies
    leave, wound (a, b, c) when net > 0 and (a, c, b) when net < 0, in ascending order of (a, b, c) — opposite pairs, the
    folded flaps of a collapse, cancel (hn_simplify_face_keys, two stable torch sorts, hn_simplify_face_net,
    hn_simplify_face_emit).  `return_used`: also (C,) int32, 1 for every cluster an emitted face uses.  One host read: F'."""
    faces, v = check_faces(faces, vertex_cluster.shape[0], "cluster_faces")
    if vertex_cluster.dtype != torch.int32 or vertex_cluster.dim() != 1:
        raise ValueError("cluster_faces: vertex_cluster must be a (V,) int32 tensor")
    L.require_gpu(vertex_cluster)
    n_clusters = int(num_clusters)
    if not 0 <= n_clusters <= v:
        raise ValueError(f"cluster_faces: {n_clusters} clusters for {v} vertices")
    dev, n_faces = faces.device, faces.shape[0]
    used = torch.zeros(n_clusters, dtype=torch.int32, device=dev)
    out = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    if n_faces and n_clusters:
        L.load()
        with torch.cuda.device(dev):
            stream = L.stream_handle()
            key_ab = torch.empty(n_faces, dtype=torch.int64, device=dev)
            key_c = torch.empty(n_faces, dtype=torch.int32, device=dev)
            sign = torch.empty(n_faces, dtype=torch.int32, device=dev)
            L.launch("hn_simplify_face_keys", L.ptr(faces), n_faces, L.ptr(vertex_cluster.contiguous()), v, L.ptr(key_ab),
                     L.ptr(key_c), L.ptr(sign), stream)
            # lexicographic order of (a, b, c): stable by c, then stable by a << 31 | b
            by_c = torch.sort(key_c, stable=True).indices
            sorted_ab, by_ab = torch.sort(key_ab[by_c], stable=True)
            perm = by_c[by_ab].contiguous()
            net = torch.empty(n_faces, dtype=torch.int32, device=dev)
            L.launch("hn_simplify_face_net", L.ptr(sorted_ab), L.ptr(key_c), L.ptr(sign), L.ptr(perm), n_faces, L.ptr(net),
                     stream)
            ends = torch.cumsum(net.abs(), 0, dtype=torch.int64)
            n_out = int(ends[-1])
            if n_out:
                out = torch.empty((n_out, 3), dtype=torch.int32, device=dev)
                L.launch("hn_simplify_face_emit", L.ptr(sorted_ab), L.ptr(key_c), L.ptr(perm), L.ptr(net), L.ptr(ends),
                         n_faces, n_clusters, n_out, L.ptr(out), L.ptr(used), stream)
    return (out, used) if return_used else out


@torch.no_grad()
def relabel_vertices(vertex_cluster: torch.Tensor, used: torch.Tensor, scan: torch.Tensor) -> torch.Tensor:
    """(V,) int32: scan[cluster] - 1 for a vertex whose cluster is used, -1 otherwise (hn_simplify_relabel); scan = the
    inclusive int32 scan of `used` (C,) int32."""
    L.require_gpu(vertex_cluster, used, scan)
    v, n_clusters = vertex_cluster.shape[0], used.shape[0]
    out = torch.empty(v, dtype=torch.int32, device=vertex_cluster.device)
    if v:
        L.load()
        with torch.cuda.device(vertex_cluster.device):
            L.launch("hn_simplify_relabel", L.ptr(vertex_cluster.contiguous()), v, L.ptr(used.contiguous()),
                     L.ptr(scan.contiguous()), n_clusters, L.ptr(out), L.stream_handle())
    return out
