"""NumPy statement of the mesh post-processing of hypernerf_torch_amd.geometry: connected components of an indexed
triangle mesh, their sizes, filtering by component, and the view directions of vertex colours.  It states the
definitions, not the kernels: union-find for the labels, the filtering rules written out plainly, float32 operations
rounded one by one for the directions.

    label[v]   = the smallest vertex id of v's component (two vertices are connected when a face holds both; a vertex no
                 face references is its own component)
    size[l]    = number of faces whose vertices carry label l (index = label, zero elsewhere)
    kept       = components with size >= max(min_faces, 1) that, when keep_largest = k is given, are among the first k in
                 the order (size descending, label ascending); vertices and faces of kept components in their old order,
                 faces re-indexed, vertex_index = the old ids of the kept vertices
    direction  = u / |u|, u = -normal or vertex - camera, |u| = sqrt((ux*ux + uy*uy) + uz*uz); (0, 0, 1) when |u| is 0
"""
import numpy as np

F32 = np.float32


def mesh_components(faces, num_vertices):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= num_vertices):
        raise ValueError("vertex id out of range")
    parent = list(range(num_vertices))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b, c in faces.tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)         # the root of a set is always its smallest member
    return np.array([find(v) for v in range(num_vertices)], dtype=np.int32).reshape(num_vertices)


def component_sizes(labels, faces):
    labels = np.asarray(labels)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    sizes = np.zeros(labels.shape[0], dtype=np.int32)
    for a in faces[:, 0].tolist():
        sizes[labels[a]] += 1
    return sizes


def kept_components(labels, sizes, min_faces=None, keep_largest=None):
    """Sorted list of the labels that stay."""
    comps = sorted(set(np.asarray(labels).tolist()))
    kept = [l for l in comps if sizes[l] >= max(int(min_faces or 0), 1)]
    if keep_largest is not None:
        ranked = sorted(comps, key=lambda l: (-int(sizes[l]), l))[:max(int(keep_largest), 0)]
        kept = [l for l in kept if l in set(ranked)]
    return kept


def filter_mesh(mesh, min_faces=None, keep_largest=None):
    """mesh: dict of arrays ('vertices' (V,3), 'faces' (F,3), any further per-vertex arrays)."""
    if min_faces is None and keep_largest is None:
        return mesh
    v = mesh["vertices"].shape[0]
    faces = np.asarray(mesh["faces"]).reshape(-1, 3)
    labels = mesh_components(faces, v)
    sizes = component_sizes(labels, faces)
    kept = np.zeros(v, dtype=bool)
    kept[kept_components(labels, sizes, min_faces, keep_largest)] = True
    vkeep = kept[labels] if v else np.zeros(0, dtype=bool)
    vertex_index = np.flatnonzero(vkeep).astype(np.int32)
    new_id = np.cumsum(vkeep) - 1
    fkeep = vkeep[faces[:, 0]] if faces.shape[0] else np.zeros(0, dtype=bool)
    out = {k: (a[vertex_index] if k not in ("faces", "vertex_index") and isinstance(a, np.ndarray) and a.ndim >= 1 and a.shape[0] == v else a)
           for k, a in mesh.items()}
    out["faces"] = new_id[faces[fkeep]].astype(np.int32).reshape(-1, 3)
    out["vertex_index"] = vertex_index
    return out


def vertex_viewdirs(vertices, normals, start, count, camera=None):
    """(count, 3) float32; rows past the mesh repeat its last vertex."""
    ref = np.asarray(vertices if camera is not None else normals, dtype=F32)
    idx = np.minimum(np.arange(start, start + count), ref.shape[0] - 1)
    with np.errstate(all="ignore"):
        u = (ref[idx] - np.asarray(camera, dtype=F32)[None, :]).astype(F32) if camera is not None else (-ref[idx]).astype(F32)
        sq = (u * u).astype(F32)
        length = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)).astype(F32)
        ok = length > 0
        d = (u / np.where(ok, length, F32(1))[:, None]).astype(F32)
    return np.where(ok[:, None], d, np.array([0.0, 0.0, 1.0], dtype=F32)[None, :]).astype(F32)


# ------------------------------------------------------------------------------------------------
# fixtures shared by the host and the GPU tests
# ------------------------------------------------------------------------------------------------
def strip(t, order="ascending", seed=0, offset=0, stride=1):
    """A triangle strip of t triangles over t + 2 positions; position i carries the vertex id order[i]."""
    n = t + 2
    if order == "ascending":
        ids = np.arange(n)
    elif order == "descending":
        ids = np.arange(n)[::-1]
    else:
        ids = np.random.default_rng(seed).permutation(n)
    ids = offset + stride * ids
    i = np.arange(t)
    return np.stack([ids[i], ids[i + 1], ids[i + 2]], axis=1).astype(np.int32)


def blobs(n=33):
    """27 separated spheres on an n^3 lattice over [-1, 1]^3, centres on a 3 x 3 x 3 arrangement, three radii (nine
    blobs each): f > 0 inside.  Equal radii give components with equal face counts only up to the lattice phase, so the
    centres sit ON lattice points: blobs of one radius are then translates of one another by whole cells."""
    x = np.linspace(-1.0, 1.0, n)
    g = np.stack(np.meshgrid(x, x, x, indexing="ij"), axis=-1)
    step = 2.0 / (n - 1)
    f = np.full((n, n, n), -1.0)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                centre = -1.0 + step * np.array([5 + 11 * a, 5 + 11 * b, 5 + 11 * c])
                radius = (0.11, 0.17, 0.23)[(a + b + c) % 3]
                f = np.maximum(f, radius - np.linalg.norm(g - centre, axis=-1))
    return f.astype(np.float32)
