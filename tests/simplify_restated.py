"""NumPy float32 restatement of mesh simplification by vertex clustering (csrc/hn_simplify.hip, geometry.simplify_mesh).

It follows the definition, operation by operation, not the kernels: every float operation is one float32 operation
rounded on its own, every sum runs over the members of a cluster in ascending vertex id and starts at +0, so the GPU's
arrays are expected to be the same bits.

    cells     idx_c = floor((v_c - origin_c) / cell_c); key = ix | iy << 21 | iz << 42; clusters = the distinct keys,
              ascending; members of a cluster in ascending vertex id
    cluster   mean = sum(p) / k
              quadric: r = p - mean; A = sum(n n^T) + (regularization * k) I; b = sum(n * ((nx*rx + ny*ry) + nz*rz));
                       adjugate rows (c00 c01 c02) (c01 c11 c12) (c02 c12 c22) of the symmetric A, each a*b - c*d:
                         c00 = ayy*azz - ayz*ayz   c01 = axz*ayz - axy*azz   c02 = axy*ayz - axz*ayy
                         c11 = axx*azz - axz*axz   c12 = axy*axz - axx*ayz   c22 = axx*ayy - axy*axy
                       det = (axx*c00 + axy*c01) + axz*c02;  d_r = ((row_r[0]*bx + row_r[1]*by) + row_r[2]*bz) / det,
                       d = 0 unless det is finite and positive;  x = mean + d, then x < lo -> lo, x > hi -> hi with
                       lo = origin + idx * cell, hi = lo + cell
              normal = s / |s|, s = sum(n), |s| = sqrt((sx*sx + sy*sy) + sz*sz); the zero vector unless |s| > 0
              colours: uint8 (2 * sum + k) // (2 k); float32 sum / k
    faces     through the cluster ids; two equal ids drop the face; rotate the smallest id to the front, (a, x, y); the
              triple is (a, min(x, y), max(x, y)), its sign +1 when x < y else -1; net = sum of the signs per triple;
              |net| copies of (a, b, c) (net > 0) or (a, c, b) (net < 0), triples in ascending lexicographic order
    compact   clusters no emitted face uses are dropped, the others keep their order; faces re-indexed
"""
import numpy as np

F32 = np.float32
BITS = 21


def vec3(x, dtype=F32):
    a = np.asarray(x, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    assert a.size == 3, x
    return a.astype(dtype)


def cell_indices(vertices, cell, origin):
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    cell, origin = vec3(cell), vec3(origin)
    return np.floor(((v - origin[None, :]).astype(F32) / cell[None, :]).astype(F32)).astype(np.int64)


def cluster_keys(vertices, cell, origin):
    """(V,) int64 keys.  The extent must have been checked: 0 <= idx < 2^21."""
    idx = cell_indices(vertices, cell, origin)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < 1 << BITS), (idx.min(), idx.max())
    return idx[:, 0] | idx[:, 1] << BITS | idx[:, 2] << (2 * BITS)


def cluster_vertices(vertices, cell, origin):
    """{'keys' (V,) int64, 'cluster_keys' (C,) int64 ascending, 'vertex_cluster' (V,) int32, 'order' (V,) int32: vertex ids
    by (key, id), 'starts' (C + 1,) int32}."""
    keys = cluster_keys(vertices, cell, origin)
    ckeys, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    starts = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(counts)])
    return {"keys": keys, "cluster_keys": ckeys, "vertex_cluster": inverse.reshape(-1).astype(np.int32),
            "order": np.argsort(keys, kind="stable").astype(np.int32), "starts": starts.astype(np.int32)}


def _sequential_sums(values, order, starts, dtype):
    """(C, n): per cluster the sum of the rows values[member] in member order, from +0, every addition rounded."""
    counts = np.diff(starts.astype(np.int64))
    acc = np.zeros((counts.size, values.shape[1]), dtype=dtype)
    for j in range(int(counts.max()) if counts.size else 0):
        live = np.flatnonzero(counts > j)
        acc[live] = (acc[live] + values[order[starts[live].astype(np.int64) + j]]).astype(dtype)
    return acc


def _dot3(a, b, dtype):
    p = (a * b).astype(dtype)
    return ((p[..., 0] + p[..., 1]).astype(dtype) + p[..., 2]).astype(dtype)


def _dop(a, b, c, d, dtype):
    return ((a * b).astype(dtype) - (c * d).astype(dtype)).astype(dtype)


def reduce_clusters(vertices, normals, colors, clusters, cell, origin, placement="quadric", regularization=0.1, dtype=F32):
    """The representatives of ALL clusters: {'vertices' (C, 3), 'normals' (C, 3) | absent, 'colors' (C, 3) | absent}.
    dtype=np.float64 runs the same statement in double precision (for error figures, not for bit comparisons)."""
    order, starts, ckeys = clusters["order"].astype(np.int64), clusters["starts"], clusters["cluster_keys"]
    cid = clusters["vertex_cluster"].astype(np.int64)
    p = np.asarray(vertices, dtype=F32).reshape(-1, 3).astype(dtype)
    k = np.diff(starts.astype(np.int64))
    kf = k.astype(dtype)[:, None]
    out = {}
    with np.errstate(all="ignore"):
        mean = (_sequential_sums(p, order, starts, dtype) / kf).astype(dtype)
        x = mean
        if placement == "quadric":
            n = np.asarray(normals, dtype=F32).reshape(-1, 3).astype(dtype)
            r = (p - mean[cid]).astype(dtype)
            along = _dot3(n, r, dtype)
            terms = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2],
                              n[:, 2] * n[:, 2], n[:, 0] * along, n[:, 1] * along, n[:, 2] * along], axis=1).astype(dtype)
            s = _sequential_sums(terms, order, starts, dtype)
            lam = (dtype(regularization) * kf[:, 0]).astype(dtype)
            axx, axy, axz, ayy, ayz, azz = (s[:, 0] + lam).astype(dtype), s[:, 1], s[:, 2], (s[:, 3] + lam).astype(dtype), \
                s[:, 4], (s[:, 5] + lam).astype(dtype)
            b = s[:, 6:9]
            c00, c01, c02 = _dop(ayy, azz, ayz, ayz, dtype), _dop(axz, ayz, axy, azz, dtype), _dop(axy, ayz, axz, ayy, dtype)
            c11, c12, c22 = _dop(axx, azz, axz, axz, dtype), _dop(axy, axz, axx, ayz, dtype), _dop(axx, ayy, axy, axy, dtype)
            rows = [np.stack(t, axis=1) for t in ((c00, c01, c02), (c01, c11, c12), (c02, c12, c22))]
            det = _dot3(np.stack([axx, axy, axz], axis=1), rows[0], dtype)
            ok = (det > 0) & np.isfinite(det)
            d = np.stack([(_dot3(row, b, dtype) / np.where(ok, det, dtype(1))).astype(dtype) for row in rows], axis=1)
            d = np.where(ok[:, None], d, dtype(0)).astype(dtype)
            idx = np.stack([(ckeys >> (BITS * c)) & ((1 << BITS) - 1) for c in range(3)], axis=1).astype(dtype)
            cell_t, origin_t = vec3(cell).astype(dtype), vec3(origin).astype(dtype)
            lo = (origin_t[None, :] + (idx * cell_t[None, :]).astype(dtype)).astype(dtype)
            hi = (lo + cell_t[None, :]).astype(dtype)
            x = (mean + d).astype(dtype)
            x = np.where(x < lo, lo, x)
            x = np.where(x > hi, hi, x)
        elif placement != "mean":
            raise ValueError(placement)
        out["vertices"] = x.astype(dtype)
        if normals is not None:
            sn = _sequential_sums(np.asarray(normals, dtype=F32).reshape(-1, 3).astype(dtype), order, starts, dtype)
            length = np.sqrt(_dot3(sn, sn, dtype)).astype(dtype)
            ok = length > 0
            out["normals"] = np.where(ok[:, None], (sn / np.where(ok, length, dtype(1))[:, None]).astype(dtype), dtype(0)).astype(dtype)
        if colors is not None:
            colors = np.asarray(colors).reshape(-1, 3)
            if colors.dtype == np.uint8:
                si = np.zeros((k.size, 3), dtype=np.int64)
                np.add.at(si, cid, colors.astype(np.int64))
                out["colors"] = ((2 * si + k[:, None]) // (2 * k[:, None])).astype(np.uint8)
            else:
                out["colors"] = (_sequential_sums(colors.astype(F32).astype(dtype), order, starts, dtype) / kf).astype(dtype)
    return out


def cluster_faces(faces, vertex_cluster):
    """(F', 3) int32 faces over CLUSTER ids (nothing compacted yet): degenerate faces dropped, opposite pairs cancelled,
    |net| copies per triple, triples ascending."""
    cid = np.asarray(vertex_cluster, dtype=np.int64)
    f = cid[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    if f.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.int32)
    first = np.argmin(f, axis=1)
    rot = np.take_along_axis(f, (first[:, None] + np.arange(3)[None, :]) % 3, axis=1)
    a, x, y = rot[:, 0], rot[:, 1], rot[:, 2]
    sign = np.where(x < y, 1, -1)
    triples = np.stack([a, np.minimum(x, y), np.maximum(x, y)], axis=1)
    uniq, inverse = np.unique(triples, axis=0, return_inverse=True)        # rows in ascending lexicographic order
    net = np.zeros(uniq.shape[0], dtype=np.int64)
    np.add.at(net, inverse.reshape(-1), sign)
    rows = np.where((net > 0)[:, None], uniq, uniq[:, [0, 2, 1]])
    return np.repeat(rows, np.abs(net), axis=0).astype(np.int32).reshape(-1, 3)


def simplify_mesh(mesh, cell, origin=None, placement="quadric", regularization=0.1, dtype=F32):
    """mesh: dict of arrays 'vertices' (V, 3) float32, 'faces' (F, 3), optional 'normals' (V, 3), 'colors' (V, 3) uint8 or
    float32 -> {'vertices', 'faces', 'normals' / 'colors' when given, 'vertex_cluster' (V,) int32}."""
    v = np.asarray(mesh["vertices"], dtype=F32).reshape(-1, 3)
    faces = np.asarray(mesh["faces"]).reshape(-1, 3)
    normals, colors = mesh.get("normals"), mesh.get("colors")
    if placement == "quadric" and normals is None:
        raise ValueError("quadric placement needs normals")
    if v.shape[0] == 0:
        out = {"vertices": v, "faces": np.zeros((0, 3), dtype=np.int32), "vertex_cluster": np.zeros(0, dtype=np.int32)}
        if normals is not None:
            out["normals"] = np.zeros((0, 3), dtype=F32)
        if colors is not None:
            out["colors"] = np.zeros((0, 3), dtype=np.asarray(colors).dtype)
        return out
    if origin is None:
        origin = v.min(axis=0)
    clusters = cluster_vertices(v, cell, origin)
    rep = reduce_clusters(v, normals, colors, clusters, cell, origin, placement, regularization, dtype)
    cf = cluster_faces(faces, clusters["vertex_cluster"])
    used = np.zeros(clusters["cluster_keys"].size, dtype=bool)
    used[cf.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    out = {k: a[used] for k, a in rep.items()}
    out["faces"] = new_id[cf].astype(np.int32).reshape(-1, 3)
    cid = clusters["vertex_cluster"]
    out["vertex_cluster"] = np.where(used[cid], new_id[cid], -1).astype(np.int32)
    return out


def edge_balance(faces):
    """True when every directed edge occurs as often as its reverse: the boundary of the face chain is zero."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return True
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    n = int(f.max()) + 1
    fwd, fc = np.unique(d[:, 0] * n + d[:, 1], return_counts=True)
    rev, rc = np.unique(d[:, 1] * n + d[:, 0], return_counts=True)
    return bool(fwd.size == rev.size and (fwd == rev).all() and (fc == rc).all())


def max_net_multiplicity(faces):
    """The largest number of copies of one oriented face."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return 0
    return int(np.unique(f, axis=0, return_counts=True)[1].max())


def hashed_colors(n, dtype, seed=0):
    """(n, 3) colours from an integer hash of the vertex id: uint8, or float32 in [0, 1)."""
    i = np.arange(3 * n, dtype=np.uint64) + np.uint64(0x9E3779B9 * (seed + 1))
    h = (i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    if dtype == np.uint8:
        return (h & np.uint64(255)).astype(np.uint8).reshape(n, 3)
    return ((h >> np.uint64(8)).astype(np.float64) / float(1 << 24)).astype(F32).reshape(n, 3)


def hashed_normals(n, seed=0):
    """(n, 3) float32 unit-ish vectors from the same hash (strips have no isosurface to take normals from)."""
    u = hashed_colors(n, np.float32, seed + 7).astype(np.float64) * 2.0 - 1.0
    return (u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-3)).astype(F32)


def hand_made():
    """A mesh made by hand for unit cells from the origin, with what simplification must give.  Cells A (0,0,0), B (1,0,0),
    C (0,1,0), D (1,1,0), G (0,0,1), E (5,5,5) are the clusters 0 .. 5 in key order.  Triple ABC is covered twice with the
    same winding (|net| = 2), BCD twice as (B, D, C) and once as (B, C, D) (net = -1), ABG once each way (net = 0: G loses
    all its faces), one face has two vertices in A (it degenerates), and no face uses the vertex in E."""
    vertices = np.array([[0.2, 0.2, 0.2], [0.6, 0.4, 0.3],            # 0, 1 in A
                         [1.2, 0.3, 0.1], [1.7, 0.5, 0.5],            # 2, 3 in B
                         [0.3, 1.2, 0.4], [0.5, 1.6, 0.2],            # 4, 5 in C
                         [1.5, 1.5, 0.5],                             # 6 in D
                         [5.5, 5.5, 5.5],                             # 7 in E, unused
                         [0.5, 0.5, 1.5]], dtype=F32)                 # 8 in G
    faces = np.array([[0, 2, 4], [3, 5, 1],                           # ABC twice
                      [2, 6, 4], [6, 5, 3], [3, 4, 6],                # (B, D, C), (D, C, B), (B, C, D)
                      [0, 2, 8], [1, 8, 3],                           # ABG and its opposite
                      [0, 1, 2]], dtype=np.int32)                     # degenerate
    mesh = {"vertices": vertices, "faces": faces, "normals": hashed_normals(9, 3), "colors": hashed_colors(9, np.uint8, 3)}
    expect = {"faces": np.array([[0, 1, 2], [0, 1, 2], [1, 3, 2]], dtype=np.int32),
              "vertex_cluster": np.array([0, 0, 1, 1, 2, 2, 3, -1, -1], dtype=np.int32), "n_clusters": 6}
    return mesh, 1.0, (0.0, 0.0, 0.0), expect
