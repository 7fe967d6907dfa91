"""NumPy float32 restatement of the marching-tetrahedra isosurface (csrc/hn_geometry.hip) and a mesh checker.

The restatement follows the kernels' definition, not their code: the same lattice, the same Kuhn split of every cell into
six tetrahedra, the same edge ownership (7 direction classes per lattice point), the same orderings (vertices by
ascending edge slot, faces by ascending cell, tetrahedron, triangle) and the same integer orientation rule.  Every float
operation is a float32 operation rounded on its own, so positions agree with the GPU to a few roundings and the face
arrays agree exactly.

    grid f[nx, ny, nz], point index p = (i*ny + j)*nz + k, position lo + (i, j, k) * (hi - lo)/(n - 1)
    inside = f >= iso (NaN is outside)
    edge slot e = 7*p + d, d = class of the edge's direction from its LOWER lattice point:
        (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
    tetrahedron q of a cell = q-th permutation pi of the axes in lexicographic order:
        v0 = origin, v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = v0 + (1,1,1)
"""
import itertools

import numpy as np

F32 = np.float32
DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], dtype=np.int64)
DIR_CLASS = {tuple(d): n for n, d in enumerate(DIRS.tolist())}
PERMS = list(itertools.permutations(range(3)))


def tet_corners(q):
    """The four corner offsets (each in {0,1}^3) of tetrahedron q of a cell."""
    pi = PERMS[q]
    v = [np.zeros(3, dtype=np.int64)]
    for axis in pi[:2]:
        nxt = v[-1].copy()
        nxt[axis] += 1
        v.append(nxt)
    v.append(np.ones(3, dtype=np.int64))
    return v


def _det3(a, b, c):
    return int(a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))


def tet_triangles(q, mask):
    """Triangles of tetrahedron q for the inside mask (bit t = corner v_t inside): a list of triangles, each three
    (corner a, corner b) pairs with a < b naming the tetrahedron edge the triangle's vertex lies on.  The winding is
    fixed by the sign of an integer determinant of lattice vectors, so that normals point from inside to outside."""
    v = tet_corners(q)
    ins = [t for t in range(4) if mask >> t & 1]
    outs = [t for t in range(4) if not mask >> t & 1]
    edge = lambda a, b: (min(a, b), max(a, b))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1 or len(outs) == 1:
        lone = ins[0] if len(ins) == 1 else outs[0]
        rest = outs if len(ins) == 1 else ins
        det = _det3(v[rest[0]] - v[lone], v[rest[1]] - v[lone], v[rest[2]] - v[lone])
        # det > 0: (P0, P1, P2) winds with its normal pointing away from the lone corner
        away = det > 0
        keep = away if len(ins) == 1 else not away
        tri = [edge(lone, rest[0]), edge(lone, rest[1]), edge(lone, rest[2])]
        return [tri if keep else [tri[0], tri[2], tri[1]]]
    i0, i1 = ins
    o0, o1 = outs
    det = _det3(v[o1] - v[o0], v[i1] - v[i0], v[o0] + v[o1] - v[i0] - v[i1])
    quad = [edge(i0, o0), edge(i0, o1), edge(i1, o1), edge(i1, o0)]
    if det < 0:
        quad = [quad[0], quad[3], quad[2], quad[1]]
    return [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]


def _steps(shape, bounds):
    lo = np.array([bounds[0], bounds[2], bounds[4]], dtype=F32)
    hi = np.array([bounds[1], bounds[3], bounds[5]], dtype=F32)
    step = (hi - lo) / (np.array(shape, dtype=F32) - F32(1))
    return lo, step.astype(F32)


def lattice_points(shape, bounds, start=0, count=None):
    """(count, 3) float32 positions of lattice points start .. start + count - 1 (an index past the lattice is clamped
    to its last point): lo + (i, j, k) * step, product and sum rounded on their own."""
    nx, ny, nz = shape
    n = nx * ny * nz
    count = n - start if count is None else count
    p = np.minimum(np.arange(start, start + count, dtype=np.int64), n - 1)
    ijk = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], axis=-1)
    lo, step = _steps(shape, bounds)
    return (lo[None, :] + (ijk.astype(F32) * step[None, :]).astype(F32)).astype(F32)


def _gradient(f, step):
    """Central differences (one-sided on the boundary) of f, float32: (nx, ny, nz, 3)."""
    g = np.zeros(f.shape + (3,), dtype=F32)
    for ax in range(3):
        n = f.shape[ax]
        hi = np.minimum(np.arange(n) + 1, n - 1)
        lo = np.maximum(np.arange(n) - 1, 0)
        width = (hi - lo).astype(F32) * step[ax]
        shp = [1, 1, 1]
        shp[ax] = n
        g[..., ax] = ((np.take(f, hi, axis=ax) - np.take(f, lo, axis=ax)).astype(F32) / width.reshape(shp).astype(F32)).astype(F32)
    return g


def extract_isosurface(f, iso, bounds):
    """{'vertices': (V,3) float32, 'normals': (V,3) float32, 'faces': (F,3) int32} of the surface f = iso."""
    f = np.ascontiguousarray(f, dtype=F32)
    nx, ny, nz = f.shape
    iso = F32(iso)
    with np.errstate(invalid="ignore"):
        inside = f >= iso
    lo, step = _steps(f.shape, bounds)
    grad = _gradient(f, step)
    n = nx * ny * nz
    slots = np.full(7 * n, -1, dtype=np.int64)
    ii, jj, kk = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    p_all = (ii * ny + jj) * nz + kk
    # pass A: crossings per edge slot
    cross = np.zeros((n, 7), dtype=bool)
    for d, (dx, dy, dz) in enumerate(DIRS.tolist()):
        a = (slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))
        b = (slice(dx, nx), slice(dy, ny), slice(dz, nz))
        cross[p_all[a].reshape(-1), d] = (inside[a] != inside[b]).reshape(-1)
    e = np.flatnonzero(cross.reshape(-1))                 # ascending edge slot = vertex order
    slots[e] = np.arange(e.size)
    # pass B: vertices and normals
    p, d = e // 7, e % 7
    ia = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], axis=-1)
    ib = ia + DIRS[d]
    fa, fb = f[ia[:, 0], ia[:, 1], ia[:, 2]], f[ib[:, 0], ib[:, 1], ib[:, 2]]
    with np.errstate(all="ignore"):
        t = ((iso - fa).astype(F32) / (fb - fa).astype(F32)).astype(F32)
        pa = (lo[None, :] + (ia.astype(F32) * step[None, :]).astype(F32)).astype(F32)
        pb = (lo[None, :] + (ib.astype(F32) * step[None, :]).astype(F32)).astype(F32)
        vertices = (pa + (t[:, None] * (pb - pa).astype(F32)).astype(F32)).astype(F32)
        ga, gb = grad[ia[:, 0], ia[:, 1], ia[:, 2]], grad[ib[:, 0], ib[:, 1], ib[:, 2]]
        g = (ga + (t[:, None] * (gb - ga).astype(F32)).astype(F32)).astype(F32)
        sq = (g * g).astype(F32)
        length = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)).astype(F32)
        ok = length > 0
        normals = np.where(ok[:, None], (-g / np.where(ok, length, F32(1))[:, None]).astype(F32), F32(0)).astype(F32)
    # pass C: faces, by cell, tetrahedron, triangle
    ci, cj, ck = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")
    ci, cj, ck = ci.reshape(-1), cj.reshape(-1), ck.reshape(-1)
    n_cells = ci.size
    per_cell = []                                          # (cell, tet, tri, face row) blocks, sorted afterwards
    for q in range(6):
        v = tet_corners(q)
        bits = [inside[ci + c[0], cj + c[1], ck + c[2]] for c in v]
        mask = sum(b.astype(np.int64) << t for t, b in enumerate(bits))
        for m in range(1, 15):
            cells = np.flatnonzero(mask == m)
            if cells.size == 0:
                continue
            for tri_no, tri in enumerate(tet_triangles(q, m)):
                ids = []
                for a, b in tri:
                    owner = ((ci[cells] + v[a][0]) * ny + cj[cells] + v[a][1]) * nz + ck[cells] + v[a][2]
                    ids.append(slots[7 * owner + DIR_CLASS[tuple((v[b] - v[a]).tolist())]])
                key = (cells * 6 + q) * 2 + tri_no
                per_cell.append(np.stack([key] + ids, axis=-1))
    if per_cell:
        rows = np.concatenate(per_cell, axis=0)
        rows = rows[np.argsort(rows[:, 0], kind="stable")]
        faces = rows[:, 1:]
    else:
        faces = np.zeros((0, 3), dtype=np.int64)
    assert n_cells >= 1 and (faces >= 0).all()
    return {"vertices": vertices.reshape(-1, 3), "normals": normals.reshape(-1, 3), "faces": faces.astype(np.int32)}


def check_mesh(vertices, faces):
    """Topology and size of a triangle mesh: every undirected edge used by exactly two faces (`closed`), every directed
    edge used once with its reverse present (`oriented`), Euler characteristic V - E + F (V = vertices the faces use),
    signed volume (positive when the normals point outwards) and area, in float64."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    if f.shape[0] == 0:
        return {"closed": True, "oriented": True, "euler": 0, "volume": 0.0, "area": 0.0, "n_vertices": 0, "n_faces": 0}
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    nv = int(f.max()) + 1
    dkey = directed[:, 0] * nv + directed[:, 1]
    rkey = directed[:, 1] * nv + directed[:, 0]
    uniq, counts = np.unique(dkey, return_counts=True)
    oriented = bool((counts == 1).all() and np.isin(rkey, uniq).all())
    und = np.sort(directed, axis=1)
    _, ucounts = np.unique(und[:, 0] * nv + und[:, 1], return_counts=True)
    closed = bool((ucounts == 2).all())
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    volume = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    area = float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)
    used = np.unique(f).size
    return {"closed": closed, "oriented": oriented, "euler": int(used - ucounts.size + f.shape[0]), "volume": volume,
            "area": area, "n_vertices": used, "n_faces": int(f.shape[0])}
