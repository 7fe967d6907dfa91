"""NumPy restatement of the mesh-distance definition (csrc/hn_mesh_distance.hip, geometry.sample_surface /
point_mesh_distance), and the small meshes its tests use.

It follows the definition, operation by operation, not the kernels: every float operation is one operation of `dtype`
rounded on its own (float32: the GPU's arrays are expected to be the same bits; float64: the ground truth of the
arithmetic), dot(u, v) = (ux*vx + uy*vy) + uz*vz.

    weights   a2 = sqrt(dot(n, n)), n = (B - A) x (C - A), every component one product minus another; 0 unless finite
              w = (int64)((a2 / max a2) * 2^24), truncated; cdf = the inclusive sum of w; W = cdf[-1]
    sample k  h_j = splitmix64(key + 3 k + j), key = splitmix64(seed); t = mulhi64(h_0, W); face = the first f with
              cdf[f] > t; u1, u2 = (h_1 >> 40) * 2^-24, (h_2 >> 40) * 2^-24; s = sqrt(u1); b = (1 - s, s * (1 - u2), s * u2);
              point = (b0*A + b1*B) + b2*C
    closest   ab = B - A, ac = C - A, ap = P - A, bp = P - B, cp = P - C
              d1 = ab.ap  d2 = ac.ap  d3 = ab.bp  d4 = ac.bp  d5 = ab.cp  d6 = ac.cp
              vc = d1*d4 - d3*d2   vb = d5*d2 - d1*d6   va = d3*d6 - d5*d4   e43 = d4 - d3   e56 = d5 - d6
              the first region that holds, q = (base + s * u) + t * ac:
                d1 <= 0 and d2 <= 0                    base A, s = t = 0
                d3 >= 0 and d4 <= d3                   base B, s = t = 0
                vc <= 0 and d1 >= 0 and d3 <= 0        base A, u = ab, s = d1 / (d1 - d3), t = 0
                d6 >= 0 and d5 <= d6                   base C, s = t = 0
                vb <= 0 and d2 >= 0 and d6 <= 0        base A, u = ac, s = d2 / (d2 - d6), t = 0
                va <= 0 and e43 >= 0 and e56 >= 0      base B, u = C - B, s = e43 / (e43 + e56), t = 0
                otherwise                              base A, u = ab, sum = (va + vb) + vc, s = vb / sum, t = vc / sum
              (u = ab where none is named); a zero denominator gives s = 0, a sum that is not > 0 gives s = t = 0
              dist2 = dot(P - q, P - q)
    query     the lexicographic minimum of (dist2, face id) over the faces with dist2 < +inf: distance = sqrt(dist2), the
              face, q; +inf, -1, NaN without one; NaN, -1, NaN for a point that is not finite; with max_distance, +inf, -1, NaN
              unless distance <= max_distance
"""
import numpy as np

F32 = np.float32
M64 = (1 << 64) - 1
WEIGHT_BITS = 24


# ---- hashes, in Python ints (the constants of tests/hashprng.py, restated) -----------------------------------------------
def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mulhi64(a: int, b: int) -> int:
    return (a * b) >> 64


# ---- sampling ----------------------------------------------------------------------------------------------------------------
def _dot(a, b, dtype):
    p = (a * b).astype(dtype)
    return ((p[..., 0] + p[..., 1]).astype(dtype) + p[..., 2]).astype(dtype)


def _dop(a, b, c, d, dtype):
    return ((a * b).astype(dtype) - (c * d).astype(dtype)).astype(dtype)


def face_weights(vertices, faces, dtype=F32):
    """(F,) twice the area of every face, 0 where not finite."""
    v = np.asarray(vertices, dtype=dtype)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = (b - a).astype(dtype), (c - a).astype(dtype)
        n = np.stack([_dop(e1[:, 1], e2[:, 2], e1[:, 2], e2[:, 1], dtype), _dop(e1[:, 2], e2[:, 0], e1[:, 0], e2[:, 2], dtype),
                      _dop(e1[:, 0], e2[:, 1], e1[:, 1], e2[:, 0], dtype)], axis=-1)
        a2 = np.sqrt(_dot(n, n, dtype)).astype(dtype)
    return np.where(np.isfinite(a2), a2, dtype(0)).astype(dtype)


def surface_cdf(vertices, faces):
    """(F,) int64: the inclusive sum of w = (int64)((a2 / max a2) * 2^24)."""
    a2 = face_weights(vertices, faces)
    m = a2.max() if a2.size else F32(0)
    if not m > 0:
        return np.zeros(a2.shape, dtype=np.int64)
    w = ((a2 / m).astype(F32) * F32(1 << WEIGHT_BITS)).astype(F32).astype(np.int64)
    return np.cumsum(w)


def sample_surface(vertices, faces, n, seed=0):
    """{'points' (n, 3) float32, 'face' (n,) int32, 'bary' (n, 3) float32}."""
    v = np.asarray(vertices, dtype=F32)
    f = np.asarray(faces, dtype=np.int64)
    cdf = surface_cdf(v, f)
    total = int(cdf[-1])
    assert total > 0
    key = splitmix64(int(seed) & M64)
    face = np.empty(n, dtype=np.int32)
    u = np.empty((n, 2), dtype=F32)
    for k in range(n):
        h = [splitmix64((key + 3 * k + j) & M64) for j in range(3)]
        face[k] = np.searchsorted(cdf, mulhi64(h[0], total), side="right")      # the first f with cdf[f] > t
        u[k] = [F32(h[1] >> 40) * F32(2.0 ** -24), F32(h[2] >> 40) * F32(2.0 ** -24)]
    s = np.sqrt(u[:, 0]).astype(F32)
    bary = np.stack([(F32(1) - s).astype(F32), (s * (F32(1) - u[:, 1]).astype(F32)).astype(F32), (s * u[:, 1]).astype(F32)], axis=-1)
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    points = (((bary[:, 0:1] * a).astype(F32) + (bary[:, 1:2] * b).astype(F32)).astype(F32) + (bary[:, 2:3] * c).astype(F32)).astype(F32)
    return {"points": points, "face": face, "bary": bary}


# ---- the closest point of a triangle ---------------------------------------------------------------------------------------
def closest_point(p, a, b, c, dtype=F32):
    """(q, dist2) for points p and corners a, b, c, all (..., 3) and broadcastable: the definition above, op for op."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=dtype) for x in (p, a, b, c)))
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = ((x - y).astype(dtype) for x, y in ((b, a), (c, a), (p, a), (p, b), (p, c)))
        d1, d2, d3, d4, d5, d6 = (_dot(x, y, dtype) for x, y in ((ab, ap), (ac, ap), (ab, bp), (ac, bp), (ab, cp), (ac, cp)))
        vc, vb, va = _dop(d1, d4, d3, d2, dtype), _dop(d5, d2, d1, d6, dtype), _dop(d3, d6, d5, d4, dtype)
        e43, e56 = (d4 - d3).astype(dtype), (d5 - d6).astype(dtype)
        zero = np.zeros_like(d1)

        def ratio(num, den):
            return np.where(den != 0, (num / np.where(den != 0, den, 1)).astype(dtype), zero).astype(dtype)

        total = ((va + vb).astype(dtype) + vc).astype(dtype)
        inside = total > 0
        regions = [      # (holds, base, u, s, t), first match wins
            ((d1 <= 0) & (d2 <= 0), a, ab, zero, zero),
            ((d3 >= 0) & (d4 <= d3), b, ab, zero, zero),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a, ab, ratio(d1, (d1 - d3).astype(dtype)), zero),
            ((d6 >= 0) & (d5 <= d6), c, ab, zero, zero),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a, ac, ratio(d2, (d2 - d6).astype(dtype)), zero),
            ((va <= 0) & (e43 >= 0) & (e56 >= 0), b, (c - b).astype(dtype), ratio(e43, (e43 + e56).astype(dtype)), zero),
            (np.ones(d1.shape, dtype=bool), a, ab, np.where(inside, (vb / np.where(inside, total, 1)).astype(dtype), zero),
             np.where(inside, (vc / np.where(inside, total, 1)).astype(dtype), zero)),
        ]
        base, u, s, t = (np.zeros_like(x) for x in (a, a, d1, d1))
        taken = np.zeros(d1.shape, dtype=bool)
        for holds, rb, ru, rs, rt in regions:
            pick = holds & ~taken
            base, u = np.where(pick[..., None], rb, base), np.where(pick[..., None], ru, u)
            s, t = np.where(pick, rs, s), np.where(pick, rt, t)
            taken |= pick
        s, t = s.astype(dtype)[..., None], t.astype(dtype)[..., None]
        q = ((base + (s * u).astype(dtype)).astype(dtype) + (t * ac).astype(dtype)).astype(dtype)
        d = (p - q).astype(dtype)
        return q, _dot(d, d, dtype)


def point_mesh_distance(points, vertices, faces, max_distance=None, dtype=F32):
    """Brute force: {'distance' (N,), 'face' (N,) int32, 'closest' (N, 3)}, the lexicographic minimum of (dist2, face)."""
    p = np.asarray(points, dtype=dtype).reshape(-1, 3)
    v = np.asarray(vertices, dtype=dtype)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = p.shape[0]
    dist = np.full(n, np.inf, dtype=dtype)
    face = np.full(n, -1, dtype=np.int32)
    closest = np.full((n, 3), np.nan, dtype=dtype)
    if f.shape[0] and n:
        q, d2 = closest_point(p[:, None, :], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None], dtype)
        d2 = np.where(np.isnan(d2), np.inf, d2)
        best = np.argmin(d2, axis=1)                 # the first of equal minima: the smallest face id
        rows = np.arange(n)
        found = d2[rows, best] < np.inf
        with np.errstate(all="ignore"):
            dist = np.where(found, np.sqrt(d2[rows, best]).astype(dtype), dist).astype(dtype)
        face = np.where(found, best, -1).astype(np.int32)
        closest = np.where(found[:, None], q[rows, best], closest).astype(dtype)
    bad = ~np.isfinite(p).all(axis=1)
    dist[bad], face[bad], closest[bad] = np.nan, -1, np.nan
    if max_distance is not None:
        far = ~bad & ~(dist <= dtype(max_distance))
        dist[far], face[far], closest[far] = np.inf, -1, np.nan
    return {"distance": dist, "face": face, "closest": closest}


# ---- meshes --------------------------------------------------------------------------------------------------------------------
def cube(half=0.5, center=(0.0, 0.0, 0.0)):
    """(vertices (8, 3) float32, faces (12, 3) int32) of the axis-aligned cube |x - center| <= half, wound outwards.  Vertex
    i has the signs (bit 0, bit 1, bit 2) of i on (x, y, z); faces 0, 1 are the +x side, split along its diagonal from
    (+, -, -) to (+, +, +)."""
    v = np.array([[(1 if i & 1 else -1), (1 if i & 2 else -1), (1 if i & 4 else -1)] for i in range(8)], dtype=np.float64)
    v = (v * half + np.asarray(center, dtype=np.float64)).astype(F32)
    quads = [(1, 3, 7, 5), (0, 4, 6, 2), (2, 6, 7, 3), (0, 1, 5, 4), (4, 5, 7, 6), (0, 2, 3, 1)]      # +x -x +y -y +z -z
    faces = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v, np.array(faces, dtype=np.int32)


def icosphere(level=2, radius=1.0):
    """(vertices, faces) of the unit icosahedron subdivided `level` times, vertices pushed onto the sphere: 20 * 4**level
    faces, wound outwards."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(F32), np.asarray(f, dtype=np.int32)


def one_triangle():
    """The triangle (0, 0, 0), (4, 0, 0), (0, 4, 0): every region of it has points with exact feet."""
    return np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], dtype=F32), np.array([[0, 1, 2]], dtype=np.int32)


def planar_quad(n=4):
    """An n x n lattice of squares in the plane z = 0.25 over [0, 1]^2, two triangles each: a mesh whose box has a
    zero-length axis."""
    g = np.linspace(0.0, 1.0, n + 1)
    v = np.array([[x, y, 0.25] for y in g for x in g], dtype=F32)
    f = []
    for j in range(n):
        for i in range(n):
            k = j * (n + 1) + i
            f += [(k, k + 1, k + n + 2), (k, k + n + 2, k + n + 1)]
    return v, np.array(f, dtype=np.int32)


def hash_points(seed, n, lo=-1.5, hi=1.5):
    """(n, 3) float32 points in [lo, hi)^3 from splitmix64(seed-keyed counter), 24 bits each."""
    key = splitmix64(int(seed) & M64)
    u = np.array([splitmix64((key + i) & M64) >> 40 for i in range(3 * n)], dtype=np.float64) * 2.0 ** -24
    return (lo + (hi - lo) * u).astype(F32).reshape(n, 3)
