"""NumPy restatement of the registration definition (csrc/hn_registration.hip, geometry.register_mesh), and
the shapes its tests use.

It follows the definition, operation by operation, not the kernels.

    transform  float32, every operation rounded on its own: row_i = (R_i0*x + R_i1*y) + R_i2*z, out_i = row_i * s + t_i; the
               direction form: out = row / sqrt((row_0^2 + row_1^2) + row_2^2), row itself unless the length is > 0; NaN for
               a point that is not finite
    inlier     distance finite and <= tau, 0 <= face < F, and in plane mode a face whose normal has a positive finite length
    terms      float64 from the float32 inputs, every operation rounded on its own (NumPy's float64 array operations are),
               dot(u, v) = (ux*vx + uy*vy) + uz*vz, cross(u, v)_x = uy*vz - uz*vy and cyclic
               point  1 | d*d | p | q | q_i*p_j (index 3 i + j) | dot(p, p) | dot(q, q)                        19 values
               plane  1 | d*d | r*r | J_a*J_b, a <= b, by rows | J_a*r                                          38 values
                      m = cross(B - A, C - A), n = m / sqrt(dot(m, m)), r = dot(p - q, n), J = [cross(p, n), n, dot(p, n)]
    order      T = 256 n_blocks threads; thread g adds the terms of the inliers among points g, g + T, ... to +0 in that
               order; a wave of 64 threads folds by x[l] += x[l + w], w = 32 .. 1; a block of 4 waves is (w0 + w1) + (w2 +
               w3); the result adds the blocks' values to +0 in block order
    solves     point: Umeyama / Horn from the moments; plane: lstsq of the 7 x 7 (6 x 6) normal equations; compose
               s <- s' s, R <- R' R, t <- s' R' t + t'; stop when angle(R') <= tol, |t'| <= tol D, |s' - 1| <= tol
"""
import math

import numpy as np

import mesh_distance_restated as MD

F32 = np.float32
THREADS, WAVE, SUMS, POINT_SUMS, MAX_BLOCKS = 256, 64, 38, 19, 1024


def default_blocks(n):
    return min(512, max(1, -(-n // (THREADS * 8))))


# ---- the transform, float32 ------------------------------------------------------------------------------------------------
def transform(points, scale, rotation, translation, direction=False):
    """(N, 3) float32; the float64 transform is rounded to float32 first."""
    p = np.asarray(points, dtype=F32).reshape(-1, 3)
    r, s, t = np.asarray(rotation, dtype=np.float64).astype(F32), F32(scale), np.asarray(translation, dtype=np.float64).astype(F32)
    with np.errstate(all="ignore"):
        prod = (r[None, :, :] * p[:, None, :]).astype(F32)                       # [k, i, j] = R_ij * p_kj
        row = ((prod[..., 0] + prod[..., 1]).astype(F32) + prod[..., 2]).astype(F32)
        if direction:
            sq = (row * row).astype(F32)
            length = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)).astype(F32)
            out = np.where(length[:, None] > 0, (row / np.where(length > 0, length, F32(1))[:, None]).astype(F32), row)
        else:
            out = ((row * s).astype(F32) + t[None]).astype(F32)
    out = np.where(np.isfinite(p).all(axis=1, keepdims=True), out, F32(np.nan))
    return out.astype(F32)


# ---- the moments, float64 --------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=-1)


def moment_terms(points, closest, distance, face, tri, tau, mode):
    """(inlier (N,) bool, terms (N, 38) float64): what every point would add; rows of points that are no inliers hold
    anything and are never added."""
    p, q = (np.asarray(x, dtype=F32).reshape(-1, 3).astype(np.float64) for x in (points, closest))
    d32 = np.asarray(distance, dtype=F32).reshape(-1)
    f = np.asarray(face, dtype=np.int64).reshape(-1)
    tri = np.asarray(tri, dtype=F32).reshape(-1, 12)
    n = p.shape[0]
    with np.errstate(all="ignore"):
        inlier = (d32 <= F32(tau)) & np.isfinite(d32) & (f >= 0) & (f < tri.shape[0])
        d = d32.astype(np.float64)
        terms = np.zeros((n, SUMS), dtype=np.float64)
        terms[:, 0] = 1.0
        terms[:, 1] = d * d
        if mode == 'point':
            terms[:, 2:5], terms[:, 5:8] = p, q
            for i in range(3):
                for j in range(3):
                    terms[:, 8 + 3 * i + j] = q[:, i] * p[:, j]
            terms[:, 17], terms[:, 18] = _dot(p, p), _dot(q, q)
        else:
            t = tri[np.where(inlier, f, 0)].astype(np.float64)
            a, b, c = t[:, 0:3], t[:, 3:6], t[:, 6:9]
            m = _cross(b - a, c - a)
            length = np.sqrt(_dot(m, m))
            inlier = inlier & (length > 0) & (length <= np.finfo(np.float64).max)
            nrm = m / length[:, None]
            r = _dot(p - q, nrm)
            jac = np.concatenate([_cross(p, nrm), nrm, _dot(p, nrm)[:, None]], axis=1)
            terms[:, 2] = r * r
            k = 3
            for ja in range(7):
                for jb in range(ja, 7):
                    terms[:, k] = jac[:, ja] * jac[:, jb]
                    k += 1
            for ja in range(7):
                terms[:, 31 + ja] = jac[:, ja] * r
    return inlier, terms


def moments(points, closest, distance, face, tri, tau, mode, n_blocks=None):
    """(38,) float64, in the documented summation order."""
    inlier, terms = moment_terms(points, closest, distance, face, tri, tau, mode)
    n = terms.shape[0]
    n_blocks = default_blocks(n) if n_blocks is None else n_blocks
    total = THREADS * n_blocks
    acc = np.zeros((total, SUMS), dtype=np.float64)
    for start in range(0, n, total):
        idx = np.arange(start, min(start + total, n))
        take = inlier[idx]
        g = idx[take] - start
        acc[g] = acc[g] + terms[idx[take]]
    acc = acc.reshape(n_blocks, THREADS // WAVE, WAVE, SUMS)
    w = WAVE // 2
    while w >= 1:
        acc[:, :, :w] = acc[:, :, :w] + acc[:, :, w:2 * w]
        w //= 2
    waves = acc[:, :, 0]
    blocks = (waves[:, 0] + waves[:, 1]) + (waves[:, 2] + waves[:, 3])
    out = np.zeros(SUMS, dtype=np.float64)
    for b in range(n_blocks):
        out = out + blocks[b]
    if mode == 'point':
        out[POINT_SUMS:] = 0.0
    return out


def moments_bound(points, closest, distance, face, tri, tau, mode):
    """(38,) N * 2^-50 * sum |term|: what any summation order of correctly rounded additions stays within, with room for a
    last-bit difference in the terms themselves."""
    inlier, terms = moment_terms(points, closest, distance, face, tri, tau, mode)
    return terms.shape[0] * 2.0 ** -50 * np.abs(terms[inlier]).sum(axis=0)


# ---- the solves, float64 ------------------------------------------------------------------------------------------------------
def rodrigues(omega):
    w = np.asarray(omega, dtype=np.float64)
    angle = math.sqrt(float(w @ w))
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    if angle < 1e-8:
        return np.eye(3) + k + k @ k / 2
    return np.eye(3) + math.sin(angle) / angle * k + (1 - math.cos(angle)) / angle ** 2 * (k @ k)


def axis_angle(axis, degrees):
    a = np.asarray(axis, dtype=np.float64)
    return rodrigues(a / np.linalg.norm(a) * math.radians(degrees))


def angle_of(rotation):
    r = np.asarray(rotation, dtype=np.float64)
    v = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    return math.atan2(np.linalg.norm(v) / 2, (np.trace(r) - 1) / 2)


def solve_point(sums, with_scale):
    n = sums[0]
    mean_p, mean_q = sums[2:5] / n, sums[5:8] / n
    cov = sums[8:17].reshape(3, 3) / n - mean_q[:, None] * mean_p[None, :]
    u, sv, vt = np.linalg.svd(cov)
    fix = np.diag([1.0, 1.0, np.sign(np.linalg.det(u @ vt))])
    rot = u @ fix @ vt
    scale = 1.0
    if with_scale:
        scale = float((sv * np.diag(fix)).sum() / (sums[17] / n - mean_p @ mean_p))
    return scale, rot, mean_q - scale * rot @ mean_p


def solve_plane(sums, with_scale):
    jtj = np.zeros((7, 7))
    k = 3
    for a in range(7):
        for b in range(a, 7):
            jtj[a, b] = jtj[b, a] = sums[k]
            k += 1
    size = 7 if with_scale else 6
    x = np.linalg.lstsq(jtj[:size, :size], -sums[31:31 + size], rcond=None)[0]
    return (1.0 + x[6] if with_scale else 1.0), rodrigues(x[:3]), x[3:6]


def compose(step, current):
    (s1, r1, t1), (s0, r0, t0) = step, current
    return s1 * s0, r1 @ r0, s1 * (r1 @ t0) + t1


def matrix_of(scale, rotation, translation):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = scale * np.asarray(rotation), translation
    return m


def pack_triangles(vertices, faces):
    v, f = np.asarray(vertices, dtype=F32), np.asarray(faces, dtype=np.int64)
    tri = np.zeros((f.shape[0], 12), dtype=F32)
    tri[:, :9] = v[f].reshape(-1, 9)
    return tri


def trim_tau(distance, trim):
    d = np.asarray(distance, dtype=F32)
    finite = np.sort(d[np.isfinite(d)])
    if trim == 1.0 or finite.size == 0:
        return F32(np.inf)
    return finite[max(math.ceil(trim * finite.size), 1) - 1]


def register(samples, vertices, faces, method='plane', with_scale=False, trim=1.0, max_distance=None, init=None,
             max_iterations=50, tol=1e-5):
    """The loop of geometry.register_mesh on given float32 samples, nearest points by brute force."""
    samples = np.asarray(samples, dtype=F32)
    v, f = np.asarray(vertices, dtype=F32), np.asarray(faces, dtype=np.int64)
    tri = pack_triangles(v, f)
    corners = v[f].reshape(-1, 3).astype(np.float64)
    diagonal = np.linalg.norm(corners.max(axis=0) - corners.min(axis=0))
    current = (1.0, np.eye(3), np.zeros(3)) if init is None else init
    need = {'point': 3, 'plane': 7 if with_scale else 6}[method]
    history, converged = [], False
    for it in range(1, max_iterations + 1):
        moved = transform(samples, *current)
        q = MD.point_mesh_distance(moved, v, f, max_distance=max_distance)
        sums = moments(moved, q['closest'], q['distance'], q['face'], tri, trim_tau(q['distance'], trim), method)
        if sums[0] < need:
            raise ValueError(f"iteration {it}: {int(sums[0])} inliers")
        history.append({'rms': math.sqrt(sums[1] / sums[0]), 'inliers': int(sums[0])})
        step = (solve_point if method == 'point' else solve_plane)(sums, with_scale)
        current = compose(step, current)
        if angle_of(step[1]) <= tol and np.linalg.norm(step[2]) <= tol * diagonal and abs(step[0] - 1) <= tol:
            converged = True
            break
    return {'scale': current[0], 'rotation': current[1], 'translation': current[2], 'matrix': matrix_of(*current),
            'iterations': it, 'converged': converged, 'history': history, 'rms': history[-1]['rms'],
            'inliers': history[-1]['inliers']}


# ---- shapes --------------------------------------------------------------------------------------------------------------------
def bumpy(level):
    """(vertices float32, faces int32): the icosphere scaled to the ellipsoid (1, 0.7, 0.5) with one bump — no symmetry, so
    registration has a single answer.  Built in float64, cast at the end."""
    v, f = MD.icosphere(level)
    v = v.astype(np.float64) * np.array([1.0, 0.7, 0.5])
    gap = v - np.array([0.6, 0.3, 0.2])
    v = v + 0.35 * np.exp(-(gap * gap).sum(axis=1) / 0.08)[:, None] * np.array([0.5, 0.6, 0.62])
    return v.astype(F32), f


def moved_copy(vertices, scale, rotation, translation):
    """The vertices under x -> s R x + t in float64, cast to float32."""
    v = np.asarray(vertices, dtype=np.float64)
    return (scale * v @ np.asarray(rotation).T + np.asarray(translation)).astype(F32)


def with_floater(vertices, faces):
    """bumpy plus a small sphere off its side: an outlier cluster that the target does not have."""
    fv, ff = MD.icosphere(1, 0.25)
    fv = (fv.astype(np.float64) + np.array([1.6, 0.9, 0.4])).astype(F32)
    return np.concatenate([vertices, fv]).astype(F32), np.concatenate([faces, ff + len(vertices)]).astype(np.int32)
