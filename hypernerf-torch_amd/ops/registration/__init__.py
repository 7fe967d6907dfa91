"""Mesh registration (csrc/hn_registration.hip): the similarity transform of a point set, the sums an ICP
iteration solves from, the trimming threshold; and the float64 NumPy half of an iteration: both solves (point to point
in closed form, point to plane by least squares), composition, the stop rule's measures, similarity matrices."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ... import _lib as L
from ..checks import INT32_MAX, check_points
from ..mesh import MD_TRI_FLOATS

__all__ = ["REG_THREADS", "REG_MAX_BLOCKS", "REG_POINT_SUMS", "REG_SUMS", "REG_PARAMS", "REG_POINTS_PER_THREAD",
           "REG_DEFAULT_MAX_BLOCKS", "REG_MODES", "REG_MIN_INLIERS", "default_moment_blocks", "check_similarity",
           "similarity_matrix", "split_similarity", "transform_points", "trim_threshold", "registration_moments",
           "rodrigues", "rotation_angle", "solve_point", "solve_plane", "compose_similarity"]

# mirrors of csrc/hn_registration.hip's limits (no macros in the header: its set of constants is that of ABI 340)
REG_THREADS = 256          # threads per workgroup of the moments launch
REG_MAX_BLOCKS = 1024      # the most workgroups (partials) a moments launch takes
REG_POINT_SUMS = 19        # values of a point-mode result
REG_SUMS = 38              # values of a plane-mode result; doubles per partial and per result
REG_PARAMS = 13            # host floats of a transform: R row-major (9), s, t (3)
# the default launch: a thread adds about this many points, up to this many workgroups (DESIGN.md 3.15 has the numbers)
REG_POINTS_PER_THREAD = 8
REG_DEFAULT_MAX_BLOCKS = 512
REG_MODES = {'point': 0, 'plane': 1}
# the fewest inliers an iteration solves from: (method, with_scale) -> count
REG_MIN_INLIERS = {('point', False): 3, ('point', True): 3, ('plane', False): 6, ('plane', True): 7}


def default_moment_blocks(n: int) -> int:
    """Workgroups of a moments launch over n points: ceil(n / (256 * 8)), 1 .. 512."""
    return min(REG_DEFAULT_MAX_BLOCKS, max(1, -(-int(n) // (REG_THREADS * REG_POINTS_PER_THREAD))))


# ---- similarity transforms, float64 on the host ------------------------------------------------------------------------------
def similarity_matrix(scale: float, rotation, translation) -> np.ndarray:
    """(4, 4) float64: x -> scale * rotation x + translation."""
    m = np.eye(4, dtype=np.float64)
    m[:3, :3] = float(scale) * np.asarray(rotation, dtype=np.float64)
    m[:3, 3] = np.asarray(translation, dtype=np.float64)
    return m


def check_similarity(matrix, what: str) -> Tuple[float, np.ndarray, np.ndarray]:
    """(scale, rotation (3, 3), translation (3,)) of a 4 x 4 similarity matrix (a tensor, an array or nested lists), float64;
    ValueError unless it is finite, its last row is (0, 0, 0, 1), its determinant is positive and its linear part is a
    rotation times one scale: |M^T M / s^2 - I| <= 1e-6 with s = det^(1/3)."""
    if isinstance(matrix, torch.Tensor):
        matrix = matrix.detach().cpu().numpy()
    try:
        m = np.asarray(matrix, dtype=np.float64)
    except (TypeError, ValueError):
        m = np.zeros(0)
    if m.shape != (4, 4) or not np.isfinite(m).all() or not (m[3] == np.array([0.0, 0.0, 0.0, 1.0])).all():
        raise ValueError(f"{what}: a transform is a finite (4, 4) matrix with the last row (0, 0, 0, 1), got {matrix!r}")
    a = m[:3, :3]
    det = float(np.linalg.det(a))
    if not det > 0.0:
        raise ValueError(f"{what}: the transform's determinant {det} is not positive (a reflection or a collapse)")
    s = det ** (1.0 / 3.0)
    r = a / s
    if not np.abs(r.T @ r - np.eye(3)).max() <= 1e-6:
        raise ValueError(f"{what}: the transform is not a similarity (a rotation times one scale)")
    u, _, vt = np.linalg.svd(r)          # the nearest rotation: what the 1e-6 lets through is taken out
    return s, u @ vt, m[:3, 3].copy()


def split_similarity(matrix) -> Tuple[float, np.ndarray, np.ndarray]:
    """check_similarity without a caller's name."""
    return check_similarity(matrix, "split_similarity")


def rodrigues(omega) -> np.ndarray:
    """exp([omega]x), float64: I + sin(a)/a K + (1 - cos(a))/a^2 K^2, the series' first terms below 1e-8."""
    w = np.asarray(omega, dtype=np.float64).reshape(3)
    a = float(np.linalg.norm(w))
    k = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if a < 1e-8:
        return np.eye(3) + k + 0.5 * (k @ k)
    return np.eye(3) + (math.sin(a) / a) * k + ((1.0 - math.cos(a)) / (a * a)) * (k @ k)


def rotation_angle(rotation) -> float:
    """The angle of a rotation matrix in radians, atan2(|vee(R - R^T)| / 2, (trace - 1) / 2): no arccos near 1."""
    r = np.asarray(rotation, dtype=np.float64)
    v = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    return float(math.atan2(0.5 * float(np.linalg.norm(v)), 0.5 * (float(np.trace(r)) - 1.0)))


def compose_similarity(step, current):
    """(s' s, R' R, s' R' t + t') of step = (s', R', t') applied after current = (s, R, t)."""
    (s1, r1, t1), (s0, r0, t0) = step, current
    return s1 * s0, r1 @ r0, s1 * (r1 @ t0) + t1


def solve_point(sums, with_scale: bool):
    """(s', R', t') that moves the points p onto their closest points q in the least-squares sense, from a point-mode
    result of registration_moments (Umeyama 1991 / Horn 1987): H = sum q p^T / n - mean(q) mean(p)^T = U D V^T, R' = U
    diag(1, 1, det(U V^T)) V^T, s' = trace(D diag(1, 1, det)) / var(p) with with_scale (1 otherwise, and when var(p) is
    0), t' = mean(q) - s' R' mean(p)."""
    m = np.asarray(sums, dtype=np.float64)
    n = m[0]
    mp, mq = m[2:5] / n, m[5:8] / n
    h = m[8:17].reshape(3, 3) / n - np.outer(mq, mp)
    u, d, vt = np.linalg.svd(h)
    sign = np.array([1.0, 1.0, 1.0 if np.linalg.det(u @ vt) >= 0.0 else -1.0])
    r = u @ np.diag(sign) @ vt
    var_p = m[17] / n - float(mp @ mp)
    s = float((d * sign).sum() / var_p) if with_scale and var_p > 0.0 else 1.0
    if not (np.isfinite(s) and s > 0.0):
        s = 1.0
    return s, r, mq - s * (r @ mp)


def solve_plane(sums, with_scale: bool):
    """(s', R', t') of one Gauss-Newton step of the point-to-plane error sum ((s' R' p + t' - q) . n)^2 linearised at the
    identity, from a plane-mode result of registration_moments: x = lstsq(J^T J, -J^T r) over (omega, t', sigma) — the
    leading 6 x 6 without with_scale — the minimum-norm solution, so that a target whose normals leave directions free
    (a plane, a sphere) gives a finite step; R' = exp([omega]x), s' = 1 + sigma."""
    m = np.asarray(sums, dtype=np.float64)
    a = np.zeros((7, 7), dtype=np.float64)
    a[np.triu_indices(7)] = m[3:31]
    a = a + np.triu(a, 1).T
    k = 7 if with_scale else 6
    x = np.linalg.lstsq(a[:k, :k], -m[31:31 + k], rcond=None)[0]
    s = 1.0 + float(x[6]) if with_scale else 1.0
    return s, rodrigues(x[:3]), x[3:6].copy()


# ---- device halves --------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def transform_points(points: torch.Tensor, scale: float, rotation, translation, direction: bool = False) -> torch.Tensor:
    """(N, 3) fp32: scale * rotation p + translation of points (N, 3) fp32 (hn_reg_transform), the float64 transform rounded
    to fp32 once; every fp32 operation rounded on its own, row_i = (R_i0*x + R_i1*y) + R_i2*z, then * scale, then + t_i.
    direction: rotation only, the result divided by its length (a zero vector stays zero).  A point that is not finite
    gives NaN.  ValueError: a transform that is not finite in fp32."""
    what = "transform_points"
    points = check_points(points, what, "points")
    with np.errstate(over="ignore"):
        params = np.concatenate([np.asarray(rotation, dtype=np.float64).reshape(9), [float(scale)],
                                 np.asarray(translation, dtype=np.float64).reshape(3)]).astype(np.float32)
    if not np.isfinite(params).all():
        raise ValueError(f"{what}: the transform is not finite in float32")
    n = points.shape[0]
    if n > INT32_MAX:
        raise ValueError(f"{what}: {n} points exceed 2**31 - 1 = {INT32_MAX}")
    L.require_gpu(points)
    out = torch.empty_like(points)
    if n == 0:
        return out
    L.load()
    with torch.cuda.device(points.device):
        L.launch("hn_reg_transform", L.ptr(points), n, (C.c_float * REG_PARAMS)(*params.tolist()), int(bool(direction)),
                 L.ptr(out), L.stream_handle())
    return out


@torch.no_grad()
def trim_threshold(distance: torch.Tensor, trim: float) -> torch.Tensor:
    """(1,) fp32 on the device: the ceil(trim * n_finite)-th smallest finite distance (torch.sort and a gather; no host
    read), +inf for trim == 1 and when no distance is finite."""
    if not 0.0 < float(trim) <= 1.0:
        raise ValueError(f"trim_threshold: trim must be in (0, 1], got {trim!r}")
    inf = torch.full((1,), float("inf"), dtype=torch.float32, device=distance.device)
    if float(trim) == 1.0 or distance.numel() == 0:
        return inf
    finite = torch.isfinite(distance)
    ordered = torch.sort(torch.where(finite, distance, inf)).values
    k = torch.ceil(float(trim) * finite.sum().double()).long()
    return ordered[(k - 1).clamp(min=0)].reshape(1)


@torch.no_grad()
def registration_moments(points: torch.Tensor, query: Dict[str, torch.Tensor], tri: torch.Tensor, tau: torch.Tensor,
                         mode: str, n_blocks: Optional[int] = None) -> torch.Tensor:
    """(38,) float64 on the device: the sums one ICP iteration solves from (hn_reg_moments), over the
    inliers — distance finite and <= tau, 0 <= face < F, and in 'plane' mode a face with a normal — of points (N, 3) fp32
    with query = grid_query's {'closest', 'distance', 'face'} for them, tri = the grid's packed triangles (F, 12), tau a
    (1,) fp32 device tensor.  'point': [n, sum d^2, sum p (3), sum q (3), sum q_i p_j (9), sum |p|^2, sum |q|^2, 0 ...];
    'plane': [n, sum d^2, sum r^2, upper triangle of J^T J (28), J^T r (7)], r = (p - q) . n, J = [p x n, n, p . n].
    n_blocks: workgroups of the launch, 1 .. 1024 (None: default_moment_blocks(N)); the summation order, and so the last
    bits, are a function of N and n_blocks, and every run gives the same bits.  No host synchronisation."""
    what = "registration_moments"
    points = check_points(points, what, "points")
    n = points.shape[0]
    if mode not in REG_MODES:
        raise ValueError(f"{what}: mode must be 'point' or 'plane', got {mode!r}")
    if n_blocks is None:
        n_blocks = default_moment_blocks(n)
    if isinstance(n_blocks, bool) or not isinstance(n_blocks, (int, np.integer)) or not 1 <= int(n_blocks) <= REG_MAX_BLOCKS:
        raise ValueError(f"{what}: n_blocks must be an int in 1 .. {REG_MAX_BLOCKS}, got {n_blocks!r}")
    try:
        closest, distance, face = query['closest'], query['distance'], query['face']
        ok = (closest.dtype == torch.float32 and tuple(closest.shape) == (n, 3) and distance.dtype == torch.float32
              and tuple(distance.shape) == (n,) and face.dtype == torch.int32 and tuple(face.shape) == (n,)
              and tri.dtype == torch.float32 and tri.dim() == 2 and tri.shape[1] == MD_TRI_FLOATS and tri.is_contiguous()
              and tau.dtype == torch.float32 and tau.numel() == 1)
    except (KeyError, TypeError, AttributeError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: query must be grid_query's result for the {n} points, tri the grid's (F, {MD_TRI_FLOATS}) "
                         "float32 triangles, tau one float32")
    if not 1 <= n <= INT32_MAX or tri.shape[0] < 1:
        raise ValueError(f"{what}: {n} points / {tri.shape[0]} faces: both must be 1 .. 2**31 - 1")
    L.require_gpu(points, closest, distance, face, tri, tau)
    dev = points.device
    if any(t.device != dev for t in (closest, distance, face, tri, tau)):
        raise ValueError(f"{what}: every tensor must live on one device")
    closest, distance, face = closest.contiguous(), distance.contiguous(), face.contiguous()
    partials = torch.empty((int(n_blocks), REG_SUMS), dtype=torch.float64, device=dev)
    sums = torch.empty(REG_SUMS, dtype=torch.float64, device=dev)
    L.load()
    with torch.cuda.device(dev):
        L.launch("hn_reg_moments", L.ptr(points), L.ptr(closest), L.ptr(distance), L.ptr(face), n, L.ptr(tri), tri.shape[0],
                 L.ptr(tau), REG_MODES[mode], int(n_blocks), L.ptr(partials), L.ptr(sums), L.stream_handle())
    return sums
