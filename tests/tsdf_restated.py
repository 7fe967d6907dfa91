"""Depth fusion's definition (csrc/hn_fusion.hip) restated in NumPy, and the closed-form scene its tests use:

  project        the forward camera model of a 24-float record, operation by operation in the order csrc/hn_camera.h writes
                 them.  With dtype float32 every operation is one correctly rounded fp32 operation (NumPy rounds every
                 elementwise operation on its own) and the kernel must give the same bits; with float64 it is the statement
                 of the same rule the fp32 one is checked against.
  integrate      hn_tsdf_integrate: the views in order, per view all lattice points at once.  With `margin` (float64 use) it
                 also counts, per lattice point, the views in which a test value lies within `margin` of its threshold.
  face_keep      hn_tsdf_face_keep, float32.
  lattice        the grid tsdf_isosurface hands to extract_isosurface: -tsdf where weight > 0, +1 elsewhere.
  sphere scene   a sphere of radius 0.5 at the origin inside bounds +-0.8, seen by 3 x 8 orbit cameras at radius 3 whose
                 depth images are the exact float64 ray-sphere distance through every pixel centre, +inf on a miss.
"""
import functools

import numpy as np

import hypernerf_torch_amd as HN
import isosurface_restated as I
import mesh_render_restated as R
import nerfies_scene as NS

F32 = np.float32
FLT_MAX = 3.402823466e38
RADIUS = 0.5
BOUNDS = (-0.8, 0.8, -0.8, 0.8, -0.8, 0.8)
ELEVATIONS = (-45.0, 0.0, 45.0)
N_AZIMUTH = 8
ORBIT_RADIUS = 3.0
FRONT_VIEW = N_AZIMUTH       # the azimuth-0, elevation-0 camera's row in sphere_cameras


def project(cam, x, y, z, dtype=F32):
    """(u, v, flag, (qx, qy, qz)) of points x, y, z (arrays of `dtype`) through the record `cam`: hn_mr_project."""
    T = dtype
    c = np.asarray(cam, dtype=F32).astype(T)
    with np.errstate(all="ignore"):
        qx, qy, qz = x - c[9], y - c[10], z - c[11]
        xc = (c[0] * qx + c[1] * qy) + c[2] * qz
        yc = (c[3] * qx + c[4] * qy) + c[5] * qz
        zc = (c[6] * qx + c[7] * qy) + c[8] * qz
        behind = zc <= T(F32(1e-6))
        bad = ~behind & ~(zc <= T(FLT_MAX))
        f, aspect, skew, cx, cy = c[12:17]
        k1, k2, k3, p1, p2 = c[17:22]
        px, py = xc / zc, yc / zc
        r = px * px + py * py
        bad |= ~behind & ~(T(1) + r * (T(3) * k1 + r * (T(5) * k2 + (r * T(7)) * k3)) > 0)
        radial = T(1) + r * (k1 + r * (k2 + k3 * r))
        xd = (px * radial + ((T(2) * p1) * px) * py) + p2 * (r + (T(2) * px) * px)
        yd = (py * radial + ((T(2) * p2) * px) * py) + p1 * (r + (T(2) * py) * py)
        u = ((f * xd) + (skew * yd)) + cx
        v = ((f * aspect) * yd) + cy
        bad |= ~behind & (~(np.abs(u) <= T(FLT_MAX)) | ~(np.abs(v) <= T(FLT_MAX)))
    flag = np.where(behind, 1, np.where(bad, 2, 0)).astype(np.int32)
    ok = flag == 0
    return np.where(ok, u, T(0)).astype(T), np.where(ok, v, T(0)).astype(T), flag, (qx, qy, qz)


def lattice_xyz(shape, bounds, dtype=F32):
    """The float32 positions hn_grid_points gives the lattice, per axis and flattened (z fastest), cast to `dtype`."""
    p = I.lattice_points(shape, bounds)
    return tuple(p[:, c].astype(dtype) for c in range(3))


def _near_threshold(u, v, flag, depth, seen, s, trunc, margin):
    """Per point: does a test of this view hang on less than `margin`?  s within margin of -trunc; or u (v) within margin
    of a pixel edge across which the outcome differs: the image border, or two pixels that hold different depths (two
    values that are not > 0 count as the same: both say nothing).  A point within margin of an edge in u AND in v counts
    whatever the pixels hold."""
    h, wd = depth.shape
    inside = (flag == 0) & (u > -margin) & (u < wd + margin) & (v > -margin) & (v < h + margin)
    ku, kv = np.rint(u), np.rint(v)
    at_u, at_v = inside & (np.abs(u - ku) < margin), inside & (np.abs(v - kv) < margin)

    def differs(row_a, col_a, row_b, col_b):
        ok = (row_a >= 0) & (row_b < h) & (col_a >= 0) & (col_b < wd)
        a = depth[np.clip(row_a, 0, h - 1), np.clip(col_a, 0, wd - 1)]
        b = depth[np.clip(row_b, 0, h - 1), np.clip(col_b, 0, wd - 1)]
        return ~ok | ~((a == b) | (~(a > 0) & ~(b > 0)))

    iu, iv = np.where(inside, ku, 0).astype(np.int64), np.where(inside, kv, 0).astype(np.int64)
    fu, fv = np.where(inside, np.floor(u), 0).astype(np.int64), np.where(inside, np.floor(v), 0).astype(np.int64)
    out = at_u & at_v
    out |= at_u & ~at_v & differs(fv, iu - 1, fv, iu)
    out |= at_v & ~at_u & differs(iv - 1, fu, iv, fu)
    return out | (seen & (np.abs(s + trunc) < margin))


def integrate(tsdf, weight, bounds, cams, depths, trunc, dtype=F32, margin=None):
    """(tsdf, weight) of `dtype` after the views cams (N, 24), depths (N, H, W) have been folded into the given volumes
    (nx, ny, nz), which are not modified.  margin: also `near` (nx, ny, nz) int, the views per lattice point in which a
    test value lies within margin of its threshold (_near_threshold)."""
    T = dtype
    shape = tuple(tsdf.shape)
    d, w = np.asarray(tsdf).astype(T).reshape(-1), np.asarray(weight).astype(T).reshape(-1)
    x, y, z = lattice_xyz(shape, bounds, T)
    cams = np.asarray(cams, dtype=F32).reshape(-1, 24)
    depths = np.asarray(depths, dtype=F32)
    n, h, wd = depths.shape
    assert cams.shape[0] == n
    trunc = T(F32(trunc))
    near = np.zeros(d.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for view in range(n):
            u, v, flag, (qx, qy, qz) = project(cams[view], x, y, z, T)
            ok = (flag == 0) & (u >= 0) & (u < T(wd)) & (v >= 0) & (v < T(h))
            col = np.where(ok, np.floor(u), 0).astype(np.int64)
            row = np.where(ok, np.floor(v), 0).astype(np.int64)
            D = depths[view][row, col].astype(T)
            seen = ok & (D > 0)
            r = np.sqrt((qx * qx + qy * qy) + qz * qz)
            s = D - r
            take = seen & ~(s < -trunc)
            t = np.fmin(T(1), s / trunc)
            new = (w * d + t) / (w + T(1))
            if margin is not None:
                near += _near_threshold(u, v, flag, depths[view], seen, s, trunc, margin)
            d = np.where(take, new, d).astype(T)
            w = np.where(take, w + T(1), w).astype(T)
    out = (d.reshape(shape), w.reshape(shape))
    return out + (near.reshape(shape),) if margin is not None else out


def face_keep(vertices, faces, weight, bounds):
    """(fkeep (F,), vkeep (V,)) int32 0 / 1: hn_tsdf_face_keep."""
    V = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    weight = np.asarray(weight, dtype=F32)
    shape = weight.shape
    lo, step = I._steps(shape, bounds)
    valid = ((faces >= 0) & (faces < len(V))).all(axis=1)
    ids = np.where(valid[:, None], faces, 0)
    keep = valid.copy()
    with np.errstate(all="ignore"):
        centroid = ((V[ids[:, 0]] + V[ids[:, 1]]) + V[ids[:, 2]]) / F32(3)
        fl = np.floor((centroid - lo[None, :]) / step[None, :])
        top = np.asarray(shape, dtype=F32) - F32(2)
        cell = np.where(fl > 0, np.minimum(fl, top[None, :]), F32(0)).astype(np.int64)
    for corner in range(8):
        keep &= weight[cell[:, 0] + (corner >> 2), cell[:, 1] + ((corner >> 1) & 1), cell[:, 2] + (corner & 1)] > 0
    vkeep = np.zeros(len(V), dtype=np.int32)
    vkeep[np.unique(faces[keep])] = 1
    return keep.astype(np.int32), vkeep


def lattice(tsdf, weight):
    """The grid whose zero level set is the surface: -tsdf where something was observed, +1 (solid) elsewhere."""
    return np.where(np.asarray(weight) > 0, -np.asarray(tsdf, dtype=F32), F32(1)).astype(F32)


# ---- the closed-form sphere scene --------------------------------------------------------------------------------------------
def sphere_focal(wh):
    return 0.45 * min(wh) * np.sqrt(9.0 - 3.0 * 0.64) / (np.sqrt(3.0) * 0.8)


def sphere_cameras(wh) -> np.ndarray:
    """(24, 24) float32: 3 elevations x 8 azimuths of orbit cameras at radius 3 around the origin, up (0, -1, 0), whose image
    holds the bounds' bounding sphere within 0.9 of its smaller side."""
    return np.concatenate([HN.orbit_cameras((0.0, 0.0, 0.0), ORBIT_RADIUS, N_AZIMUTH, el, up=(0.0, -1.0, 0.0),
                                            focal=sphere_focal(wh), image_wh=wh) for el in ELEVATIONS], axis=0)


def host_rays(rec, wh) -> np.ndarray:
    """(H*W, 8) float64: the rays through the pixel centres (i + 0.5, j + 0.5) of the record (nerfies_scene.rays_f64)."""
    return NS.rays_f64(R.camera_dict(rec, wh), 0.0, 0.0)


def sphere_depth(rec, wh, radius=RADIUS, centre=(0.0, 0.0, 0.0)) -> np.ndarray:
    """(H, W) float32: the exact (float64, rounded once) distance along the unit ray of every pixel centre to the sphere,
    +inf where the ray misses it or the sphere lies behind the camera; from inside, the far intersection."""
    rays = host_rays(rec, wh)
    o, d = rays[:, 0:3] - np.asarray(centre, dtype=np.float64), rays[:, 3:6]
    b = (o * d).sum(-1)
    c = (o * o).sum(-1) - radius * radius
    disc = b * b - c
    with np.errstate(invalid="ignore"):
        root = np.sqrt(np.where(disc >= 0, disc, np.nan))
        t = np.where(-b - root > 0, -b - root, -b + root)
    t = np.where((disc >= 0) & (t > 0), t, np.inf)
    return t.reshape(wh[1], wh[0]).astype(F32)


@functools.lru_cache(maxsize=None)
def sphere_scene(wh):
    """(cams (24, 24) float32, depths (24, H, W) float32) of the sphere scene at image size wh = (W, H)."""
    cams = sphere_cameras(wh)
    depths = np.stack([sphere_depth(rec, wh) for rec in cams])
    for a in (cams, depths):
        a.setflags(write=False)
    return cams, depths


def default_trunc(shape, bounds=BOUNDS) -> float:
    """fuse_depth's default: 4 times the largest lattice spacing."""
    return 4.0 * max((bounds[2 * c + 1] - bounds[2 * c]) / (shape[c] - 1) for c in range(3))


@functools.lru_cache(maxsize=None)
def sphere_volume(res, wh, views=None, dtype=F32):
    """(tsdf, weight) restated on the res^3 lattice over BOUNDS from the sphere scene's views (None: all 24; else a tuple of
    rows), with the default trunc.  Read-only: shared among tests."""
    cams, depths = sphere_scene(wh)
    if views is not None:
        cams, depths = cams[list(views)], depths[list(views)]
    shape = (res, res, res)
    zero = np.zeros(shape, dtype=dtype)
    out = integrate(zero, zero, BOUNDS, cams, depths, default_trunc(shape), dtype)
    for a in out:
        a.setflags(write=False)
    return out


def edge_crossings(grid, weight, bounds, directions=I.DIRS):
    """Positions (float64, (n, 3)) where the linear interpolant of `grid` along the lattice edges of the given directions
    (all seven tetrahedron edge directions by default) crosses zero (ends of different `>= 0` status), and a mask of the
    crossings whose edge has a never-observed end (weight == 0)."""
    g = np.asarray(grid, dtype=np.float64)
    nx, ny, nz = g.shape
    pts = I.lattice_points(g.shape, bounds).astype(np.float64).reshape(nx, ny, nz, 3)
    inside = g >= 0
    unseen = ~(np.asarray(weight) > 0)
    out, solid = [], []
    for dx, dy, dz in np.asarray(directions).tolist():
        a = (slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))
        b = (slice(dx, nx), slice(dy, ny), slice(dz, nz))
        cut = inside[a] != inside[b]
        fa, fb = g[a][cut], g[b][cut]
        t = (0.0 - fa) / (fb - fa)
        out.append(pts[a][cut] + t[:, None] * (pts[b][cut] - pts[a][cut]))
        solid.append(unseen[a][cut] | unseen[b][cut])
    return np.concatenate(out), np.concatenate(solid)
