"""The mesh renderer's definition (csrc/hn_mesh_render.hip) restated in NumPy:

  cast          the ray caster, operation by operation in the order the definition writes them.  With dtype float32 every
                operation is one correctly rounded fp32 operation (NumPy rounds every elementwise operation on its own), and
                the kernel must give the same bits; with dtype float64 it is the brute-force caster of the same rule the
                fp32 statement is checked against, and it can report which pixels are ambiguous.
  shade         the shading, in float32.
  project       the forward camera model of a 24-float record in float64 (the closed form of the system the ray generator
                inverts by Newton steps), and camera_dict, which turns a record into tests/nerfies_scene.py's camera.
  record        a 24-float record from plain numbers.
"""
import numpy as np

F32 = np.float32
BLOCK = 64           # faces per vectorised block: a (pixels, BLOCK) slab per intermediate


def record(position, f, cx, cy, orientation=None, aspect=1.0, skew=0.0, k=(0.0, 0.0, 0.0), p=(0.0, 0.0)):
    rec = np.zeros(24, dtype=np.float64)
    rec[0:9] = np.eye(3).reshape(-1) if orientation is None else np.asarray(orientation, dtype=np.float64).reshape(-1)
    rec[9:12] = position
    rec[12:17] = (f, aspect, skew, cx, cy)
    rec[17:20] = k
    rec[20:22] = p
    return rec.astype(np.float32)


def camera_dict(rec, wh):
    """A record as the camera dict of tests/nerfies_scene.py (rays_f64, project_f64), in float64."""
    r = np.asarray(rec, dtype=np.float64)
    return {"orientation": r[0:9].reshape(3, 3), "position": r[9:12], "focal_length": float(r[12]),
            "pixel_aspect_ratio": float(r[13]), "skew": float(r[14]), "principal_point": r[15:17],
            "radial_distortion": r[17:20], "tangential_distortion": r[20:22], "image_size": (int(wh[0]), int(wh[1]))}


def project(rec, points):
    """World points (N, 3) -> (pixel coordinates (N, 2), z in the camera frame (N,)), float64."""
    r = np.asarray(rec, dtype=np.float64)
    local = (np.asarray(points, dtype=np.float64) - r[9:12]) @ r[0:9].reshape(3, 3).T
    z = local[:, 2]
    with np.errstate(all="ignore"):
        x, y = local[:, 0] / z, local[:, 1] / z
        k1, k2, k3, p1, p2 = r[17:22]
        rr = x * x + y * y
        radial = 1.0 + rr * (k1 + rr * (k2 + k3 * rr))
        xd = x * radial + 2.0 * p1 * x * y + p2 * (rr + 2.0 * x * x)
        yd = y * radial + 2.0 * p2 * x * y + p1 * (rr + 2.0 * y * y)
        u = r[12] * xd + r[14] * yd + r[15]
        v = r[12] * r[13] * yd + r[16]
    return np.stack([u, v], -1), z


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _edge(d, P, Q, ip, iq):
    """The value of the directed edge P -> Q in canonical order: (pixels, faces); ip, iq: (faces,)."""
    fwd = _dot(d, _cross(P, Q))
    bwd = -_dot(d, _cross(Q, P))
    return np.where((ip < iq)[None, :], fwd, bwd)


def cast(vertices, faces, rays, dtype=np.float32, margin=None):
    """{'face': (P,) int32, 'depth': (P,) dtype, 'bary': (P, 3) dtype} of rays (P, >= 6): the definition, brute force.
    margin (float64 use): also 'ambiguous' (P,) bool — for some face the ray crosses at t > 0, with the edge values
    divided by the sum of their magnitudes, the ray is inside or within `margin` of the face AND the smallest magnitude is
    below `margin`."""
    V = np.asarray(vertices).astype(dtype)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    rays = np.asarray(rays)
    n_pix = rays.shape[0]
    o = [rays[:, c].astype(dtype)[:, None] for c in range(3)]
    d = [rays[:, 3 + c].astype(dtype)[:, None] for c in range(3)]
    best_t = np.full(n_pix, np.inf, dtype=dtype)
    best_f = np.full(n_pix, -1, dtype=np.int32)
    best_e = np.zeros((n_pix, 3), dtype=dtype)
    ambiguous = np.zeros(n_pix, dtype=bool)
    rows = np.arange(n_pix)
    with np.errstate(all="ignore"):
        for start in range(0, faces.shape[0], BLOCK):
            ids = faces[start:start + BLOCK]
            ia, ib, ic = ids[:, 0], ids[:, 1], ids[:, 2]
            ok = (ia >= 0) & (ib >= 0) & (ic >= 0) & (ia < len(V)) & (ib < len(V)) & (ic < len(V))
            distinct = ok & (ia != ib) & (ib != ic) & (ia != ic)
            sa, sb, sc = (np.where(ok, i, 0) for i in (ia, ib, ic))
            va, vb, vc = ([V[s, c][None, :] for c in range(3)] for s in (sa, sb, sc))
            A = [va[c] - o[c] for c in range(3)]
            B = [vb[c] - o[c] for c in range(3)]
            Cc = [vc[c] - o[c] for c in range(3)]
            ea, eb, ec = _edge(d, B, Cc, ib, ic), _edge(d, Cc, A, ic, ia), _edge(d, A, B, ia, ib)
            inside = (((ea >= 0) & (eb >= 0) & (ec >= 0)) | ((ea <= 0) & (eb <= 0) & (ec <= 0))) & \
                ~((ea == 0) & (eb == 0) & (ec == 0))
            n = _cross([vb[c] - va[c] for c in range(3)], [vc[c] - va[c] for c in range(3)])
            den, num = _dot(d, n), _dot(A, n)
            t = num / den
            crossed = distinct[None, :] & (den != 0) & (t > 0) & (t < np.inf)
            hit = inside & crossed
            if margin is not None:
                total = (np.abs(ea) + np.abs(eb)) + np.abs(ec)
                na, nb, nc = ea / total, eb / total, ec / total
                lo, hi = np.minimum(np.minimum(na, nb), nc), np.maximum(np.maximum(na, nb), nc)
                near = np.maximum(lo, -hi) >= -margin            # inside (>= 0) or within margin of it, either winding
                small = np.minimum(np.minimum(np.abs(na), np.abs(nb)), np.abs(nc)) < margin
                ambiguous |= (crossed & near & small).any(axis=1)
            tt = np.where(hit, t, np.inf).astype(dtype)
            k = np.argmin(tt, axis=1)                        # the first minimum: the smallest face id of the block
            tk = tt[rows, k]
            better = tk < best_t                             # strictly: an equal t keeps the earlier, smaller id
            best_t = np.where(better, tk, best_t)
            best_f = np.where(better, (start + k).astype(np.int32), best_f)
            for c, e in enumerate((ea, eb, ec)):
                best_e[:, c] = np.where(better, e[rows, k], best_e[:, c])
        got = best_f >= 0
        s = (best_e[:, 0] + best_e[:, 1]) + best_e[:, 2]
        bary = np.where(got[:, None], best_e / s[:, None], 0).astype(dtype)
    out = {"face": best_f, "depth": np.where(got, best_t, 0).astype(dtype), "bary": bary}
    if margin is not None:
        out["ambiguous"] = ambiguous
    return out


def quantise(rgb):
    """rgb8 = floor(255 rgb + 0.5), in float32."""
    rgb = np.asarray(rgb, dtype=F32)
    return np.floor(F32(255.0) * rgb + F32(0.5)).astype(np.uint8)


def shade(vertices, faces, normals, colors, rays, face, bary, shading="headlight", ambient=0.3, background=(1.0, 1.0, 1.0),
          base_color=(0.8, 0.8, 0.8)):
    """{'normal', 'rgb' (float32), 'rgb8'} of (P,) face / (P, 3) bary, as hn_mesh_shade computes them."""
    V = np.asarray(vertices, dtype=F32)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    face = np.asarray(face).reshape(-1)
    w = np.asarray(bary, dtype=F32).reshape(-1, 3)
    d = np.asarray(rays)[:, 3:6].astype(F32)
    n_pix = face.shape[0]
    hit = (face >= 0) & (face < faces.shape[0])
    ids = faces[np.where(hit, face, 0)] if faces.shape[0] else np.zeros((n_pix, 3), dtype=np.int64)
    hit &= ((ids >= 0) & (ids < len(V))).all(axis=1)
    ids = np.where(hit[:, None], ids, 0)
    if len(V) == 0:
        V = np.zeros((1, 3), dtype=F32)
    ambient = F32(ambient)
    with np.errstate(all="ignore"):
        if normals is not None:
            Nn = np.asarray(normals, dtype=F32)
            Nn = Nn if len(Nn) else np.zeros((1, 3), dtype=F32)
            N = (w[:, 0:1] * Nn[ids[:, 0]] + w[:, 1:2] * Nn[ids[:, 1]]) + w[:, 2:3] * Nn[ids[:, 2]]
        else:
            e1, e2 = V[ids[:, 1]] - V[ids[:, 0]], V[ids[:, 2]] - V[ids[:, 0]]
            N = np.stack(_cross(e1.T, e2.T), -1)
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        N = np.where((length > 0)[:, None], N / length[:, None], F32(0)).astype(F32)
        k = np.ones(n_pix, dtype=F32)
        if shading == "headlight":
            k = ambient + (F32(1.0) - ambient) * np.abs((N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2])
        if colors is None:
            col = np.broadcast_to(np.asarray(base_color, dtype=F32), (n_pix, 3))
        else:
            cc = np.asarray(colors)
            cc = cc.astype(F32) / F32(255.0) if cc.dtype == np.uint8 else cc.astype(F32)
            cc = cc if len(cc) else np.zeros((1, 3), dtype=F32)
            col = (w[:, 0:1] * cc[ids[:, 0]] + w[:, 1:2] * cc[ids[:, 1]]) + w[:, 2:3] * cc[ids[:, 2]]
        x = col * k[:, None]
        lo = np.where(x > 0, x, F32(0))
        rgb = np.where(lo < 1, lo, F32(1)).astype(F32)
    rgb = np.where(hit[:, None], rgb, np.asarray(background, dtype=F32)[None, :]).astype(F32)
    N = np.where(hit[:, None], N, F32(0)).astype(F32)
    return {"normal": N, "rgb": rgb, "rgb8": quantise(rgb)}
