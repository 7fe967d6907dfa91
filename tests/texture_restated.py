"""The texture atlas (csrc/hn_texture.hip) restated in NumPy float32, FACE BY FACE: the layout walks the
faces in their sorted order and hands out cells one after the other, the rasteriser walks the faces and scatters each
one's texels into the atlas.  The kernels go the other way (a thread per cell, a thread per texel that looks its cell
up), so the two can disagree.  Every float32 operation is one NumPy operation, in the order of the definition."""
import numpy as np

import mesh_render_restated as R

F32 = np.float32
GUTTER = 7


def face_side(V, ids, texel, min_cell, max_cell):
    """The cell side of one face: the smallest power of two s in [min_cell, max_cell] with m <= (L texel)^2, L = s - 7, m
    the largest squared edge length; max_cell when none reaches.  Ids out of range: None."""
    if min(ids) < 0 or max(ids) >= len(V):
        return None
    m = F32(0.0)
    with np.errstate(all="ignore"):
        for p, q in ((ids[0], ids[1]), (ids[1], ids[2]), (ids[2], ids[0])):
            e = V[q] - V[p]
            x = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            if x > m:
                m = x
        s = min_cell
        while s < max_cell:
            reach = F32(s - GUTTER) * F32(texel)
            if m <= reach * reach:
                return s
            s *= 2
    return max_cell


def demorton(m):
    """(x, y): x from the even bits of m, y from the odd bits."""
    x = y = 0
    bit = 0
    while m:
        x |= (m & 1) << bit
        y |= ((m >> 1) & 1) << bit
        m >>= 2
        bit += 1
    return x, y


def layout(vertices, faces, texel, min_cell=16, max_cell=256):
    """{'uv' (F, 3, 2) float32, 'size' (W_t, H_t), 'cell_start' (n, 2), 'cell_side' (n,), 'cell_face' (n, 2) int32, 'sides':
    the side of every face}; ValueError for a vertex id out of range."""
    V = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    n_faces = len(faces)
    sides = [face_side(V, [int(i) for i in faces[f]], texel, min_cell, max_cell) for f in range(n_faces)]
    if any(s is None for s in sides):
        raise ValueError("a face holds a vertex id out of range")
    order = sorted(range(n_faces), key=lambda f: (-sides[f], f))
    uv = np.zeros((n_faces, 3, 2), dtype=F32)
    starts, cell_sides, cell_faces = [], [], []
    cursor = 0                                   # the Morton index of the next cell, in min_cell x min_cell units
    k = 0
    while k < n_faces:
        f0 = order[k]
        s = sides[f0]
        f1 = order[k + 1] if k + 1 < n_faces and sides[order[k + 1]] == s else -1
        k += 1 if f1 < 0 else 2
        x, y = demorton(cursor)
        ox, oy = x * min_cell, y * min_cell
        cursor += (s // min_cell) ** 2
        starts.append((ox, oy))
        cell_sides.append(s)
        cell_faces.append((f0, f1))
        L = s - GUTTER
        uv[f0] = [(ox + 1.5, oy + 1.5), (ox + 1.5 + L, oy + 1.5), (ox + 1.5, oy + 1.5 + L)]
        if f1 >= 0:
            uv[f1] = [(ox + s - 1.5, oy + s - 1.5), (ox + s - 1.5 - L, oy + s - 1.5), (ox + s - 1.5, oy + s - 1.5 - L)]
    width = min_cell
    while (width // min_cell) ** 2 < cursor:
        width *= 2
    # half the height when every cell ends in the upper half of the square (an empty atlas keeps one cell's square)
    half = bool(starts) and width > min_cell and all(oy + s <= width // 2 for (_, oy), s in zip(starts, cell_sides))
    return {"uv": uv, "size": (width, width // 2 if half else width),
            "cell_start": np.asarray(starts, dtype=np.int32).reshape(-1, 2), "cell_side": np.asarray(cell_sides, dtype=np.int32),
            "cell_face": np.asarray(cell_faces, dtype=np.int32).reshape(-1, 2), "sides": np.asarray(sides, dtype=np.int32)}


def _unit(N):
    """N / |N| per row and whether the length is > 0."""
    with np.errstate(all="ignore"):
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        ok = length > 0
        return np.where(ok[:, None], N / length[:, None], F32(0)).astype(F32), ok


def rasterize(vertices, faces, normals, lay):
    """{'owner' (H_t, W_t) int32, 'position', 'normal' (H_t, W_t, 3) float32}: every face writes the texels of its half."""
    V = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    Nn = None if normals is None else np.asarray(normals, dtype=F32).reshape(-1, 3)
    w, h = lay["size"]
    owner = np.full((h, w), -1, dtype=np.int32)
    position = np.zeros((h, w, 3), dtype=F32)
    normal = np.zeros((h, w, 3), dtype=F32)
    for (ox, oy), s, pair in zip(lay["cell_start"].tolist(), lay["cell_side"].tolist(), lay["cell_face"].tolist()):
        jj, ii = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        L = F32(s - GUTTER)
        for half, f in enumerate(pair):
            if f < 0:
                continue
            mine = (ii + jj <= s - 2) if half == 0 else (ii + jj >= s)
            i, j = ii[mine], jj[mine]
            x, y = i.astype(F32) + F32(0.5), j.astype(F32) + F32(0.5)
            if half:
                x, y = F32(s) - x, F32(s) - y
            with np.errstate(all="ignore"):
                b1 = (x - F32(1.5)) / L
                b2 = (y - F32(1.5)) / L
                b0 = (F32(1.0) - b1) - b2
                a, b, c = (int(t) for t in faces[f])
                P = (b0[:, None] * V[a][None, :] + b1[:, None] * V[b][None, :]) + b2[:, None] * V[c][None, :]
                e1, e2 = V[b] - V[a], V[c] - V[a]
                flat, flat_ok = _unit(np.asarray(R._cross(e1, e2), dtype=F32)[None, :])
                if Nn is not None:
                    mixed = (b0[:, None] * Nn[a][None, :] + b1[:, None] * Nn[b][None, :]) + b2[:, None] * Nn[c][None, :]
                    N, ok = _unit(mixed.astype(F32))
                    N = np.where(ok[:, None], N, flat)
                else:
                    N = np.broadcast_to(flat, P.shape)
            owner[oy + j, ox + i] = f
            position[oy + j, ox + i] = P.astype(F32)
            normal[oy + j, ox + i] = N.astype(F32)
    return {"owner": owner, "position": position, "normal": normal}


def chart_uv(uv, face, bary):
    """(u, v) float32 per pixel: the barycentric mix of the face's corners, clamped to their bounding box; zeros for -1."""
    q = np.asarray(uv, dtype=F32)[np.where(face >= 0, face, 0)]               # (P, 3, 2)
    w = np.asarray(bary, dtype=F32)
    with np.errstate(all="ignore"):
        t = (w[:, 0:1] * q[:, 0] + w[:, 1:2] * q[:, 1]) + w[:, 2:3] * q[:, 2]
        lo, hi = q.min(axis=1), q.max(axis=1)
        above = np.where(t > lo, t, lo)
        return np.where(above < hi, above, hi).astype(F32)


def fetch_set(uv, face, bary):
    """(P, 4, 2) int: the texels (i, j) a bilinear fetch at chart_uv reads — (i0, j0), (i1, j0), (i0, j1), (i1, j1)."""
    t = chart_uv(uv, face, bary)
    i0 = np.floor(t[:, 0] - F32(0.5)).astype(np.int64)
    j0 = np.floor(t[:, 1] - F32(0.5)).astype(np.int64)
    return np.stack([np.stack([i0, j0], -1), np.stack([i0 + 1, j0], -1), np.stack([i0, j0 + 1], -1),
                     np.stack([i0 + 1, j0 + 1], -1)], axis=1)


def sample(uv, texture, face, bary, filter="bilinear"):
    """(P, 3) float32: the texture's colour at every pixel with a face (zeros elsewhere), before shading."""
    tex = np.asarray(texture)
    tex = tex.astype(F32) / F32(255.0) if tex.dtype == np.uint8 else tex.astype(F32)
    h, w = tex.shape[:2]
    t = chart_uv(uv, face, bary)
    with np.errstate(all="ignore"):
        if filter == "nearest":
            i = np.clip(np.floor(t[:, 0]).astype(np.int64), 0, w - 1)
            j = np.clip(np.floor(t[:, 1]).astype(np.int64), 0, h - 1)
            col = tex[j, i]
        else:
            ax, ay = t[:, 0] - F32(0.5), t[:, 1] - F32(0.5)
            fi, fj = np.floor(ax), np.floor(ay)
            fx, fy = (ax - fi)[:, None], (ay - fj)[:, None]
            i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
            i1, j1 = np.clip(i0 + 1, 0, w - 1), np.clip(j0 + 1, 0, h - 1)
            i0, j0 = np.clip(i0, 0, w - 1), np.clip(j0, 0, h - 1)
            top = tex[j0, i0] + fx * (tex[j0, i1] - tex[j0, i0])
            bot = tex[j1, i0] + fx * (tex[j1, i1] - tex[j1, i0])
            col = top + fy * (bot - top)
    return np.where((face >= 0)[:, None], col, F32(0)).astype(F32)


def shade(vertices, faces, normals, uv, texture, rays, face, bary, shading="headlight", ambient=0.3,
          background=(1.0, 1.0, 1.0), filter="bilinear"):
    """{'normal', 'rgb', 'rgb8'} as hn_tex_shade computes them: the mesh renderer's shading (mesh_render_restated.shade) of a
    per-pixel colour — its normal and headlight factor, then colour * k, the clamp and the quantiser."""
    face = np.asarray(face).reshape(-1)
    base = R.shade(vertices, faces, normals, None, rays, face, bary, shading, ambient, background, (1.0, 1.0, 1.0))
    col = sample(uv, texture, face, bary, filter)
    V, n_faces = np.asarray(vertices), np.asarray(faces).reshape(-1, 3)
    hit = (face >= 0) & (face < len(n_faces))
    ids = n_faces[np.where(hit, face, 0)] if len(n_faces) else np.zeros((len(face), 3), dtype=np.int64)
    hit &= ((ids >= 0) & (ids < len(V))).all(axis=1)
    with np.errstate(all="ignore"):
        # base colour 1: R.shade's rgb is clamp(k) — k itself, since 0 <= k <= 1 (or NaN -> 0, as x * NaN gives below)
        N = base["normal"]
        d = np.asarray(rays)[:, 3:6].astype(F32)
        k = np.ones(len(face), dtype=F32)
        if shading == "headlight":
            k = F32(ambient) + (F32(1.0) - F32(ambient)) * np.abs((N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2])
        x = col * k[:, None]
        lo = np.where(x > 0, x, F32(0))
        rgb = np.where(lo < 1, lo, F32(1)).astype(F32)
    rgb = np.where(hit[:, None], rgb, np.asarray(background, dtype=F32)[None, :]).astype(F32)
    return {"normal": N, "rgb": rgb, "rgb8": R.quantise(rgb)}
