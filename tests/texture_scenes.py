"""Meshes shared by the texture atlas's CPU and GPU tests (test_texture_host.py, test_gpu_texture.py): name -> mesh dict of
NumPy arrays, and the texel length / cell sides each is laid out with."""
import functools

import numpy as np

import hashprng as H

F32 = np.float32
MAX_CELL = 64            # the tests' largest cell: atlases stay within 512 x 512
TEXEL = {"tetra": 0.08, "bumpy": 0.055, "bumpy_plus": 0.055, "empty": 0.055}


def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=F32) * F32(0.6)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    return v, f


def icosphere(level):
    """The icosahedron subdivided `level` times, on the unit sphere, outward winding: 20 * 4^level faces."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int32)


def _with_normals(v, f):
    """Area-weighted vertex normals in float64, rounded once (only inputs: nothing is compared against them)."""
    v64 = v.astype(np.float64)
    n = np.zeros_like(v64)
    fn = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return (n / np.where(length > 0, length, 1.0)).astype(F32)


@functools.lru_cache(maxsize=None)
def mesh(name: str) -> dict:
    """'tetra' (4 faces, no normals), 'bumpy' (the icosphere subdivided twice, every vertex scaled radially by a hashed
    factor in [0.25, 1.75]: 320 faces of very different sizes, with normals), 'bumpy_plus' (bumpy + a collinear zero-area face + a
    face longer than the largest cell reaches + a face of one vertex three times; their vertices appended), 'empty'."""
    if name == "tetra":
        v, f = tetrahedron()
        return {"vertices": v, "faces": f}
    if name == "empty":
        return {"vertices": np.zeros((0, 3), dtype=F32), "faces": np.zeros((0, 3), dtype=np.int32)}
    v, f = icosphere(2)
    scale = 0.25 + 1.5 * H.uniform01(7, "texture_bumpy", len(v)).astype(np.float64)
    v = (v * scale[:, None]).astype(F32)
    if name == "bumpy":
        return {"vertices": v, "faces": f, "normals": _with_normals(v, f)}
    if name == "bumpy_plus":
        extra = np.array([[2.0, 0.0, 0.0], [2.0, 0.5, 0.0], [2.0, 0.25, 0.0],          # collinear: zero area
                          [-2.0, -2.0, 2.0], [2.5, -2.0, 2.0], [-2.0, 2.5, 2.0]], dtype=F32)
        n = len(v)
        v = np.concatenate([v, extra])
        f = np.concatenate([f, np.array([[n, n + 1, n + 2], [n + 3, n + 4, n + 5], [n, n, n]], dtype=np.int32)])
        return {"vertices": v, "faces": f, "normals": _with_normals(v, f)}
    raise KeyError(name)


NAMES = ("tetra", "bumpy", "bumpy_plus", "empty")


def hashed_barycentrics(seed: int, n: int) -> np.ndarray:
    """(n, 3) float32 barycentric weights, uniform over the triangle, from the hash stream."""
    u = H.uniform01(seed, "texture_bary", 2 * n).reshape(n, 2)
    s = np.sqrt(u[:, 0])
    return np.stack([F32(1.0) - s, s * (F32(1.0) - u[:, 1]), s * u[:, 1]], axis=-1).astype(F32)


def smoke_tetrahedron(device) -> float:
    """Bake the tetrahedron's own positions as colours and look at it: the largest error of the rendered colour against
    0.5 + 0.5 x at the hit points (asserted below 2e-4).  One end-to-end run of atlas, rasteriser, bake and sampler."""
    import torch
    import hypernerf_torch_amd as HN
    import mesh_render_scenes as MS
    m = {k: torch.from_numpy(v).to(device) for k, v in mesh("tetra").items()}
    atlas = HN.texture_atlas(m, TEXEL["tetra"], 16, MAX_CELL)
    texture = HN.bake_texture(m, atlas, lambda p, n: (0.5 + 0.5 * p).contiguous(), dtype=torch.float32)
    cam = torch.from_numpy(MS.camera("plain", MS.WH)).to(device)
    img = HN.render_textured_mesh(m, atlas, texture, HN.camera_rays(cam, MS.WH[0], MS.WH[1], 0.0, 6.0), cam, MS.WH, shading="none")
    hit = img["face"] >= 0
    x = (img["bary"][hit][:, :, None] * m["vertices"][m["faces"][img["face"][hit].long()].long()]).sum(1)
    err = float((img["rgb"][hit] - (0.5 + 0.5 * x)).abs().max())
    assert int(hit.sum()) > 200 and err < 2e-4, (int(hit.sum()), err)
    return err
