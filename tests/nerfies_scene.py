"""Seeded synthetic Nerfies-format captures (scene.json, dataset.json, metadata.json, camera/<id>.json,
rgb/<k>x/<id>.png, camera-paths/<name>/*.json) for the dataset tests and the g24 golden generator, with the float64
statements the tests check the kernels against:

  rays_f64     the camera model as the package documents it (pixel -> ray: intrinsics, 10 Newton steps of undistortion,
               rotation), restated in NumPy float64 with every sum written out (no BLAS: the rows are reproducible)
  project_f64  the closed-form forward model (world point -> pixel: rotate, divide, distort, intrinsics).  It shares
               no formula with the Newton iteration, so rays_f64 followed by project_f64 returning to the pixel centre
               guards the restatement itself.
"""
import json
import os

import numpy as np

NEWTON_STEPS = 10
CAMERA_PATH = "orbit"
STRONG = dict(radial=(-0.2, 0.05, 0.0), tangential=(0.01, -0.01), skew=0.3, aspect=1.02)


def _rotation(rng) -> np.ndarray:
    """A random proper rotation (QR of a Gaussian matrix, signs fixed)."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def _camera(rng, full_wh, kind: str) -> dict:
    """One camera at full resolution, as camera/<id>.json stores it.  kind: 'plain' (no distortion), 'strong', or
    'real' (HyperNeRF's magnitudes)."""
    w, h = full_wh
    cam = {
        "orientation": _rotation(rng).tolist(),
        "position": rng.uniform(-2.0, 2.0, 3).tolist(),
        "focal_length": float(0.8 * w * rng.uniform(0.95, 1.05)),
        "principal_point": [float(w / 2 + rng.uniform(-0.9, 0.9)), float(h / 2 + rng.uniform(-0.9, 0.9))],
        "image_size": [int(w), int(h)],
        "skew": 0.0,
        "pixel_aspect_ratio": 1.0,
        "radial_distortion": [0.0, 0.0, 0.0],
        "tangential_distortion": [0.0, 0.0],
    }
    if kind == "strong":
        cam.update(skew=STRONG["skew"], pixel_aspect_ratio=STRONG["aspect"],
                   radial_distortion=list(STRONG["radial"]), tangential_distortion=list(STRONG["tangential"]))
    elif kind == "real":
        cam["radial_distortion"] = [float(0.04 * rng.uniform(0.8, 1.2)), float(-0.10 * rng.uniform(0.8, 1.2)), 0.0]
        cam["tangential_distortion"] = [float(1e-3 * rng.uniform(-1, 1)), float(1e-3 * rng.uniform(-1, 1))]
    return cam


def make_scene(seed: int, wh=(24, 16), n_train: int = 5, n_val: int = 2, image_scale: int = 2) -> dict:
    """A capture as plain data (write_scene puts it on disk): `wh` is the size of the images under rgb/<image_scale>x;
    the camera files are at image_scale times that.  Every image has its own camera — a random rotation, f about
    0.8 W, a principal point off-centre by a fraction of a pixel; camera 0 has no distortion, camera 1 is the strong
    one (STRONG), the rest are near HyperNeRF's real magnitudes.  Train and val ids interleave in `ids`, and warp_id is
    a scrambled numbering, so the position of an id in any list is not its warp_id.  One camera path of 3 cameras."""
    rng = np.random.RandomState(seed)
    w, h = wh
    full_wh = (w * image_scale, h * image_scale)
    n = n_train + n_val
    ids = [f"frame_{k:03d}" for k in range(n)]
    val_pos = set(np.linspace(2, n - 1, n_val).astype(int).tolist()) if n_val else set()     # cameras 0, 1 train
    assert len(val_pos) == n_val
    train_ids = [i for k, i in enumerate(ids) if k not in val_pos]
    val_ids = [i for k, i in enumerate(ids) if k in val_pos]
    warp = rng.permutation(n) + n            # every warp_id is past every list position
    metadata = {i: {"warp_id": int(warp[k]), "appearance_id": int((k * 2) % (n + 1)), "camera_id": int(k % 2)}
                for k, i in enumerate(ids)}
    cameras = {i: _camera(rng, full_wh, ("plain", "strong")[k] if k < 2 else "real") for k, i in enumerate(ids)}
    yy, xx = np.mgrid[0:h, 0:w]
    pixels = {}
    for k, i in enumerate(ids):
        base = np.stack([xx * (255.0 / max(w - 1, 1)), yy * (255.0 / max(h - 1, 1)),
                         128 + 100 * np.sin((xx + 2 * yy + 7 * k) / 5.0)], -1)
        base[(xx // 5 + yy // 4 + k) % 2 == 0] *= 0.4
        base += rng.normal(0, 10, base.shape)
        pixels[i] = np.clip(np.round(base), 0, 255).astype(np.uint8)
    path = [_camera(rng, full_wh, ("real", "plain", "strong")[k]) for k in range(3)]
    return {"scene": {"scale": 0.37, "center": [0.4, -0.2, 1.1], "near": 0.05, "far": 1.9},
            "ids": ids, "train_ids": train_ids, "val_ids": val_ids, "metadata": metadata, "cameras": cameras,
            "pixels": pixels, "image_scale": int(image_scale), "camera_path": path}


def write_png_rgb(path: str, img: np.ndarray) -> None:
    """(H, W, 3) uint8 -> an 8-bit RGB PNG (colour type 2), standard library only, filter type 0."""
    import struct
    import zlib
    a = np.ascontiguousarray(img, dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), a.reshape(h, w * 3)], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_scene(root: str, scene: dict) -> str:
    """Write a capture in the Nerfies layout."""
    def dump(rel, obj):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(obj, f)
    dump("scene.json", scene["scene"])
    dump("dataset.json", {"count": len(scene["ids"]), "num_exemplars": len(scene["train_ids"]), "ids": scene["ids"],
                          "train_ids": scene["train_ids"], "val_ids": scene["val_ids"]})
    dump("metadata.json", scene["metadata"])
    rgb = os.path.join(root, "rgb", f"{scene['image_scale']}x")
    os.makedirs(rgb, exist_ok=True)
    for i in scene["ids"]:
        dump(os.path.join("camera", f"{i}.json"), scene["cameras"][i])
        write_png_rgb(os.path.join(rgb, f"{i}.png"), scene["pixels"][i])
    for k, cam in enumerate(scene["camera_path"]):
        dump(os.path.join("camera-paths", CAMERA_PATH, f"{k:06d}.json"), cam)
    return root


# ---- a scene as flat arrays (the g24 fixture) and back ---------------------------------------------------------------
def _camera_row(cam: dict) -> np.ndarray:
    return np.concatenate([np.ravel(cam["orientation"]), cam["position"], [cam["focal_length"]], cam["principal_point"],
                           cam["image_size"], [cam["skew"], cam["pixel_aspect_ratio"]], cam["radial_distortion"],
                           cam["tangential_distortion"]]).astype(np.float64)


def _camera_from_row(r: np.ndarray) -> dict:
    r = [float(v) for v in r]
    return {"orientation": [r[0:3], r[3:6], r[6:9]], "position": r[9:12], "focal_length": r[12],
            "principal_point": r[13:15], "image_size": [int(r[15]), int(r[16])], "skew": r[17],
            "pixel_aspect_ratio": r[18], "radial_distortion": r[19:22], "tangential_distortion": r[22:24]}


def scene_to_arrays(scene: dict) -> dict:
    ids = scene["ids"]
    return {"ids": np.array(ids), "train_ids": np.array(scene["train_ids"]), "val_ids": np.array(scene["val_ids"]),
            "metadata": np.array([[scene["metadata"][i][k] for k in ("warp_id", "appearance_id", "camera_id")]
                                  for i in ids], dtype=np.int64),
            "cameras": np.stack([_camera_row(scene["cameras"][i]) for i in ids]),
            "path_cameras": np.stack([_camera_row(c) for c in scene["camera_path"]]),
            "pixels": np.stack([scene["pixels"][i] for i in ids]),
            "scene": np.array([scene["scene"]["scale"], *scene["scene"]["center"], scene["scene"]["near"],
                               scene["scene"]["far"]], dtype=np.float64),
            "image_scale": np.int64(scene["image_scale"])}


def scene_from_arrays(a: dict) -> dict:
    ids = [str(i) for i in a["ids"]]
    sc = [float(v) for v in a["scene"]]
    return {"scene": {"scale": sc[0], "center": sc[1:4], "near": sc[4], "far": sc[5]},
            "ids": ids, "train_ids": [str(i) for i in a["train_ids"]], "val_ids": [str(i) for i in a["val_ids"]],
            "metadata": {i: {"warp_id": int(m[0]), "appearance_id": int(m[1]), "camera_id": int(m[2])}
                         for i, m in zip(ids, a["metadata"])},
            "cameras": {i: _camera_from_row(r) for i, r in zip(ids, a["cameras"])},
            "pixels": {i: np.asarray(p, dtype=np.uint8) for i, p in zip(ids, a["pixels"])},
            "image_scale": int(a["image_scale"]), "camera_path": [_camera_from_row(r) for r in a["path_cameras"]]}


# ---- the float64 statements -----------------------------------------------------------------------------------------
def scaled_camera(cam: dict, image_scale, scene: dict) -> dict:
    """A camera file's content -> the camera the loader must arrive at: scaled by 1 / image_scale, then recentred."""
    s = 1.0 / image_scale
    return {"orientation": np.asarray(cam["orientation"], dtype=np.float64),
            "position": (np.asarray(cam["position"], dtype=np.float64) - np.asarray(scene["center"])) * scene["scale"],
            "focal_length": cam["focal_length"] * s,
            "principal_point": np.asarray(cam["principal_point"], dtype=np.float64) * s,
            "image_size": tuple(int(round(v * s)) for v in cam["image_size"]),
            "skew": float(cam["skew"]), "pixel_aspect_ratio": float(cam["pixel_aspect_ratio"]),
            "radial_distortion": np.asarray(cam["radial_distortion"], dtype=np.float64),
            "tangential_distortion": np.asarray(cam["tangential_distortion"], dtype=np.float64)}


def undistort_f64(xd, yd, k, p, steps: int = NEWTON_STEPS):
    k1, k2, k3 = (float(v) for v in k)
    p1, p2 = (float(v) for v in p)
    x, y = xd.copy(), yd.copy()
    for _ in range(steps):
        r = x * x + y * y
        d = 1.0 + r * (k1 + r * (k2 + k3 * r))
        fx = d * x + 2.0 * p1 * x * y + p2 * (r + 2.0 * x * x) - xd
        fy = d * y + 2.0 * p2 * x * y + p1 * (r + 2.0 * y * y) - yd
        d_r = k1 + r * (2.0 * k2 + 3.0 * k3 * r)
        d_x, d_y = 2.0 * x * d_r, 2.0 * y * d_r
        fx_x = d + d_x * x + 2.0 * p1 * y + 6.0 * p2 * x
        fx_y = d_y * x + 2.0 * p1 * x + 2.0 * p2 * y
        fy_x = d_x * y + 2.0 * p2 * y + 2.0 * p1 * x
        fy_y = d + d_y * y + 2.0 * p2 * x + 6.0 * p1 * y
        den = fy_x * fx_y - fx_x * fy_y
        ok = np.abs(den) > 1e-9
        safe = np.where(ok, den, 1.0)
        x = x + np.where(ok, (fx * fy_y - fy * fx_y) / safe, 0.0)
        y = y + np.where(ok, (fy * fx_x - fx * fy_x) / safe, 0.0)
    return x, y


def rays_f64(cam: dict, near: float, far: float, image_id=None) -> np.ndarray:
    """(H*W, 8|9) float64 rows [o, d, near, far(, id)] of a scaled camera, pixel (col i, row j) at row j*W + i."""
    w, h = cam["image_size"]
    j, i = np.mgrid[0:h, 0:w]
    i, j = i.reshape(-1).astype(np.float64), j.reshape(-1).astype(np.float64)
    f, aspect, skew = cam["focal_length"], cam["pixel_aspect_ratio"], cam["skew"]
    cx, cy = (float(v) for v in cam["principal_point"])
    y = (j + 0.5 - cy) / (f * aspect)
    x = (i + 0.5 - cx - y * skew) / f
    if np.any(cam["radial_distortion"] != 0) or np.any(cam["tangential_distortion"] != 0):
        x, y = undistort_f64(x, y, cam["radial_distortion"], cam["tangential_distortion"])
    ln = np.sqrt(x * x + y * y + 1.0)
    lx, ly, lz = x / ln, y / ln, 1.0 / ln
    rot = cam["orientation"]
    d = np.stack([rot[0, c] * lx + rot[1, c] * ly + rot[2, c] * lz for c in range(3)], -1)
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    cols = [np.broadcast_to(cam["position"], d.shape), d, np.full((len(d), 1), float(near)),
            np.full((len(d), 1), float(far))]
    if image_id is not None:
        cols.append(np.full((len(d), 1), float(image_id)))
    return np.concatenate(cols, -1)


def project_f64(cam: dict, points: np.ndarray) -> np.ndarray:
    """World points (N, 3) -> pixel coordinates (N, 2) through the forward model: into the camera frame, perspective
    division, distortion in closed form, intrinsics."""
    local = (points - cam["position"]) @ cam["orientation"].T
    x, y = local[:, 0] / local[:, 2], local[:, 1] / local[:, 2]
    k1, k2, k3 = cam["radial_distortion"]
    p1, p2 = cam["tangential_distortion"]
    r = x * x + y * y
    radial = 1.0 + r * (k1 + r * (k2 + k3 * r))
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r + 2.0 * x * x)
    yd = y * radial + 2.0 * p2 * x * y + p1 * (r + 2.0 * y * y)
    f = cam["focal_length"]
    u = f * xd + cam["skew"] * yd + cam["principal_point"][0]
    v = f * cam["pixel_aspect_ratio"] * yd + cam["principal_point"][1]
    return np.stack([u, v], -1)


def split_cameras(scene: dict, split: str, metadata_key: str = "warp_id", test_id: int = 0):
    """[(scaled camera, id column value)] of a split, in the loader's order."""
    if split == "test":
        return [(scaled_camera(c, scene["image_scale"], scene["scene"]), test_id) for c in scene["camera_path"]]
    return [(scaled_camera(scene["cameras"][i], scene["image_scale"], scene["scene"]), scene["metadata"][i][metadata_key])
            for i in scene[f"{split}_ids"]]


def split_rays_f64(scene: dict, split: str, **kw) -> np.ndarray:
    near, far = scene["scene"]["near"], scene["scene"]["far"]
    return np.concatenate([rays_f64(c, near, far, i) for c, i in split_cameras(scene, split, **kw)], 0)
