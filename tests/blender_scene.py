"""Seeded synthetic Blender (nerf_synthetic) scenes — transforms_{train,val,test}.json + RGBA PNGs — for the dataset
tests and the g23 golden generator."""
import json
import os
import struct
import zlib

import numpy as np

SPLIT_FRAMES = (("train", 5), ("val", 8), ("test", 3))
CAMERA_ANGLE_X = 0.6911112070083618          # nerf_synthetic's value


def _look_at_origin(center: np.ndarray) -> np.ndarray:
    """A 4 x 4 camera-to-world matrix at `center` looking at the origin (camera looks down -z, z up in the world)."""
    z = center / np.linalg.norm(center)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, :3] = np.stack([x, np.cross(z, x), z], axis=1)
    m[:3, 3] = center
    return m


def make_scene(seed: int = 23, size: int = 64, frames=SPLIT_FRAMES):
    """{split: (pixels (n, size, size, 4) uint8, poses (n, 4, 4) float64)}: cameras on a jittered sphere of radius 4
    around the origin; images of coloured 8 x 8 blocks over a gradient with an object-like alpha — an opaque disc, a
    soft edge 12 pixels wide, a fully transparent surround — whose centre is jittered by +-4 pixels.  The colour is
    non-zero everywhere, under alpha == 0 too: a resize must not leak it into the visible pixels."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    scale = size / 64.0
    out = {}
    for split, n in frames:
        pix = np.empty((n, size, size, 4), dtype=np.uint8)
        poses = np.empty((n, 4, 4))
        for k in range(n):
            th, ph = rng.uniform(0, 2 * np.pi), rng.uniform(0.15, 1.2)
            c = (4.0 + rng.normal(0, 0.05)) * np.array([np.cos(th) * np.cos(ph), np.sin(th) * np.cos(ph), np.sin(ph)])
            poses[k] = _look_at_origin(c)
            blocks = rng.randint(30, 256, (-(-size // 8), -(-size // 8), 3))
            base = np.kron(blocks, np.ones((8, 8, 1)))[:size, :size] * 0.8
            base += np.stack([xx, yy, (xx + 2 * yy) % 50], -1) * (50.0 / size)
            cy, cx = size / 2 + rng.randint(-4, 5) * scale, size / 2 + rng.randint(-4, 5) * scale
            r = np.hypot(yy - cy, xx - cx) / scale
            pix[k, ..., :3] = np.clip(np.round(base), 1, 255)
            pix[k, ..., 3] = (np.clip((26 - r) / 12, 0, 1) * 255).astype(np.uint8)
        out[split] = (pix, poses)
    return out


def write_png_rgba(path: str, img: np.ndarray) -> None:
    """(H, W, 4) uint8 -> an 8-bit RGBA PNG (colour type 6), standard library only, filter type 0."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 4
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), a.reshape(h, w * 4)], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_scene(root: str, scene) -> str:
    """Write a scene in nerf_synthetic layout: transforms_<split>.json and <split>/r_<k>.png."""
    for split, (pix, poses) in scene.items():
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for k, (img, pose) in enumerate(zip(pix, poses)):
            write_png_rgba(os.path.join(root, split, f"r_{k}.png"), img)
            frames.append({"file_path": f"./{split}/r_{k}", "rotation": 0.012566370614359171,
                           "transform_matrix": [[float(v) for v in row] for row in pose]})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": CAMERA_ANGLE_X, "frames": frames}, f)
    return root
