"""Seeded synthetic LLFF scenes (forward-facing rig, poses_bounds.npy + images/*.png) for the dataset tests and the
g22 golden generator."""
import os

import numpy as np


def make_scene(n_images: int = 6, h: int = 60, w: int = 80, seed: int = 22, focal: float = 70.0):
    """(pixels (n, h, w, 3) uint8, poses_bounds (n, 17) float64): cameras on a jittered 3 x 2 grid looking down -z
    (LLFF stores the rotation as "down right back"), bounds jittered around [2, 6], images of smooth gradients with
    sharp edges and noise (so that a resize exercises negative filter lobes and clamping)."""
    rng = np.random.RandomState(seed)
    pb = np.zeros((n_images, 17))
    for k in range(n_images):
        ax, ay = rng.normal(0, 0.05, 2)
        cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
        rot = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        t = np.array([0.3 * (k % 3) - 0.3, 0.25 * (k // 3) - 0.1, 0.0]) + rng.normal(0, 0.03, 3)
        x, y, z = rot[:, 0], rot[:, 1], rot[:, 2]
        llff = np.stack([-y, x, z, t, np.array([h, w, focal])], axis=1)       # (3, 5): down, right, back, t, hwf
        pb[k, :15] = llff.reshape(-1)
        pb[k, 15:] = [2.0 + rng.uniform(-0.3, 0.3), 6.0 + rng.uniform(-1.0, 1.0)]
    yy, xx = np.mgrid[0:h, 0:w]
    pix = np.empty((n_images, h, w, 3), dtype=np.uint8)
    for k in range(n_images):
        base = np.stack([xx * (255.0 / max(w - 1, 1)), yy * (255.0 / max(h - 1, 1)),
                         128 + 100 * np.sin((xx + 2 * yy + 7 * k) / 5.0)], -1)
        base[(xx // 9 + yy // 7 + k) % 2 == 0] *= 0.35
        base += rng.normal(0, 12, base.shape)
        base[h // 3:h // 3 + 3] = 255
        pix[k] = np.clip(np.round(base), 0, 255).astype(np.uint8)
    return pix, pb


def write_scene(root: str, pixels: np.ndarray, poses_bounds: np.ndarray) -> str:
    """Write a scene in LLFF layout (lossless PNGs through the package's write_png)."""
    from hypernerf_torch_amd.inference import write_png
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    for k, img in enumerate(pixels):
        write_png(os.path.join(root, "images", f"img_{k:03d}.png"), img)
    np.save(os.path.join(root, "poses_bounds.npy"), poses_bounds)
    return root
