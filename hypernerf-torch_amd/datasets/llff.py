"""The LLFF forward-facing dataset of the reference (datasets/llff.py), resident on the GPU.

Pose math runs on the host in float64 NumPy (the reference's values); images are decoded on the host, resized on the
GPU by Pillow's LANCZOS filter restated bit-exactly in HIP (ops.data.resize_lanczos_u8), and kept on the device as
uint8.  Rays are generated on the GPU (hn_generate_rays).  `all_rays` / `all_rgbs` — the reference's (N, 8|9) and
(N, 3) fp32 tensors — are built on first access only: a training run fed by `RayBatcher` gathers each batch straight
from the uint8 stack and the poses (hn_ray_batch) and never holds 36 bytes per ray.
"""
from __future__ import annotations

import glob
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from ..ops import data as ops_data
from . import image_io
from .base import GpuRayDataset, u8_to_unit

SPLITS = ("train", "val", "test")      # and any split ending in 'train' (the test path over the training poses)


# --------------------------------------------------------------------------------------------
# host pose math (float64)
# --------------------------------------------------------------------------------------------
def _unit(v: np.ndarray) -> np.ndarray:
    return v / np.linalg.norm(v)


def average_poses(poses: np.ndarray) -> np.ndarray:
    """(N, 3, 4) camera-to-world poses -> the (3, 4) average pose: centre = mean position, z = the normalised mean z
    axis, x = normalise(mean y x z), y = z x x."""
    center = poses[:, :, 3].mean(axis=0)
    z = _unit(poses[:, :, 2].mean(axis=0))
    x = _unit(np.cross(poses[:, :, 1].mean(axis=0), z))
    y = np.cross(z, x)
    return np.stack([x, y, z, center], axis=1)


def center_poses(poses: np.ndarray):
    """Express every pose in the frame of the average pose: (centred (N, 3, 4) poses, (4, 4) world-to-average)."""
    avg = np.eye(4)
    avg[:3] = average_poses(poses)
    to_avg = np.linalg.inv(avg)
    homo = np.concatenate([poses, np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (len(poses), 1, 4))], axis=1)
    return (to_avg @ homo)[:, :3], to_avg


def create_spiral_poses(radii: np.ndarray, focus_depth: float, n_poses: int = 120) -> np.ndarray:
    """Two turns of a spiral (angles 0 .. 4 pi, endpoint excluded) around the origin, each pose looking from its
    centre away from the point (0, 0, -focus_depth) with y as the up hint."""
    out = []
    for t in np.linspace(0, 4 * np.pi, n_poses + 1)[:-1]:
        c = np.array([np.cos(t), -np.sin(t), -np.sin(0.5 * t)]) * radii
        z = _unit(c - np.array([0, 0, -focus_depth]))
        x = _unit(np.cross(np.array([0, 1, 0]), z))
        out.append(np.stack([x, np.cross(z, x), z, c], axis=1))
    return np.stack(out, axis=0)


def create_spheric_poses(radius: float, n_poses: int = 120) -> np.ndarray:
    """A circle of poses around the vertical axis, tilted 36 degrees down, at distance `radius` (and lifted by
    0.9 radius)."""
    def mat(rows):
        return np.array(rows, dtype=np.float64)
    flip = mat([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    phi = -np.pi / 5
    tilt = mat([[1, 0, 0, 0], [0, np.cos(phi), -np.sin(phi), 0], [0, np.sin(phi), np.cos(phi), 0], [0, 0, 0, 1]])
    move = mat([[1, 0, 0, 0], [0, 1, 0, -0.9 * radius], [0, 0, 1, radius], [0, 0, 0, 1]])
    out = []
    for th in np.linspace(0, 2 * np.pi, n_poses + 1)[:-1]:
        turn = mat([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1]])
        out.append((flip @ (turn @ tilt @ move))[:3])
    return np.stack(out, axis=0)


def read_poses_bounds(root_dir: str, img_wh, spheric_poses: bool) -> Dict:
    """poses_bounds.npy -> the reference's host quantities (llff.py read_meta, steps 1-3): focal rescaled to img_wh,
    poses converted from "down right back" to "right up back" and centred, the val index (pose closest to the
    centre), bounds and translations scaled so that the nearest depth sits at 1/0.75, and the ray bounds."""
    pb = np.load(os.path.join(root_dir, 'poses_bounds.npy'))
    raw = pb[:, :15].reshape(-1, 3, 5)
    bounds = pb[:, -2:].copy()
    h, w, focal = raw[0, :, -1]
    if h * img_wh[0] != w * img_wh[1]:
        raise ValueError(f'You must set @img_wh to have the same aspect ratio as ({w}, {h}) !')
    focal = focal * (img_wh[0] / w)
    poses = np.concatenate([raw[..., 1:2], -raw[..., :1], raw[..., 2:4]], axis=-1)
    poses, pose_avg = center_poses(poses)
    val_idx = int(np.argmin(np.linalg.norm(poses[..., 3], axis=1)))
    scale = bounds.min() * 0.75
    bounds /= scale
    poses[..., 3] /= scale
    if spheric_poses:
        near = bounds.min()
        far = min(8 * near, bounds.max())
    else:
        near, far = 0, 1
    return {'focal': focal, 'poses': poses, 'pose_avg': pose_avg, 'bounds': bounds, 'val_idx': val_idx,
            'near': near, 'far': far, 'n_poses': len(pb)}


def render_poses(poses: np.ndarray, bounds: np.ndarray, split: str, spheric_poses: bool) -> np.ndarray:
    """The render path of the test splits: the training poses for '*train', else a spiral (radii = 90th percentile
    of |translation|, focus depth 3.5) or, for spheric scenes, a circle at 1.1 x the nearest bound."""
    if split.endswith('train'):
        return poses
    if not spheric_poses:
        return create_spiral_poses(np.percentile(np.abs(poses[..., 3]), 90, axis=0), 3.5)
    return create_spheric_poses(1.1 * bounds.min())


# --------------------------------------------------------------------------------------------
# the dataset
# --------------------------------------------------------------------------------------------
class LLFFDataset(GpuRayDataset):
    def __init__(self, root_dir: str, split: str = 'train', img_wh=(504, 378), spheric_poses: bool = False,
                 val_num: int = 1, include_idx: bool = False, device=None, use_pillow: bool = True):
        """The reference's constructor (datasets/llff.py:174-193).  `device` (default: the current GPU) holds the
        images and generated rays; `use_pillow=False` decodes with the package's own PNG reader even when Pillow is
        installed."""
        super().__init__(device)
        self.root_dir = root_dir
        self.split = split
        self.img_wh = tuple(int(v) for v in img_wh)
        self.spheric_poses = bool(spheric_poses)
        self.val_num = max(1, val_num)
        self.include_idx = bool(include_idx)
        self.white_back = False
        self._use_pillow = use_pillow
        if include_idx and split not in ('train', 'val'):
            # the reference fails here with AttributeError in __getitem__ (val_idx_list is set for 'val' only)
            raise ValueError(f"include_idx=True is not supported for split '{split}': the reference's test splits "
                             "carry no image index")
        self.read_meta()

    def read_meta(self):
        self.image_paths = sorted(glob.glob(os.path.join(self.root_dir, 'images/*')))
        self.num_instance = len(self.image_paths)
        meta = read_poses_bounds(self.root_dir, self.img_wh, self.spheric_poses)
        if self.split in ('train', 'val') and meta['n_poses'] != len(self.image_paths):
            raise ValueError('Mismatch between number of images and number of poses! Please rerun COLMAP! '
                             f"({meta['n_poses']} poses, {len(self.image_paths)} images)")
        self.focal = meta['focal']
        self.poses, self.pose_avg, self.bounds = meta['poses'], meta['pose_avg'], meta['bounds']
        self.val_idx = meta['val_idx']
        self.near, self.far = meta['near'], meta['far']
        if self.split == 'train':
            self.train_ids: List[int] = [i for i in range(len(self.image_paths)) if i != self.val_idx]
            self._load_train_images()
        elif self.split == 'val':
            self.c2w_val = self.poses[self.val_idx]
            self.image_path_val = self.image_paths[self.val_idx]
            if self.include_idx:
                self.val_idx_list = [self.val_idx]
            self._val_rgbs = None
        else:
            self.poses_test = render_poses(self.poses, self.bounds, self.split, self.spheric_poses)

    # ---- images ----------------------------------------------------------------------------------
    def _decode(self, path: str, check_aspect: bool = True) -> np.ndarray:
        img = image_io.load_rgb8(path, use_pillow=self._use_pillow)
        if check_aspect and img.shape[0] * self.img_wh[0] != img.shape[1] * self.img_wh[1]:
            raise ValueError(f'{path} has different aspect ratio than img_wh, please check your data!')
        return img

    def _to_device_resized(self, img: np.ndarray) -> torch.Tensor:
        x = torch.from_numpy(img).to(self.device)
        return ops_data.resize_lanczos_u8(x, self.img_wh)

    def _load_train_images(self):
        """Every image's aspect ratio is checked from its header before any pixel reaches the device; then one image
        at a time is decoded, uploaded and resized (host memory: one decoded image, as the reference)."""
        w, h = self.img_wh
        paths = [self.image_paths[i] for i in self.train_ids]
        for path in paths:
            iw, ih = image_io.image_size(path, use_pillow=self._use_pillow)
            if ih * w != iw * h:
                raise ValueError(f'{path} has different aspect ratio than img_wh, please check your data!')
        self.rgb8 = torch.empty((len(paths), h, w, 3), dtype=torch.uint8, device=self.device)
        for k, path in enumerate(paths):
            self.rgb8[k] = self._to_device_resized(self._decode(path))
        self.c2w = torch.tensor(self.poses[self.train_ids], dtype=torch.float32).to(self.device).contiguous()
        self.image_ids = torch.tensor(self.train_ids, dtype=torch.float32).to(self.device)

    # ---- rays --------------------------------------------------------------------------------------
    def _rays_of(self, c2w: torch.Tensor, image_id: Optional[int]) -> torch.Tensor:
        w, h = self.img_wh
        return ops_data.generate_rays(h, w, float(self.focal), c2w, near=float(self.near), far=float(self.far),
                                      ndc=not self.spheric_poses, ndc_near=1.0, image_id=image_id)

    def _build_all_rays(self) -> torch.Tensor:
        return torch.cat([self._rays_of(self.c2w[k], i if self.include_idx else None)
                          for k, i in enumerate(self.train_ids)], 0)

    @property
    def n_rays(self) -> int:
        w, h = self.img_wh
        return len(self.train_ids) * h * w

    def gather_batch(self, perm: torch.Tensor, state: torch.Tensor, rows: int, rays: torch.Tensor,
                     rgbs: torch.Tensor) -> None:
        """RayBatcher's launch: rows perm[cursor : cursor + rows] of all_rays / all_rgbs, gathered from the uint8 stack
        and the poses by one launch."""
        w, h = self.img_wh
        ops_data.ray_batch(perm, state, rows, h, w, float(self.focal), self.c2w, self.rgb8, rays, rgbs,
                           near=float(self.near), far=float(self.far), ndc=not self.spheric_poses, ndc_near=1.0,
                           image_ids=self.image_ids)

    def __len__(self):
        if self.split == 'train':
            return self.n_rays
        if self.split == 'val':
            return self.val_num
        return len(self.poses_test)

    def _view(self, idx):
        pose = self.c2w_val if self.split == 'val' else self.poses_test[idx]
        c2w = torch.tensor(pose, dtype=torch.float32).to(self.device)
        image_id = self.val_idx_list[0] if self.include_idx else None
        w, h = self.img_wh
        sample = {'rays': self._rays_of(c2w, image_id), 'c2w': c2w, 'hw': (h, w)}
        if self.split == 'val':
            if self._val_rgbs is None:
                img = self._to_device_resized(self._decode(self.image_path_val, check_aspect=False))
                self._val_rgbs = u8_to_unit(img.reshape(-1, 3))
            sample['rgbs'] = self._val_rgbs
        return sample
