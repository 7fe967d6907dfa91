"""The Blender (nerf_synthetic) dataset of the reference (datasets/blender.py), resident on the GPU.

`transforms_{split}.json` is read on the host (focal in float64).  The RGBA images are decoded on the host one at a
time, resized on the GPU as Pillow resizes an RGBA image — LANCZOS in premultiplied alpha, restated bit-exactly in HIP
(ops.data.resize_lanczos_rgba8) — and kept on the device as uint8 RGBA: 4 bytes per ray where the reference's fp32
`all_rays` / `all_rgbs` take 44.  The training colour is the reference's blend onto white, `rgb * a + (1 - a)` in
fp32; it is not a u8 / 255 value, so it is computed where it is consumed: by hn_blend_white_u8 for `all_rgbs` and the
val / test samples, and inside the gather launch (hn_ray_batch_rgba) for a training run fed by `RayBatcher`.
`all_rays` / `all_rgbs` are built on first access only.

The reference's class has no `include_idx` (its train.py passes one and would raise TypeError): neither has this one.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from ..ops import data as ops_data
from . import image_io
from .base import GpuRayDataset

SPLITS = ("train", "val", "test")
VAL_IMAGES = 8               # the reference validates on 8 images only ("to support <= 8 gpus")


def read_transforms(root_dir: str, split: str, img_wh):
    """transforms_{split}.json -> (meta, focal): the focal length of an 800-pixel-wide render from `camera_angle_x`,
    rescaled to img_wh, in float64 as the reference computes it (blender.py:28-31)."""
    with open(os.path.join(root_dir, f"transforms_{split}.json"), 'r') as f:
        meta = json.load(f)
    focal = 0.5 * 800 / np.tan(0.5 * meta['camera_angle_x'])
    focal *= img_wh[0] / 800
    return meta, focal


class BlenderDataset(GpuRayDataset):
    def __init__(self, root_dir: str, split: str = 'train', img_wh=(800, 800), device=None, use_pillow: bool = True):
        """The reference's constructor (datasets/blender.py:12-20).  `device` (default: the current GPU) holds the
        images and generated rays; `use_pillow=False` decodes with the package's own PNG reader even when Pillow is
        installed."""
        super().__init__(device)
        self.root_dir = root_dir
        self.split = split
        if img_wh[0] != img_wh[1]:
            raise ValueError('image width must equal image height!')
        self.img_wh = tuple(int(v) for v in img_wh)
        self.white_back = True
        self._use_pillow = use_pillow
        self.read_meta()

    def read_meta(self):
        self.meta, self.focal = read_transforms(self.root_dir, self.split, self.img_wh)
        self.near = 2.0                  # bounds, common for all scenes
        self.far = 6.0
        self.bounds = np.array([self.near, self.far])
        frames = self.meta['frames']
        self.poses = [np.array(f['transform_matrix'])[:3, :4] for f in frames]
        self.image_paths = [os.path.join(self.root_dir, f"{f['file_path']}.png") for f in frames]
        if self.split == 'train':
            self._load_train_images()

    # ---- images ----------------------------------------------------------------------------------
    def _to_device_resized(self, path: str) -> torch.Tensor:
        x = torch.from_numpy(image_io.load_rgba8(path, use_pillow=self._use_pillow)).to(self.device)
        return ops_data.resize_lanczos_rgba8(x, self.img_wh)

    def _load_train_images(self):
        """One image at a time is decoded, uploaded and resized (host memory: one decoded image, as the reference)."""
        w, h = self.img_wh
        self.rgba8 = torch.empty((len(self.image_paths), h, w, 4), dtype=torch.uint8, device=self.device)
        for k, path in enumerate(self.image_paths):
            self.rgba8[k] = self._to_device_resized(path)
        self.c2w = torch.tensor(np.stack(self.poses), dtype=torch.float32).to(self.device).contiguous()

    # ---- rays --------------------------------------------------------------------------------------
    ray_cols = 8

    def _rays_of(self, c2w: torch.Tensor) -> torch.Tensor:
        w, h = self.img_wh
        return ops_data.generate_rays(h, w, float(self.focal), c2w, near=self.near, far=self.far, ndc=False)

    def _build_all_rays(self) -> torch.Tensor:
        return torch.cat([self._rays_of(c) for c in self.c2w], 0)

    def _build_all_rgbs(self) -> torch.Tensor:
        """Every pixel blended onto white."""
        return ops_data.blend_white_u8(self.rgba8)

    @property
    def n_rays(self) -> int:
        w, h = self.img_wh
        return len(self.image_paths) * h * w

    def gather_batch(self, perm: torch.Tensor, state: torch.Tensor, rows: int, rays: torch.Tensor,
                     rgbs: torch.Tensor) -> None:
        """RayBatcher's launch: rows perm[cursor : cursor + rows] of all_rays / all_rgbs, gathered and blended from
        the RGBA stack by one launch (no NDC, 8 columns)."""
        w, h = self.img_wh
        ops_data.ray_batch_rgba(perm, state, rows, h, w, float(self.focal), self.c2w, self.rgba8, rays, rgbs,
                                near=self.near, far=self.far, ndc=False)

    def __len__(self):
        if self.split == 'train':
            return self.n_rays
        if self.split == 'val':
            return VAL_IMAGES
        return len(self.meta['frames'])

    def _index_range(self):
        return -len(self.poses), min(len(self), len(self.poses))

    def _view(self, idx):
        c2w = torch.tensor(self.poses[idx], dtype=torch.float32).to(self.device)
        rgbs, valid_mask = ops_data.blend_white_u8(self._to_device_resized(self.image_paths[idx]), with_mask=True)
        w, h = self.img_wh
        return {'rays': self._rays_of(c2w), 'rgbs': rgbs, 'c2w': c2w, 'valid_mask': valid_mask, 'hw': (h, w)}
