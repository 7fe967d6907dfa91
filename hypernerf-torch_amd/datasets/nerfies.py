"""A Nerfies-format capture (the layout of every published Nerfies / HyperNeRF scene), resident on the GPU.

    root_dir/scene.json                 scale, center, near, far (near / far already in scaled scene units)
    root_dir/dataset.json               ids, train_ids, val_ids
    root_dir/metadata.json              {id: {warp_id, appearance_id, camera_id}}
    root_dir/camera/<id>.json           orientation (3 x 3, world to camera, rows), position, focal_length,
                                        principal_point, image_size [W, H], skew, pixel_aspect_ratio,
                                        radial_distortion [k1, k2, k3], tangential_distortion [p1, p2]
    root_dir/rgb/<image_scale>x/<id>.png
    root_dir/camera-paths/<name>/*.json cameras only, for novel-view rendering (optional)
    root_dir/points.npy                 (M, 3) static background points of the structure-from-motion run (optional)

Everything is read on the host with the standard library and NumPy (float64).  A camera is loaded as the Nerfies code
base loads it: scaled by 1 / image_scale (focal length and principal point multiplied, image size rounded; skew, aspect
ratio and distortion unchanged), then moved into the scene frame, position = (position - center) * scale.  Every image
has its own camera, so the device holds one record of 24 floats per image (`camera_record`) next to the uint8 image
stack, and rays are generated where they are consumed: hn_generate_rays_nerfies for `all_rays` and the val / test
samples, hn_ray_batch_nerfies inside the gather launch for a training run fed by `RayBatcher` — one device function
under both.  The ray row is [o, d, near, far, id] with the scene's near / far and id = the image's `metadata_key` entry
of metadata.json; there is no NDC and no white background.  The model is built with
`NerfModel(near=ds.near, far=ds.far, ...)` and its GLO tables are sized from `ds.num_embeddings`.

Images are not resized on load (Nerfies ships pre-scaled folders): a missing rgb/<image_scale>x is a ValueError.

`background_points` (points.npy in the scene frame, on the device) and `warp_ids` feed `losses.BackgroundLoss`,
HyperNeRF's background regularization.
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib as L
from ..ops import data as ops_data
from . import image_io
from .base import GpuRayDataset, u8_to_unit

SPLITS = ("train", "val", "test")
METADATA_KEYS = ("warp_id", "appearance_id", "camera_id")
CAM_FLOATS = L.HN_NERFIES_CAM_FLOATS    # the camera record of hn_kernels.h
_CAMERA_KEYS = ("orientation", "position", "focal_length", "principal_point", "image_size", "skew",
                "pixel_aspect_ratio", "radial_distortion", "tangential_distortion")


def _read_json(path: str):
    try:
        with open(path, 'r') as f:
            return json.load(f)
    except FileNotFoundError:
        raise ValueError(f"{path} is missing") from None
    except json.JSONDecodeError as e:
        raise ValueError(f"{path} is not valid JSON: {e}") from None


def load_camera(path: str, image_scale: float = 1, scene_center=(0.0, 0.0, 0.0), scene_scale: float = 1.0) -> Dict:
    """camera/<id>.json -> the camera at 1 / image_scale of its resolution, in the scene frame (float64):
    {'orientation' (3, 3), 'position' (3,), 'focal_length', 'principal_point' (2,), 'image_size' (W, H) ints, 'skew',
    'pixel_aspect_ratio', 'radial_distortion' (3,), 'tangential_distortion' (2,)}."""
    raw = _read_json(path)
    missing = [k for k in _CAMERA_KEYS if k not in raw]
    if missing:
        raise ValueError(f"{path}: camera keys missing: {missing}")
    s = 1.0 / image_scale
    cam = {
        'orientation': np.asarray(raw['orientation'], dtype=np.float64).reshape(3, 3),
        'position': (np.asarray(raw['position'], dtype=np.float64).reshape(3)
                     - np.asarray(scene_center, dtype=np.float64)) * float(scene_scale),
        'focal_length': float(raw['focal_length']) * s,
        'principal_point': np.asarray(raw['principal_point'], dtype=np.float64).reshape(2) * s,
        'image_size': tuple(int(round(float(v) * s)) for v in raw['image_size']),
        'skew': float(raw['skew']),
        'pixel_aspect_ratio': float(raw['pixel_aspect_ratio']),
        'radial_distortion': np.asarray(raw['radial_distortion'], dtype=np.float64).reshape(3),
        'tangential_distortion': np.asarray(raw['tangential_distortion'], dtype=np.float64).reshape(2),
    }
    if not cam['focal_length'] > 0 or not cam['pixel_aspect_ratio'] > 0 or min(cam['image_size']) <= 0:
        raise ValueError(f"{path}: focal_length, pixel_aspect_ratio and image_size must be positive")
    return cam


def camera_record(cam: Dict) -> np.ndarray:
    """A loaded camera -> the (24,) fp32 record the kernels read: orientation (9, rows), position (3), f, aspect, skew,
    cx, cy, k1, k2, k3, p1, p2, two zeros."""
    rec = np.zeros(CAM_FLOATS, dtype=np.float64)
    rec[0:9] = cam['orientation'].reshape(-1)
    rec[9:12] = cam['position']
    rec[12:15] = (cam['focal_length'], cam['pixel_aspect_ratio'], cam['skew'])
    rec[15:17] = cam['principal_point']
    rec[17:20] = cam['radial_distortion']
    rec[20:22] = cam['tangential_distortion']
    return rec.astype(np.float32)


def load_points(path: str, scene_center=(0.0, 0.0, 0.0), scene_scale: float = 1.0) -> np.ndarray:
    """points.npy -> the (M, 3) background points in the scene frame, (points - center) * scale in float64 as a camera
    position is moved, then fp32."""
    try:
        pts = np.load(path, allow_pickle=False)
    except FileNotFoundError:
        raise ValueError(f"{path} is missing") from None
    except (OSError, ValueError) as e:
        raise ValueError(f"{path} is not a readable .npy array: {e}") from None
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0 or not np.issubdtype(pts.dtype, np.number):
        raise ValueError(f"{path}: expected (M, 3) numbers with M >= 1, got {pts.shape} {pts.dtype}")
    pts = (pts.astype(np.float64) - np.asarray(scene_center, dtype=np.float64).reshape(3)) * float(scene_scale)
    return pts.astype(np.float32)


class NerfiesDataset(GpuRayDataset):
    def __init__(self, root_dir: str, split: str = 'train', image_scale: int = 4, include_idx: bool = True,
                 metadata_key: str = 'warp_id', camera_path: Optional[str] = None, test_id: int = 0, device=None,
                 use_pillow: bool = True):
        """split 'train' / 'val': the images of dataset.json's train_ids / val_ids at rgb/<image_scale>x.  split
        'test': the cameras of camera-paths/<camera_path>/ sorted by name, rays only, every row carrying `test_id`.
        metadata_key: which entry of metadata.json fills the id column ('warp_id', 'appearance_id' or 'camera_id');
        include_idx=False gives 8-column rows.  `device` (default: the current GPU) holds the images and generated
        rays; `use_pillow=False` decodes with the package's own PNG reader even when Pillow is installed."""
        if split not in SPLITS:
            raise ValueError(f"split must be one of {SPLITS} (got '{split}')")
        if metadata_key not in METADATA_KEYS:
            raise ValueError(f"metadata_key must be one of {METADATA_KEYS} (got '{metadata_key}')")
        if split == 'test' and camera_path is None:
            raise ValueError("split 'test' needs camera_path (a directory name under camera-paths/)")
        super().__init__(device)
        self.root_dir = root_dir
        self.split = split
        self.image_scale = image_scale
        self.include_idx = bool(include_idx)
        self.metadata_key = metadata_key
        self.camera_path = camera_path
        self.test_id = int(test_id)
        self.white_back = False
        self._use_pillow = use_pillow
        self.read_meta()

    # ---- host metadata ---------------------------------------------------------------------------
    def _load_camera(self, path: str) -> Dict:
        return load_camera(path, self.image_scale, self.scene_center, self.scene_scale)

    def read_meta(self):
        root = self.root_dir
        scene_path = os.path.join(root, 'scene.json')
        scene = _read_json(scene_path)
        for k in ('scale', 'center', 'near', 'far'):
            if k not in scene:
                raise ValueError(f"{scene_path}: '{k}' is missing")
        self.scene_scale = float(scene['scale'])
        self.scene_center = np.asarray(scene['center'], dtype=np.float64).reshape(3)
        self.near, self.far = float(scene['near']), float(scene['far'])
        self.bounds = np.array([self.near, self.far])

        dataset_path = os.path.join(root, 'dataset.json')
        dataset = _read_json(dataset_path)
        for k in ('ids', 'train_ids', 'val_ids'):
            if k not in dataset:
                raise ValueError(f"{dataset_path}: '{k}' is missing")
        self.all_ids: List[str] = [str(i) for i in dataset['ids']]
        self.train_ids: List[str] = [str(i) for i in dataset['train_ids']]
        self.val_ids: List[str] = [str(i) for i in dataset['val_ids']]

        metadata_path = os.path.join(root, 'metadata.json')
        self.metadata: Dict[str, Dict] = _read_json(metadata_path)
        self.num_embeddings = {}
        for name in ('warp', 'appearance', 'camera'):
            vals = [int(m[name + '_id']) for m in self.metadata.values() if name + '_id' in m]
            self.num_embeddings[name] = (max(vals) + 1) if vals else 0

        if self.split == 'test':
            cam_dir = os.path.join(root, 'camera-paths', self.camera_path)
            paths = sorted(glob.glob(os.path.join(cam_dir, '*.json')))
            if not paths:
                raise ValueError(f"{cam_dir} holds no camera (*.json)")
            self.ids = [os.path.splitext(os.path.basename(p))[0] for p in paths]
            self.camera_files = paths
            self.image_paths: List[str] = []
            self.metadata_ids = [self.test_id] * len(paths)
        else:
            self.ids = self.train_ids if self.split == 'train' else self.val_ids
            if not self.ids:
                raise ValueError(f"{dataset_path}: '{self.split}_ids' is empty")
            self.metadata_ids = []
            for i in self.ids:
                if i not in self.metadata or self.metadata_key not in self.metadata[i]:
                    raise ValueError(f"{metadata_path} has no '{self.metadata_key}' for id '{i}' of {self.split}_ids")
                self.metadata_ids.append(int(self.metadata[i][self.metadata_key]))
            self.camera_files = [os.path.join(root, 'camera', f'{i}.json') for i in self.ids]
            rgb_dir = os.path.join(root, 'rgb', f'{self.image_scale}x')
            if not os.path.isdir(rgb_dir):
                raise ValueError(f"{rgb_dir} is missing: images are not resized on load (Nerfies ships one folder per "
                                 "scale)")
            self.image_paths = [os.path.join(rgb_dir, f'{i}.png') for i in self.ids]
        self.cameras = [self._load_camera(p) for p in self.camera_files]
        self.img_wh = self.cameras[0]['image_size']
        for path, cam in zip(self.camera_files, self.cameras):
            if cam['image_size'] != self.img_wh:
                raise ValueError(f"{path}: image_size {cam['image_size']} differs from {self.img_wh} of "
                                 f"{self.camera_files[0]}: all cameras of one split must share one image size")
        # every image's header against its camera, before any pixel reaches the device
        for path in self.image_paths:
            if not os.path.isfile(path):
                raise ValueError(f"{path} is missing")
            size = tuple(int(v) for v in image_io.image_size(path, use_pillow=self._use_pillow))
            if size != self.img_wh:
                raise ValueError(f"{path} is {size[0]} x {size[1]}, its camera at 1/{self.image_scale} scale says "
                                 f"{self.img_wh[0]} x {self.img_wh[1]}")
        self.camera_table = np.stack([camera_record(c) for c in self.cameras])
        if self.split == 'train':
            self._load_train_images()

    # ---- background regularization -------------------------------------------------------------------
    @property
    def background_points(self) -> torch.Tensor:
        """(M, 3) fp32 on the dataset's device: root_dir/points.npy in the scene frame (`load_points`), read on first
        use."""
        pts = getattr(self, '_background_points', None)
        if pts is None:
            host = load_points(os.path.join(self.root_dir, 'points.npy'), self.scene_center, self.scene_scale)
            pts = self._background_points = torch.from_numpy(host).to(self.device).contiguous()
        return pts

    @property
    def warp_ids(self) -> List[int]:
        """The sorted distinct warp_id values of dataset.json's train_ids."""
        missing = [i for i in self.train_ids if i not in self.metadata or 'warp_id' not in self.metadata[i]]
        if missing:
            raise ValueError(f"{os.path.join(self.root_dir, 'metadata.json')} has no 'warp_id' for id '{missing[0]}' "
                             "of train_ids")
        return sorted({int(self.metadata[i]['warp_id']) for i in self.train_ids})

    # ---- images ----------------------------------------------------------------------------------
    def _decode(self, path: str) -> torch.Tensor:
        img = image_io.load_rgb8(path, use_pillow=self._use_pillow)
        if img.shape[1::-1] != self.img_wh:
            raise ValueError(f"{path} decodes to {img.shape[1]} x {img.shape[0]}, its camera says "
                             f"{self.img_wh[0]} x {self.img_wh[1]}")
        return torch.from_numpy(img).to(self.device)

    def _load_train_images(self):
        """One image at a time is decoded and uploaded (host memory: one decoded image)."""
        w, h = self.img_wh
        self.rgb8 = torch.empty((len(self.image_paths), h, w, 3), dtype=torch.uint8, device=self.device)
        for k, path in enumerate(self.image_paths):
            self.rgb8[k] = self._decode(path)
        self.cams = torch.from_numpy(self.camera_table).to(self.device).contiguous()
        self.c2w = self.cams
        self.image_ids = torch.tensor(self.metadata_ids, dtype=torch.float32).to(self.device)

    # ---- rays --------------------------------------------------------------------------------------
    def camera_record(self, idx: int) -> torch.Tensor:
        """The (24,) fp32 camera record of image `idx` of this split, on the dataset's device: the camera the rays of
        that image come from, as geometry.render_mesh takes it."""
        return torch.from_numpy(self.camera_table[idx]).to(self.device)

    def _rays_of(self, cam: torch.Tensor, image_id: int) -> torch.Tensor:
        w, h = self.img_wh
        return ops_data.generate_rays_nerfies(h, w, cam, near=self.near, far=self.far,
                                              image_id=image_id if self.include_idx else None)

    def _build_all_rays(self) -> torch.Tensor:
        return torch.cat([self._rays_of(self.cams[k], i) for k, i in enumerate(self.metadata_ids)], 0)

    @property
    def n_rays(self) -> int:
        w, h = self.img_wh
        return len(self.ids) * h * w

    def gather_batch(self, perm: torch.Tensor, state: torch.Tensor, rows: int, rays: torch.Tensor,
                     rgbs: torch.Tensor) -> None:
        """RayBatcher's launch: rows perm[cursor : cursor + rows] of all_rays / all_rgbs, gathered from the uint8 stack
        and the camera table by one launch."""
        w, h = self.img_wh
        ops_data.ray_batch_nerfies(perm, state, rows, h, w, self.cams, self.rgb8, rays, rgbs, near=self.near,
                                   far=self.far, image_ids=self.image_ids)

    def __len__(self):
        return self.n_rays if self.split == 'train' else len(self.ids)

    def _view(self, idx):
        cam = torch.from_numpy(self.camera_table[idx]).to(self.device)
        w, h = self.img_wh
        sample = {'rays': self._rays_of(cam, self.metadata_ids[idx]), 'camera': cam, 'hw': (h, w)}
        if self.split == 'val':
            sample['rgbs'] = u8_to_unit(self._decode(self.image_paths[idx]).reshape(-1, 3))
        return sample
