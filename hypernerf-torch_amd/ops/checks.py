"""Argument validators that more than one ops module, or geometry.py, uses.  Each returns its argument as the kernels
take it (detached, contiguous) or raises ValueError naming the caller (`what`)."""
from __future__ import annotations

import torch

from .data import NERFIES_CAM_FLOATS

__all__ = ["INT32_MAX", "float3", "check_points", "check_faces", "check_mesh_faces", "check_camera", "check_rays"]

INT32_MAX = 2 ** 31 - 1


def float3(x, what: str):
    try:
        seq = x.tolist() if hasattr(x, "tolist") else x
        vals = [float(v) for v in seq] if isinstance(seq, (list, tuple)) else [float(seq)] * 3
    except (TypeError, ValueError):
        vals = []
    if len(vals) != 3:
        raise ValueError(f"{what} must be a number or three numbers, got {x!r}")
    return vals


def check_points(t, what: str, name: str, rows=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: {name} must be a (V, 3) tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if rows is not None and t.shape[0] != rows:
        raise ValueError(f"{what}: {t.shape[0]} {name} for {rows} vertices")
    return t.detach().contiguous()


def check_faces(faces, num_vertices, what: str):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be a (F, 3) tensor")
    if faces.dtype != torch.int32:
        raise ValueError(f"{what}: faces must be int32, got {faces.dtype}")
    v = int(num_vertices)
    if v < 0 or v > INT32_MAX or faces.shape[0] > INT32_MAX:
        raise ValueError(f"{what}: {v} vertices / {faces.shape[0]} faces outside 0 .. 2**31 - 1 = {INT32_MAX}")
    if not faces.is_cuda:
        raise ValueError(f"{what}: faces must live on the GPU (there is no CPU fallback)")
    return faces.detach().contiguous(), v


def check_mesh_faces(faces, what: str) -> torch.Tensor:
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{what}: faces must be a (F, 3) int32 tensor")
    return faces.detach().contiguous()


def check_camera(camera, what: str) -> torch.Tensor:
    if not isinstance(camera, torch.Tensor) and hasattr(camera, "__array__"):
        camera = torch.as_tensor(camera)
    if (not isinstance(camera, torch.Tensor) or tuple(camera.shape) != (NERFIES_CAM_FLOATS,)
            or camera.dtype != torch.float32):
        raise ValueError(f"{what}: camera must be a ({NERFIES_CAM_FLOATS},) float32 record")
    return camera.detach().contiguous()


def check_rays(rays, n_pixels: int, what: str) -> torch.Tensor:
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] < 6 or rays.dtype != torch.float32:
        raise ValueError(f"{what}: rays must be a (H*W, >= 6) float32 tensor")
    if rays.shape[0] != n_pixels:
        raise ValueError(f"{what}: {rays.shape[0]} rays for an image of {n_pixels} pixels")
    return rays.detach().contiguous()
