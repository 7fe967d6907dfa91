"""What the GPU-resident datasets share: the device, the lazily built train-only `all_rays` / `all_rgbs`, the row width
and the indexing of `__getitem__`."""
from __future__ import annotations

import torch
from torch.utils.data import Dataset

_U8_TO_FLOAT = None


def u8_to_unit(x: torch.Tensor) -> torch.Tensor:
    """uint8 -> fp32 x / 255 rounded once (torchvision's ToTensor; a device multiply by 1/255 would differ in the last
    bit for some values): a 256-entry table divided on the host, gathered on the device."""
    global _U8_TO_FLOAT
    if _U8_TO_FLOAT is None:
        _U8_TO_FLOAT = torch.arange(256, dtype=torch.float32) / 255
    return _U8_TO_FLOAT.to(x.device)[x.long()]


class GpuRayDataset(Dataset):
    """A subclass sets `split`, `include_idx` (or a fixed `ray_cols`) and `n_rays`, and supplies `_build_all_rays()`,
    `_build_all_rgbs()` (default: `rgb8` as u8 / 255), `__len__` and `_view(idx)`, the sample of a val / test image.
    Together with the subclass's `gather_batch` this is what `RayBatcher` reads."""

    def __init__(self, device=None):
        self._device = device
        self._all_rays = self._all_rgbs = None

    @property
    def device(self) -> torch.device:
        if self._device is None:
            self._device = torch.device('cuda', torch.cuda.current_device())
        return torch.device(self._device)

    @property
    def ray_cols(self) -> int:
        return 9 if self.include_idx else 8

    def _train_only(self, name: str) -> None:
        if self.split != 'train':
            raise AttributeError(f"{name} exists for the 'train' split only (this is '{self.split}')")

    @property
    def all_rays(self) -> torch.Tensor:
        """(N_train*H*W, ray_cols) fp32 on the device, built on first access."""
        self._train_only('all_rays')
        if self._all_rays is None:
            self._all_rays = self._build_all_rays()
        return self._all_rays

    @property
    def all_rgbs(self) -> torch.Tensor:
        """(N_train*H*W, 3) fp32 in [0, 1] on the device, built on first access."""
        self._train_only('all_rgbs')
        if self._all_rgbs is None:
            self._all_rgbs = self._build_all_rgbs()
        return self._all_rgbs

    def _build_all_rgbs(self) -> torch.Tensor:
        return u8_to_unit(self.rgb8.reshape(-1, 3))

    def _index_range(self):
        return -len(self), len(self)

    def __getitem__(self, idx):
        if self.split == 'train':
            return {'rays': self.all_rays[idx], 'rgbs': self.all_rgbs[idx]}
        lo, hi = self._index_range()
        if not lo <= idx < hi:
            raise IndexError(idx)             # ends iteration (evaluate_images loops over the dataset)
        return self._view(idx)
