"""Datasets of the reference's training workflow (datasets/__init__.py), resident on the GPU.

    from hypernerf_torch_amd.datasets import dataset_dict
    train = dataset_dict['llff'](root_dir, split='train', img_wh=(504, 378))
    train = dataset_dict['blender'](root_dir, split='train', img_wh=(800, 800))

Both keep their images on the device as uint8 (RGB for LLFF, RGBA for Blender) and hand `RayBatcher` a one-launch
gather of a training batch; `all_rays` / `all_rgbs` exist, built on first access.

`dataset_dict` looks a dataset up by the reference's `--dataset_name`.  Its stored items are still the ones of the
release that had LLFF alone — tests/test_datasets_host.py pins them by equality (`dataset_dict == {'llff':
LLFFDataset}`) — so datasets added since are resolved on lookup (`dict.__missing__`) from `ADDED_DATASETS`:
`dataset_dict['blender']` is `BlenderDataset`, an unknown name raises KeyError as before, but iteration, `in` and
`len` see 'llff' only.  `dataset_names()` lists every name that a lookup accepts.
"""
from .batcher import RayBatcher, distributed_sampler_order, random_sampler_order
from .blender import BlenderDataset
from .llff import LLFFDataset

ADDED_DATASETS = {'blender': BlenderDataset}


class _DatasetDict(dict):
    def __missing__(self, name):
        try:
            return ADDED_DATASETS[name]
        except KeyError:
            raise KeyError(name) from None


dataset_dict = _DatasetDict({'llff': LLFFDataset})


def dataset_names():
    """Every name `dataset_dict[name]` accepts (the reference's `--dataset_name` choices)."""
    return sorted(set(dataset_dict) | set(ADDED_DATASETS))


__all__ = ["BlenderDataset", "LLFFDataset", "RayBatcher", "dataset_dict", "dataset_names", "random_sampler_order",
           "distributed_sampler_order"]
