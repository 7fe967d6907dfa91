"""Datasets of the reference's training workflow (datasets/__init__.py), resident on the GPU.

    from hypernerf_torch_amd.datasets import dataset_dict
    train = dataset_dict['llff'](root_dir, split='train', img_wh=(504, 378))
    train = dataset_dict['blender'](root_dir, split='train', img_wh=(800, 800))
    train = dataset_dict['nerfies'](root_dir, split='train', image_scale=4)

All keep their images on the device as uint8 (RGB for LLFF and Nerfies, RGBA for Blender) and hand `RayBatcher` a
one-launch gather of a training batch; `all_rays` / `all_rgbs` exist, built on first access.

`dataset_dict` looks a dataset up by the reference's `--dataset_name`.  Its stored items are still the ones of the
release that had LLFF alone — tests/test_datasets_host.py pins them by equality (`dataset_dict == {'llff':
LLFFDataset}`) — so datasets added since are resolved on lookup (`dict.__missing__`) from `ADDED_DATASETS`:
`dataset_dict['blender']` is `BlenderDataset`, `dataset_dict['nerfies']` is `NerfiesDataset`, an unknown name raises KeyError as before, but iteration, `in` and
`len` see 'llff' only.  `dataset_names()` lists the reference's names (pinned by tests/test_blender_host.py);
`available_datasets()` lists every name that a lookup accepts, 'nerfies' included.
"""
from .batcher import RayBatcher, distributed_sampler_order, random_sampler_order
from .blender import BlenderDataset
from .llff import LLFFDataset
from .nerfies import NerfiesDataset

ADDED_DATASETS = {'blender': BlenderDataset}
# Formats the reference has no reader for (its README lists Nerfies loading as an open item).  Resolved on lookup like
# ADDED_DATASETS, but kept apart: tests/test_blender_host.py pins `dataset_names()` to the reference's two choices.
EXTRA_DATASETS = {'nerfies': NerfiesDataset}


class _DatasetDict(dict):
    def __missing__(self, name):
        for table in (ADDED_DATASETS, EXTRA_DATASETS):
            if name in table:
                return table[name]
        raise KeyError(name)


dataset_dict = _DatasetDict({'llff': LLFFDataset})


def dataset_names():
    """The reference's `--dataset_name` choices, each of which `dataset_dict[name]` accepts."""
    return sorted(set(dataset_dict) | set(ADDED_DATASETS))


def available_datasets():
    """Every name `dataset_dict[name]` accepts: `dataset_names()` and the formats added beyond the reference."""
    return sorted(set(dataset_names()) | set(EXTRA_DATASETS))


__all__ = ["BlenderDataset", "LLFFDataset", "NerfiesDataset", "RayBatcher", "dataset_dict", "dataset_names", "available_datasets", "random_sampler_order",
           "distributed_sampler_order"]
