"""Datasets of the reference's training workflow (datasets/__init__.py), resident on the GPU.

    from hypernerf_torch_amd.datasets import dataset_dict
    train = dataset_dict['llff'](root_dir, split='train', img_wh=(504, 378))

The Blender dataset is not ported.
"""
from .batcher import RayBatcher, distributed_sampler_order, random_sampler_order
from .llff import LLFFDataset

dataset_dict = {'llff': LLFFDataset}

__all__ = ["LLFFDataset", "RayBatcher", "dataset_dict", "random_sampler_order", "distributed_sampler_order"]
