"""Per-step training batches gathered on the GPU (hn_ray_batch, hn_ray_batch_rgba, hn_ray_batch_nerfies), in the order a shuffled DataLoader
reads them.

`RayBatcher(dataset, batch_size, generator=g)` reproduces `DataLoader(dataset, batch_size, shuffle=True,
generator=g)` over `dataset.all_rays` / `dataset.all_rgbs` bit for bit — without building those tensors: each batch
is gathered from the dataset's uint8 image stack and poses by one launch (the dataset's `gather_batch`) that reads a
device permutation at a device cursor and advances the cursor itself, so the launch can sit at the head of a captured
training graph
(`TrainStep(model, batcher=...)`).  The permutation is host plumbing, drawn once per epoch and copied into the
captured buffer in place.  With torch.distributed initialised the order is DistributedSampler's (shuffle=True,
drop_last=False) for this rank.

Epochs: an epoch's order is drawn when its first batch is taken (the first step, or `__iter__`), for `self.epoch`,
which then advances by one.  `set_epoch(e)` before an epoch's first step sets the epoch that step draws for (the
DistributedSampler idiom); without it the epochs count 0, 1, 2, ...  `end_epoch()` drops what is left of the current
epoch, so that the next step starts a new one.
"""
from __future__ import annotations

import math
from typing import Iterator, Optional, Tuple

import torch
import torch.distributed as dist

from .. import _lib as L


def random_sampler_order(n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """One epoch of `DataLoader(shuffle=True, generator=generator)` (torch 2.x): the random draws it makes, in its
    order — the iterator's base seed, the sampler's permutation, and the permutation RandomSampler draws (and drops)
    when the epoch runs out.  Without a generator the sampler seeds a private one from the global generator."""
    torch.empty((), dtype=torch.int64).random_(generator=generator)           # _BaseDataLoaderIter._base_seed
    if generator is None:
        g = torch.Generator()
        g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    else:
        g = generator
    perm = torch.randperm(n, generator=g)
    torch.randperm(n, generator=g)                                              # num_samples % n == 0: empty tail
    return perm


def distributed_sampler_order(n: int, rank: int, world: int, seed: int = 0, epoch: int = 0) -> torch.Tensor:
    """This rank's indices of `DistributedSampler(shuffle=True, seed=seed, drop_last=False)` at `epoch`: a
    permutation seeded by seed + epoch, padded from its head to a multiple of `world`, taken at rank::world."""
    g = torch.Generator()
    g.manual_seed(seed + epoch)
    perm = torch.randperm(n, generator=g)
    total = math.ceil(n / world) * world
    if total > n:
        reps = math.ceil((total - n) / n)
        perm = torch.cat([perm, perm.repeat(reps)[:total - n]])
    return perm[rank:total:world].clone()


class RayBatcher:
    def __init__(self, dataset, batch_size: int, generator: Optional[torch.Generator] = None, drop_last: bool = False,
                 seed: int = 0, group=None):
        """dataset: an LLFFDataset, a BlenderDataset or a NerfiesDataset of split 'train' (anything with `split`,
        `n_rays`, `ray_cols`, `device` and `gather_batch(perm, state, rows, rays, rgbs)`).  generator / drop_last:
        DataLoader's; seed: DistributedSampler's (used only with torch.distributed initialised)."""
        if getattr(dataset, 'split', None) != 'train' or not hasattr(dataset, 'gather_batch'):
            raise ValueError("RayBatcher needs a 'train' split dataset")
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.generator = generator
        self.drop_last = bool(drop_last)
        self.seed = int(seed)
        self.group = group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.n_rays = dataset.n_rays
        self.n_samples = math.ceil(self.n_rays / self.world)          # this rank's share per epoch
        if self.drop_last and self.n_samples < self.batch_size:
            raise ValueError("drop_last with fewer rays than one batch leaves no step")
        self.epoch = 0
        dev = dataset.device
        self.perm = torch.zeros(self.n_samples, dtype=torch.int64, device=dev)
        self.state = torch.zeros(3, dtype=torch.int64, device=dev)      # [cursor, arrival counter, error flag]
        self.rays = torch.empty((self.batch_size, dataset.ray_cols), dtype=torch.float32, device=dev)
        self.rgbs = torch.empty((self.batch_size, 3), dtype=torch.float32, device=dev)
        self._host_perm = None
        self.position = None           # steps taken in the current epoch (None: no epoch drawn yet)

    # ---- sizes ------------------------------------------------------------------------------------------
    @property
    def steps_per_epoch(self) -> int:
        if self.drop_last:
            return self.n_samples // self.batch_size
        return -(-self.n_samples // self.batch_size)

    def __len__(self) -> int:
        return self.steps_per_epoch

    def batch_rows(self, step: int) -> int:
        """Rays in batch `step` of an epoch (the last one is short unless drop_last)."""
        return min(self.batch_size, self.n_samples - step * self.batch_size)

    @property
    def short_rows(self) -> int:
        """Rays in the short last batch of an epoch, 0 when there is none."""
        return 0 if self.drop_last else self.n_samples % self.batch_size

    # ---- epochs -----------------------------------------------------------------------------------------
    def set_epoch(self, epoch: int) -> None:
        """The epoch the next permutation is drawn for (DistributedSampler.set_epoch; a single process draws from
        the generator and ignores it, as RandomSampler does).  Call it before the epoch's first step: an epoch whose
        order is already drawn keeps it."""
        self.epoch = int(epoch)

    def end_epoch(self) -> None:
        """Drop the rest of the current epoch: the next step draws a new order."""
        self.position = None

    def check(self) -> None:
        """Raise if a gather read outside the permutation or the dataset (its rows were written as NaN).  Reads one
        device word: a host sync."""
        if int(self.state[2].item()) != 0:
            raise L.HnError("the batch gather read past the end of the epoch's permutation or found an index outside "
                              "the dataset (the batch rows were NaN): the host's epoch bookkeeping is out of step")

    def begin_epoch(self) -> None:
        """Draw the next epoch's order and put it in the device buffer, cursor at 0.  Checks the previous epoch's
        gathers first (one host sync per epoch, none per step)."""
        self.check()
        if self.distributed:
            order = distributed_sampler_order(self.n_rays, self.rank, self.world, self.seed, self.epoch)
        else:
            order = random_sampler_order(self.n_rays, self.generator)
        self.epoch += 1
        host = order.pin_memory() if self.perm.is_cuda else order
        self.perm.copy_(host, non_blocking=True)
        self._host_perm = host            # alive until the copy has run
        self.state.zero_()
        self.position = 0

    @property
    def epoch_done(self) -> bool:
        return self.position is None or self.position >= self.steps_per_epoch

    def views(self, rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.rays[:rows], self.rgbs[:rows]

    def launch(self, rows: int) -> None:
        """Gather the next `rows` rays at the device cursor into rays[:rows] / rgbs[:rows] (graph-capturable)."""
        self.dataset.gather_batch(self.perm, self.state, rows, self.rays, self.rgbs)

    def next_rows(self) -> int:
        """Host bookkeeping of one step: start an epoch if the last one ran out, return this step's row count."""
        if self.epoch_done:
            self.begin_epoch()
        rows = self.batch_rows(self.position)
        self.position += 1
        return rows

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """One epoch, eagerly: (rays, rgbs) views of the static buffers per step, overwritten by the next step."""
        self.begin_epoch()
        for _ in range(self.steps_per_epoch):
            rows = self.next_rows()
            self.launch(rows)
            yield self.views(rows)
