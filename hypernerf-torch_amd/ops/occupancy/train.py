"""Occupancy grids for the training step: TrainOccupancy owns an OccupancyStack, rebuilds its grids from
the field on a schedule between the replays of a captured step, and clips a step's rays against them (clip_batch) into
buffers that stay fixed under a graph.  `training.TrainStep(occupancy=TrainOccupancy(...))` drives it."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ..mesh import check_lattice
from . import (CLIP_BATCH_KEYS, OccupancyStack, _check_bounds, _check_cells, _check_dilate, _check_ids, _check_sigma_min,
               _resolution, check_occupancy, clip_batch, occupancy_grid)

__all__ = ["TrainOccupancy"]


def _count(value, name: str, least: int, what: str) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or value < least:
        raise ValueError(f"{what}: {name} must be an int >= {least}, got {value!r}")
    return value


class TrainOccupancy:
    """Occupancy grids for the training step: `TrainStep(..., occupancy=TrainOccupancy(...))` clips every
    ray of a step to the occupied cells of ITS frame's grid — ONE hn_occ_clip_batch launch at the head of the captured
    step — and renders the clipped rows with the original directions as view directions, so the model spends its samples
    where the field is; the grids are rebuilt from the field between replays, on a schedule.

    The grids live in an ops.occupancy.OccupancyStack over the cells of a lattice of `resolution` points over `bounds`;
    `ids` are the frame ids that get one (shared=True: ONE grid for all of them, the union over the frames).  A ray of
    any other id is not clipped.  builder(frame_id) -> occupancy dict is, by default,
    occupancy_grid(model, bounds, resolution, frame_id, sigma_min, dilate, level, chunk).
    clip_far=None means `not model.use_sample_at_infinity`: a model trained with the sample at infinity needs its far end
    (DESIGN.md 3.18), and the front-only clip ends each ray's walk at the first occupied cell.

    Schedule, with k the number of steps begun so far: before step k the grids are refreshed iff k >= warmup_steps and
    (k - warmup_steps) % refresh_every == 0.  A refresh builds the next `frames_per_refresh` ids in ascending order,
    round robin.  Per frame: stack.set(id, builder(id)); a frame not yet visited stays all-occupied.  Shared: every
    fresh grid is ORed into a pending grid, and when the round wraps the pending grid becomes the live one and is
    cleared; until the first wrap the live grid is all-occupied.  An all-occupied grid whose box holds a ray's
    [near, far] segment leaves the row's bits as they are, so the warm-up trains exactly as without the keyword."""

    def __init__(self, model, bounds, resolution, ids, sigma_min: float, dilate: int = 1, shared: bool = False,
                 warmup_steps: int = 256, refresh_every: int = 16, frames_per_refresh: int = 1,
                 clip_far: Optional[bool] = None, min_span: Optional[float] = None, level: str = 'fine',
                 chunk: int = 1 << 20, builder=None, device=None):
        what = "TrainOccupancy"
        shape, bounds = check_lattice(_resolution(resolution), bounds, what)
        cells = _check_cells(tuple(n - 1 for n in shape), what)
        bounds = _check_bounds(cells, bounds, what)
        ids = _check_ids(ids, what)
        self.sigma_min = _check_sigma_min(sigma_min, what)
        self.dilate = _check_dilate(dilate, what)
        self.warmup_steps = _count(warmup_steps, "warmup_steps", 0, what)
        self.refresh_every = _count(refresh_every, "refresh_every", 1, what)
        self.frames_per_refresh = _count(frames_per_refresh, "frames_per_refresh", 1, what)
        if level not in ('coarse', 'fine'):
            raise ValueError(f"{what}: level must be 'coarse' or 'fine', got {level!r}")
        if int(chunk) < 1:
            raise ValueError(f"{what}: chunk must be positive, got {chunk}")
        if min_span is not None and not (isinstance(min_span, (int, float)) and 0.0 <= float(min_span) < float("inf")):
            raise ValueError(f"{what}: min_span must be None or finite and not negative, got {min_span!r}")
        if builder is not None and not callable(builder):
            raise ValueError(f"{what}: builder must be callable, got {builder!r}")
        self.model, self.resolution, self.level, self.chunk = model, shape, level, int(chunk)
        self.clip_far = (not getattr(model, 'use_sample_at_infinity', True)) if clip_far is None else bool(clip_far)
        self.min_span = None if min_span is None else float(min_span)
        self.builder = builder if builder is not None else self._build
        if device is None:
            device = next(model.parameters()).device
        self.stack = OccupancyStack(cells, bounds, ids, shared=shared, device=device)
        # shared mode: the union of the round in progress; it replaces the live grid (slot 0) when the round wraps
        self.pending = torch.zeros_like(self.stack.bits[0]) if self.stack.shared else None
        self.steps_begun = 0      # k
        self.cursor = 0           # the next id of the round robin, an index into stack.ids
        self.refreshes = 0
        self._out: Dict[tuple, Dict[str, torch.Tensor]] = {}     # clip_batch's buffers per (rows, columns): fixed under a graph

    def _build(self, frame_id: int):
        return occupancy_grid(self.model, self.stack.bounds, self.resolution, frame_id, self.sigma_min, self.dilate,
                              level=self.level, chunk=self.chunk)

    def due(self) -> bool:
        k = self.steps_begun - self.warmup_steps
        return k >= 0 and k % self.refresh_every == 0

    def before_step(self) -> None:
        """What TrainStep.step() calls ahead of the step's launches or replay: the refresh that is due, then k += 1."""
        if self.due():
            self.refresh()
        self.steps_begun += 1

    @torch.no_grad()
    def refresh(self) -> None:
        """Rebuild the grids of the next `frames_per_refresh` ids.  Host-side, outside any graph; the model's
        train / eval state is put back (a captured step froze it)."""
        stack = self.stack
        training = getattr(self.model, 'training', None)
        try:
            for _ in range(self.frames_per_refresh):
                frame_id = stack.ids[self.cursor]
                occ = self.builder(frame_id)
                if stack.shared:
                    bits, cells, bounds = check_occupancy(occ, "TrainOccupancy.refresh")
                    if cells != stack.cells or bounds != stack.bounds:
                        raise ValueError(f"TrainOccupancy.refresh: the builder's occupancy has cells {cells} over {bounds}, "
                                         f"the stack {stack.cells} over {stack.bounds}")
                    self.pending.bitwise_or_(bits)
                else:
                    stack.set(frame_id, occ)
                self.cursor += 1
                if self.cursor == len(stack.ids):
                    self.cursor = 0
                    if stack.shared:
                        stack.bits[0].copy_(self.pending)
                        self.pending.zero_()
        finally:
            if training is not None and getattr(self.model, 'training', None) != training:
                self.model.train(training)
        self.refreshes += 1

    def clip(self, rays: torch.Tensor) -> Dict[str, torch.Tensor]:
        """ops.occupancy.clip_batch of a step's rays over [model.near, model.far], into buffers kept per batch shape."""
        key = tuple(rays.shape)
        out = self._out.get(key)
        if out is None:
            n, ld = key
            sizes = {'rays': ((n, ld), torch.float32), 'viewdirs': ((n, 3), torch.float32),
                     'affine': ((n, 2), torch.float32), 'hit': ((n,), torch.uint8), 'hit_count': ((), torch.int64)}
            out = self._out[key] = {k: torch.zeros(sizes[k][0], dtype=sizes[k][1], device=rays.device)
                                    for k in CLIP_BATCH_KEYS}
        return clip_batch(rays, self.stack, self.model.near, self.model.far, clip_far=self.clip_far,
                          min_span=self.min_span, out=out)

    def state_dict(self) -> Dict:
        return {'stack': self.stack.state_dict(), 'pending': None if self.pending is None else self.pending.clone(),
                'steps_begun': self.steps_begun, 'cursor': self.cursor, 'refreshes': self.refreshes}

    def load_state_dict(self, state: Dict) -> None:
        self.stack.load_state_dict(state['stack'])
        if (self.pending is None) != (state['pending'] is None):
            raise ValueError("TrainOccupancy.load_state_dict: the state is that of another mode (shared differs)")
        if self.pending is not None:
            with torch.no_grad():
                self.pending.copy_(state['pending'])
        self.steps_begun, self.cursor, self.refreshes = int(state['steps_begun']), int(state['cursor']), int(state['refreshes'])
