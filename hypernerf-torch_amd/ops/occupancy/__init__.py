"""Empty-space skipping for the render path (csrc/hn_occupancy.hip): a density lattice as one bit per
lattice cell, its dilation and population count, rays clipped to the occupied part of [near, far], and the map of a
clipped ray's results back to true distances.  For the training step: OccupancyStack, grids of several
frames in one fixed buffer, and clip_batch, one graph-capturable launch that clips every ray against its frame's grid;
train.py holds TrainOccupancy, which keeps such a stack current for training.TrainStep.

An occupancy is a dict {'bits': (cx, cy, words) int64 on the GPU, 'cells': (cx, cy, cz), 'bounds': six floats}: the
lattice of (cx + 1, cy + 1, cz + 1) points over `bounds` has cx * cy * cz cells, words = ceil(cz / 64), and bit b of word w
of row (i, j) is cell (i, j, 64 w + b) (the sign bit of the int64 is bit 63); the bits past cz are zero."""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib as L
from ..checks import INT32_MAX
from ..mesh import check_lattice, check_volume

__all__ = ["OCC_MAX_CELLS", "OCC_MAX_RAY_LD", "OCC_KEYS", "check_occupancy", "occupancy_mark", "occupancy_dilate",
           "occupancy_count", "occupancy_from_density", "occupancy_grid", "occupancy_union", "occupancy_fraction", "clip_rays",
           "unclip", "OccupancyCache", "OccupancyStack", "CLIP_BATCH_KEYS", "clip_batch"]

# mirrors of csrc/hn_occupancy.hip's limits (no macros in the header: its set of constants is that of ABI 340)
OCC_MAX_CELLS = 2048      # cells per axis
OCC_MAX_RAY_LD = 64       # floats per ray row
OCC_KEYS = ('rgb', 'depth', 'acc', 'med_depth')      # the per-ray results unclip knows how to map back


def _check_cells(cells, what: str):
    try:
        cells = tuple(int(v) for v in cells)
    except (TypeError, ValueError):
        cells = ()
    if len(cells) != 3 or min(cells) < 1 or max(cells) > OCC_MAX_CELLS:
        raise ValueError(f"{what}: cells must be three counts in 1 .. {OCC_MAX_CELLS}, got {cells!r}")
    return cells


def _check_bounds(cells, bounds, what: str):
    _, bounds = check_lattice(tuple(c + 1 for c in cells), bounds, what)
    if not all(math.isfinite(v) for v in bounds):
        raise ValueError(f"{what}: bounds must be finite, got {bounds}")
    return bounds


def _check_bits(bits, cells, what: str) -> torch.Tensor:
    shape = (cells[0], cells[1], (cells[2] + 63) // 64)
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int64 or tuple(bits.shape) != shape:
        raise ValueError(f"{what}: bits must be a {shape} int64 tensor for cells {cells}")
    if not bits.is_contiguous():
        raise ValueError(f"{what}: bits must be C-contiguous")
    return bits.detach()


def check_occupancy(occ, what: str):
    """(bits, cells, bounds) of an occupancy dict as the hn_occ entry points take them, or ValueError.  The device is the
    caller's to check, after its other arguments."""
    if not isinstance(occ, dict) or not all(k in occ for k in ('bits', 'cells', 'bounds')):
        raise ValueError(f"{what}: an occupancy is a dict with 'bits', 'cells' and 'bounds', as occupancy_from_density "
                         "returns it")
    cells = _check_cells(occ['cells'], what)
    bounds = _check_bounds(cells, occ['bounds'], what)
    return _check_bits(occ['bits'], cells, what), cells, bounds


def _check_dilate(dilate, what: str) -> int:
    if isinstance(dilate, bool) or not isinstance(dilate, (int, np.integer)) or not 0 <= int(dilate) <= OCC_MAX_CELLS:
        raise ValueError(f"{what}: dilate must be an int in 0 .. {OCC_MAX_CELLS}, got {dilate!r}")
    return int(dilate)


def _check_sigma_min(sigma_min, what: str) -> float:
    try:
        sigma_min = float(sigma_min)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: sigma_min must be a number, got {sigma_min!r}") from None
    if math.isnan(sigma_min):
        raise ValueError(f"{what}: sigma_min must not be NaN")
    return sigma_min


@torch.no_grad()
def occupancy_mark(grid: torch.Tensor, sigma_min: float) -> torch.Tensor:
    """(nx-1, ny-1, ceil((nz-1)/64)) int64 bits of the density lattice grid (nx, ny, nz) fp32 (hn_occ_mark): a cell is
    occupied iff one of its 8 corners is >= sigma_min or NaN.  No host synchronisation; the same bits on every run."""
    what = "occupancy_mark"
    grid = check_volume(grid, what, "grid")
    (nx, ny, nz), _ = check_lattice(grid.shape, (0.0, 1.0) * 3, what)
    cells = _check_cells((nx - 1, ny - 1, nz - 1), what)
    sigma_min = _check_sigma_min(sigma_min, what)
    if not grid.is_cuda:
        raise ValueError(f"{what}: grid must live on the GPU (there is no CPU fallback)")
    L.load()
    bits = torch.empty((cells[0], cells[1], (cells[2] + 63) // 64), dtype=torch.int64, device=grid.device)
    with torch.cuda.device(grid.device):
        L.launch("hn_occ_mark", L.ptr(grid), nx, ny, nz, sigma_min, L.ptr(bits), L.stream_handle())
    return bits


@torch.no_grad()
def occupancy_dilate(bits: torch.Tensor, cells, times: int = 1) -> torch.Tensor:
    """`bits` dilated `times` times by the 3 x 3 x 3 cube (hn_occ_dilate, ping-pong between two buffers): a cell is set iff a
    cell within `times` steps along every axis was.  Nothing wraps at the faces, the padding bits stay zero; times = 0
    gives `bits` itself."""
    what = "occupancy_dilate"
    cells = _check_cells(cells, what)
    bits = _check_bits(bits, cells, what)
    times = _check_dilate(times, what)
    if not bits.is_cuda:
        raise ValueError(f"{what}: bits must live on the GPU (there is no CPU fallback)")
    if times == 0:
        return bits
    L.load()
    src, dst = bits, torch.empty_like(bits)
    spare = torch.empty_like(bits) if times > 1 else None
    with torch.cuda.device(bits.device):
        for _ in range(times):
            L.launch("hn_occ_dilate", L.ptr(src), L.ptr(dst), cells[0], cells[1], cells[2], L.stream_handle())
            src, dst = dst, (spare if src is bits else src)
    return src


@torch.no_grad()
def occupancy_count(bits: torch.Tensor) -> torch.Tensor:
    """A 0-d int64 tensor on the device of `bits`: the number of set bits (hn_occ_count).  No host synchronisation."""
    what = "occupancy_count"
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int64 or bits.numel() < 1 or bits.numel() > INT32_MAX:
        raise ValueError(f"{what}: bits must be an int64 tensor of 1 .. 2**31 - 1 words")
    if not bits.is_contiguous():
        raise ValueError(f"{what}: bits must be C-contiguous")
    if not bits.is_cuda:
        raise ValueError(f"{what}: bits must live on the GPU (there is no CPU fallback)")
    L.load()
    count = torch.empty((), dtype=torch.int64, device=bits.device)
    with torch.cuda.device(bits.device):
        L.launch("hn_occ_count", L.ptr(bits.detach()), bits.numel(), L.ptr(count), L.stream_handle())
    return count


@torch.no_grad()
def occupancy_from_density(grid: torch.Tensor, bounds, sigma_min: float, dilate: int = 1) -> Dict:
    """The occupancy {'bits', 'cells', 'bounds'} of a density lattice as geometry.density_grid returns it ((nx, ny, nz) fp32
    over `bounds`): occupancy_mark(grid, sigma_min), then occupancy_dilate `dilate` times.  A lattice can miss structure
    thinner than a cell: a low `sigma_min` and `dilate` >= 1 are the caller's guard against that."""
    what = "occupancy_from_density"
    grid = check_volume(grid, what, "grid")
    shape, bounds = check_lattice(grid.shape, bounds, what)
    cells = _check_cells(tuple(n - 1 for n in shape), what)
    bounds = _check_bounds(cells, bounds, what)
    sigma_min = _check_sigma_min(sigma_min, what)
    dilate = _check_dilate(dilate, what)
    if not grid.is_cuda:
        raise ValueError(f"{what}: grid must live on the GPU (there is no CPU fallback)")
    bits = occupancy_dilate(occupancy_mark(grid, sigma_min), cells, dilate)
    return {'bits': bits, 'cells': cells, 'bounds': bounds}


def _resolution(resolution):
    if isinstance(resolution, (int, np.integer)):
        return (int(resolution),) * 3
    return tuple(resolution)


@torch.no_grad()
def occupancy_grid(model, bounds, resolution, frame_id: int, sigma_min: float, dilate: int = 1, level: str = 'fine',
                   chunk: int = 1 << 20, render_opts=None) -> Dict:
    """occupancy_from_density(geometry.density_grid(model, bounds, resolution, frame_id, level, chunk), bounds, sigma_min,
    dilate): the occupancy of frame `frame_id` on the cells of a lattice of `resolution` points (an int or three)."""
    from ...geometry import density_grid
    what = "occupancy_grid"
    shape, bounds = check_lattice(_resolution(resolution), bounds, what)
    _check_bounds(_check_cells(tuple(n - 1 for n in shape), what), bounds, what)
    _check_sigma_min(sigma_min, what)
    _check_dilate(dilate, what)
    grid = density_grid(model, bounds, shape, frame_id, level=level, chunk=chunk, render_opts=render_opts)
    return occupancy_from_density(grid, bounds, sigma_min, dilate)


@torch.no_grad()
def occupancy_union(a: Dict, b: Dict) -> Dict:
    """The occupancy whose cells are occupied in `a` or in `b` (torch.bitwise_or); both must have the same cells and
    bounds.  E.g. the union over the frames of a sequence, for a renderer that keeps one grid."""
    what = "occupancy_union"
    bits_a, cells_a, bounds_a = check_occupancy(a, what)
    bits_b, cells_b, bounds_b = check_occupancy(b, what)
    if cells_a != cells_b or bounds_a != bounds_b:
        raise ValueError(f"{what}: the occupancies differ in cells or bounds: {cells_a} over {bounds_a}, {cells_b} over "
                         f"{bounds_b}")
    if bits_a.device != bits_b.device:
        raise ValueError(f"{what}: the occupancies must live on one device")
    return {'bits': torch.bitwise_or(bits_a, bits_b), 'cells': cells_a, 'bounds': bounds_a}


@torch.no_grad()
def occupancy_fraction(occ: Dict) -> float:
    """The occupied share of the cells, 0 .. 1 (occupancy_count over cx * cy * cz).  One host read."""
    bits, cells, _ = check_occupancy(occ, "occupancy_fraction")
    return int(occupancy_count(bits)) / float(cells[0] * cells[1] * cells[2])


def _check_interval(near, far, what: str):
    try:
        near, far = float(near), float(far)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: near and far must be numbers, got {near!r}, {far!r}") from None
    if not (math.isfinite(near) and math.isfinite(far) and far > near):
        raise ValueError(f"{what}: near and far must be finite with far > near, got {near}, {far}")
    return near, far


@torch.no_grad()
def clip_rays(rays: torch.Tensor, occ: Dict, near: float, far: float, clip_far: bool = True,
              min_span: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """Rays (N, >= 6) fp32 rows [o, d, ...] clipped to the occupied cells of `occ` (hn_occ_clip_rays, one launch):
      't'       (N, 2)  (t0, t1): the entry of the first and the exit of the last occupied cell the ray crosses inside
                        [near, far]; space outside the grid's box is empty
      'hit'     (N,)    uint8: 0 for a ray that meets no occupied cell (or is not finite); its t is (near, far)
      'rays'    (N, ld) the rows re-parametrised so that a model sampling z in its scalar [near, far] samples [t0, t1] of
                        the input ray: o' = o + d * a, d' = b * d, the other columns copied
      'affine'  (N, 2)  (a, b) with true distance = a + b * z, b = (t1 - t0) / (far - near), a = t0 - b * near
    A miss, and every ray with (t0, t1) == (near, far), keeps its row bit for bit and has affine (0, 1).  Render the new
    rows with the ORIGINAL directions as 'viewdirs' and map the results back with unclip.  clip_far=False keeps
    t1 = far.  min_span: the shortest interval a hit may have (it grows symmetrically, clamped to [near, far]); None = the
    smallest cell edge.  No host synchronisation."""
    what = "clip_rays"
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or not 6 <= rays.shape[1] <= OCC_MAX_RAY_LD \
            or rays.dtype != torch.float32:
        raise ValueError(f"{what}: rays must be a (N, 6 .. {OCC_MAX_RAY_LD}) float32 tensor")
    if rays.shape[0] > INT32_MAX:
        raise ValueError(f"{what}: {rays.shape[0]} rays exceed 2**31 - 1")
    bits, cells, bounds = check_occupancy(occ, what)
    near, far = _check_interval(near, far, what)
    if min_span is None:
        min_span = min((bounds[2 * c + 1] - bounds[2 * c]) / cells[c] for c in range(3))
    try:
        min_span = float(min_span)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: min_span must be a number or None, got {min_span!r}") from None
    if not (math.isfinite(min_span) and min_span >= 0.0):
        raise ValueError(f"{what}: min_span must be finite and not negative, got {min_span}")
    if not (rays.is_cuda and bits.is_cuda):
        raise ValueError(f"{what}: rays and the occupancy must live on the GPU (there is no CPU fallback)")
    if rays.device != bits.device:
        raise ValueError(f"{what}: rays and the occupancy must live on one device")
    rays = rays.detach().contiguous()
    n, ld = rays.shape
    dev = rays.device
    out = {'rays': torch.empty_like(rays), 't': torch.empty((n, 2), dtype=torch.float32, device=dev),
           'hit': torch.empty((n,), dtype=torch.uint8, device=dev),
           'affine': torch.empty((n, 2), dtype=torch.float32, device=dev)}
    if n:
        L.load()
        with torch.cuda.device(dev):
            L.launch("hn_occ_clip_rays", L.ptr(rays), n, ld, L.ptr(bits), cells[0], cells[1], cells[2],
                     (C.c_float * 6)(*bounds), near, far, 1 if clip_far else 0, min_span, L.ptr(out['t']), L.ptr(out['hit']),
                     L.ptr(out['rays']), L.ptr(out['affine']), L.stream_handle())
    return out


@torch.no_grad()
def unclip(res: Dict[str, torch.Tensor], affine: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The per-ray results of a model that rendered clip_rays' rows, as those of the input rays: with (a, b) = affine,
      depth      = a * res['weights'].sum(-1) + b * res['depth']
      med_depth  = a + b * res['med_depth']
    and every other key unchanged ('rgb' and 'acc' do not depend on the parametrisation).  depth is sum_i w_i z_i over the
    samples, and z_true = a + b z: the constant needs the sum of the SAME weights — not 'acc', which under
    use_sample_at_infinity leaves the last sample out while depth keeps it.  A new dict; `res` is not changed."""
    what = "unclip"
    if not isinstance(res, dict):
        raise ValueError(f"{what}: res must be a dict of per-ray results")
    if not isinstance(affine, torch.Tensor) or affine.dim() != 2 or affine.shape[1] != 2:
        raise ValueError(f"{what}: affine must be a (N, 2) tensor, as clip_rays returns it")
    n = affine.shape[0]
    out = dict(res)
    a, b = affine[:, 0], affine[:, 1]
    if 'depth' in res:
        if 'weights' not in res:
            raise ValueError(f"{what}: mapping 'depth' back needs the level's 'weights' (their sum, not 'acc')")
        depth, weights = res['depth'], res['weights']
        if depth.shape[0] != n or weights.shape[0] != n:
            raise ValueError(f"{what}: {depth.shape[0]} depths / {weights.shape[0]} weight rows for {n} rays")
        out['depth'] = (a * weights.reshape(n, -1).sum(-1) + b * depth.reshape(n)).view(depth.shape)
    if 'med_depth' in res:
        med = res['med_depth']
        if med.shape[0] != n:
            raise ValueError(f"{what}: {med.shape[0]} median depths for {n} rays")
        out['med_depth'] = (a + b * med.reshape(n)).view(med.shape)
    return out


class OccupancyCache:
    """Occupancies of a deforming scene, one per frame, built on first use: .get(frame_id) is
    occupancy_grid(model, bounds, resolution, frame_id, sigma_min, dilate, level, chunk), kept for the `max_entries` most
    recently used frames.  `builds` counts the grids built."""

    def __init__(self, model, bounds, resolution, sigma_min: float, dilate: int = 1, max_entries: int = 8,
                 level: str = 'fine', chunk: int = 1 << 20):
        what = "OccupancyCache"
        shape, self.bounds = check_lattice(_resolution(resolution), bounds, what)
        self.cells = _check_cells(tuple(n - 1 for n in shape), what)
        _check_bounds(self.cells, self.bounds, what)
        self.resolution = shape
        self.sigma_min = _check_sigma_min(sigma_min, what)
        self.dilate = _check_dilate(dilate, what)
        if isinstance(max_entries, bool) or not isinstance(max_entries, (int, np.integer)) or int(max_entries) < 1:
            raise ValueError(f"{what}: max_entries must be a positive int, got {max_entries!r}")
        if int(chunk) < 1:
            raise ValueError(f"{what}: chunk must be positive, got {chunk}")
        self.max_entries = int(max_entries)
        self.model, self.level, self.chunk = model, level, int(chunk)
        self.builds = 0
        self._entries = OrderedDict()

    def get(self, frame_id: int) -> Dict:
        if isinstance(frame_id, bool) or not isinstance(frame_id, (int, np.integer)):
            raise ValueError(f"OccupancyCache.get: frame_id must be an int, got {frame_id!r}")
        frame_id = int(frame_id)
        if frame_id in self._entries:
            self._entries.move_to_end(frame_id)
            return self._entries[frame_id]
        occ = occupancy_grid(self.model, self.bounds, self.resolution, frame_id, self.sigma_min, self.dilate,
                             level=self.level, chunk=self.chunk)
        self.builds += 1
        self._entries[frame_id] = occ
        while len(self._entries) > self.max_entries:
            self._entries.popitem(last=False)
        return occ

    def __len__(self):
        return len(self._entries)


def _check_ids(ids, what: str):
    try:
        ids = list(ids)
    except TypeError:
        raise ValueError(f"{what}: ids must be a sequence of frame ids, got {ids!r}") from None
    if not ids or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0 or int(v) >= INT32_MAX
                      for v in ids):
        raise ValueError(f"{what}: ids must be one or more ints in 0 .. 2**31 - 2, got {ids!r}")
    ids = [int(v) for v in ids]
    if len(set(ids)) != len(ids):
        raise ValueError(f"{what}: ids must be distinct, got {ids!r}")
    return tuple(sorted(ids))


class OccupancyStack:
    """The occupancies of several frames over ONE lattice, in buffers whose storage never changes after construction — what
    a captured training step reads (clip_batch):
      bits        (n_slots, cx, cy, words) int64: the grids, each in the layout of an occupancy's 'bits'
      slot_of_id  (max(ids) + 1,) int32: the slot of a frame id, -1 for an id without a grid
      cells, bounds, ids (ascending), shared
    `ids` are the distinct frame ids that get a grid: a slot each, or (shared=True) slot 0 for all of them.  Every grid
    starts all-occupied (the padding bits past cz zero), which clips no ray whose [near, far] lies in the box.  set() and
    fill() write in place, so a replayed graph sees them."""

    def __init__(self, cells, bounds, ids, shared: bool = False, device='cuda'):
        what = "OccupancyStack"
        self.cells = _check_cells(cells, what)
        self.bounds = _check_bounds(self.cells, bounds, what)
        self.ids = _check_ids(ids, what)
        self.shared = bool(shared)
        self.n_slots = 1 if self.shared else len(self.ids)
        cx, cy, cz = self.cells
        words = (cz + 63) // 64
        if self.n_slots * cx * cy * words > INT32_MAX:
            raise ValueError(f"{what}: {self.n_slots} grids of {self.cells} cells exceed 2**31 - 1 words")
        slots = np.full(self.ids[-1] + 1, -1, dtype=np.int32)
        for slot, fid in enumerate(self.ids):
            slots[fid] = 0 if self.shared else slot
        self.slot_of_id = torch.from_numpy(slots).to(device)
        self.bits = torch.empty((self.n_slots, cx, cy, words), dtype=torch.int64, device=device)
        self.fill(True)

    def fill(self, all_occupied: bool) -> None:
        """Every grid all-occupied (True) or empty (False), in place."""
        with torch.no_grad():
            if not all_occupied:
                self.bits.zero_()
                return
            self.bits.fill_(-1)
            tail = self.cells[2] % 64
            if tail:
                self.bits[..., -1] = (1 << tail) - 1

    def slot(self, frame_id: int) -> int:
        """The slot of a frame id, or ValueError when it has no grid."""
        if isinstance(frame_id, bool) or not isinstance(frame_id, (int, np.integer)) or int(frame_id) not in self.ids:
            raise ValueError(f"OccupancyStack: {frame_id!r} is not one of the ids {self.ids}")
        return 0 if self.shared else self.ids.index(int(frame_id))

    def set(self, key, occ: Dict, slot: bool = False) -> None:
        """Copy the bits of occupancy `occ` (same cells and bounds) into the grid of frame id `key` — or, with slot=True,
        into slot `key` — in place."""
        what = "OccupancyStack.set"
        if slot:
            if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < self.n_slots:
                raise ValueError(f"{what}: slot must be an int in 0 .. {self.n_slots - 1}, got {key!r}")
            at = int(key)
        else:
            at = self.slot(key)
        bits, cells, bounds = check_occupancy(occ, what)
        if cells != self.cells or bounds != self.bounds:
            raise ValueError(f"{what}: the occupancy has cells {cells} over {bounds}, the stack {self.cells} over {self.bounds}")
        if bits.device != self.bits.device:
            raise ValueError(f"{what}: the occupancy lives on {bits.device}, the stack on {self.bits.device}")
        with torch.no_grad():
            self.bits[at].copy_(bits)

    def occupancy(self, frame_id: int) -> Dict:
        """The occupancy dict of a frame: 'bits' is a VIEW of its slot (clip_rays, occupancy_fraction and
        render_image(occupancy=) take it)."""
        return {'bits': self.bits[self.slot(frame_id)], 'cells': self.cells, 'bounds': self.bounds}

    def state_dict(self) -> Dict:
        return {'bits': self.bits.clone(), 'slot_of_id': self.slot_of_id.clone(), 'cells': self.cells, 'bounds': self.bounds,
                'ids': self.ids, 'shared': self.shared}

    def load_state_dict(self, state: Dict) -> None:
        what = "OccupancyStack.load_state_dict"
        if (tuple(state['cells']) != self.cells or tuple(float(v) for v in state['bounds']) != self.bounds
                or tuple(state['ids']) != self.ids or bool(state['shared']) != self.shared):
            raise ValueError(f"{what}: the state is that of another stack (cells, bounds, ids or shared differ)")
        if tuple(state['bits'].shape) != tuple(self.bits.shape) or state['bits'].dtype != torch.int64:
            raise ValueError(f"{what}: bits must be a {tuple(self.bits.shape)} int64 tensor")
        with torch.no_grad():
            self.bits.copy_(state['bits'])


CLIP_BATCH_KEYS = ('rays', 'viewdirs', 'affine', 'hit', 'hit_count')


@torch.no_grad()
def clip_batch(rays: torch.Tensor, stack: OccupancyStack, near: float, far: float, clip_far: bool = True,
               min_span: Optional[float] = None, out: Optional[Dict[str, torch.Tensor]] = None,
               id_col: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """clip_rays for a batch that mixes frames (hn_occ_clip_batch, ONE graph-capturable launch): every row of rays
    (N, 6 .. 64) fp32 is clipped against the grid `stack` holds for the frame id in its column `id_col` (None: column 8
    when there is one, as prepare_ray_dict reads it; otherwise, and for a negative id_col, every ray has id 0).
      'rays'      (N, ld)  as clip_rays' — bit for bit, per frame — the row itself for an id without a grid
      'viewdirs'  (N, 3)   the INPUT rows' directions: render 'rays' with these as 'viewdirs'
      'affine'    (N, 2)   (a, b) as clip_rays'; (0, 1) without a grid
      'hit'       (N,)     uint8
      'hit_count' ()       int64 on the device: hit.sum()
    clip_far=False keeps t1 = far and ends each walk at the first occupied cell.  `out`: a dict of these five tensors to
    write into instead of allocating (a captured step replays on them).  The launch reads stack.bits and
    stack.slot_of_id where they are: a replay sees every set() / fill() since.  No host synchronisation."""
    what = "clip_batch"
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or not 6 <= rays.shape[1] <= OCC_MAX_RAY_LD \
            or rays.dtype != torch.float32:
        raise ValueError(f"{what}: rays must be a (N, 6 .. {OCC_MAX_RAY_LD}) float32 tensor")
    n, ld = rays.shape
    if n > INT32_MAX:
        raise ValueError(f"{what}: {n} rays exceed 2**31 - 1")
    if not isinstance(stack, OccupancyStack):
        raise ValueError(f"{what}: stack must be an OccupancyStack, got {type(stack).__name__}")
    near, far = _check_interval(near, far, what)
    cells, bounds = stack.cells, stack.bounds
    if min_span is None:
        min_span = min((bounds[2 * c + 1] - bounds[2 * c]) / cells[c] for c in range(3))
    try:
        min_span = float(min_span)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: min_span must be a number or None, got {min_span!r}") from None
    if not (math.isfinite(min_span) and min_span >= 0.0):
        raise ValueError(f"{what}: min_span must be finite and not negative, got {min_span}")
    if id_col is None:
        id_col = 8 if ld > 8 else -1
    if isinstance(id_col, bool) or not isinstance(id_col, (int, np.integer)) or int(id_col) >= ld or 0 <= int(id_col) < 6:
        raise ValueError(f"{what}: id_col must be negative or a column in 6 .. {ld - 1}, got {id_col!r}")
    id_col = max(int(id_col), -1)
    if not (rays.is_cuda and stack.bits.is_cuda):
        raise ValueError(f"{what}: rays and the stack must live on the GPU (there is no CPU fallback)")
    if rays.device != stack.bits.device:
        raise ValueError(f"{what}: rays and the stack must live on one device")
    dev = rays.device
    shapes = {'rays': ((n, ld), torch.float32), 'viewdirs': ((n, 3), torch.float32), 'affine': ((n, 2), torch.float32),
              'hit': ((n,), torch.uint8), 'hit_count': ((), torch.int64)}
    if out is None:
        rays = rays.detach().contiguous()
        out = {k: torch.empty(shape, dtype=dtype, device=dev) for k, (shape, dtype) in shapes.items()}
    else:
        if not rays.is_contiguous():
            raise ValueError(f"{what}: with out= the rays must be C-contiguous (nothing is allocated)")
        rays = rays.detach()
        if not isinstance(out, dict) or set(out) != set(shapes):
            raise ValueError(f"{what}: out must be a dict with the keys {CLIP_BATCH_KEYS}")
        for k, (shape, dtype) in shapes.items():
            t = out[k]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev \
                    or not t.is_contiguous():
                raise ValueError(f"{what}: out['{k}'] must be a C-contiguous {shape} {dtype} tensor on {dev}")
        if n and out['rays'].data_ptr() == rays.data_ptr():
            raise ValueError(f"{what}: out['rays'] must not be the input rays")
    if n == 0:
        out['hit_count'].zero_()
        return out
    L.load()
    with torch.cuda.device(dev):
        L.launch("hn_occ_clip_batch", L.ptr(rays), n, ld, id_col, L.ptr(stack.bits), stack.n_slots, cells[0], cells[1],
                 cells[2], L.ptr(stack.slot_of_id), stack.slot_of_id.numel(), (C.c_float * 6)(*bounds), near, far,
                 1 if clip_far else 0, min_span, L.ptr(out['rays']), L.ptr(out['viewdirs']), L.ptr(out['affine']),
                 L.ptr(out['hit']), L.ptr(out['hit_count']), L.stream_handle())
    return out
