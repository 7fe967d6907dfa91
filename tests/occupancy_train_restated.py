"""hn_occ_clip_batch restated in NumPy: the slot lookup of a ray's frame id, then the fp32 walk of
tests/occupancy_restated.py on that slot's grid.  The kernel's early exit (clip_far == 0 ends the walk at the first counted
cell) changes no result bit, so the restatement walks on.  No GPU."""
import numpy as np

import occupancy_restated as R

F = np.float32


def all_occupied_bits(cells):
    """(cx, cy, words) int64 of a grid with every cell set and zero padding: what an OccupancyStack starts with."""
    return R.pack(np.ones(cells, dtype=bool))


def slots_of(values, slot_of_id, n_slots):
    """(N,) int64, -1 for "no grid": values are the float32 ids of the rays; v picks slot_of_id[(int)v] when it is finite and
    0 <= (int)v < n_ids ((int) truncates towards zero, so -0.5 is id 0 and 2.5 is id 2); a slot outside [0, n_slots) is no
    grid either."""
    v = np.asarray(values, dtype=F)
    slot_of_id = np.asarray(slot_of_id, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (v > F(-1.0)) & (v < F(2.0 ** 31))
    ids = np.where(ok, np.trunc(np.where(ok, v, 0)), 0).astype(np.int64)
    ok &= ids < slot_of_id.size
    slot = np.where(ok, slot_of_id[np.where(ok, ids, 0)], -1)
    return np.where((slot >= 0) & (slot < n_slots), slot, -1)


def clip_batch(rays, grids, slot_of_id, bounds, near, far, clip_far=True, min_span=0.0, id_col=None):
    """{'rays', 'viewdirs', 'affine', 'hit', 'hit_count', 't', 'slot'} as hn_occ_clip_batch gives them ('t' and 'slot' for
    the tests' own use): grids is the list of (cx, cy, cz) bool arrays of the stack's slots; id_col None reads column 8
    when there is one, a negative id_col (or fewer columns) gives every ray id 0."""
    rays = np.ascontiguousarray(rays, dtype=F)
    n, ld = rays.shape
    if id_col is None:
        id_col = 8 if ld > 8 else -1
    values = rays[:, id_col] if id_col >= 0 else np.zeros(n, dtype=F)
    slot = slots_of(values, slot_of_id, len(grids))
    out = {'rays': rays.copy(), 'viewdirs': rays[:, 3:6].copy(), 'hit': np.zeros(n, dtype=np.uint8),
           'affine': np.tile(np.asarray([0.0, 1.0], dtype=F), (n, 1)),
           't': np.tile(np.asarray([near, far], dtype=F), (n, 1)), 'slot': slot}
    for s, grid in enumerate(grids):
        rows = np.nonzero(slot == s)[0]
        if rows.size == 0:
            continue
        part = R.clip_rays(rays[rows], grid, bounds, near, far, clip_far=clip_far, min_span=min_span)
        for k in ('rays', 'hit', 'affine', 't'):
            out[k][rows] = part[k]
    out['hit_count'] = np.int64(out['hit'].sum())
    return out
