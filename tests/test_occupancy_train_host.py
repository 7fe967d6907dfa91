"""Training-time occupancy without a GPU: OccupancyStack on CPU tensors, TrainOccupancy's refresh schedule
with a stub builder, the NumPy slot lookup, every refusal of the host halves and of the C ABI, and TrainStep(occupancy=)
under data parallelism."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import occupancy_restated as R
import occupancy_train_restated as RT
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.ops import occupancy as OPS
from hypernerf_torch_amd.training import TrainOccupancy, TrainStep

B = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
CELLS = (3, 4, 70)            # two words per row, the second with 6 valid bits
IDS = (0, 2, 5)


def grid_for(frame_id, cells=CELLS):
    """A different, partly occupied grid per frame id."""
    return np.random.default_rng(100 + frame_id).random(cells) < 0.3


def occ_for(frame_id, cells=CELLS, bounds=B):
    return {'bits': torch.from_numpy(R.pack(grid_for(frame_id, cells))), 'cells': cells, 'bounds': bounds}


def full_bits(cells=CELLS):
    return torch.from_numpy(RT.all_occupied_bits(cells))


# ---- 1. OccupancyStack ------------------------------------------------------------------------------------------------------------
def test_stack_starts_all_occupied_and_writes_in_place():
    stack = HN.OccupancyStack(CELLS, B, [5, 0, 2], device='cpu')
    assert stack.ids == IDS and stack.n_slots == 3 and not stack.shared
    assert stack.bits.shape == (3, 3, 4, 2) and stack.bits.dtype == torch.int64
    assert stack.slot_of_id.dtype == torch.int32 and stack.slot_of_id.tolist() == [0, -1, 1, -1, -1, 2]
    for slot in range(3):
        assert torch.equal(stack.bits[slot], full_bits())
    cells, pad = R.unpack(stack.bits[1].numpy(), CELLS[2])
    assert cells.all() and not pad.any()                        # every valid bit set, the padding bits past cz zero
    where = (stack.bits.data_ptr(), stack.slot_of_id.data_ptr())
    stack.set(2, occ_for(2))
    assert torch.equal(stack.bits[1], occ_for(2)['bits']) and torch.equal(stack.bits[0], full_bits())
    assert torch.equal(stack.bits[2], full_bits())
    stack.set(2, occ_for(5), slot=True)                         # a slot index instead of an id
    assert torch.equal(stack.bits[2], occ_for(5)['bits'])
    view = stack.occupancy(5)
    assert view['cells'] == CELLS and view['bounds'] == B and view['bits'].data_ptr() == stack.bits[2].data_ptr()
    OPS.check_occupancy(view, "test")                           # a 3.18 occupancy dict
    stack.fill(False)
    assert not stack.bits.any() and not view['bits'].any()      # the view follows
    stack.fill(True)
    assert torch.equal(stack.bits[2], full_bits())
    assert (stack.bits.data_ptr(), stack.slot_of_id.data_ptr()) == where
    whole = HN.OccupancyStack((2, 2, 64), B, [1], device='cpu')  # cz a multiple of 64: no padding bits
    assert (whole.bits == -1).all()


def test_shared_stack_maps_every_id_to_slot_zero():
    stack = HN.OccupancyStack(CELLS, B, IDS, shared=True, device='cpu')
    assert stack.n_slots == 1 and stack.bits.shape == (1, 3, 4, 2) and stack.slot_of_id.tolist() == [0, -1, 0, -1, -1, 0]
    stack.set(5, occ_for(5))
    assert torch.equal(stack.occupancy(0)['bits'], occ_for(5)['bits'])


def test_stack_state_dict_round_trip():
    a = HN.OccupancyStack(CELLS, B, IDS, device='cpu')
    a.set(0, occ_for(0))
    state = a.state_dict()
    a.fill(False)
    assert state['bits'].any()                                  # a copy, not a view
    b = HN.OccupancyStack(CELLS, B, IDS, device='cpu')
    where = b.bits.data_ptr()
    b.load_state_dict(state)
    assert torch.equal(b.bits[0], occ_for(0)['bits']) and torch.equal(b.bits[1], full_bits()) and b.bits.data_ptr() == where
    with pytest.raises(ValueError, match="another stack"):
        HN.OccupancyStack(CELLS, B, (0, 2, 6), device='cpu').load_state_dict(state)
    with pytest.raises(ValueError, match="another stack"):
        HN.OccupancyStack(CELLS, B, IDS, shared=True, device='cpu').load_state_dict(state)


def test_stack_refuses_bad_arguments():
    for ids in ([], [0, -1], [1, 1], [0.5], [True], None, [2 ** 31]):
        with pytest.raises(ValueError, match="ids"):
            HN.OccupancyStack(CELLS, B, ids, device='cpu')
    with pytest.raises(ValueError, match="cells"):
        HN.OccupancyStack((3, 4), B, IDS, device='cpu')
    with pytest.raises(ValueError, match="cells"):
        HN.OccupancyStack((3, 4, 2049), B, IDS, device='cpu')
    with pytest.raises(ValueError):                             # hi <= lo
        HN.OccupancyStack(CELLS, (-1.0, 1.0, 1.0, 1.0, -1.0, 1.0), IDS, device='cpu')
    with pytest.raises(ValueError):
        HN.OccupancyStack(CELLS, (-1.0, 1.0, -1.0, float("inf"), -1.0, 1.0), IDS, device='cpu')
    with pytest.raises(ValueError):                             # five bounds for three axes
        HN.OccupancyStack(CELLS, B[:5], IDS, device='cpu')
    stack = HN.OccupancyStack(CELLS, B, IDS, device='cpu')
    with pytest.raises(ValueError, match="cells"):              # a set with other cells
        stack.set(0, occ_for(0, cells=(3, 4, 5)))
    with pytest.raises(ValueError, match="cells"):              # ... or other bounds
        stack.set(0, occ_for(0, bounds=(-2.0, 1.0, -1.0, 1.0, -1.0, 1.0)))
    with pytest.raises(ValueError, match="not one of the ids"):
        stack.set(1, occ_for(0))
    with pytest.raises(ValueError, match="not one of the ids"):
        stack.occupancy(3)
    with pytest.raises(ValueError, match="slot"):
        stack.set(3, occ_for(0), slot=True)
    with pytest.raises(ValueError, match="occupancy is a dict"):
        stack.set(0, "grid")
    assert torch.equal(stack.bits[0], full_bits())              # nothing was written


# ---- 2. the schedule --------------------------------------------------------------------------------------------------------------
def stub_model():
    return types.SimpleNamespace(use_sample_at_infinity=True, near=0.5, far=6.0, training=True)


def scheduled(shared, **kw):
    calls = []

    def builder(frame_id):
        calls.append(frame_id)
        return occ_for(frame_id)
    args = dict(warmup_steps=3, refresh_every=2, frames_per_refresh=2)
    args.update(kw)
    occ = TrainOccupancy(stub_model(), B, tuple(c + 1 for c in CELLS), {0, 2, 5}, 0.5, shared=shared, builder=builder,
                         device='cpu', **args)
    return occ, calls


def test_schedule_builds_the_ids_round_robin_in_per_frame_mode():
    """warmup_steps=3, refresh_every=2, frames_per_refresh=2, ids {0, 2, 5}: nothing before steps 0-2, then before step 3
    ids 0 and 2, before step 5 ids 5 and 0, before step 7 ids 2 and 5, before step 9 ids 0 and 2; every build lands in its
    frame's slot and an unvisited frame stays all-occupied."""
    occ, calls = scheduled(False)
    assert occ.stack.ids == IDS and occ.stack.cells == CELLS and occ.clip_far is False
    built_before = {}
    for step in range(10):
        seen = len(calls)
        occ.before_step()
        built_before[step] = calls[seen:]
        if step < 3:
            assert all(torch.equal(occ.stack.bits[s], full_bits()) for s in range(3))       # the warm-up: all-occupied
        if step == 3:
            assert torch.equal(occ.stack.bits[0], occ_for(0)['bits']) and torch.equal(occ.stack.bits[1], occ_for(2)['bits'])
            assert torch.equal(occ.stack.bits[2], full_bits())                              # frame 5: not visited yet
        if step == 5:
            assert torch.equal(occ.stack.bits[2], occ_for(5)['bits'])
    assert built_before == {0: [], 1: [], 2: [], 3: [0, 2], 4: [], 5: [5, 0], 6: [], 7: [2, 5], 8: [], 9: [0, 2]}
    assert occ.steps_begun == 10 and occ.refreshes == 4 and occ.cursor == 2


def test_schedule_swaps_the_shared_grid_when_the_round_wraps():
    occ, calls = scheduled(True)
    union = torch.from_numpy(R.pack(grid_for(0) | grid_for(2) | grid_for(5)))
    assert occ.stack.n_slots == 1 and occ.pending is not None
    live = []
    for step in range(8):
        occ.before_step()
        live.append(occ.stack.bits[0].clone())
    for step in range(5):                                       # before step 5 the round has not wrapped: all-occupied
        assert torch.equal(live[step], full_bits()), step
    assert calls == [0, 2, 5, 0, 2, 5]
    # the refresh before step 5 builds 5 (the round wraps: live = 0 | 2 | 5, pending cleared), then 0 into the new round
    assert torch.equal(live[5], union) and torch.equal(live[6], union)
    # the refresh before step 7 builds 2 and 5: the round wraps again with the same union
    assert torch.equal(live[7], union) and not occ.pending.any()
    assert not torch.equal(union, full_bits())


def test_schedule_edge_cases_and_state():
    occ, calls = scheduled(False, warmup_steps=0, refresh_every=1, frames_per_refresh=1)
    for _ in range(4):
        occ.before_step()
    assert calls == [0, 2, 5, 0]
    state = occ.state_dict()
    other, other_calls = scheduled(False, warmup_steps=0, refresh_every=1, frames_per_refresh=1)
    other.load_state_dict(state)
    other.before_step()
    assert other_calls == [2] and torch.equal(other.stack.bits, occ.stack.bits)
    model = stub_model()
    model.training = True
    flips = TrainOccupancy(model, B, 4, [1], 0.5, builder=lambda fid: (setattr(model, 'training', False), occ_for(1, (3, 3, 3)))[1],
                           warmup_steps=0, refresh_every=1, clip_far=True, device='cpu')
    model.train = lambda mode: setattr(model, 'training', mode)
    flips.before_step()
    assert model.training is True and flips.clip_far is True    # a builder that left the model in eval mode: put back
    wrong = TrainOccupancy(stub_model(), B, 4, [1], 0.5, builder=lambda fid: occ_for(1), warmup_steps=0, refresh_every=1,
                           device='cpu')
    with pytest.raises(ValueError, match="cells"):
        wrong.before_step()


def test_train_occupancy_refuses_bad_arguments():
    def make(**kw):
        args = dict(model=stub_model(), bounds=B, resolution=5, ids=[0, 1], sigma_min=0.5, builder=lambda fid: None, device='cpu')
        args.update(kw)
        return TrainOccupancy(**args)
    make()
    for bad in (dict(ids=[0, -2]), dict(ids=[3, 3]), dict(ids=[]), dict(resolution=1), dict(resolution=(5, 5)),
                dict(bounds=(0.0, 1.0, 0.0, 1.0, 1.0, 1.0)), dict(bounds=(0.0, 1.0, 0.0, 1.0)), dict(sigma_min=float("nan")),
                dict(dilate=-1), dict(warmup_steps=-1), dict(refresh_every=0), dict(frames_per_refresh=0), dict(refresh_every=1.5),
                dict(level='medium'), dict(chunk=0), dict(min_span=-1.0), dict(min_span=float("inf")), dict(builder="grid")):
        with pytest.raises(ValueError):
            make(**bad)


# ---- 3. the slot lookup, restated ---------------------------------------------------------------------------------------------------
def test_restated_slot_lookup():
    slot_of_id = [1, -1, 0, 7, 2]
    values = np.asarray([0, 1, 2, 3, 4, 5, -1, -0.5, 2.5, np.nan, np.inf, -np.inf, 1e30, -0.0, 4.999], dtype=np.float32)
    got = RT.slots_of(values, slot_of_id, 3)
    #                   0   1  2   3 (slot 7 >= n_slots)  4  5 (>= n_ids)  -1  -0.5 -> id 0  2.5 -> id 2
    assert got.tolist() == [1, -1, 0, -1, 2, -1, -1, 1, 0, -1, -1, -1, -1, 1, 2]


def test_restated_clip_batch_is_the_walk_per_slot():
    rays = R.probe_rays(n=300, seed=3)
    rays[:, 8] = np.random.default_rng(4).choice([0, 1, 2, 3, -1, np.nan, 1.5], size=300)
    grids = [R.probe_grid(seed=11), R.probe_grid(seed=12)]
    out = RT.clip_batch(rays, grids, [1, -1, 0], R.BOUNDS, R.NEAR, R.FAR)
    assert set(out['slot'].tolist()) == {-1, 0, 1}
    for slot, values in ((1, (0,)), (0, (2,)), (-1, (1, 1.5, 3, -1))):
        rows = np.isin(rays[:, 8], values)
        assert rows.any() and (out['slot'][rows] == slot).all()
    rows = out['slot'] == 0
    want = R.clip_rays(rays[rows], grids[0], R.BOUNDS, R.NEAR, R.FAR)
    assert out['rays'][rows].tobytes() == want['rays'].tobytes() and np.array_equal(out['hit'][rows], want['hit'])
    none = out['slot'] == -1
    assert np.isnan(rays[none, 8]).any()
    assert out['rays'][none].tobytes() == rays[none].tobytes() and not out['hit'][none].any()
    assert (out['affine'][none] == (0.0, 1.0)).all() and out['hit_count'] == out['hit'].sum() > 0
    assert np.array_equal(out['viewdirs'], rays[:, 3:6])
    keep = RT.clip_batch(rays, grids, [1, -1, 0], R.BOUNDS, R.NEAR, R.FAR, clip_far=False)
    assert (keep['t'][:, 1] == np.float32(R.FAR)).all() and np.array_equal(keep['t'][:, 0], out['t'][:, 0])
    one = RT.clip_batch(rays[:, :8], grids, [1, -1, 0], R.BOUNDS, R.NEAR, R.FAR)      # no id column: every ray has id 0
    assert (one['slot'] == 1).all()


# ---- 4. clip_batch's refusals, before any device work ---------------------------------------------------------------------------------
def test_clip_batch_refuses_bad_arguments():
    stack = HN.OccupancyStack(CELLS, B, IDS, device='cpu')
    rays = torch.zeros((4, 9))
    for bad_rays in (torch.zeros((4, 5)), torch.zeros((4, 65)), torch.zeros((4, 9), dtype=torch.float64), torch.zeros(36), "rays"):
        with pytest.raises(ValueError, match="rays must be"):
            HN.clip_batch(bad_rays, stack, 0.5, 6.0)
    with pytest.raises(ValueError, match="OccupancyStack"):
        HN.clip_batch(rays, stack.occupancy(0), 0.5, 6.0)
    for near, far in ((6.0, 0.5), (0.5, 0.5), (0.5, float("inf")), (float("nan"), 6.0), ("a", 6.0)):
        with pytest.raises(ValueError, match="near and far"):
            HN.clip_batch(rays, stack, near, far)
    for span in (-1.0, float("nan"), "wide"):
        with pytest.raises(ValueError, match="min_span"):
            HN.clip_batch(rays, stack, 0.5, 6.0, min_span=span)
    for col in (3, 9, 1.0, True):
        with pytest.raises(ValueError, match="id_col"):
            HN.clip_batch(rays, stack, 0.5, 6.0, id_col=col)
    with pytest.raises(ValueError, match="on the GPU"):         # everything else was fine: no CPU fallback
        HN.clip_batch(rays, stack, 0.5, 6.0)
    assert F.clip_batch is HN.clip_batch is OPS.clip_batch and F.OccupancyStack is HN.OccupancyStack is OPS.OccupancyStack


def test_c_abi_refuses_bad_arguments_without_a_launch():
    """Every status is decided on the host before any launch (the pointers are made up or NULL)."""
    lib = L.load()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    bounds = (ctypes.c_float * 6)(*B)

    def clip(**kw):
        a = dict(rays=p, n=4, ld=9, id_col=8, bits=p, n_slots=2, cx=3, cy=3, cz=3, slots=p, n_ids=4, bounds=bounds, near=0.5,
                 far=6.0, clip_far=1, min_span=0.0, out=None, dirs=None, affine=None, hit=None, count=None)
        a.update(kw)
        return lib.hn_occ_clip_batch(a['rays'], a['n'], a['ld'], a['id_col'], a['bits'], a['n_slots'], a['cx'], a['cy'], a['cz'],
                                     a['slots'], a['n_ids'], a['bounds'], a['near'], a['far'], a['clip_far'], a['min_span'],
                                     a['out'], a['dirs'], a['affine'], a['hit'], a['count'], None)

    assert clip(rays=None) == -3 and clip(bits=None) == -3 and clip(slots=None) == -3
    for bad in (dict(n=0), dict(n=2 ** 31), dict(ld=5), dict(ld=65), dict(id_col=9), dict(id_col=5), dict(id_col=0),
                dict(ld=8, id_col=8), dict(n_slots=0), dict(n_ids=0), dict(cx=0), dict(cz=2049), dict(bounds=None),
                dict(bounds=(ctypes.c_float * 6)(0, 1, 0, 1, 1, 1)), dict(bounds=(ctypes.c_float * 6)(0, 1, 0, float("inf"), 0, 1)),
                dict(far=0.5), dict(far=float("inf")), dict(near=float("nan")), dict(min_span=-1.0),
                dict(min_span=float("nan")), dict(out=p)):
        assert clip(**bad) == -2, bad
    assert len(L.ARGTYPES["hn_occ_clip_batch"]) == 22 and "hn_occ_clip_batch" in L.EXPORTS
    assert L.load().hn_version() == 340 and len(L.STRUCTS) == 17      # a plain-argument entry point: the ABI's structs stay
    del q


# ---- 5. TrainStep(occupancy=) ---------------------------------------------------------------------------------------------------
def test_trainstep_refuses_occupancy_under_data_parallelism(tmp_path):
    import torch.distributed as dist
    model = torch.nn.Linear(3, 3)
    occ = TrainOccupancy(model, B, 5, [0], 0.5, builder=lambda fid: None, clip_far=False, device='cpu')
    with pytest.raises(ValueError, match="TrainOccupancy"):
        TrainStep(model, occupancy="grid")
    with pytest.raises(ValueError, match="another model"):
        TrainStep(torch.nn.Linear(3, 3), occupancy=occ)
    dist.init_process_group("gloo", store=dist.FileStore(os.path.join(str(tmp_path), "store"), 1), rank=0, world_size=1)
    try:
        with pytest.raises(ValueError, match="data parallelism"):
            TrainStep(model, force_dp=True, occupancy=occ)
    finally:
        dist.destroy_process_group()
