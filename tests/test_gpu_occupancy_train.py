"""Training-time occupancy on the GPU (csrc/hn_occupancy.hip's hn_occ_clip_batch): the batch clip against
clip_rays per frame and against the NumPy restatement of tests/occupancy_train_restated.py, bit for bit; a replayed graph
that sees the stack's updates; and TrainStep(occupancy=) — identical to the plain step under all-occupied grids, intact
across real refreshes, equal to a hand-run clip + model call under a partial grid, one more launch per step."""
import json
import os

import numpy as np
import pytest
import torch

import hashprng as H
import hypernerf_torch_amd as HN
import occupancy_restated as R
import occupancy_train_restated as RT
from gpu_common import DEV, EMB, load_hash, rays_for
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd.datasets import LLFFDataset, RayBatcher
from hypernerf_torch_amd.hypernerf import model_utils, models
from hypernerf_torch_amd.losses import MSELoss
from hypernerf_torch_amd.training import _EXTRA, TrainOccupancy, TrainStep
from llff_scene import make_scene, write_scene

pytestmark = pytest.mark.gpu

# the probe of DESIGN.md 3.18 and a second geometry of the same edge (0.25: every plane is exact in fp32) whose rows
# cross a word boundary (70 cells along z)
GEOMETRIES = {"probe": (R.CELLS, R.BOUNDS), "two_words": ((5, 4, 70), (-0.5, 0.75, -0.5, 0.5, -8.75, 8.75))}
STACK_IDS = (0, 1, 2, 3, 5)          # n_ids = 6; id 4 has no grid
ID_VALUES = np.asarray([0, 1, 2, 3, 4, 5, 6, -1, np.nan, 2.5], dtype=np.float32)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def make_stack(name):
    """Slots 0-2 (ids 0, 1, 2): different random grids, about 14 % occupied; slot 3 (id 3): empty; slot 4 (id 5): full."""
    cells, bounds = GEOMETRIES[name]
    rng = np.random.default_rng(sum(cells))
    grids = [rng.random(cells) < 0.14 for _ in range(3)] + [np.zeros(cells, dtype=bool), np.ones(cells, dtype=bool)]
    stack = HN.OccupancyStack(cells, bounds, STACK_IDS, device=DEV)
    for fid, grid in zip(STACK_IDS, grids):
        stack.set(fid, {'bits': gpu(R.pack(grid)), 'cells': cells, 'bounds': bounds})
    return stack, grids


def probe_rays(n=1024):
    rays = R.probe_rays(n=n, seed=5)
    rays[:, 8] = np.random.default_rng(6).choice(ID_VALUES, size=n)
    return rays


# ---- 1. the kernel against clip_rays and the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("clip_far", [True, False])
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_clip_batch_is_clip_rays_per_frame_bit_for_bit(geometry, clip_far):
    stack, grids = make_stack(geometry)
    cells, bounds = GEOMETRIES[geometry]
    assert stack.slot_of_id.tolist() == [0, 1, 2, 3, -1, 4]
    rays9 = probe_rays()
    for rays in (rays9, np.ascontiguousarray(rays9[:, :8])):          # 8 columns: id_col = -1, every ray has id 0
        n, ld = rays.shape
        for min_span in (0.0, None):
            span = 0.25 if min_span is None else min_span             # None: the smallest cell edge
            out = HN.clip_batch(gpu(rays), stack, R.NEAR, R.FAR, clip_far=clip_far, min_span=min_span)
            got = host(out)
            want = RT.clip_batch(rays, grids, stack.slot_of_id.tolist(), bounds, R.NEAR, R.FAR, clip_far=clip_far,
                                 min_span=span)
            for k in ('rays', 'viewdirs', 'affine', 'hit'):
                assert got[k].tobytes() == want[k].tobytes(), (k, ld, min_span)
            assert got['hit_count'].shape == () and int(got['hit_count']) == int(got['hit'].sum()) == int(want['hit_count'])
            assert got['viewdirs'].tobytes() == rays[:, 3:6].tobytes()
            slot = want['slot']
            for s, fid in enumerate(STACK_IDS):
                rows = np.nonzero(slot == s)[0]
                if ld == 8 and s != 0:
                    assert rows.size == 0
                    continue
                assert rows.size > 50, (s, rows.size)
                ref = host(HN.clip_rays(gpu(rays[rows]), stack.occupancy(fid), R.NEAR, R.FAR, clip_far=clip_far,
                                        min_span=min_span))
                for k in ('rays', 'affine', 'hit'):
                    assert got[k][rows].tobytes() == ref[k].tobytes(), (k, s, ld, min_span)
                assert ref['t'].tobytes() == want['t'][rows].tobytes(), (s, ld, min_span)
                if s < 3:
                    assert 0 < ref['hit'].sum() < rows.size               # a random grid: hits and misses
                if s == 3:
                    assert ref['hit'].sum() == 0                          # the empty grid
            none = slot == -1
            if ld == 9:
                assert none.sum() > 200 and np.isnan(rays[none, 8]).any() and (rays[none, 8] == 4).any()
                assert (slot[rays[:, 8] == 2.5] == 2).all()              # (int)2.5 is id 2
            assert got['rays'][none].tobytes() == rays[none].tobytes() and not got['hit'][none].any()
            assert (got['affine'][none] == (0.0, 1.0)).all()
            assert not got['hit'][slot == 3].any() and got['rays'][slot == 3].tobytes() == rays[slot == 3].tobytes()
            if clip_far is False:
                hit = got['hit'] == 1                                     # the far end stays: a + b * far == far
                b = got['affine'][hit, 1].astype(np.float64)
                assert np.abs(got['affine'][hit, 0] + b * R.FAR - R.FAR).max() < 1e-5 * R.FAR
            # the same rows from three calls into caller-owned buffers
            bufs = {'rays': torch.zeros((n, ld), device=DEV), 'viewdirs': torch.zeros((n, 3), device=DEV),
                    'affine': torch.zeros((n, 2), device=DEV), 'hit': torch.zeros((n,), dtype=torch.uint8, device=DEV)}
            dev_rays, counts = gpu(rays), []
            for a, b_ in ((0, 1), (1, 333), (333, n)):
                part = {k: v[a:b_] for k, v in bufs.items()}
                part['hit_count'] = torch.zeros((), dtype=torch.int64, device=DEV)
                back = HN.clip_batch(dev_rays[a:b_], stack, R.NEAR, R.FAR, clip_far=clip_far, min_span=min_span, out=part)
                assert back is part and back['rays'].data_ptr() == bufs['rays'][a:b_].data_ptr()
                counts.append(int(part['hit_count']))
            for k in bufs:
                assert bufs[k].cpu().numpy().tobytes() == got[k].tobytes(), (k, ld, min_span)      # bytes: the NaN ids
            assert sum(counts) == int(got['hit_count'])
    none = HN.clip_batch(gpu(rays9[:0]), stack, R.NEAR, R.FAR)
    assert none['rays'].shape == (0, 9) and none['viewdirs'].shape == (0, 3) and int(none['hit_count']) == 0


# ---- 2. hand-made rays --------------------------------------------------------------------------------------------------------------
def test_clip_batch_handmade_rays():
    rays, names = R.handmade_rays()                                       # every row has frame id 7
    probe, full = R.probe_grid(), np.ones(R.CELLS, dtype=bool)
    stack = HN.OccupancyStack(R.CELLS, R.BOUNDS, [7, 9], device=DEV)
    stack.set(7, {'bits': gpu(R.pack(probe)), 'cells': R.CELLS, 'bounds': R.BOUNDS})
    both = np.concatenate([rays, rays])
    both[len(rays):, 8] = 9                                               # ... and once more against the full grid of id 9
    for clip_far in (True, False):
        got = host(HN.clip_batch(gpu(both), stack, R.NEAR, R.FAR, clip_far=clip_far, min_span=0.0))
        assert np.isfinite(got['affine']).all()
        for fid, rows, cells in ((7, slice(0, len(rays)), probe), (9, slice(len(rays), None), full)):
            ref = host(HN.clip_rays(gpu(both[rows]), stack.occupancy(fid), R.NEAR, R.FAR, clip_far=clip_far, min_span=0.0))
            want = R.clip_rays(both[rows], cells, R.BOUNDS, R.NEAR, R.FAR, clip_far=clip_far)
            for k in ('rays', 'affine', 'hit'):
                assert got[k][rows].tobytes() == ref[k].tobytes() == want[k].tobytes(), (k, fid, clip_far)
            for name, h, row, src in zip(names, got['hit'][rows], got['rays'][rows], both[rows]):
                if any(w in name for w in ("NaN", "inf", "misses", "away", "outside")):
                    assert h == 0, name
                if h == 0:
                    assert row.tobytes() == src.tobytes(), name
                else:
                    assert np.isfinite(row).all(), name
        full_hits = got['hit'][len(rays):]
        assert full_hits[names.index("origin inside, first cell")] == 1 and full_hits[names.index("axis-parallel +x")] == 1
        assert full_hits[names.index("-0.0 components")] == 1 and full_hits[names.index("zero direction inside")] == 1
        assert int(got['hit_count']) == int(got['hit'].sum())


# ---- 3. a replayed graph sees the stack's updates --------------------------------------------------------------------------------------
def test_replayed_graph_sees_fill_and_set():
    rays_np = R.probe_rays(n=777, seed=8)
    rays_np[:, 8] = 7
    rays = gpu(rays_np)
    stack = HN.OccupancyStack(R.CELLS, R.BOUNDS, [7], device=DEV)
    out = {'rays': torch.zeros_like(rays), 'viewdirs': torch.zeros((777, 3), device=DEV),
           'affine': torch.zeros((777, 2), device=DEV), 'hit': torch.zeros((777,), dtype=torch.uint8, device=DEV),
           'hit_count': torch.zeros((), dtype=torch.int64, device=DEV)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        HN.clip_batch(rays, stack, R.NEAR, R.FAR, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        HN.clip_batch(rays, stack, R.NEAR, R.FAR, out=out)

    def replayed():
        for v in out.values():
            v.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}

    first = replayed()
    eager = HN.clip_batch(rays, stack, R.NEAR, R.FAR)
    for k in out:
        assert torch.equal(first[k], eager[k]), k
    assert 100 < int(first['hit_count']) < 777                          # all-occupied: the rays that cross the box
    stack.fill(False)
    empty = replayed()
    assert int(empty['hit_count']) == 0 and not empty['hit'].any() and torch.equal(empty['rays'], rays)
    assert (empty['affine'] == torch.tensor([0.0, 1.0], device=DEV)).all()
    stack.set(7, {'bits': gpu(R.pack(R.probe_grid())), 'cells': R.CELLS, 'bounds': R.BOUNDS})
    partial = replayed()
    eager = HN.clip_batch(rays, stack, R.NEAR, R.FAR)
    for k in out:
        assert torch.equal(partial[k], eager[k]), k
    assert 0 < int(partial['hit_count']) < int(first['hit_count'])
    want = RT.clip_batch(rays_np, [R.probe_grid()], stack.slot_of_id.tolist(), R.BOUNDS, R.NEAR, R.FAR, min_span=0.25)
    assert partial['rays'].cpu().numpy().tobytes() == want['rays'].tobytes()


# ---- TrainStep(occupancy=) ---------------------------------------------------------------------------------------------------------------
ROWS, NC, NF = 64, 8, 8
KW = dict(hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True, view_fourier_dim=6)
BOX = (-8.0, 8.0) * 3          # |o| <= 1.74 and far * |d| <= 1.6: every ray's [near, far] segment lies inside


def _model(seed, precision="fp32"):
    HN.set_precision(precision)
    m = models.NerfModel(EMB, n_samples_coarse=NC, n_samples_fine=NF, noise_std=None, **KW)
    load_hash(m, seed)
    return m.to(DEV)


def _inputs(seed):
    """64 rays, every one of ANOTHER frame.  The gradient of a GLO table row is a float atomic add per ray
    (hn_embed_backward): with three or more rays on one row its last bits depend on their arrival order, and two plain
    runs already differ (measured: 1 .. 33 of 800 entries after one step, everything a step later).  One ray per frame
    leaves nothing to reorder, so "bit for bit" below is a statement about the feature."""
    o, d, _ = rays_for(seed, ROWS)
    ids = torch.from_numpy(np.random.default_rng(seed).permutation(100)[:ROWS].astype(np.float32))[:, None]
    rays = torch.cat([o, d, torch.zeros(ROWS, 1), torch.ones(ROWS, 1), ids], dim=1).to(DEV)
    rgbs = H.uniform(seed, "rgbs", (ROWS, 3), 0.1, 0.9).to(DEV)
    return rays, rgbs


def _rng(seed, step):
    return {"t_rand": H.uniform(seed + step, "t", (ROWS, NC), 0, 1).to(DEV),
            "u": H.uniform(seed + step, "u", (ROWS, NF), 0, 1).to(DEV)}


def _frame_ids(rays):
    return sorted({int(v) for v in rays[:, 8].tolist()})


@pytest.fixture(scope="module")
def llff_root(tmp_path_factory):
    # 65 frames of ONE pixel: a batch of 64 rays is an epoch and holds every training frame once (see _inputs)
    pixels, poses_bounds = make_scene(n_images=65, h=1, w=1, seed=22, focal=1.0)
    return write_scene(str(tmp_path_factory.mktemp("occupancy_train")), pixels, poses_bounds)


# ---- 4. identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_all_occupied_grids_train_the_plain_step_bit_for_bit(use_graph):
    """fp32, injected draws: under TrainOccupancy(warmup_steps=100) every grid stays all-occupied, the box holds every
    ray's [near, far] segment, so every affine is (0, 1), every row keeps its bits, and four steps leave the arena of a
    plain TrainStep from the same seed."""
    seed = 61
    rays, rgbs = _inputs(seed)
    arenas, logs = {}, {}
    for name in ("plain", "occupancy"):
        m = _model(seed)
        occ = None
        if name == "occupancy":
            occ = TrainOccupancy(m, BOX, 9, _frame_ids(rays), 0.5, warmup_steps=100)
            clip = HN.clip_batch(rays, occ.stack, m.near, m.far, clip_far=occ.clip_far)
            assert (clip['affine'] == torch.tensor([0.0, 1.0], device=DEV)).all() and torch.equal(clip['rays'], rays)
            assert int(clip['hit_count']) == ROWS and occ.clip_far is False
        ts = TrainStep(m, lr=1e-3, use_graph=use_graph, occupancy=occ)
        logs[name] = [ts.step(rays, rgbs, rng=_rng(seed, i)) for i in range(4)]
        arenas[name] = ts.arena.data.clone()
        assert (ts._graph is not None) == use_graph
        if occ is not None:
            assert occ.steps_begun == 4 and occ.refreshes == 0
    diff = (arenas["plain"] - arenas["occupancy"]).abs()
    print(f"graph={use_graph}: max |diff| {float(diff.max()):.3e}, entries that differ {int((diff > 0).sum())}")
    for a, b in zip(logs["plain"], logs["occupancy"]):
        assert torch.equal(a["train/loss"], b["train/loss"]) and torch.equal(a["train/psnr"], b["train/psnr"])
        assert float(b["train/occupancy_hit"]) == 1.0 and float(b["train/occupancy_span"]) == 1.0
        assert "train/occupancy_hit" not in a
    assert torch.equal(arenas["plain"], arenas["occupancy"])
    assert not torch.equal(arenas["plain"], TrainStep(_model(seed), lr=1e-3).arena.data)      # the four steps moved it


@pytest.mark.parametrize("use_graph", [False, True])
def test_all_occupied_grids_with_a_batcher_train_the_plain_step_bit_for_bit(llff_root, use_graph):
    """The same with the batch gathered inside the step (RayBatcher over a synthetic LLFF scene of 64 training frames of
    one pixel: every step is an epoch in a new order): the clip launch follows the gather launch and reads the batch it
    wrote."""
    seed = 63
    ds = LLFFDataset(llff_root, split="train", img_wh=(1, 1), include_idx=True)
    ids = _frame_ids(ds.all_rays)
    assert len(ds) == ROWS and len(ids) == ROWS
    arenas, logs = {}, {}
    for name in ("plain", "occupancy"):
        m = _model(seed)
        # the rig spreads its 65 cameras over several units: a box that holds all of their NDC rays for certain
        occ = TrainOccupancy(m, (-64.0, 64.0) * 3, 9, ids, 0.5, warmup_steps=100) if name == "occupancy" else None
        ts = TrainStep(m, lr=1e-3, use_graph=use_graph, occupancy=occ,
                       batcher=RayBatcher(ds, ROWS, generator=torch.Generator().manual_seed(9)))
        logs[name] = [ts.step(rng=_rng(seed, i)) for i in range(4)]
        arenas[name] = ts.arena.data.clone()
        if occ is not None:
            clip = HN.clip_batch(ts.batcher.rays, occ.stack, m.near, m.far, clip_far=False)
            assert (clip['affine'] == torch.tensor([0.0, 1.0], device=DEV)).all()
    diff = (arenas["plain"] - arenas["occupancy"]).abs()
    print(f"graph={use_graph}: max |diff| {float(diff.max()):.3e}, entries that differ {int((diff > 0).sum())}")
    for a, b in zip(logs["plain"], logs["occupancy"]):
        assert torch.equal(a["train/loss"], b["train/loss"])
        assert float(b["train/occupancy_hit"]) == 1.0
    assert torch.equal(arenas["plain"], arenas["occupancy"])
    assert len({float(lg["train/loss"]) for lg in logs["plain"]}) == 4          # four batches in four orders, a moving model


# ---- 5. a real refresh leaves the step intact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_refreshes_between_replays_leave_the_step_intact(precision):
    """sigma_min = 0 marks every cell of a refreshed grid (!(sigma < 0)), so the grids stay all-occupied while every step
    after the first is preceded by a no-grad query of the field for one frame: six graphed steps leave the parameters and
    every logged loss of the plain run, bit for bit."""
    seed = 65
    rays, rgbs = _inputs(seed)
    ids = _frame_ids(rays)
    runs, hits = {}, []
    for name in ("plain", "occupancy"):
        m = _model(seed, precision)
        occ = TrainOccupancy(m, BOX, 9, ids, 0.0, warmup_steps=1, refresh_every=1) if name == "occupancy" else None
        ts = TrainStep(m, lr=1e-3, use_graph=True, occupancy=occ)
        steps = []
        for i in range(6):
            log = ts.step(rays, rgbs, rng=_rng(seed, i))
            steps.append((ts.arena.data.clone(), log))
            assert m.training and ts._graph is not None
            if occ is not None:
                print(f"{precision} step {i}: occupancy_hit {float(log['train/occupancy_hit'])!r}")
                hits.append((float(log["train/occupancy_hit"]), float(log["train/occupancy_span"])))
        runs[name] = steps
        if occ is not None:
            assert occ.refreshes == 5 and occ.cursor == 5 % len(ids)
            full = gpu(RT.all_occupied_bits(occ.stack.cells))
            assert all(torch.equal(occ.stack.bits[s], full) for s in range(occ.stack.n_slots))
    for i, ((pa, la), (pb, lb)) in enumerate(zip(runs["plain"], runs["occupancy"])):
        diff = (pa - pb).abs()
        print(f"{precision} step {i}: max |diff| {float(diff.max()):.3e}, entries that differ {int((diff > 0).sum())}, "
              f"loss {float(la['train/loss']):.8f} / {float(lb['train/loss']):.8f}")
    for i, ((pa, la), (pb, lb)) in enumerate(zip(runs["plain"], runs["occupancy"])):
        assert torch.equal(la["train/loss"], lb["train/loss"]) and torch.equal(la["train/psnr"], lb["train/psnr"]), i
        assert torch.equal(pa, pb), i
    assert not torch.equal(runs["plain"][0][0], runs["plain"][5][0])
    assert hits == [(1.0, 1.0)] * 6, hits


# ---- 6. a partial grid --------------------------------------------------------------------------------------------------------------
def _half_grid():
    cells = np.zeros((8, 8, 8), dtype=bool)
    cells[4:] = True                                                     # x >= 0 of the box (-2, 2)^3
    return {'bits': gpu(R.pack(cells)), 'cells': (8, 8, 8), 'bounds': (-2.0, 2.0) * 3}


def _partial(rays, m):
    """One shared grid for the frames of `rays` (one ray per frame, see _inputs), set by hand through one frame id."""
    ids = _frame_ids(rays)
    occ = TrainOccupancy(m, (-2.0, 2.0) * 3, 9, ids, 0.5, shared=True, warmup_steps=100)
    occ.stack.set(ids[0], _half_grid())
    return occ


def test_partial_grid_step_is_the_hand_run_clip_and_model_call():
    seed = 67
    rays, rgbs = _inputs(seed)
    rng = _rng(seed, 0)
    # the step's forward + backward, eager
    m = _model(seed)
    occ = _partial(rays, m)
    ts = TrainStep(m, lr=1e-3, use_graph=False, occupancy=occ)
    ts._rays, ts._rgbs, ts._rng = rays.clone(), rgbs.clone(), rng
    ts._forward_backward()
    ts.optimizer.finish_gradients()
    torch.cuda.synchronize()
    grad, log = ts.arena.grad.clone(), {k: v.clone() for k, v in ts._log.items()}
    # by hand, from the same parameters and draws
    m2 = _model(seed)
    ts2 = TrainStep(m2, lr=1e-3, use_graph=False)
    clip = HN.clip_batch(rays, occ.stack, m2.near, m2.far, clip_far=False)
    ray_dict = model_utils.prepare_ray_dict(clip['rays'])
    ray_dict['viewdirs'] = clip['viewdirs']
    results = m2(ray_dict, dict(_EXTRA), rng=rng)
    loss = MSELoss()(results, rgbs)
    F.backward(loss, 1.0)
    ts2.optimizer.finish_gradients()
    torch.cuda.synchronize()
    hit = float(log["train/occupancy_hit"])
    print(f"loss {float(log['train/loss']):.8f} / by hand {float(loss):.8f}; hit {hit}; span {float(log['train/occupancy_span'])}")
    assert torch.equal(log["train/loss"], loss.detach())
    assert torch.equal(grad, ts2.arena.grad) and bool(grad.abs().sum() > 0)
    assert 0.0 < hit < 1.0 and hit == float(clip['hit'].sum()) / ROWS
    assert torch.equal(log["train/occupancy_span"], clip['affine'][:, 1].mean()) and float(log["train/occupancy_span"]) < 1.0
    assert torch.equal(clip['viewdirs'], rays[:, 3:6]) and not torch.equal(clip['rays'], rays)
    # and it is another step than the plain one
    m3 = _model(seed)
    ts3 = TrainStep(m3, lr=1e-3, use_graph=False)
    ts3._rays, ts3._rgbs, ts3._rng = rays.clone(), rgbs.clone(), rng
    ts3._forward_backward()
    assert not torch.equal(ts3._log["train/loss"], log["train/loss"])


def test_partial_grid_graphed_step_equals_the_eager_step():
    seed = 67
    rays, rgbs = _inputs(seed)
    res = {}
    for use_graph in (False, True):
        m = _model(seed)
        ts = TrainStep(m, lr=1e-3, use_graph=use_graph, occupancy=_partial(rays, m))
        log = ts.step(rays, rgbs, rng=_rng(seed, 0))
        res[use_graph] = (ts.arena.data.clone(), log)
        assert (ts._graph is not None) == use_graph
    diff = (res[True][0] - res[False][0]).abs()
    print(f"graph vs eager: max |diff| {float(diff.max()):.3e}, entries that differ {int((diff > 0).sum())}")
    for k in ("train/loss", "train/psnr", "train/occupancy_hit", "train/occupancy_span"):
        assert torch.equal(res[True][1][k], res[False][1][k]), k
    assert 0.0 < float(res[True][1]["train/occupancy_hit"]) < 1.0
    assert torch.equal(res[True][0], res[False][0])


# ---- 7. the launch list -----------------------------------------------------------------------------------------------------------------
class _Spy:
    """Names of the launches made through _lib.launch while active (eager code only)."""

    def __enter__(self):
        self.names, self._orig = [], L.launch

        def spy(name, *a, **k):
            self.names.append(name)
            return self._orig(name, *a, **k)
        L.launch = spy
        return self

    def __exit__(self, *exc):
        L.launch = self._orig
        return False


def _eager_launches(ts, rays, rgbs, steps=2):
    with _Spy() as spy:
        for _ in range(steps):
            ts.step(rays, rgbs)
    torch.cuda.synchronize()
    return spy.names


def test_occupancy_adds_one_launch_at_the_head_of_each_step(golden_dir):
    """Without the keyword two eager steps make the launches of tests/golden/g26_trainstep_launches.json; with it, the same
    list with ONE hn_occ_clip_batch in front of each step's first launch (the counter's memset node is no entry-point
    launch), nothing else changed or reordered."""
    with open(os.path.join(golden_dir, "g26_trainstep_launches.json")) as f:
        want = json.load(f)["launches"]
    seed = 45
    o, d, idx = rays_for(seed, ROWS)
    rays = torch.cat([o, d, torch.zeros(ROWS, 1), torch.ones(ROWS, 1), idx.float()[:, None]], dim=1).to(DEV)
    rgbs = H.uniform(seed, "rgbs", (ROWS, 3), 0.1, 0.9).to(DEV)
    F.seed_draws(5)
    got = _eager_launches(TrainStep(_model(seed), lr=1e-3, use_graph=False), rays, rgbs)
    assert got == want, (got, want)
    assert not any(n.startswith("hn_occ_") for n in got)
    m = _model(seed)
    occ = TrainOccupancy(m, BOX, 9, _frame_ids(rays), 0.5, warmup_steps=100)
    with_occ = _eager_launches(TrainStep(m, lr=1e-3, use_graph=False, occupancy=occ), rays, rgbs)
    half = len(want) // 2
    assert want[0] == want[half] == "hn_render_prologue" and want.count("hn_render_prologue") == 2
    expect = ["hn_occ_clip_batch"] + want[:half] + ["hn_occ_clip_batch"] + want[half:]
    assert with_occ == expect, (with_occ, expect)
