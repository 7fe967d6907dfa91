"""Occupancy grids and ray clipping on the GPU (csrc/hn_occupancy.hip): the four kernels against the NumPy
restatement and the float64 interval property of tests/occupancy_restated.py, the re-parametrisation, the wiring through
inference.render_image with a stub field, bit identity on a real NerfModel, and occupancy_grid / OccupancyCache."""
import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import occupancy_restated as R
from gpu_common import DEV, EMB, load_hash, rays_for
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import inference
from hypernerf_torch_amd.hypernerf import model_utils, models

pytestmark = pytest.mark.gpu


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_occ(cells_bool, bounds):
    return {'bits': gpu(R.pack(cells_bool)), 'cells': tuple(cells_bool.shape), 'bounds': tuple(float(v) for v in bounds)}


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. mark ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(13, 11, 10), (3, 3, 64), (3, 3, 65), (3, 3, 66), (4, 3, 131)])
def test_mark_is_the_restatement_bit_for_bit(shape):
    rng = np.random.default_rng(sum(shape))
    grid = rng.uniform(0.0, 1.2, size=shape).astype(np.float32)      # sigma_min = 1: about one point in six is dense
    flat = grid.reshape(-1)
    picks = rng.choice(flat.size, size=12, replace=False)
    flat[picks[0:4]] = 0.0
    flat[picks[4:6]] = np.nan
    flat[picks[6:8]] = np.inf
    flat[picks[8:10]] = 1.0                                          # equal to sigma_min: occupied
    flat[picks[10:12]] = -np.inf
    want = R.pack(R.mark(grid, 1.0))
    got = F.occupancy_mark(gpu(grid), 1.0)
    again = F.occupancy_mark(gpu(grid), 1.0)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want) and torch.equal(got, again)
    assert 0 < R.popcount(want) < np.prod([n - 1 for n in shape])
    only_nan = np.zeros(shape, dtype=np.float32)
    only_nan[1, 1, shape[2] - 1] = np.nan
    bits = F.occupancy_mark(gpu(only_nan), 1e30).cpu().numpy()
    assert np.array_equal(bits, R.pack(R.mark(only_nan, 1e30))) and R.popcount(bits) == 4
    assert int(F.occupancy_count(gpu(want))) == R.popcount(want)


# ---- 2. dilate, count ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cz", [9, 64, 65, 130])
def test_dilate_and_count(cz):
    rng = np.random.default_rng(200 + cz)
    cells = rng.random((5, 4, cz)) < 0.02
    cells[0, 0, 0] = cells[4, 3, cz - 1] = cells[4, 0, 0] = True      # corners and faces: nothing wraps
    if cz > 64:
        cells[2, 2, 63] = cells[1, 0, 64] = True                      # cell 63 reaches cell 64 and the reverse
    bits = gpu(R.pack(cells))
    for radius in (1, 2, 3):
        got = F.occupancy_dilate(bits, cells.shape, radius).cpu().numpy()
        back, pad = R.unpack(got, cz)
        want = R.dilate(cells, radius)
        assert np.array_equal(back, want) and not pad.any()
        assert int(F.occupancy_count(gpu(got))) == want.sum()
    if cz > 64:
        one = np.zeros((1, 1, cz), dtype=bool)
        one[0, 0, 63] = True
        grown = R.unpack(F.occupancy_dilate(gpu(R.pack(one)), one.shape).cpu().numpy(), cz)[0]
        assert np.nonzero(grown[0, 0])[0].tolist() == [62, 63, 64]
        one[:] = False
        one[0, 0, 64] = True
        grown = R.unpack(F.occupancy_dilate(gpu(R.pack(one)), one.shape).cpu().numpy(), cz)[0]
        assert np.nonzero(grown[0, 0])[0].tolist() == ([63, 64, 65] if cz > 65 else [63, 64])
    assert F.occupancy_dilate(bits, cells.shape, 0).data_ptr() == bits.data_ptr()      # no launch, no copy
    assert torch.equal(bits, gpu(R.pack(cells)))                      # the input is never written
    occ = HN.occupancy_from_density(gpu(np.where(R.dilate(cells, 0), 2.0, 0.0).astype(np.float32)), R.BOUNDS, 1.0, dilate=0)
    assert abs(HN.occupancy_fraction(occ) - R.mark(np.where(cells, 2.0, 0.0), 1.0).mean()) < 1e-12


# ---- 3. clip: the interval property ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    occupied, rays = R.probe_grid(), R.probe_rays()
    return occupied, rays, to_occ(occupied, R.BOUNDS)


def test_clip_satisfies_the_interval_property(probe):
    """The issue's probe: 12 x 10 x 9 cells, about 15 % occupied, 4000 rays, near 0.5, far 6, eps = 32 ulp of far; at most
    1 % of the rays may have a cell between required and allowed; hits and misses both above 10 %.  The NumPy restatement
    measured 0.1 % / 62.7 % / 37.3 % on these rays."""
    occupied, rays, occ = probe
    out = host(HN.clip_rays(gpu(rays), occ, R.NEAR, R.FAR, min_span=0.0))
    shares = R.check_intervals(rays, occupied, R.BOUNDS, R.NEAR, R.FAR, out['t'], out['hit'])
    print(shares)
    assert shares['ambiguous'] <= 0.01
    assert shares['hit'] > 0.10 and shares['miss'] > 0.10
    want = R.clip_rays(rays, occupied, R.BOUNDS, R.NEAR, R.FAR)
    for k in ('t', 'hit', 'affine', 'rays'):
        assert out[k].tobytes() == want[k].tobytes(), k
    # however the rays are split into calls
    parts = [host(HN.clip_rays(gpu(rays[a:b]), occ, R.NEAR, R.FAR, min_span=0.0)) for a, b in ((0, 1), (1, 1235), (1235, 4000))]
    for k in out:
        assert np.concatenate([p[k] for p in parts]).tobytes() == out[k].tobytes(), k
    none = HN.clip_rays(gpu(rays[:0]), occ, R.NEAR, R.FAR)
    assert none['t'].shape == (0, 2) and none['rays'].shape == (0, 9)


def test_clip_handmade_rays(probe):
    occupied, _, occ = probe
    rays, names = R.handmade_rays()
    full_cells = np.ones(R.CELLS, dtype=bool)
    for cells, o in ((occupied, occ), (full_cells, to_occ(full_cells, R.BOUNDS))):
        out = host(HN.clip_rays(gpu(rays), o, R.NEAR, R.FAR, min_span=0.0))
        R.check_intervals(rays, cells, R.BOUNDS, R.NEAR, R.FAR, out['t'], out['hit'], need_required=False)
        assert np.isfinite(out['t']).all() and np.isfinite(out['affine']).all()
        want = R.clip_rays(rays, cells, R.BOUNDS, R.NEAR, R.FAR)
        assert out['t'].tobytes() == want['t'].tobytes() and out['hit'].tobytes() == want['hit'].tobytes()
        for name, h, row, src in zip(names, out['hit'], out['rays'], rays):
            if any(w in name for w in ("NaN", "inf", "misses", "away", "outside")):
                assert h == 0, name
            if h == 0:
                assert row.tobytes() == src.tobytes(), name
            else:
                assert np.isfinite(row).all(), name
    o = to_occ(full_cells, R.BOUNDS)
    thin = host(HN.clip_rays(gpu(rays), o, R.NEAR, R.FAR, min_span=0.0))
    graze = names.index("grazes the corner (1.5, 1.25, z)")
    inside = names.index("origin inside, first cell")
    ends = names.index("far ends inside")
    assert thin['hit'][graze] == 1 and thin['t'][graze, 1] - thin['t'][graze, 0] < 1e-3
    assert thin['t'][inside, 0] == np.float32(R.NEAR) and thin['t'][ends, 1] == np.float32(R.FAR)
    wide = host(HN.clip_rays(gpu(rays), o, R.NEAR, R.FAR))                       # min_span: the cell edge, 0.25
    assert abs((wide['t'][graze, 1] - wide['t'][graze, 0]) - 0.25) < 1e-6
    assert abs(wide['t'][graze].sum() - thin['t'][graze].sum()) < 1e-6
    assert (wide['t'][:, 0] >= np.float32(R.NEAR)).all() and (wide['t'][:, 1] <= np.float32(R.FAR)).all()
    keep = host(HN.clip_rays(gpu(rays), o, R.NEAR, R.FAR, clip_far=False, min_span=0.0))
    assert (keep['t'][:, 1] == np.float32(R.FAR)).all() and np.array_equal(keep['t'][:, 0], thin['t'][:, 0])


# ---- 4. the re-parametrisation --------------------------------------------------------------------------------------------------
def test_clipped_rows_sample_the_clipped_interval(probe):
    _, rays, occ = probe
    out = host(HN.clip_rays(gpu(rays), occ, R.NEAR, R.FAR))
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    o2, d2 = out['rays'][:, 0:3].astype(np.float64), out['rays'][:, 3:6].astype(np.float64)
    t0, t1 = out['t'][:, 0:1].astype(np.float64), out['t'][:, 1:2].astype(np.float64)
    a, b = out['affine'][:, 0:1].astype(np.float64), out['affine'][:, 1:2].astype(np.float64)
    scale = max(np.abs(o).max() + R.FAR * np.abs(d).max(), 1.0)
    for z in (R.NEAR, 0.5 * (R.NEAR + R.FAR), R.FAR):
        assert np.abs((o2 + d2 * z) - (o + d * (t0 + (z - R.NEAR) * b))).max() <= 1e-5 * scale
        assert np.abs((a + b * z) - (t0 + (z - R.NEAR) * b)).max() <= 1e-5 * R.FAR
    assert np.abs((a + b * R.FAR) - t1).max() <= 1e-5 * R.FAR
    assert np.array_equal(out['rays'][:, 6:], rays[:, 6:]) and len(np.unique(rays[:, 8])) > 10      # column 8 passes through
    miss = out['hit'] == 0
    assert miss.sum() > 400 and out['rays'][miss].tobytes() == rays[miss].tobytes()
    assert (out['affine'][miss] == (0.0, 1.0)).all() and (out['t'][miss] == (R.NEAR, R.FAR)).all()
    moved = (out['hit'] == 1) & ((out['t'][:, 0] > R.NEAR) | (out['t'][:, 1] < R.FAR))
    assert moved.sum() > 400 and (out['affine'][moved, 1] < 1.0).all()


# ---- 5. the wiring, with a stub in the field's place ----------------------------------------------------------------------------
SPHERE = 0.5
WEIGHTS = (0.6, 0.3, 0.1)


class SphereStub(torch.nn.Module):
    """What inference.render_image needs of a model.  The analytic sphere of radius 0.5 at the origin in the z of the rows
    it is given: three samples, all at the hit, with weights 0.6, 0.3, 0.1 — and, as under use_sample_at_infinity, an acc
    that leaves the last one out (0.9), so that un-mapping depth with acc instead of the weights' sum is wrong by
    0.1 a.  rgb is a function of the view direction.  It records what it receives."""
    near, far = 0.5, 6.0

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward(self, ray_dict, extra, **kw):
        o, d = ray_dict["origins"].double(), ray_dict["directions"].double()
        v = ray_dict["viewdirs"]
        self.calls.append({"origins": ray_dict["origins"].clone(), "directions": ray_dict["directions"].clone(),
                           "viewdirs": None if v is None else v.clone(), "kw": kw,
                           "ids": ray_dict["metadata"]["warp"].reshape(-1).clone()})
        v = (ray_dict["directions"] if v is None else v).double()
        aa, bb, cc = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - SPHERE ** 2
        disc = bb * bb - aa * cc
        hit = disc >= 0
        z = (-bb - torch.sqrt(torch.where(hit, disc, torch.zeros_like(disc)))) / aa
        z = torch.where(hit, z, torch.full_like(z, self.near))
        weights = hit[:, None] * torch.tensor(WEIGHTS, dtype=torch.float64, device=o.device)
        out = {"rgb": (0.5 + 0.5 * v / v.norm(dim=-1, keepdim=True)).float(), "depth": (weights.sum(-1) * z).float(),
               "acc": weights[:, :-1].sum(-1).float(), "weights": weights.float(), "med_depth": z.float()}
        return {level: out for level in ("coarse", "fine")}


def sphere_scene():
    wh = (24, 18)
    cam = HN.orbit_cameras((0.0, 0.0, 0.0), 3.0, 1, 20.0, focal=30.0, image_wh=wh)[0]
    rays = HN.camera_rays(gpu(cam), wh[0], wh[1], SphereStub.near, SphereStub.far)
    rays = torch.cat([rays, torch.full((rays.shape[0], 1), 5.0, device=DEV)], dim=1)
    rays[:, 3:6] *= 1.3                                                       # not unit: distances are in units of |d|
    bounds = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)
    pts = np.stack(np.meshgrid(*[np.linspace(-1, 1, 17)] * 3, indexing="ij"), axis=-1)
    grid = np.where(np.linalg.norm(pts, axis=-1) <= SPHERE, 10.0, 0.0).astype(np.float32)
    occ = HN.occupancy_from_density(gpu(grid), bounds, 5.0, dilate=1)
    o, d = rays[:, 0:3].double().cpu().numpy(), rays[:, 3:6].double().cpu().numpy()
    aa, bb, cc = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - SPHERE ** 2
    disc = bb * bb - aa * cc
    truth = (-bb - np.sqrt(np.maximum(disc, 0.0))) / aa
    return rays, occ, truth, disc > 1e-3


def test_render_image_unmaps_with_the_weights_and_keeps_the_view_directions():
    rays, occ, truth, on_sphere = sphere_scene()
    assert 0.02 < HN.occupancy_fraction(occ) < 0.5 and on_sphere.sum() > 30
    model = SphereStub().to(DEV)
    keys = ('rgb', 'depth', 'acc', 'med_depth')
    plain = inference.render_image(model, rays, chunk=4096, keys=keys)
    assert model.calls[0]["viewdirs"] is None and model.calls[0]["kw"] == {}
    del model.calls[:]
    got = inference.render_image(model, rays, chunk=4096, keys=keys, occupancy=occ)
    clip = HN.clip_rays(rays, occ, model.near, model.far)
    assert len(model.calls) == 1 and model.calls[0]["kw"] == {}
    seen = model.calls[0]
    assert torch.equal(seen["viewdirs"], rays[:, 3:6]) and torch.equal(seen["origins"], clip['rays'][:, 0:3])
    assert torch.equal(seen["directions"], clip['rays'][:, 3:6]) and (seen["ids"] == 5).all()
    a = clip['affine'][:, 0].cpu().numpy()
    assert (np.abs(a[on_sphere]) > 0.5).all()              # the clip moved these rays: an acc-based un-map is off by 0.1 a
    depth, med = got['depth'].cpu().numpy(), got['med_depth'].cpu().numpy()
    assert np.abs(depth[on_sphere] - truth[on_sphere]).max() <= 1e-4
    assert np.abs(med[on_sphere] - truth[on_sphere]).max() <= 1e-4
    assert np.abs(plain['depth'].cpu().numpy()[on_sphere] - truth[on_sphere]).max() <= 1e-4
    assert torch.equal(got['rgb'], plain['rgb']) and torch.equal(got['acc'], plain['acc'])
    assert (got['acc'].cpu().numpy()[on_sphere] == np.float32(0.9)).all()
    # in several chunks, and with near / far given: handed on to the model
    del model.calls[:]
    again = inference.render_image(model, rays, chunk=100, keys=keys, occupancy=occ, near=0.5, far=6.0)
    assert len(model.calls) == 5 and all(c["kw"] == {"near": 0.5, "far": 6.0} for c in model.calls)
    for k in keys:
        assert torch.equal(again[k], got[k]), k
    with pytest.raises(ValueError, match="keys"):
        inference.render_image(model, rays, keys=('rgb', 'weights'), occupancy=occ)


def test_render_image_skips_the_misses():
    rays, occ, truth, on_sphere = sphere_scene()
    model = SphereStub().to(DEV)
    clip = HN.clip_rays(rays, occ, model.near, model.far)
    hit = clip['hit'].bool()
    assert 30 < int(hit.sum()) < rays.shape[0] - 30
    keys = ('rgb', 'depth', 'acc', 'med_depth')
    got = inference.render_image(model, rays, chunk=4096, keys=keys, occupancy=occ, miss='skip', miss_rgb=(1.0, 0.5, 0.25))
    full = inference.render_image(model, rays, chunk=4096, keys=keys, occupancy=occ)
    seen = model.calls[0]
    assert seen["origins"].shape[0] == int(hit.sum()) and torch.equal(seen["origins"], clip['rays'][hit][:, 0:3])
    assert torch.equal(seen["viewdirs"], rays[hit][:, 3:6])
    for k in keys:
        assert got[k].shape == full[k].shape and torch.equal(got[k][hit], full[k][hit]), k
    assert (got['rgb'][~hit] == torch.tensor([1.0, 0.5, 0.25], device=DEV)).all()
    assert (got['depth'][~hit] == 0).all() and (got['acc'][~hit] == 0).all() and (got['med_depth'][~hit] == 0).all()
    assert not on_sphere[~hit.cpu().numpy()].any()                       # nothing of the sphere was skipped
    black = inference.render_image(model, rays, keys=('rgb',), occupancy=occ, miss='skip')
    assert (black['rgb'][~hit] == 0).all()
    depths = HN.depth_images_from_field(model, HN.orbit_cameras((0.0, 0.0, 0.0), 3.0, 1, 20.0, focal=30.0, image_wh=(24, 18)),
                                        (24, 18), 5, model.near, model.far, acc_min=0.8, occupancy=occ)
    plain = HN.depth_images_from_field(model, HN.orbit_cameras((0.0, 0.0, 0.0), 3.0, 1, 20.0, focal=30.0, image_wh=(24, 18)),
                                       (24, 18), 5, model.near, model.far, acc_min=0.8)
    finite = torch.isfinite(plain)
    assert torch.equal(torch.isfinite(depths), finite) and finite.sum() > 30
    # depth / acc: the stub's acc of 0.9 divides both alike
    assert (depths[finite] - plain[finite]).abs().max() <= 2e-4


# ---- 6. identity on the real model ----------------------------------------------------------------------------------------------
def test_real_model_with_an_occupancy_is_bit_identical():
    """fp32, deterministic sampling.  An all-occupied grid whose box holds every ray's [near, far] segment clips nothing:
    b = 1, a = 0, and render_image gives the bits it gives without an occupancy.  A partial grid gives the bits of clip,
    model call with the original view directions and unclip done by hand."""
    old = HN.get_precision()
    HN.set_precision("fp32")
    try:
        m = models.NerfModel(EMB, near=0.5, far=3.0, n_samples_coarse=8, n_samples_fine=8, noise_std=None,
                             hyper_slice_method="bendy_sheet", use_nerf_embed=True, use_alpha_cond=True)
        load_hash(m, 31)
        m = m.to(DEV)
        m.use_stratified_sampling = False
        b = 48
        o, d, idx = rays_for(31, b)
        rays = torch.cat([o, d, torch.full((b, 1), 0.5), torch.full((b, 1), 3.0), idx.float()[:, None]], dim=1).to(DEV)
        keys = ('rgb', 'depth', 'acc', 'med_depth')
        plain = inference.render_image(m, rays, chunk=4096, keys=keys)
        box = (-8.0, 8.0) * 3                                   # |o| <= 1.74, far * |d| <= 4.8
        everything = to_occ(np.ones((4, 5, 70), dtype=bool), box)
        clip = HN.clip_rays(rays, everything, m.near, m.far)
        assert clip['hit'].all() and torch.equal(clip['rays'], rays)
        assert (clip['affine'] == torch.tensor([0.0, 1.0], device=DEV)).all()
        same = inference.render_image(m, rays, chunk=4096, keys=keys, occupancy=everything)
        for k in keys:
            assert torch.equal(same[k], plain[k]), k
        chunked = inference.render_image(m, rays, chunk=4096, keys=keys, occupancy=everything, miss='skip')
        for k in keys:
            assert torch.equal(chunked[k].reshape(plain[k].shape), plain[k]), k
        # a partial grid
        cells = np.random.default_rng(5).random((8, 8, 8)) < 0.3
        part = to_occ(cells, (-2.0, 2.0) * 3)
        got = inference.render_image(m, rays, chunk=4096, keys=keys, occupancy=part)
        clip = HN.clip_rays(rays, part, m.near, m.far)
        moved = (clip['affine'][:, 1] < 1.0)
        assert 8 < int(moved.sum()) and int(clip['hit'].sum()) < b
        rd = model_utils.prepare_ray_dict(clip['rays'])
        rd['viewdirs'] = rays[:, 3:6]
        res = m(rd, dict(inference._EXTRA))['fine']
        hand = HN.unclip({k: res[k] for k in keys + ('weights',)}, clip['affine'])
        for k in keys:
            assert torch.equal(got[k], hand[k]), k
        assert not torch.equal(got['depth'][moved], plain['depth'][moved])
        miss = ~clip['hit'].bool()
        for k in keys:                                           # a missed ray is rendered exactly as without the grid
            assert torch.allclose(got[k][miss], plain[k][miss], rtol=0, atol=0), k
    finally:
        HN.set_precision(old)


# ---- 7. occupancy_grid, OccupancyCache ----------------------------------------------------------------------------------------
class BlobField(torch.nn.Module):
    """query_points of an analytic field: a Gaussian blob whose centre moves with the frame id."""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.frames = []

    def query_points(self, points, metadata, level='fine', viewdirs=None, render_opts=None):
        frame = int(metadata['warp'][0])
        if not self.frames or self.frames[-1] != frame:
            self.frames.append(frame)
        centre = torch.tensor([0.05 * frame - 0.3, 0.1, -0.2], device=points.device)
        return {'sigma': 20.0 * torch.exp(-((points - centre) ** 2).sum(-1) / 0.08)}


def test_occupancy_grid_and_cache():
    model = BlobField().to(DEV)
    bounds, shape, sigma_min = (-1.0, 1.0, -0.8, 0.9, -1.0, 0.7), (13, 11, 10), 2.0
    grid = HN.density_grid(model, bounds, shape, 3).cpu().numpy()
    assert 0.01 < (grid >= sigma_min).mean() < 0.5
    occ = HN.occupancy_grid(model, bounds, shape, 3, sigma_min, dilate=0)
    assert occ['cells'] == (12, 10, 9) and occ['bounds'] == bounds and occ['bits'].shape == (12, 10, 1)
    cells = R.mark(grid, sigma_min)
    assert np.array_equal(occ['bits'].cpu().numpy(), R.pack(cells))
    for i, j, k in zip(*np.nonzero(grid >= sigma_min)):          # a dense lattice point lies in occupied cells only
        assert cells[max(i - 1, 0):i + 1, max(j - 1, 0):j + 1, max(k - 1, 0):k + 1].all()
    grown = HN.occupancy_grid(model, bounds, shape, 3, sigma_min, dilate=2, chunk=300)
    assert np.array_equal(grown['bits'].cpu().numpy(), R.pack(R.dilate(cells, 2)))
    assert abs(HN.occupancy_fraction(grown) - R.dilate(cells, 2).mean()) < 1e-12
    both = HN.occupancy_union(occ, HN.occupancy_grid(model, bounds, shape, 9, sigma_min, dilate=0))
    other = R.mark(HN.density_grid(model, bounds, shape, 9).cpu().numpy(), sigma_min)
    assert np.array_equal(both['bits'].cpu().numpy(), R.pack(cells | other)) and (cells != other).any()
    del model.frames[:]
    cache = HN.OccupancyCache(model, bounds, shape, sigma_min, dilate=0)
    first = cache.get(3)
    assert cache.get(3) is first and torch.equal(first['bits'], occ['bits'])
    cache.get(9)
    cache.get(3)
    assert cache.builds == 2 and model.frames == [3, 9]
    # evaluate_images asks the cache for the frame in column 8 of each image's rays
    stub = SphereStub().to(DEV)
    rays, _, _, _ = sphere_scene()
    fake = HN.OccupancyCache(model, (-1.0, 1.0) * 3, 9, 1e-3, dilate=1)
    out = inference.evaluate_images(stub, [{'rays': rays, 'hw': (18, 24)}], occupancy=fake)
    assert fake.builds == 1 and model.frames[-1] == 5 and out['images'][0].shape == (18, 24, 3)
    plain = inference.evaluate_images(stub, [{'rays': rays, 'hw': (18, 24)}])
    assert torch.equal(out['images'][0], plain['images'][0])
