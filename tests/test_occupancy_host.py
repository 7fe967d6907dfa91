"""Occupancy grids and ray clipping without a GPU: the NumPy restatement of csrc/hn_occupancy.hip against the float64
statement, the bit layout, the dilation, every refusal of the host halves and of the C ABI, the exports."""
import ctypes

import numpy as np
import pytest
import torch

import hypernerf_torch_amd as HN
import occupancy_restated as R
from hypernerf_torch_amd import _lib as L
from hypernerf_torch_amd import functional as F
from hypernerf_torch_amd import inference
from hypernerf_torch_amd.ops import occupancy as OPS

B = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)


def occ_dict(cells=(3, 4, 5), bounds=B, bits=None):
    if bits is None:
        shape = (cells[0], cells[1], (cells[2] + 63) // 64) if len(cells) == 3 else (3, 4, 1)
        bits = torch.zeros(shape, dtype=torch.int64)
    return {'bits': bits, 'cells': cells, 'bounds': bounds}


# ---- 1. the restated walk satisfies the interval property ---------------------------------------------------------------------
def test_restated_walk_satisfies_the_interval_property():
    """Grid 12 x 10 x 9 over the issue's box, about 15 % occupied, 4000 rays, near 0.5, far 6: the float32 walk contains the
    required cells and stays inside the allowed ones within 32 ulp of far; at most 1 % of the rays have a cell in between;
    hits and misses are both above 10 %."""
    occupied, rays = R.probe_grid(), R.probe_rays()
    assert 0.10 < occupied.mean() < 0.20
    out = R.clip_rays(rays, occupied, R.BOUNDS, R.NEAR, R.FAR)
    shares = R.check_intervals(rays, occupied, R.BOUNDS, R.NEAR, R.FAR, out['t'], out['hit'])
    print(shares)
    assert shares['ambiguous'] <= 0.01
    assert shares['hit'] > 0.10 and shares['miss'] > 0.10


def test_the_property_refuses_a_wrong_interval():
    """The checker is not vacuous: an interval cut short, one grown past the allowed cells and a dropped hit all fail."""
    occupied, rays = R.probe_grid(), R.probe_rays(400)
    out = R.clip_rays(rays, occupied, R.BOUNDS, R.NEAR, R.FAR)
    hit = out['hit'].astype(bool)
    long_ones = hit & (out['t'][:, 1] - out['t'][:, 0] > 0.3) & (out['t'][:, 0] > R.NEAR + 0.1)
    assert long_ones.sum() > 10
    for change in ("short", "long", "dropped"):
        t, h = out['t'].copy(), out['hit'].copy()
        r = np.nonzero(long_ones)[0][3]
        if change == "short":
            t[r, 0] += 0.1
        elif change == "long":
            t[r, 0] -= 0.05
        else:
            h[r], t[r] = 0, (R.NEAR, R.FAR)
        with pytest.raises(AssertionError):
            R.check_intervals(rays, occupied, R.BOUNDS, R.NEAR, R.FAR, t, h)


def test_restated_handmade_rays():
    """The degenerate rays: inside the allowed cells, finite, the rays that are not finite and the ones off the box miss."""
    rays, names = R.handmade_rays()
    for occupied in (R.probe_grid(), np.ones(R.CELLS, dtype=bool)):
        out = R.clip_rays(rays, occupied, R.BOUNDS, R.NEAR, R.FAR)
        R.check_intervals(rays, occupied, R.BOUNDS, R.NEAR, R.FAR, out['t'], out['hit'], need_required=False)
        assert np.isfinite(out['t']).all() and np.isfinite(out['affine']).all()
        for name, h, row, src in zip(names, out['hit'], out['rays'], rays):
            if any(w in name for w in ("NaN", "inf", "misses", "away", "outside")):
                assert h == 0, name
            if h == 0:
                assert row.tobytes() == src.tobytes(), name
    full = R.clip_rays(rays, np.ones(R.CELLS, dtype=bool), R.BOUNDS, R.NEAR, R.FAR)
    graze = names.index("grazes the corner (1.5, 1.25, z)")
    assert full['hit'][graze] == 1 and full['t'][graze, 1] - full['t'][graze, 0] < 1e-3
    wide = R.clip_rays(rays, np.ones(R.CELLS, dtype=bool), R.BOUNDS, R.NEAR, R.FAR, min_span=0.25)
    assert abs((wide['t'][graze, 1] - wide['t'][graze, 0]) - 0.25) < 1e-6
    assert abs((wide['t'][graze].sum() - full['t'][graze].sum())) < 1e-6      # symmetric
    keep = R.clip_rays(rays, np.ones(R.CELLS, dtype=bool), R.BOUNDS, R.NEAR, R.FAR, clip_far=False)
    assert (keep['t'][:, 1] == np.float32(R.FAR)).all() and (keep['t'][:, 0] == full['t'][:, 0]).all()


def test_restated_reparametrisation():
    occupied, rays = R.probe_grid(), R.probe_rays(500)
    out = R.clip_rays(rays, occupied, R.BOUNDS, R.NEAR, R.FAR)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    o2, d2 = out['rays'][:, 0:3].astype(np.float64), out['rays'][:, 3:6].astype(np.float64)
    t0, b = out['t'][:, 0:1].astype(np.float64), out['affine'][:, 1:2].astype(np.float64)
    for z in (R.NEAR, 0.5 * (R.NEAR + R.FAR), R.FAR):
        assert np.abs((o2 + d2 * z) - (o + d * (t0 + (z - R.NEAR) * b))).max() <= 1e-5 * 10.0
    assert (out['rays'][:, 6:] == rays[:, 6:]).all()
    miss = out['hit'] == 0
    assert out['rays'][miss].tobytes() == rays[miss].tobytes() and (out['affine'][miss] == (0.0, 1.0)).all()


# ---- 2. layout, mark, dilation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cz", [1, 9, 63, 64, 65, 130])
def test_packing_layout_and_padding(cz):
    rng = np.random.default_rng(cz)
    cells = rng.random((3, 2, cz)) < 0.4
    bits = R.pack(cells)
    assert bits.shape == (3, 2, (cz + 63) // 64) and bits.dtype == np.int64
    for i, j, k in [(0, 0, 0), (2, 1, cz - 1), (1, 0, cz // 2)]:
        assert bool((int(bits[i, j, k // 64]) >> (k % 64)) & 1) == bool(cells[i, j, k])
    back, pad = R.unpack(bits, cz)
    assert (back == cells).all() and not pad.any() and R.popcount(bits) == cells.sum()


def test_mark_restated():
    grid = np.zeros((4, 3, 5), dtype=np.float32)
    grid[1, 1, 2] = 2.0
    cells = R.mark(grid, 2.0)                      # a value equal to sigma_min counts
    want = np.zeros((3, 2, 4), dtype=bool)
    want[0:2, 0:2, 1:3] = True
    assert (cells == want).all()
    assert not R.mark(grid, 2.5).any()
    grid[3, 2, 4] = np.nan
    assert R.mark(grid, 1e30)[2, 1, 3] and R.mark(grid, 1e30).sum() == 1
    grid[3, 2, 4] = np.inf
    assert R.mark(grid, 1e30)[2, 1, 3]


@pytest.mark.parametrize("cz", [9, 64, 65, 130])
def test_word_dilation_equals_the_cube_maximum(cz):
    rng = np.random.default_rng(100 + cz)
    cells = rng.random((5, 4, cz)) < 0.03
    cells[0, 0, 0] = cells[4, 3, cz - 1] = True                 # corners: nothing wraps
    if cz > 64:
        cells[2, 2, 63] = cells[1, 1, 64] = True                # across a word boundary, both ways
    bits = R.pack(cells)
    for radius in (1, 2, 3):
        bits = R.dilate_words(bits, cz)
        got, pad = R.unpack(bits, cz)
        assert (got == R.dilate(cells, radius)).all() and not pad.any()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs, word", [
    (dict(grid=torch.zeros((4, 4))), "grid"),
    (dict(grid=torch.zeros((4, 4, 4), dtype=torch.float64)), "grid"),
    (dict(grid=torch.zeros((4, 4, 8))[:, :, ::2]), "grid"),
    (dict(grid=torch.zeros((1, 4, 4))), "2 points"),
    (dict(grid=torch.zeros((2, 2, 2051))), "cells"),
    (dict(bounds=(0.0, 1.0, 0.0, 1.0, 0.0, -1.0)), "bounds"),
    (dict(bounds=(0.0, float("inf"), 0.0, 1.0, 0.0, 1.0)), "bounds"),
    (dict(bounds=(0.0, 1.0)), "bounds"),
    (dict(sigma_min=float("nan")), "sigma_min"),
    (dict(sigma_min="dense"), "sigma_min"),
    (dict(dilate=-1), "dilate"),
    (dict(dilate=1.5), "dilate"),
    (dict(dilate=True), "dilate"),
    (dict(), "GPU"),
])
def test_occupancy_from_density_refuses(kwargs, word):
    args = dict(grid=torch.zeros((4, 4, 4)), bounds=B, sigma_min=1.0, dilate=1)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        HN.occupancy_from_density(**args)


@pytest.mark.parametrize("kwargs, word", [
    (dict(resolution=(4, 4)), "three sides"),
    (dict(resolution=1), "2 points"),
    (dict(resolution=(2, 2, 4000)), "cells"),
    (dict(bounds=(1.0, 0.0, 0.0, 1.0, 0.0, 1.0)), "bounds"),
    (dict(sigma_min=None), "sigma_min"),
    (dict(dilate=5000), "dilate"),
])
def test_occupancy_grid_and_cache_refuse_before_touching_the_model(kwargs, word):
    args = dict(model=None, bounds=B, resolution=8, frame_id=0, sigma_min=1.0, dilate=1)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        HN.occupancy_grid(**args)
    del args['frame_id']
    with pytest.raises(ValueError, match=word):
        HN.OccupancyCache(**args)


def test_cache_refuses_its_own_arguments():
    for kw, word in ((dict(max_entries=0), "max_entries"), (dict(max_entries=2.5), "max_entries"), (dict(chunk=0), "chunk")):
        with pytest.raises(ValueError, match=word):
            HN.OccupancyCache(None, B, 8, 1.0, **kw)
    with pytest.raises(ValueError, match="frame_id"):
        HN.OccupancyCache(None, B, 8, 1.0).get(1.5)


@pytest.mark.parametrize("occ, word", [
    ("grid", "dict"),
    ({'bits': torch.zeros((3, 4, 1), dtype=torch.int64)}, "dict"),
    (occ_dict(cells=(3, 4)), "cells"),
    (occ_dict(cells=(0, 4, 5)), "cells"),
    (occ_dict(bits=torch.zeros((3, 4, 1), dtype=torch.int32)), "bits"),
    (occ_dict(bits=torch.zeros((3, 4, 2), dtype=torch.int64)), "bits"),
    (occ_dict(bits=torch.zeros((3, 4, 2), dtype=torch.int64)[:, :, ::2]), "contiguous"),
    (occ_dict(bounds=(0.0, 0.0, 0.0, 1.0, 0.0, 1.0)), "bounds"),
    (occ_dict(bounds=(0.0, float("nan"), 0.0, 1.0, 0.0, 1.0)), "bounds"),
])
def test_an_occupancy_is_checked(occ, word):
    for fn in (lambda: HN.occupancy_fraction(occ), lambda: HN.occupancy_union(occ, occ_dict()),
               lambda: HN.occupancy_union(occ_dict(), occ), lambda: HN.clip_rays(torch.zeros((2, 8)), occ, 0.0, 1.0)):
        with pytest.raises(ValueError, match=word):
            fn()


def test_union():
    a, b = occ_dict(), occ_dict()
    a['bits'][0, 0, 0], b['bits'][0, 0, 0], b['bits'][2, 3, 0] = 0b0101, 0b0011, -2 ** 63
    u = HN.occupancy_union(a, b)
    assert u['bits'][0, 0, 0] == 0b0111 and u['bits'][2, 3, 0] == -2 ** 63 and u['cells'] == (3, 4, 5) and u['bounds'] == B
    assert a['bits'][0, 0, 0] == 0b0101
    with pytest.raises(ValueError, match="differ"):
        HN.occupancy_union(a, occ_dict(cells=(3, 4, 6)))
    with pytest.raises(ValueError, match="differ"):
        HN.occupancy_union(a, occ_dict(bounds=(-1.0, 1.0, -1.0, 1.0, -1.0, 2.0)))


@pytest.mark.parametrize("kwargs, word", [
    (dict(rays=torch.zeros((4, 5))), "rays"),
    (dict(rays=torch.zeros((4, 65))), "rays"),
    (dict(rays=torch.zeros((4, 8), dtype=torch.float64)), "rays"),
    (dict(rays=torch.zeros((8,))), "rays"),
    (dict(near=1.0, far=1.0), "far > near"),
    (dict(near=float("nan")), "near"),
    (dict(far=float("inf")), "far"),
    (dict(near="close"), "near"),
    (dict(min_span=-0.1), "min_span"),
    (dict(min_span=float("inf")), "min_span"),
    (dict(min_span="wide"), "min_span"),
    (dict(), "GPU"),
])
def test_clip_rays_refuses(kwargs, word):
    args = dict(rays=torch.zeros((4, 8)), occ=occ_dict(), near=0.5, far=6.0)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        HN.clip_rays(**args)


def test_the_lower_ops_refuse():
    with pytest.raises(ValueError, match="GPU"):
        F.occupancy_mark(torch.zeros((4, 4, 4)), 1.0)
    with pytest.raises(ValueError, match="sigma_min"):
        F.occupancy_mark(torch.zeros((4, 4, 4)), float("nan"))
    with pytest.raises(ValueError, match="GPU"):
        F.occupancy_dilate(torch.zeros((3, 3, 1), dtype=torch.int64), (3, 3, 3))
    with pytest.raises(ValueError, match="bits"):
        F.occupancy_dilate(torch.zeros((3, 3, 2), dtype=torch.int64), (3, 3, 3))
    with pytest.raises(ValueError, match="dilate"):
        F.occupancy_dilate(torch.zeros((3, 3, 1), dtype=torch.int64), (3, 3, 3), times=-2)
    with pytest.raises(ValueError, match="GPU"):
        F.occupancy_count(torch.zeros((3, 3, 1), dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        F.occupancy_count(torch.zeros((3, 3, 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        F.occupancy_count(torch.zeros((0,), dtype=torch.int64))


def test_unclip_uses_the_weights_not_acc():
    """depth = sum w z with z_true = a + b z: the constant goes with the sum of the same weights.  Under
    use_sample_at_infinity acc leaves the last sample out, so an acc-based map is off by a * w_last."""
    weights = torch.tensor([[0.2, 0.3, 0.4], [0.0, 0.5, 0.1]])
    z = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])
    affine = torch.tensor([[2.0, 0.25], [0.0, 1.0]])
    z_true = affine[:, 0:1] + affine[:, 1:2] * z
    res = {'depth': (weights * z).sum(-1), 'acc': weights[:, :-1].sum(-1), 'weights': weights,
           'med_depth': z[:, 1], 'rgb': torch.rand(2, 3)}
    out = HN.unclip(res, affine)
    assert torch.allclose(out['depth'], (weights * z_true).sum(-1), atol=1e-6)
    assert torch.allclose(out['med_depth'], z_true[:, 1], atol=1e-6)
    assert out['rgb'] is res['rgb'] and out['acc'] is res['acc'] and res['depth'][0] != out['depth'][0]
    assert torch.equal(out['depth'][1], res['depth'][1]) and torch.equal(out['med_depth'][1], res['med_depth'][1])   # (0, 1): the bits
    assert not torch.allclose(affine[:, 0] * res['acc'] + affine[:, 1] * res['depth'], out['depth'], atol=1e-3)
    for bad, word in ((dict(res="x"), "dict"), (dict(affine=torch.zeros(2)), "affine"),
                      (dict(res={'depth': res['depth']}), "weights"),
                      (dict(res={'depth': res['depth'][:1], 'weights': weights}), "depths"),
                      (dict(res={'med_depth': z[:1, 1]}), "median")):
        args = dict(res=res, affine=affine)
        args.update(bad)
        with pytest.raises(ValueError, match=word):
            HN.unclip(**args)


class _NoModel:
    near, far = 0.5, 6.0

    def __call__(self, *a, **k):
        raise AssertionError("the model must not run")


def test_render_image_refuses_before_rendering():
    rays = torch.zeros((4, 9))
    for kw, word in ((dict(occupancy=occ_dict(), miss='drop'), "miss"), (dict(miss='skip'), "needs an occupancy"),
                     (dict(occupancy=occ_dict(), keys=('rgb', 'weights')), "keys"),
                     (dict(occupancy=occ_dict(), miss_rgb=(1.0, 0.0)), "miss_rgb"),
                     (dict(occupancy=occ_dict(cells=(3, 4))), "cells"),
                     (dict(occupancy=occ_dict(), near=2.0, far=1.0), "far > near"),
                     (dict(occupancy=occ_dict()), "GPU")):
        with pytest.raises(ValueError, match=word):
            inference.render_image(_NoModel(), rays, **kw)


def test_a_cache_needs_one_frame_id_per_image():
    class Cache(OPS.OccupancyCache):
        def __init__(self):
            self.asked = []

        def get(self, frame_id):
            self.asked.append(frame_id)
            return "grid"

    cache = Cache()
    rays = torch.zeros((6, 9))
    rays[:, 8] = 12
    assert inference._image_occupancy(cache, rays, 0) == "grid" and cache.asked == [12]
    assert inference._image_occupancy({"an": "occupancy"}, rays[:, :8], 0) == {"an": "occupancy"}
    with pytest.raises(ValueError, match="column 8"):
        inference._image_occupancy(cache, rays[:, :8], 3)
    rays[2, 8] = 13
    with pytest.raises(ValueError, match="one integer id per image"):
        inference._image_occupancy(cache, rays, 3)
    with pytest.raises(ValueError, match="column 8"):
        inference.evaluate_images(_NoModel(), [{'rays': rays[:, :8]}], occupancy=cache)


def test_evaluate_images_hands_occupancy_and_clip_far_on(monkeypatch):
    seen = []

    def fake(model, rays, **kw):
        seen.append(kw)
        return {'rgb': torch.zeros((rays.shape[0], 3)), 'depth': torch.zeros(rays.shape[0])}

    monkeypatch.setattr(inference, "render_image", fake)
    sample = {'rays': torch.zeros((6, 8)), 'hw': (2, 3)}
    inference.evaluate_images(None, [sample])
    inference.evaluate_images(None, [sample], occupancy="occ", clip_far=False)
    assert seen[0] == dict(chunk=16384, keys=('rgb', 'depth'), group=None)             # without the keyword: today's call
    assert seen[1] == dict(chunk=16384, keys=('rgb', 'depth'), group=None, occupancy="occ", clip_far=False)


def test_cache_builds_each_frame_once_and_forgets_the_oldest(monkeypatch):
    built = []
    monkeypatch.setattr(OPS, "occupancy_grid", lambda model, bounds, res, fid, s, d, **kw: built.append((fid, res, s, d, kw)) or {"frame": fid})
    cache = HN.OccupancyCache("model", B, 8, 0.5, dilate=2, max_entries=2, chunk=4096)
    assert cache.get(3) is cache.get(3) and cache.get(4)["frame"] == 4 and cache.builds == 2 and len(cache) == 2
    assert built[0] == (3, (8, 8, 8), 0.5, 2, {"level": "fine", "chunk": 4096})
    cache.get(3)
    cache.get(5)                        # 4 is the least recently used one now
    assert cache.builds == 3 and len(cache) == 2
    cache.get(3)
    assert cache.builds == 3
    cache.get(4)
    assert cache.builds == 4


def test_geometry_passes_the_occupancy_through(monkeypatch):
    G = HN.geometry
    seen = []
    monkeypatch.setattr(G, "depth_images_from_field", lambda *a, **k: seen.append(k) or "depths")
    monkeypatch.setattr(G, "fuse_depth", lambda *a, **k: "volume")
    monkeypatch.setattr(G, "tsdf_isosurface", lambda v, b: {"faces": 1})
    monkeypatch.setattr(G, "_finish_mesh", lambda mesh, *a: mesh)
    cams = np.zeros((1, 24), dtype=np.float32)
    G.extract_mesh_fused("model", B, 5, 3, cams, (8, 6), 0.1, 4.0, occupancy="occ", chunk=64)
    G.extract_mesh_fused("model", B, 5, 3, cams, (8, 6), 0.1, 4.0)
    assert seen == [{"chunk": 64, "occupancy": "occ"}, {}]


# ---- 4. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_without_a_launch():
    """Every status below is decided on the host before any launch (the pointers are made up or NULL: a launch would
    fault, and there is no GPU here)."""
    lib = L.load()
    p = ctypes.c_void_p(4096)
    bounds = (ctypes.c_float * 6)(*B)
    assert lib.hn_occ_mark(None, 4, 4, 4, 1.0, p, None) == -3 and lib.hn_occ_mark(p, 4, 4, 4, 1.0, None, None) == -3
    assert lib.hn_occ_mark(p, 1, 4, 4, 1.0, p, None) == -2 and lib.hn_occ_mark(p, 4, 4, 2050, 1.0, p, None) == -2
    assert lib.hn_occ_mark(p, 4, 4, 4, float("nan"), p, None) == -2
    assert lib.hn_occ_mark(p, 1024, 1024, 1024, 1.0, p, None) == -2
    assert lib.hn_occ_dilate(None, p, 3, 3, 3, None) == -3 and lib.hn_occ_dilate(p, None, 3, 3, 3, None) == -3
    assert lib.hn_occ_dilate(p, p, 3, 3, 3, None) == -2 and lib.hn_occ_dilate(p, ctypes.c_void_p(8192), 3, 0, 3, None) == -2
    assert lib.hn_occ_dilate(p, ctypes.c_void_p(8192), 3, 3, 2049, None) == -2
    assert lib.hn_occ_count(None, 4, p, None) == -3 and lib.hn_occ_count(p, 4, None, None) == -3
    assert lib.hn_occ_count(p, 0, p, None) == -2 and lib.hn_occ_count(p, 2 ** 31, p, None) == -2

    def clip(**kw):
        a = dict(rays=p, n=4, ld=8, bits=p, cx=3, cy=3, cz=3, bounds=bounds, near=0.5, far=6.0, clip_far=1, min_span=0.0,
                 t=None, hit=None, out=None, affine=None)
        a.update(kw)
        return lib.hn_occ_clip_rays(a['rays'], a['n'], a['ld'], a['bits'], a['cx'], a['cy'], a['cz'], a['bounds'], a['near'],
                                    a['far'], a['clip_far'], a['min_span'], a['t'], a['hit'], a['out'], a['affine'], None)

    assert clip(rays=None) == -3 and clip(bits=None) == -3
    for bad in (dict(n=0), dict(n=2 ** 31), dict(ld=5), dict(ld=65), dict(cx=0), dict(cz=2049), dict(bounds=None),
                dict(bounds=(ctypes.c_float * 6)(0, 1, 0, 1, 1, 1)), dict(bounds=(ctypes.c_float * 6)(0, 1, 0, float("inf"), 0, 1)),
                dict(far=0.5), dict(far=float("inf")), dict(near=float("nan")), dict(min_span=-1.0),
                dict(min_span=float("nan")), dict(out=p)):
        assert clip(**bad) == -2, bad


def test_binding_and_exports():
    names = {"hn_occ_mark", "hn_occ_dilate", "hn_occ_count", "hn_occ_clip_rays"}
    assert names <= set(L.EXPORTS) and names <= set(L.ARGTYPES) and "hn_occupancy.hip" in L.SOURCES
    assert len(L.ARGTYPES["hn_occ_mark"]) == 7 and len(L.ARGTYPES["hn_occ_dilate"]) == 6
    assert len(L.ARGTYPES["hn_occ_count"]) == 4 and len(L.ARGTYPES["hn_occ_clip_rays"]) == 17
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert L.ARGTYPES["hn_occ_clip_rays"] == [p, ctypes.c_longlong, i, p, i, i, i, p, f, f, i, f, p, p, p, p, p]
    assert L.load().hn_version() == 340 and len(L.STRUCTS) == 17
    assert HN.ops.occupancy is OPS and "occupancy" in HN.ops.__all__ and "hn_occupancy.hip" in HN.ops.__doc__
    for name in OPS.__all__:
        assert getattr(F, name) is getattr(OPS, name), name
    for name in ("occupancy_from_density", "occupancy_grid", "occupancy_union", "occupancy_fraction", "clip_rays", "unclip",
                 "OccupancyCache"):
        assert getattr(HN, name) is getattr(HN.geometry, name) is getattr(OPS, name), name
